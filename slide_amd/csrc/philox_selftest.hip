// philox_selftest.hip -- slide_philox_normal_selftest (include/slide_hip.h): writes the noise the DDPM update kernels draw in
// their registers (ddpm_update.h philox_normal) for a run of consecutive elements, so a test can feed the same values to the
// explicit-noise path of those kernels and compare the generator itself with a restatement.
#include "ddpm_update.h"
#include "../../include/slide_hip.h"

namespace {

__global__ __launch_bounds__(256) void philox_normal_selftest_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                                     uint32_t nonce, uint32_t elem0, int n,
                                                                     float *__restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = philox_normal(seed_lo, seed_hi, step, elem0 + (uint32_t)i, nonce);
}

}  // namespace

// (the five words are the bit patterns of the generator's 32-bit unsigned inputs)
extern "C" int slide_philox_normal_selftest(int seed_lo, int seed_hi, int step, int nonce, int elem0, int n, float *out,
                                            slide_stream_t stream) {
  if (n < 0 || (n > 0 && !out)) return -2;
  if (n == 0) return 0;
  hipLaunchKernelGGL(philox_normal_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (uint32_t)seed_lo, (uint32_t)seed_hi, (uint32_t)step, (uint32_t)nonce, (uint32_t)elem0, n, out);
  return (int)hipGetLastError();
}
