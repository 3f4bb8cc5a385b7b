// lane_reduce_selftest.hip -- slide_lane_reduce_selftest (include/slide_hip.h): one wave runs the transposing lane reduction of
// lane_reduce.h and the all-reduce it replaced on the same values and writes out what every lane holds after each, so a test
// can compare the two bit for bit without going through a GEMM.
#include "gemm_common.h"
#include "lane_reduce.h"
#include "../../include/slide_hip.h"

namespace {

template <int NV>
__global__ __launch_bounds__(64) void lane_reduce_selftest_kernel(const float *in, float *out_new, float *out_old) {
  const int lane = threadIdx.x;
  float v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = in[lane * NV + i];
#pragma unroll
  for (int i = 0; i < NV; ++i) out_old[lane * NV + i] = lane_group_sum<32>(v[i]);
  lane_half_sums<NV>(v, lane);
  constexpr int NR = lane_half_regs(NV);
#pragma unroll
  for (int j = 0; j < NR; ++j) out_new[lane * NR + j] = v[j];
}

}  // namespace

extern "C" int slide_lane_reduce_selftest(const float *in, float *out_new, float *out_old, int nv, slide_stream_t stream) {
  if (!in || !out_new || !out_old) return -2;
  hipStream_t s = (hipStream_t)stream;
  switch (nv) {
    case 4: hipLaunchKernelGGL(lane_reduce_selftest_kernel<4>, dim3(1), dim3(64), 0, s, in, out_new, out_old); break;
    case 8: hipLaunchKernelGGL(lane_reduce_selftest_kernel<8>, dim3(1), dim3(64), 0, s, in, out_new, out_old); break;
    case 16: hipLaunchKernelGGL(lane_reduce_selftest_kernel<16>, dim3(1), dim3(64), 0, s, in, out_new, out_old); break;
    case 32: hipLaunchKernelGGL(lane_reduce_selftest_kernel<32>, dim3(1), dim3(64), 0, s, in, out_new, out_old); break;
    case 64: hipLaunchKernelGGL(lane_reduce_selftest_kernel<64>, dim3(1), dim3(64), 0, s, in, out_new, out_old); break;
    default: return -2;
  }
  return (int)hipGetLastError();
}
