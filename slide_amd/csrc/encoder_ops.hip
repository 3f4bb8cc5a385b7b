// encoder_ops.hip -- gfx950 kernels of the ENCODE side of autoencoder training (include/slide_train.h): the maximum over a sample's
// rows with its backward (Pnet2Stage, pointnet2/models/pnet.py:32-40: per-point Mlp -> max over the points -> [per-point | global]
// Mlp -> max over the points) and the diagonal Gaussian posterior with its KL term and backward
// (pointnet2/data_utils/distributions.py:4-43, applied twice by point_upsample_decoder.py:96-147).
//
// These tensors are SMALL at the product's shapes (16 key points x 16 or 32 channels per sample; 16 rows into the maximum): nothing
// here is bandwidth- or compute-bound and no throughput is claimed.  What the kernels buy is the launch count of a captured training
// step (one launch where torch composes amax + argmax + scatter, or one launch per elementwise step and reduction of the posterior
// and its KL) and reductions with a FIXED order: a sample's result depends on S, C and the strides only, never on B or on the sample's
// position in the batch, as slide_col_sums_seg and the Chamfer reduction guarantee for theirs.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/slide_train.h"

namespace {

// ---------------------------------------------------------------------------------------------------- max over a sample's rows
// col_sums_seg_kernel's layout (train_ops.hip): a thread owns 4 consecutive channels, cn = ld / 4 threads cover a row, rt = 256 / cn
// rows are in flight; thread row pr scans rows pr, pr + rt, ... in ascending order and keeps the FIRST maximum (strict >), then one
// thread per column merges the rt candidates, ties to the lower row.  One workgroup per sample.
__global__ __launch_bounds__(256) void col_max_seg_kernel(int S, int C, int ld, const float *__restrict__ x, float *__restrict__ out,
                                                          int *__restrict__ arg) {
  __shared__ float rv[256 * 4];
  __shared__ int ri[256 * 4];
  const int cn = ld / 4, rt = 256 / cn;
  const int pr = threadIdx.x / cn, pc = threadIdx.x - pr * cn;
  const int b = blockIdx.x;
  if (pr < rt) {
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int a[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    const float *xs = x + ((size_t)b * (size_t)S) * ld + pc * 4;
    for (int r = pr; r < S; r += rt) {
      const float4 v = *reinterpret_cast<const float4 *>(xs + (size_t)r * ld);
      const float va[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (va[j] > m[j] || a[j] == INT_MAX) {
          m[j] = va[j];
          a[j] = r;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rv[pr * ld + pc * 4 + j] = m[j];
      ri[pr * ld + pc * 4 + j] = a[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < ld; c += 256) {
    float m = rv[c];
    int a = ri[c];  // (thread row 0 always holds row 0: S >= 1)
    for (int r = 1; r < rt; ++r) {
      const float v = rv[r * ld + c];
      const int i = ri[r * ld + c];
      if (i != INT_MAX && (v > m || (v == m && i < a))) {
        m = v;
        a = i;
      }
    }
    const bool valid = c < C;
    out[(size_t)b * ld + c] = valid ? m : 0.f;
    arg[(size_t)b * ld + c] = valid ? a : -1;
  }
}

// dx[(b, s)][c] = dy[b][c] where arg[b][c] == s, else 0: a gather, every element stored once by the thread that owns it
__global__ __launch_bounds__(256) void col_max_seg_bwd_kernel(int S, int ld, const int *__restrict__ arg, const float *__restrict__ dy,
                                                              float *__restrict__ dx, size_t total4) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total4) return;
  const int cn = ld / 4;
  const size_t row = gid / cn;
  const int c0 = (int)(gid - row * cn) * 4;
  const size_t b = row / S;
  const int s = (int)(row - b * S);
  const int4 a = *reinterpret_cast<const int4 *>(arg + b * ld + c0);
  const float4 d = *reinterpret_cast<const float4 *>(dy + b * ld + c0);
  *reinterpret_cast<float4 *>(dx + row * ld + c0) =
      make_float4(a.x == s ? d.x : 0.f, a.y == s ? d.y : 0.f, a.z == s ? d.z : 0.f, a.w == s ? d.w : 0.f);
}

// ---------------------------------------------------------------------------------------------------- diagonal Gaussian posterior
constexpr float LV_MIN = -30.f, LV_MAX = 20.f;

// One workgroup per sample.  Thread t owns the elements e = t, t + 256, ... of the sample's S x ldz output block (row e / ldz,
// column e % ldz; columns >= C are written as zero) and adds its KL terms in that order; the 256 partial sums go through a fixed
// tree: the xor butterfly of a wave (partners 32, 16, 8, 4, 2, 1), then the four wave sums in ascending wave.  (ONE value per lane:
// train_ops.hip's block_sum shape; lane_reduce.h's transposing butterfly pays off for many values per lane.)
__global__ __launch_bounds__(256) void gauss_posterior_fwd_kernel(int S, int C, int ldp, int ldz, const float *__restrict__ params,
                                                                  const float *__restrict__ eps, float *__restrict__ z,
                                                                  float *__restrict__ kl) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const int n = S * ldz;
  const float *ps = params + ((size_t)b * S) * ldp;
  const size_t zo = ((size_t)b * S) * ldz;
  float acc = 0.f;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int s = e / ldz, c = e - s * ldz;
    float zv = 0.f;
    if (c < C) {
      const float mean = ps[(size_t)s * ldp + c];
      const float lv = fminf(fmaxf(ps[(size_t)s * ldp + C + c], LV_MIN), LV_MAX);
      zv = eps ? mean + expf(0.5f * lv) * eps[zo + e] : mean;
      if (kl) acc += mean * mean + expf(lv) - 1.f - lv;
    }
    z[zo + e] = zv;
  }
  if (!kl) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) kl[b] = 0.5f * (((red[0] + red[1]) + red[2]) + red[3]);
}

// dparams [B*S][ldp] in full, everything recomputed from params: one thread per element
__global__ __launch_bounds__(256) void gauss_posterior_bwd_kernel(int S, int C, int ldp, int ldz, const float *__restrict__ params,
                                                                  const float *__restrict__ eps, const float *__restrict__ dz,
                                                                  const float *__restrict__ dkl, float *__restrict__ dparams, size_t total) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const size_t row = gid / ldp;
  const int col = (int)(gid - row * ldp);
  float g = 0.f;
  if (col < 2 * C) {
    const int c = col < C ? col : col - C;
    const float dk = dkl ? dkl[row / S] : 0.f;
    const float dzv = dz ? dz[row * ldz + c] : 0.f;
    if (col < C) {
      g = dzv + dk * params[row * ldp + c];
    } else {
      const float raw = params[row * ldp + col];
      if (raw >= LV_MIN && raw <= LV_MAX) {  // torch.clamp's backward passes the gradient AT both bounds
        const float t1 = eps ? dzv * eps[row * ldz + c] * 0.5f * expf(0.5f * raw) : 0.f;
        g = t1 + dk * 0.5f * (expf(raw) - 1.f);
      }
    }
  }
  dparams[gid] = g;
}

inline bool bad_ld(int ld) { return ld <= 0 || ld % 32 || ld > 1024; }

}  // namespace

extern "C" {

int slide_col_max_seg(int B, int S, int C, int ld, const float *x, float *out, int *arg, slide_stream_t stream) {
  if (bad_ld(ld) || B < 0 || S < 0 || C < 0 || C > ld) return -3;
  if (B == 0) return 0;
  if (S == 0 || !x || !out || !arg) return -3;
  hipLaunchKernelGGL(col_max_seg_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, S, C, ld, x, out, arg);
  return (int)hipGetLastError();
}

int slide_col_max_seg_bwd(int B, int S, int ld, const int *arg, const float *dy, float *dx, slide_stream_t stream) {
  if (bad_ld(ld) || B < 0 || S < 0) return -3;
  if (B == 0) return 0;
  if (S == 0 || !arg || !dy || !dx) return -3;
  const size_t total4 = (size_t)B * S * (ld / 4);
  if ((total4 + 255) / 256 > 0x7fffffffull) return -3;
  hipLaunchKernelGGL(col_max_seg_bwd_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S, ld, arg, dy, dx,
                     total4);
  return (int)hipGetLastError();
}

int slide_gauss_posterior_fwd(int B, int S, int C, int ldp, int ldz, const float *params, const float *eps, float *z, float *kl,
                              slide_stream_t stream) {
  if (bad_ld(ldp) || bad_ld(ldz) || B < 0 || S < 0 || C < 1 || 2 * C > ldp || C > ldz) return -3;
  if (B == 0) return 0;
  if (S == 0 || (long long)S * ldz > INT_MAX || !params || !z) return -3;
  hipLaunchKernelGGL(gauss_posterior_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, S, C, ldp, ldz, params, eps, z, kl);
  return (int)hipGetLastError();
}

int slide_gauss_posterior_bwd(int B, int S, int C, int ldp, int ldz, const float *params, const float *eps, const float *dz,
                              const float *dkl, float *dparams, slide_stream_t stream) {
  if (bad_ld(ldp) || bad_ld(ldz) || B < 0 || S < 0 || C < 1 || 2 * C > ldp || C > ldz) return -3;
  if (B == 0) return 0;
  if (S == 0 || !params || !dparams) return -3;
  const size_t total = (size_t)B * S * ldp;
  if ((total + 255) / 256 > 0x7fffffffull) return -3;
  hipLaunchKernelGGL(gauss_posterior_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S, C, ldp, ldz,
                     params, eps, dz, dkl, dparams, total);
  return (int)hipGetLastError();
}

}  // extern "C"
