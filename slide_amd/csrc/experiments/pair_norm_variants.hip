// pair_norm_variants.hip -- the fp16 forms of the pair-table pass as a launch of its own (SLIDE_OP_PAIR_NORM): opt-in variants
// that lost their A/B against the pass fused into the per-point GEMM (SLIDE_OP_PAIR_FIRST), experiments build only.
// pair_norm.hip hands them every SLIDE_OP_PAIR_NORM that is not the float version 2.
#include "gemm_common.h"
#include "launch.h"
#include "pair_norm.h"

namespace {

// ------------------------------------------------------------------------------------------------ pair-table normalisation
// One workgroup per (sample, 256-channel chunk), one channel per thread: the thread builds its channel's a[0..15] and
// b[0..15] in registers / LDS, walks the sample's pairs for the statistics of its 32-channel block's mode, and writes the
// fp16 tables the generated-X GEMMs and the PAIR residual read.  Cost: 16 K pair evaluations per channel and sample.
template <bool FP>
__global__ __launch_bounds__(256) void pair_norm_kernel(int ld, const float *__restrict__ y, const float *__restrict__ xyz,
                                                        const float *__restrict__ wa, const float *__restrict__ wb,
                                                        const SlideEpi *__restrict__ epi, _Float16 *__restrict__ ta,
                                                        _Float16 *__restrict__ tb, const int *__restrict__ nbr,
                                                        const float *__restrict__ d2t, const float *__restrict__ wt,
                                                        const float *__restrict__ vv_in, float *__restrict__ vv_out) {
  __shared__ float sx[48];
  __shared__ int sq[16 * 8];
  __shared__ float sd[16 * 8], sw[16 * 8];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int c = blockIdx.x * 256 + tid;
  if (tid < 48) sx[tid] = xyz[(size_t)b * 48 + tid];
  if (FP && tid < 128) {
    const int slot = (b * 16 + (tid >> 3)) * 16 + (tid & 7);
    sq[tid] = nbr[slot]; sd[tid] = d2t[slot]; sw[tid] = wt[slot];
  }
  __syncthreads();
  if (c >= ld) return;  // (whole waves: ld is a multiple of 32 and group sizes divide 32)
  const SlideEpi e = epi[c >> 5];
  const int cl = c & 31;
  float av[16], bv[16];
  const float4 ca = *reinterpret_cast<const float4 *>(wa + (size_t)c * 4), cb = *reinterpret_cast<const float4 *>(wb + (size_t)c * 4);
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    const float x0 = sx[p * 3], x1 = sx[p * 3 + 1], x2 = sx[p * 3 + 2];
    av[p] = y[((size_t)b * 16 + p) * ld + c] + (ca.x * x0 + ca.y * x1 + ca.z * x2);
    bv[p] = cb.x * x0 + cb.y * x1 + cb.z * x2;
  }
  float vd = 0.f, vw = 0.f;
  if (FP) { vd = vv_in[c]; vw = vv_in[ld + c]; }
  float g = 1.f, sh = 0.f;
  if (e.mode != SLIDE_EPI_RAW) {
    const bool pre_relu = (e.flags & SLIDE_F_PRE_RELU) != 0;
    float s = 0.f, ss = 0.f;
    if (!FP) {
#pragma unroll
      for (int p = 0; p < 16; ++p)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float v = av[q] + bv[p];
          if (pre_relu) v = fmaxf(v, 0.f);
          s += v; ss = fmaf(v, v, ss);
        }
    } else {
      __shared__ float sa[16][257];
#pragma unroll
      for (int p = 0; p < 16; ++p) sa[p][tid] = av[p];  // (a thread reads back only its own column: no barrier needed)
#pragma unroll
      for (int p = 0; p < 16; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int sl = p * 8 + j;
          float v = sa[sq[sl]][tid] + bv[p] + sd[sl] * vd + sw[sl] * vw;
          if (pre_relu) v = fmaxf(v, 0.f);
          s += v; ss = fmaf(v, v, ss);
        }
    }
    if (e.mode == SLIDE_EPI_STATS) {
      e.stats_sum[(size_t)b * e.stats_bs + cl] = s * e.stats_scale;
      e.stats_sq[(size_t)b * e.stats_bs + cl] = ss * e.stats_scale;
    } else {  // NORM: groups of e.gs physical channels (a power of two <= 32: lanes of one wave)
      for (int m = 1; m < e.gs; m <<= 1) {
        s += __shfl_xor(s, m, 64);
        ss += __shfl_xor(ss, m, 64);
      }
      const float mean = s * e.inv_count;
      const float var = fmaxf(ss * e.inv_count - mean * mean, 0.f);
      g = e.gamma[cl] * __builtin_amdgcn_rsqf(var + GN_EPS);
      sh = e.beta[cl] - mean * g;
      if (cl >= e.n_norm) { g = 1.f; sh = 0.f; }  // MyGroupNorm leaves the last C % G channels as they are
    }
  }
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    ta[((size_t)b * 16 + p) * ld + c] = (_Float16)(av[p] * g + sh);
    tb[((size_t)b * 16 + p) * ld + c] = (_Float16)(bv[p] * g);
  }
  if (FP) {
    vv_out[(size_t)b * 2 * ld + c] = vd * g;
    vv_out[(size_t)b * 2 * ld + ld + c] = vw * g;
  }
}

}  // namespace

// SLIDE_OP_PAIR_NORM with fp16 tables: the two-launch form of the pair-table pass (SLIDE_PAIR_FUSED=0) and its
// one-workgroup-per-sample version (SLIDE_PAIR_NORM_V2=1); the default plans run SLIDE_OP_PAIR_FIRST (gemm_ring.hip)
int slide_launch_pair_norm_variants(const SlideOp &o, hipStream_t s) {
  const int B = o.i[0], ld = o.i[1], K = o.i[2];
  if (B <= 0 || ld <= 0 || ld % 32) return -3;
  const SlideGnFin *fin = (const SlideGnFin *)o.p[12];
  if (o.i[3] == 2) {  // version 2: one workgroup per sample, joint [query | key] GroupNorm finalised here (p[12], may be NULL)
    if (ld > 2048) return -3;
    // passes of equal size: every thread handles ceil(ld / nthr) channels (1056 channels: 2 x 544, not 1024 + 32)
    const int npass = (ld + 1023) / 1024, nthr = ((ld + npass - 1) / npass + 63) / 64 * 64;
    const dim3 grid(B), blk(nthr < 1024 ? nthr : 1024);
    if (K == 16)
      hipLaunchKernelGGL(pair_norm2_kernel<false>, grid, blk, 0, s, ld, (const float *)o.p[0], (const float *)o.p[1],
                         (const float *)o.p[2], (const float *)o.p[3], (const SlideEpi *)o.p[4], (_Float16 *)o.p[5],
                         (_Float16 *)o.p[6], (const int *)nullptr, (const float *)nullptr, (const float *)nullptr,
                         (const float *)nullptr, (float *)nullptr, fin);
    else if (K == 8) {
      if (!o.p[7] || !o.p[8] || !o.p[9] || !o.p[10] || !o.p[11]) return -3;
      allow_dynamic_lds<&pair_norm2_kernel<true>>(16 * 1025 * 4);
      hipLaunchKernelGGL(pair_norm2_kernel<true>, grid, blk, (size_t)16 * 1025 * 4, s, ld, (const float *)o.p[0],
                         (const float *)o.p[1], (const float *)o.p[2], (const float *)o.p[3], (const SlideEpi *)o.p[4],
                         (_Float16 *)o.p[5], (_Float16 *)o.p[6], (const int *)o.p[7], (const float *)o.p[8],
                         (const float *)o.p[9], (const float *)o.p[10], (float *)o.p[11], fin);
    } else return -5;
    return (int)hipGetLastError();
  }
  const dim3 grid((ld + 255) / 256, B), blk(256);
  if (K == 16)
    hipLaunchKernelGGL(pair_norm_kernel<false>, grid, blk, 0, s, ld, (const float *)o.p[0], (const float *)o.p[1],
                       (const float *)o.p[2], (const float *)o.p[3], (const SlideEpi *)o.p[4], (_Float16 *)o.p[5],
                       (_Float16 *)o.p[6], (const int *)nullptr, (const float *)nullptr, (const float *)nullptr,
                       (const float *)nullptr, (float *)nullptr);
  else if (K == 8) {
    if (!o.p[7] || !o.p[8] || !o.p[9] || !o.p[10] || !o.p[11]) return -3;
    hipLaunchKernelGGL(pair_norm_kernel<true>, grid, blk, 0, s, ld, (const float *)o.p[0], (const float *)o.p[1],
                       (const float *)o.p[2], (const float *)o.p[3], (const SlideEpi *)o.p[4], (_Float16 *)o.p[5],
                       (_Float16 *)o.p[6], (const int *)o.p[7], (const float *)o.p[8], (const float *)o.p[9],
                       (const float *)o.p[10], (float *)o.p[11]);
  } else return -5;
  return (int)hipGetLastError();
}
