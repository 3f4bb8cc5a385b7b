// chamfer.hip -- gfx950 kernels behind metrics_point_cloud.chamfer_and_f1 (the reference's Chamfer / F1 metric module).
//
// Two launches per metric call:
//   chamfer_nn_kernel      nearest neighbour (K = 1) of every valid point of x in y AND of every valid point of y in x, one
//                          launch for both directions.  The shared distance recipe (kernel_util.h sqdist3; -ffp-contract=off), the
//                          search set scanned in index order with a strict `<`: the result is the (distance, index)-lexicographic
//                          minimum, bit-equal to slide_knn_points(K = 1) (ties -> lower index).
//   chamfer_reduce_kernel  per cloud and direction: sum d, sum sqrt d, count d < threshold and, with per-point features, the
//                          reference's normal term (mse / cos) and its square root, summed in a FIXED order (a strided per-thread
//                          pass, then a fixed LDS tree): a pair's numbers do not depend on its batch or its position in it.
//
// Why two directed passes and not one pass that updates row AND column minima: the directed search costs 9 VALU instructions
// per (query, point) pair (6 for the distance, compare + two selects); a single pass saves the second distance (6 of 18 per
// pair in both directions) but has to reduce each column's minimum across the wave (a 64-bit min over six DPP steps per point
// and wave) and merge it across workgroups with 64-bit atomics into a buffer that must be pre-filled -- a second kernel or a
// memset, plus atomics whose traffic grows with P1 / 256 per point.  The directed form needs no atomics and no pre-fill, keeps
// bit-equality with slide_knn_points trivially, and is VALU-bound at a known rate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_hip.h"
#include "kernel_util.h"
#include "launch.h"

namespace {

__device__ __forceinline__ int clamp_len(const int64_t *lengths, int b, int n) {
  if (!lengths) return n;
  const int64_t l = lengths[b];
  return l < 0 ? 0 : (l > n ? n : (int)l);
}

constexpr int NN_NT = 256;              // threads per workgroup
constexpr int NN_QPT = 2;               // queries per thread: one broadcast LDS read feeds 2 x 64 pairs per wave
constexpr int NN_TQ = NN_NT * NN_QPT;   // queries per workgroup
constexpr int NN_TILE = 1024;           // search points per LDS tile (16 KB)
constexpr int NN_CH = 8;                // points per unrolled step (the tile is padded to a multiple of it)

// x (nb, n1, *) with a point stride of sx floats, y (nb, n2, *) with sy; xyz are the first three floats of a point.
// Tiles [0, t1) of a pair search x's points in y (-> d1, i1), tiles [t1, t1 + t2) y's points in x (-> d2, i2).
// Queries keep their coordinates in registers; the search set is staged through LDS as float4.  Slots of a query beyond its
// cloud's length, and every slot when the searched cloud is empty, hold (0, 0).
__global__ __launch_bounds__(NN_NT) void chamfer_nn_kernel(int nb, int n1, int n2, const float *__restrict__ x, int sx,
                                                           const float *__restrict__ y, int sy,
                                                           const int64_t *__restrict__ lx, const int64_t *__restrict__ ly,
                                                           float *__restrict__ d1, int64_t *__restrict__ i1,
                                                           float *__restrict__ d2, int64_t *__restrict__ i2) {
  __shared__ float4 tile[NN_TILE];
  const int t1 = (n1 + NN_TQ - 1) / NN_TQ, t2 = (n2 + NN_TQ - 1) / NN_TQ;
  const SearchBlock sb = search_block(nb, t1 + t2);
  if (!sb.valid) return;
  const int b = sb.b, tid = threadIdx.x;
  const bool rev = sb.tile >= t1;
  const int nq = rev ? n2 : n1, ns = rev ? n1 : n2;
  const int sq = rev ? sy : sx, ss = rev ? sx : sy;
  const float *q = (rev ? y : x) + (size_t)b * nq * sq;
  const float *s = (rev ? x : y) + (size_t)b * ns * ss;
  const int lq = clamp_len(rev ? ly : lx, b, nq), ls = clamp_len(rev ? lx : ly, b, ns);
  float *od = (rev ? d2 : d1) + (size_t)b * nq;
  int64_t *oi = (rev ? i2 : i1) + (size_t)b * nq;
  const int q0 = (rev ? sb.tile - t1 : sb.tile) * NN_TQ;

  float ax[NN_QPT], ay[NN_QPT], az[NN_QPT], best[NN_QPT];
  int bi[NN_QPT];
#pragma unroll
  for (int r = 0; r < NN_QPT; ++r) {
    const int i = q0 + r * NN_NT + tid;
    ax[r] = ay[r] = az[r] = 0.f;
    if (i < lq) {
      const float *a = q + (size_t)i * sq;
      ax[r] = a[0]; ay[r] = a[1]; az[r] = a[2];
    }
    best[r] = INFINITY;
    bi[r] = 0;
  }
  // a workgroup whose queries are all beyond the cloud's length only writes its zeros
  const int nact = min(max(lq - q0, 0), NN_TQ);
  for (int t0 = 0; nact > 0 && t0 < ls; t0 += NN_TILE) {
    const int tn = min(NN_TILE, ls - t0);
    const int tnp = (tn + NN_CH - 1) / NN_CH * NN_CH;  // padded with points at "infinity": never closer than a real point
    __syncthreads();
    for (int p = tid; p < tnp; p += NN_NT) {
      if (p < tn) {
        const float *c = s + (size_t)(t0 + p) * ss;
        tile[p] = make_float4(c[0], c[1], c[2], 0.f);
      } else {
        tile[p] = make_float4(3e38f, 3e38f, 3e38f, 0.f);
      }
    }
    __syncthreads();
    for (int k0 = 0; k0 < tnp; k0 += NN_CH) {
#pragma unroll
      for (int u = 0; u < NN_CH; ++u) {
        const float4 c = tile[k0 + u];
        const int j = t0 + k0 + u;
#pragma unroll
        for (int r = 0; r < NN_QPT; ++r) {
          const float d = sqdist3(ax[r], ay[r], az[r], c.x, c.y, c.z);
          const bool lt = d < best[r];
          best[r] = lt ? d : best[r];
          bi[r] = lt ? j : bi[r];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NN_QPT; ++r) {
    const int i = q0 + r * NN_NT + tid;
    if (i < nq) {
      const bool ok = i < lq && ls > 0;
      od[i] = ok ? best[r] : 0.f;
      oi[i] = ok ? (int64_t)bi[r] : 0;
    }
  }
}

constexpr int RD_NT = 256;
constexpr int RD_OUT = 5;  // per (pair, direction): sum d, sum sqrt d, count d < threshold, sum term, sum sqrt term

// the reference's normal terms between a point's features a and its nearest neighbour's b (F channels each):
//   mode 1 (mse): sum_c (a_c - b_c)^2
//   mode 2 (cos): 1 - |cosine_similarity(a, b, eps = 1e-6)| in torch 2.x's formula: each vector divided by its L2 norm
//                 clamped to at least eps, then the dot product of the two -- bit-equal to torch 2.10's CPU result for F = 3
__device__ __forceinline__ float feature_term(const float *a, const float *b, int F, int mode) {
  if (mode == 1) {
    float t = 0.f;
    for (int c = 0; c < F; ++c) {
      const float e = a[c] - b[c];
      t = t + e * e;
    }
    return t;
  }
  float na = 0.f, nb = 0.f;
  for (int c = 0; c < F; ++c) {  // torch's CPU vector_norm: an fma chain in channel order
    na = fmaf(a[c], a[c], na);
    nb = fmaf(b[c], b[c], nb);
  }
  na = fmaxf(sqrtf(na), 1e-6f);
  nb = fmaxf(sqrtf(nb), 1e-6f);
  float dot = 0.f;
  for (int c = 0; c < F; ++c) dot = dot + (a[c] / na) * (b[c] / nb);
  return 1.f - fabsf(dot);
}

// One workgroup per (pair, direction): block 2 b + dir.  Direction 0 reduces (d1, i1) over x's valid points with features fx
// (own) and fy (of the neighbours), direction 1 (d2, i2) over y's.  Features: row stride sfx / sfy floats, F channels, mode 0 =
// none.  Sums are accumulated in double: each thread its strided points in index order, then a fixed tree over the threads.
__global__ __launch_bounds__(RD_NT) void chamfer_reduce_kernel(int n1, int n2, const float *__restrict__ d1,
                                                               const int64_t *__restrict__ i1, const float *__restrict__ d2,
                                                               const int64_t *__restrict__ i2, const int64_t *__restrict__ lx,
                                                               const int64_t *__restrict__ ly, float threshold, int F, int mode,
                                                               const float *__restrict__ fx, int sfx,
                                                               const float *__restrict__ fy, int sfy,
                                                               float *__restrict__ out) {
  __shared__ double red[RD_OUT - 1][RD_NT];
  __shared__ int redc[RD_NT];
  const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, tid = threadIdx.x;
  const int n = dir ? n2 : n1, no = dir ? n1 : n2;
  const int len = clamp_len(dir ? ly : lx, b, n);
  const float *d = (dir ? d2 : d1) + (size_t)b * n;
  const int64_t *ix = (dir ? i2 : i1) + (size_t)b * n;
  const float *fa = nullptr, *fb = nullptr;
  int sa = 0, so = 0;
  if (mode) {
    sa = dir ? sfy : sfx;
    so = dir ? sfx : sfy;
    fa = (dir ? fy : fx) + (size_t)b * n * sa;
    fb = (dir ? fx : fy) + (size_t)b * no * so;
  }
  double s0 = 0.0, s1 = 0.0, s3 = 0.0, s4 = 0.0;
  int cnt = 0;
  for (int i = tid; i < len; i += RD_NT) {
    const float v = d[i];
    s0 += (double)v;
    s1 += (double)sqrtf(v);
    cnt += v < threshold ? 1 : 0;
    if (mode) {
      int64_t j = ix[i];
      j = j < 0 ? 0 : (j >= no ? no - 1 : j);
      const float t = feature_term(fa + (size_t)i * sa, fb + (size_t)j * so, F, mode);
      s3 += (double)t;
      s4 += (double)sqrtf(t);
    }
  }
  red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s3; red[3][tid] = s4;
  redc[tid] = cnt;
  __syncthreads();
  for (int w = RD_NT / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < RD_OUT - 1; ++k) red[k][tid] += red[k][tid + w];
      redc[tid] += redc[tid + w];
    }
    __syncthreads();
  }
  if (tid < RD_OUT) {
    float *o = out + (size_t)blockIdx.x * RD_OUT;
    o[tid] = tid == 2 ? (float)redc[0] : (float)red[tid < 2 ? tid : tid - 1][0];
  }
}

}  // namespace

extern "C" {

int slide_chamfer_nn(int b, int n1, int n2, const float *x, int sx, const float *y, int sy, const int64_t *x_lengths,
                     const int64_t *y_lengths, float *d1, int64_t *i1, float *d2, int64_t *i2, slide_stream_t stream) {
  if (b <= 0 || n1 <= 0 || n2 <= 0) return 0;
  if (sx < 3 || sy < 3) return -2;
  const int tiles = (n1 + NN_TQ - 1) / NN_TQ + (n2 + NN_TQ - 1) / NN_TQ;
  hipLaunchKernelGGL(chamfer_nn_kernel, dim3(search_grid(b, tiles)), dim3(NN_NT), 0, (hipStream_t)stream, b, n1, n2, x, sx, y,
                     sy, x_lengths, y_lengths, d1, i1, d2, i2);
  return LAUNCH_STATUS();
}

int slide_chamfer_reduce(int b, int n1, int n2, const float *d1, const int64_t *i1, const float *d2, const int64_t *i2,
                         const int64_t *x_lengths, const int64_t *y_lengths, float threshold, int F, int mode,
                         const float *fx, int sfx, const float *fy, int sfy, float *out, slide_stream_t stream) {
  if (b <= 0 || n1 <= 0 || n2 <= 0) return 0;
  if (mode < 0 || mode > 2) return -2;
  if (mode && (F <= 0 || !fx || !fy || !i1 || !i2 || sfx < F || sfy < F)) return -2;
  hipLaunchKernelGGL(chamfer_reduce_kernel, dim3((unsigned)(2 * b)), dim3(RD_NT), 0, (hipStream_t)stream, n1, n2, d1, i1, d2, i2,
                     x_lengths, y_lengths, threshold, F, mode, fx, sfx, fy, sfy, out);
  return LAUNCH_STATUS();
}

}  // extern "C"
