// chamfer_bwd.hip -- gfx950 backward of the fused Chamfer path (chamfer.hip: chamfer_nn_kernel + chamfer_reduce_kernel, feature term
// `mse` or none, no lengths): the gradient of the (B, 2, 5) per-cloud sums with respect to both clouds, one launch.
//
// A point p of direction `dir` with nearest neighbour q (squared distance d, feature term t = sum_c (fp_c - fq_c)^2) feeds
//   sum d, sum sqrt d     ->  v = 2 a (p_xyz - q_xyz),  a = g[dir][0] + g[dir][1] / (2 sqrt d)
//   sum t, sum sqrt t     ->  w = 2 c (fp - fq),        c = g[dir][3] + g[dir][4] / (2 sqrt t)
// with +v, +w for p and -v, -w for q (g = the incoming gradient dred; column 2, the F1 count, has none).  Where d == 0 (t == 0) the
// square root's part is DEFINED as 0 -- the subgradient 0; torch's autograd yields NaN there (0 * inf) -- so the gradients are finite
// for all finite inputs.
//
// The scatter (-v, -w into q) is written as a GATHER so that every output element is stored exactly once, by one thread, in a fixed
// order -- no float atomics, no zero-initialised output, results bit-reproducible and independent of the cloud's position in the
// batch: a workgroup owns BW_TQ target points of one cloud; a thread keeps its targets' rows and gradients in registers, starts each
// gradient with the target's own term and then scans the OTHER direction's index array in ascending source order (staged through
// LDS as int32, broadcast reads of four indices) adding a source's term when its neighbour is the target.  Matches are rare (one per
// target on average), so the source's row and distance are fetched from global memory (L2) only under the match branch; the scan
// itself is two integer compares per (target, source) pair against about ten VALU operations per pair of the forward search.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_train.h"
#include "kernel_util.h"
#include "launch.h"

namespace {

constexpr int BW_NT = 256;              // threads per workgroup
constexpr int BW_TPT = 2;               // targets per thread: one broadcast LDS read feeds 2 x 64 x 4 pairs per wave
constexpr int BW_TQ = BW_NT * BW_TPT;   // targets per workgroup
constexpr int BW_TILE = 1024;           // source indices per LDS tile (4 KB)
constexpr int BW_FMAX = 16;             // most feature channels (register accumulators)

// g0 + g1 / (2 sqrt v), the square root's part 0 where v == 0 (and for a v that is not a positive number)
__device__ __forceinline__ float coef(float g0, float g1, float v) { return g0 + (v > 0.f ? g1 / (2.f * sqrtf(v)) : 0.f); }

template <int FM>
struct Target {
  float p[3 + (FM ? FM : 1)];  // the target's row: xyz, then F features
  float g[3 + (FM ? FM : 1)];  // its gradient
};

// the term of source point s (row srow, squared distance ds to its neighbour -- this target) in the target's gradient: -v, -w
template <int FM>
__device__ __forceinline__ void add_incoming(Target<FM> &t, const float *__restrict__ srow, float ds, const float *__restrict__ gs, int F) {
  const float k = 2.f * coef(gs[0], gs[1], ds);
#pragma unroll
  for (int c = 0; c < 3; ++c) t.g[c] = t.g[c] - k * (srow[c] - t.p[c]);
  if (FM) {
    float e[FM ? FM : 1], tt = 0.f;
#pragma unroll
    for (int c = 0; c < FM; ++c) {
      e[c] = c < F ? srow[3 + c] - t.p[3 + c] : 0.f;
      if (c < F) tt = tt + e[c] * e[c];  // chamfer.hip's feature_term (mse): the source's own features first, channel order
    }
    const float kc = 2.f * coef(gs[3], gs[4], tt);
#pragma unroll
    for (int c = 0; c < FM; ++c) t.g[3 + c] = t.g[3 + c] - kc * e[c];
  }
}

// x (nb, n1, *) rows of sx floats, y (nb, n2, *) rows of sy: xyz then F <= FM features.  (d1, i1) / (d2, i2): chamfer_nn's output for
// (x, y).  dred (nb, 2, 5).  Tiles [0, t1) of a pair write dx (nb, n1, 3 + F) for BW_TQ points of x each, tiles [t1, t1 + t2) dy; a
// NULL output has no tiles.
template <int FM>
__global__ __launch_bounds__(BW_NT) void chamfer_cd_bwd_kernel(int nb, int n1, int n2, int F, const float *__restrict__ x, int sx,
                                                               const float *__restrict__ y, int sy, const float *__restrict__ d1,
                                                               const int64_t *__restrict__ i1, const float *__restrict__ d2,
                                                               const int64_t *__restrict__ i2, const float *__restrict__ dred,
                                                               float *__restrict__ dx, float *__restrict__ dy) {
  __shared__ int4 tile[BW_TILE / 4];
  const int t1 = dx ? (n1 + BW_TQ - 1) / BW_TQ : 0, t2 = dy ? (n2 + BW_TQ - 1) / BW_TQ : 0;
  const SearchBlock tb = search_block(nb, t1 + t2);  // every tile of one cloud pair -- both directions -- on one XCD
  if (!tb.valid) return;
  const int b = tb.b, tid = threadIdx.x;
  const bool rev = tb.tile >= t1;  // the targets are y's points
  const int nt = rev ? n2 : n1, ns = rev ? n1 : n2;
  const int st = rev ? sy : sx, ss = rev ? sx : sy;
  const float *T = (rev ? y : x) + (size_t)b * nt * st;
  const float *S = (rev ? x : y) + (size_t)b * ns * ss;
  const float *dT = (rev ? d2 : d1) + (size_t)b * nt, *dS = (rev ? d1 : d2) + (size_t)b * ns;
  const int64_t *iT = (rev ? i2 : i1) + (size_t)b * nt, *iS = (rev ? i1 : i2) + (size_t)b * ns;
  const float *gT = dred + ((size_t)b * 2 + (rev ? 1 : 0)) * 5, *gS = dred + ((size_t)b * 2 + (rev ? 0 : 1)) * 5;
  float *out = (rev ? dy : dx) + (size_t)b * nt * (3 + F);
  const int q0 = (rev ? tb.tile - t1 : tb.tile) * BW_TQ;

  // own-direction term: the gradient's first summand
  Target<FM> tg[BW_TPT];
  int id[BW_TPT];
#pragma unroll
  for (int r = 0; r < BW_TPT; ++r) {
    const int p = q0 + r * BW_NT + tid;
    id[r] = p < nt ? p : -2;  // (never equal to a staged index: pads are -1)
#pragma unroll
    for (int c = 0; c < 3 + FM; ++c) tg[r].p[c] = tg[r].g[c] = 0.f;
    if (p < nt) {
      const float *a = T + (size_t)p * st;
      int64_t j = iT[p];
      j = j < 0 ? 0 : (j >= ns ? ns - 1 : j);
      const float *q = S + (size_t)j * ss;
      const float k = 2.f * coef(gT[0], gT[1], dT[p]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        tg[r].p[c] = a[c];
        tg[r].g[c] = k * (a[c] - q[c]);
      }
      if (FM) {
        float e[FM ? FM : 1], tt = 0.f;
#pragma unroll
        for (int c = 0; c < FM; ++c) {
          tg[r].p[3 + c] = c < F ? a[3 + c] : 0.f;
          e[c] = c < F ? a[3 + c] - q[3 + c] : 0.f;
          if (c < F) tt = tt + e[c] * e[c];
        }
        const float kc = 2.f * coef(gT[3], gT[4], tt);
#pragma unroll
        for (int c = 0; c < FM; ++c) tg[r].g[3 + c] = kc * e[c];
      }
    }
  }

  // incoming terms, ascending source index
  int *tile_i = reinterpret_cast<int *>(tile);
  for (int t0 = 0; t0 < ns; t0 += BW_TILE) {
    const int tn = min(BW_TILE, ns - t0);
    const int tnp = (tn + 3) & ~3;
    __syncthreads();
    for (int s = tid; s < tnp; s += BW_NT) tile_i[s] = s < tn ? (int)iS[t0 + s] : -1;
    __syncthreads();
    for (int k0 = 0; k0 < tnp; k0 += 4) {
      const int4 j4 = tile[k0 >> 2];
      const int j[4] = {j4.x, j4.y, j4.z, j4.w};
      bool any = false;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < BW_TPT; ++r) any |= j[u] == id[r];
      if (any) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int r = 0; r < BW_TPT; ++r) {
            if (j[u] == id[r]) {
              const int s = t0 + k0 + u;
              add_incoming<FM>(tg[r], S + (size_t)s * ss, dS[s], gS, F);
            }
          }
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < BW_TPT; ++r) {
    const int p = q0 + r * BW_NT + tid;
    if (p < nt) {
      float *o = out + (size_t)p * (3 + F);
#pragma unroll
      for (int c = 0; c < 3 + FM; ++c)
        if (c < 3 + F) o[c] = tg[r].g[c];
    }
  }
}

template <int FM>
int launch_bwd(int b, int n1, int n2, int f, const float *x, int sx, const float *y, int sy, const float *d1, const int64_t *i1,
               const float *d2, const int64_t *i2, const float *dred, float *dx, float *dy, hipStream_t stream) {
  const int tiles = (dx ? (n1 + BW_TQ - 1) / BW_TQ : 0) + (dy ? (n2 + BW_TQ - 1) / BW_TQ : 0);
  hipLaunchKernelGGL(chamfer_cd_bwd_kernel<FM>, dim3(search_grid(b, tiles)), dim3(BW_NT), 0, stream, b, n1, n2, f, x, sx, y, sy, d1, i1,
                     d2, i2, dred, dx, dy);
  return LAUNCH_STATUS();
}

}  // namespace

extern "C" {

int slide_chamfer_cd_bwd(int b, int n1, int n2, int f, const float *x, int sx, const float *y, int sy, const float *d1,
                         const int64_t *i1, const float *d2, const int64_t *i2, const float *dred, float *dx, float *dy,
                         slide_stream_t stream) {
  if (b <= 0 || n1 <= 0 || n2 <= 0) return 0;
  if (f < 0 || f > BW_FMAX || sx < 3 + f || sy < 3 + f) return -2;
  if (!x || !y || !d1 || !i1 || !d2 || !i2 || !dred) return -2;
  if (!dx && !dy) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (f == 0) return launch_bwd<0>(b, n1, n2, f, x, sx, y, sy, d1, i1, d2, i2, dred, dx, dy, s);
  if (f <= 3) return launch_bwd<3>(b, n1, n2, f, x, sx, y, sy, d1, i1, d2, i2, dred, dx, dy, s);
  return launch_bwd<BW_FMAX>(b, n1, n2, f, x, sx, y, sy, d1, i1, d2, i2, dred, dx, dy, s);
}

}  // extern "C"
