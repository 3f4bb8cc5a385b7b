// chamfer_pairwise.hip -- the all-pairs Chamfer matrix behind metrics_point_cloud.generation_metrics (the reference's
// pvd/metrics/evaluation_metrics.py, CD half: MMD-CD / COV-CD / 1-NNA-CD of a generated set against a reference set).
//
// One launch per matrix.  One 256-thread workgroup per pair (i, j) searches BOTH directions and reduces them in place; the only
// global store is the pair's four floats [direction][sum d, sum sqrt d].  Against chamfer.hip's two launches per row block:
//   * no neighbour index: the minimum VALUE does not depend on scan order or tie handling, so the strict-compare + two selects per
//     (query, point) become one v_min_f32 and the distance stays bit-equal to chamfer_nn_kernel's;
//   * no per-point (d, i) round trip through HBM and no second launch: a thread keeps its queries' sums in double registers.  A
//     thread holds queries q0 + tid, q0 + 256 + tid, ... of every query tile and walks a cloud's tiles in order, so it adds its
//     points t, t + 256, ... in index order -- chamfer_reduce_kernel's order -- and the same LDS tree finishes the sum.  Every
//     entry is bit-equal to chamfer_reduce(chamfer_nn(x[i], y[j])) and does not depend on m, n, the pair's position or `symmetric`;
//   * symmetric form (y is x): pairs j < i exit at once; pair (i, j) also stores its mirror out[j, i, d] = out[i, j, 1 - d] (the same
//     two searches seen from the other cloud).  The diagonal is computed like any other pair.
// The shared distance recipe (kernel_util.h sqdist3; the file is built with -ffp-contract=off).  The norm expansion |a|^2 + |b|^2 - 2 a.b (and
// with it any MFMA form) is excluded: it is not bit-equal and cancels badly for near points.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_hip.h"
#include "kernel_util.h"
#include "launch.h"

namespace {

constexpr int PW_NT = 256;     // threads per workgroup (the reduction order depends on it: chamfer_reduce_kernel's RD_NT)
constexpr int PW_TILE = 1024;  // search points per LDS tile, as three coordinate planes (12 KB)
constexpr int PW_CH = 8;       // points per unrolled step (the tile is padded to a multiple of it)

// One query tile of one direction: QPT queries per thread (q0 + r * 256 + tid, r < QPT) of q (nq points, stride sq) against all of
// s (ns points, stride ss); the minimum and its square root are added to the thread's sums in the order of r.  The search set is
// staged through LDS as coordinate PLANES and read back four points per ds_read_b128 (every lane the same address: a broadcast), so
// a step of 8 points costs 6 LDS reads for 8 * QPT * 64 pairs per wave.
template <int QPT>
__device__ __forceinline__ void query_tile(const float *__restrict__ q, int q0, int nq, int sq, const float *__restrict__ s, int ns,
                                           int ss, float (*tile)[PW_TILE], int tid, double &s0, double &s1) {
  float ax[QPT], ay[QPT], az[QPT], best[QPT];
#pragma unroll
  for (int r = 0; r < QPT; ++r) {
    const int i = q0 + r * PW_NT + tid;
    ax[r] = ay[r] = az[r] = 0.f;
    if (i < nq) {
      const float *a = q + (size_t)i * sq;
      ax[r] = a[0]; ay[r] = a[1]; az[r] = a[2];
    }
    best[r] = INFINITY;
  }
  for (int t0 = 0; t0 < ns; t0 += PW_TILE) {
    const int tn = min(PW_TILE, ns - t0);
    const int tnp = (tn + PW_CH - 1) / PW_CH * PW_CH;  // padded with points at "infinity": never closer than a real point
    __syncthreads();
    for (int p = tid; p < tnp; p += PW_NT) {
      float cx = 3e38f, cy = 3e38f, cz = 3e38f;
      if (p < tn) {
        const float *c = s + (size_t)(t0 + p) * ss;
        cx = c[0]; cy = c[1]; cz = c[2];
      }
      tile[0][p] = cx; tile[1][p] = cy; tile[2][p] = cz;
    }
    __syncthreads();
    for (int k0 = 0; k0 < tnp; k0 += PW_CH) {
#pragma unroll
      for (int u = 0; u < PW_CH; u += 4) {
        const float4 cx = *reinterpret_cast<const float4 *>(&tile[0][k0 + u]);
        const float4 cy = *reinterpret_cast<const float4 *>(&tile[1][k0 + u]);
        const float4 cz = *reinterpret_cast<const float4 *>(&tile[2][k0 + u]);
#pragma unroll
        for (int r = 0; r < QPT; ++r) {
          best[r] = fminf(best[r], sqdist3(ax[r], ay[r], az[r], cx.x, cy.x, cz.x));
          best[r] = fminf(best[r], sqdist3(ax[r], ay[r], az[r], cx.y, cy.y, cz.y));
          best[r] = fminf(best[r], sqdist3(ax[r], ay[r], az[r], cx.z, cy.z, cz.z));
          best[r] = fminf(best[r], sqdist3(ax[r], ay[r], az[r], cx.w, cy.w, cz.w));
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < QPT; ++r) {
    if (q0 + r * PW_NT + tid < nq) {
      s0 += (double)best[r];
      s1 += (double)sqrtf(best[r]);
    }
  }
}

// One direction of one pair: the thread's sums over its points t, t + 256, ... in index order.  Tiles of 1024 queries (four per
// thread: half the LDS reads per pair) while more than 512 remain, then one of 512 (two per thread: no idle query slots for a
// small cloud or a short tail).
__device__ __forceinline__ void directed_sums(const float *__restrict__ q, int nq, int sq, const float *__restrict__ s, int ns,
                                              int ss, float (*tile)[PW_TILE], int tid, double &s0, double &s1) {
  s0 = 0.0;
  s1 = 0.0;
  int q0 = 0;
  for (; nq - q0 > 2 * PW_NT; q0 += 4 * PW_NT) query_tile<4>(q, q0, nq, sq, s, ns, ss, tile, tid, s0, s1);
  if (q0 < nq) query_tile<2>(q, q0, nq, sq, s, ns, ss, tile, tid, s0, s1);
}

// x (m, p, *) with a point stride of sx floats, y (n, q, *) with sy; xyz are the first three floats of a point.  out (m, n, 2, 2).
// Block map: the XCD-aware map of the search kernels with the reference cloud j in the place of the batch -- block L runs on XCD
// L % 8 and takes j = 8 k + L % 8, consecutive blocks of an XCD take consecutive i: the workgroups that share y[j] share an L2.
__global__ __launch_bounds__(PW_NT) void chamfer_pairwise_kernel(int m, int n, int p, int q, const float *__restrict__ x, int sx,
                                                                 const float *__restrict__ y, int sy, int symmetric,
                                                                 float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tile[3][PW_TILE];
  __shared__ double red[4][PW_NT];
  const int L = blockIdx.x, g = L >> 3, tid = threadIdx.x;
  const int i = g % m, j = (g / m) * 8 + (L & 7);
  if (j >= n || (symmetric && j < i)) return;
  const float *xi = x + (size_t)i * p * sx;
  const float *yj = y + (size_t)j * q * sy;
  double s[4];
  directed_sums(xi, p, sx, yj, q, sy, tile, tid, s[0], s[1]);
  directed_sums(yj, q, sy, xi, p, sx, tile, tid, s[2], s[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int w = PW_NT / 2; w > 0; w >>= 1) {  // chamfer_reduce_kernel's tree
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + w];
    }
    __syncthreads();
  }
  if (tid < 4) {
    const float v = (float)red[tid][0];
    out[((size_t)i * n + j) * 4 + tid] = v;
    if (symmetric && j != i) out[((size_t)j * n + i) * 4 + (tid ^ 2)] = v;
  }
}

}  // namespace

extern "C" {

int slide_chamfer_pairwise(int m, int n, int p, int q, const float *x, int sx, const float *y, int sy, int symmetric, float *out,
                           slide_stream_t stream) {
  if (sx < 3 || sy < 3) return -2;
  if (symmetric && (m != n || p != q)) return -2;
  if (m <= 0 || n <= 0 || p <= 0 || q <= 0) return 0;
  const int64_t grid = (int64_t)8 * ((n + 7) / 8) * m;
  if (grid > 0x7fffffffLL) return -2;
  hipLaunchKernelGGL(chamfer_pairwise_kernel, dim3((unsigned)grid), dim3(PW_NT), 0, (hipStream_t)stream, m, n, p, q, x, sx, y, sy,
                     symmetric ? 1 : 0, out);
  return LAUNCH_STATUS();
}

}  // extern "C"
