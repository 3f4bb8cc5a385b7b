// occupancy_grid.hip -- the occupancy counters behind the JSD generation metric (metrics_point_cloud.generation_metrics:
// entropy_of_occupancy_grid / jsd_between_point_cloud_sets; the reference's pvd/metrics/evaluation_metrics.py, JSD block, where a
// CPU nearest-neighbour query against the grid and two Python loops per cloud do this work).
//
// Every point of S clouds of P points is assigned to its nearest ADMISSIBLE cell of an R^3 lattice; counts[c] is the number of points
// that chose cell c, clouds[c] the number of clouds with at least one such point (the reference's grid_bernoulli_rvars).  The host
// owns the grid: `axis` holds the R float32 cell-centre coordinates of one axis (strictly ascending; cell (i, j, k) sits at
// (axis[i], axis[j], axis[k]), flat index c = (i R + j) R + k) and `rowmask` one 32-bit word per (i, j) row, bit k set when cell
// (i, j, k) is admissible (R <= 32 keeps a row in one word).  The kernel never decides sphere membership.
//
// The nearest rule, in fp32 with contraction off (build.py: -ffp-contract=off; the fmaf calls below are the only fused steps):
//     d32(p, c) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)),  dx = fl(p.x - axis[i]), dy = fl(p.y - axis[j]), dz = fl(p.z - axis[k])
//   (the distance recipe, kernel_util.h sqdist3, split across the loops below: dxx, dxy).
//   1. Lattice step.  Per axis: index 0 when p <= axis[0], R - 1 when p >= axis[R - 1]; else the bracket axis[lo] <= p < axis[lo + 1]
//      is found by bisection and lo + 1 is taken only when |fl(p - axis[lo + 1])| < |fl(p - axis[lo])| (an exact midpoint keeps the
//      lower index).  Every rounding step of d32 is monotone, so the cell (i*, j*, k*) of the three per-axis results attains the
//      minimum of d32 over ALL R^3 cells; of the cells at exactly equal distance from p (p on a bisector plane: up to 8) it is the
//      one with the lowest flat index.  If it is admissible it is the answer.
//   2. Scan step, only for points whose lattice cell is not admissible (near or outside the sphere's surface, un-normalised
//      clouds): the admissible cell with the smallest d32, of several with an equal d32 the lowest flat index.  Rows are visited in
//      flat order with a strict compare; a row (or a whole slab i) whose partial distance already reaches the best so far is skipped
//      (it cannot hold a strictly smaller distance: monotone rounding again), which does not change the result.
//   A point with a non-finite coordinate is not counted; bit 0 of *flag is set (the Python wrapper raises ValueError).  If no cell
//   at all is admissible nothing is counted and bit 1 is set.
//
// Shape: one 256-thread workgroup per cloud, points in tiles of 256.  The cloud's Bernoulli variable is a bitmap of R^3 bits in LDS
// (ds_or), added to `clouds` once per cloud; `counts` takes one no-return integer atomic per point.  Points that need the scan step are
// queued in LDS and scanned 256 at a time (full waves also when only a few points per tile are flagged); axis and rowmask are
// staged in LDS (at most 128 B + 4 KB), the bitmap is at most 4 KB.  All accumulation is integer atomics: exact, independent of the
// order of points and clouds, bit-reproducible.  The outputs are ACCUMULATED into (the caller zero-fills counts, clouds and flag).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_hip.h"
#include "launch.h"

namespace {

constexpr int OG_NT = 256;    // threads per workgroup = points per tile
constexpr int OG_RMAX = 32;   // a row of cells is one 32-bit mask word
constexpr int OG_QCAP = 512;  // scan queue: fewer than 256 left over + at most 256 new per tile

struct OgShared {
  float axis[OG_RMAX];
  uint32_t rowmask[OG_RMAX * OG_RMAX];
  uint32_t bits[OG_RMAX * OG_RMAX * OG_RMAX / 32];  // the cloud's occupancy bitmap
  int queue[OG_QCAP];
  int qn;
};

// step 1 of the nearest rule for one axis
__device__ __forceinline__ int axis_nearest(float p, const float *ax, int R) {
  if (p <= ax[0]) return 0;
  if (p >= ax[R - 1]) return R - 1;
  int lo = 0, hi = R - 1;  // ax[lo] <= p < ax[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ax[mid] <= p) lo = mid; else hi = mid;
  }
  return fabsf(p - ax[hi]) < fabsf(p - ax[lo]) ? hi : lo;
}

// step 2: lexicographic minimum of (d32, flat index) over the admissible cells; -1 when there is none
__device__ __forceinline__ int scan_nearest(float px, float py, float pz, const OgShared &sh, int R) {
  float best = INFINITY;
  int bc = -1;
  for (int i = 0; i < R; ++i) {
    const float dx = px - sh.axis[i];
    const float dxx = dx * dx;
    if (!(dxx < best || bc < 0)) continue;
    for (int j = 0; j < R; ++j) {
      uint32_t w = sh.rowmask[i * R + j];
      const float dy = py - sh.axis[j];
      const float dxy = fmaf(dy, dy, dxx);
      if (w == 0u || !(dxy < best || bc < 0)) continue;
      while (w) {
        const int k = __builtin_ctz(w);
        w &= w - 1u;
        const float dz = pz - sh.axis[k];
        const float d = fmaf(dz, dz, dxy);
        if (d < best || bc < 0) {
          best = d;
          bc = (i * R + j) * R + k;
        }
      }
    }
  }
  return bc;
}

__global__ __launch_bounds__(OG_NT) void occupancy_grid_kernel(int P, const float *__restrict__ pts, int sp, int R,
                                                               const float *__restrict__ axis, const uint32_t *__restrict__ rowmask,
                                                               int *__restrict__ counts, int *__restrict__ clouds,
                                                               int *__restrict__ cells, int *__restrict__ flag) {
  __shared__ OgShared sh;
  const int tid = threadIdx.x;
  const int nwords = (R * R * R + 31) >> 5;
  const float *cloud = pts + (size_t)blockIdx.x * P * sp;
  int *cell_out = cells ? cells + (size_t)blockIdx.x * P : nullptr;
  if (tid < R) sh.axis[tid] = axis[tid];
  for (int r = tid; r < R * R; r += OG_NT) sh.rowmask[r] = rowmask[r];
  for (int w = tid; w < nwords; w += OG_NT) sh.bits[w] = 0u;
  if (tid == 0) sh.qn = 0;
  __syncthreads();

  auto commit = [&](int pt, int c) {
    if (c >= 0) {
      atomicOr(&sh.bits[c >> 5], 1u << (c & 31));
      atomicAdd(&counts[c], 1);
    }
    if (cell_out) cell_out[pt] = c;
  };
  auto scan_batch = [&](int first, int n) {  // queue[first, first + n), n <= 256
    if (tid < n) {
      const int pt = sh.queue[first + tid];
      const float *a = cloud + (size_t)pt * sp;
      const int c = scan_nearest(a[0], a[1], a[2], sh, R);
      if (c < 0) atomicOr(flag, 2);
      commit(pt, c);
    }
  };

  for (int t0 = 0; t0 < P; t0 += OG_NT) {
    const int pt = t0 + tid;
    if (pt < P) {
      const float *a = cloud + (size_t)pt * sp;
      const float px = a[0], py = a[1], pz = a[2];
      if (!(isfinite(px) && isfinite(py) && isfinite(pz))) {
        atomicOr(flag, 1);
        commit(pt, -1);
      } else {
        const int i = axis_nearest(px, sh.axis, R), j = axis_nearest(py, sh.axis, R), k = axis_nearest(pz, sh.axis, R);
        if ((sh.rowmask[i * R + j] >> k) & 1u) commit(pt, (i * R + j) * R + k);
        else sh.queue[atomicAdd(&sh.qn, 1)] = pt;  // < 256 queued before this tile + <= 256 now: within OG_QCAP
      }
    }
    __syncthreads();
    const int qn = sh.qn;
    __syncthreads();    // every thread has read the same qn before the next tile (or the drain below) changes it
    if (qn >= OG_NT) {  // uniform
      scan_batch(qn - OG_NT, OG_NT);
      __syncthreads();
      if (tid == 0) sh.qn = qn - OG_NT;
      __syncthreads();
    }
  }
  scan_batch(0, sh.qn);  // fewer than 256 left
  __syncthreads();
  for (int w = tid; w < nwords; w += OG_NT) {
    uint32_t b = sh.bits[w];
    while (b) {
      const int k = __builtin_ctz(b);
      b &= b - 1u;
      atomicAdd(&clouds[(w << 5) + k], 1);
    }
  }
}

}  // namespace

extern "C" {

int slide_occupancy_grid(int s, int p, const float *pts, int sp, int r, const float *axis, const uint32_t *rowmask, int *counts,
                         int *clouds, int *cells, int *flag, slide_stream_t stream) {
  if (sp < 3 || r < 2 || r > OG_RMAX || s < 0 || p < 0) return -2;
  if ((int64_t)s * p > 0x7fffffffLL) return -2;  // counts are 32-bit
  if (s == 0 || p == 0) return 0;
  if (!pts || !axis || !rowmask || !counts || !clouds || !flag) return -2;
  hipLaunchKernelGGL(occupancy_grid_kernel, dim3((unsigned)s), dim3(OG_NT), 0, (hipStream_t)stream, p, pts, sp, r, axis, rowmask,
                     counts, clouds, cells, flag);
  return LAUNCH_STATUS();
}

}  // extern "C"
