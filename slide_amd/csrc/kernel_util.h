// kernel_util.h -- what the geometry kernels (point ops, Chamfer / EMD, marching cubes, mesh sampling / components, refine front)
// share: the distance recipe, the XCD-aware block map, the packed-mesh lookup, the workgroup prefix scan and the workgroup
// max / min.  Internal: not part of the C ABI under include/.  Everything here is integer arithmetic or an order-free max / min,
// except sqdist3, whose rounding is pinned below.  Floating-point SUMS are not here: their order is part of each kernel's result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// THE squared distance of two points.  The contract: identical points are at distance 0 exactly, and every search kernel (knn,
// ball query, three_nn, FPS, Chamfer, all-pairs CD / EMD, the engine's PREP_POINTS) and the oracle (oracle/ops_cpu.c) agree bit for
// bit -- neighbour indices, tie order and the Chamfer sums rest on it.  Contraction is off INSIDE the function, so its bits do not
// depend on the flags of the including file; the two fmaf are the only fused steps.  A change here changes all of them together.
// (occupancy_grid.hip evaluates the same expression split across its loops.)
__device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// XCD-aware (batch element, tile) block map of the search kernels, of chamfer_nn_kernel and of its backward.  Every workgroup of a
// batch element streams that element's WHOLE search set; consecutive workgroup ids go to consecutive XCDs (block L runs on XCD
// L % 8 -- relied on for speed only), so with a (tile, b) grid the eight tiles of an element ran on eight XCDs and each private L2
// fetched the set once more (ball_query moved 6.5x its algorithmic bytes at n = 8192).  Here the grid is linear and id L -> XCD
// L % 8 takes the elements b = 8 k + L % 8: all tiles of an element run on ONE XCD and its set is fetched once.
struct SearchBlock { int b, tile; bool valid; };
__device__ __forceinline__ SearchBlock search_block(int nb, int tiles) {
  const int L = blockIdx.x, x = L & 7, q = L >> 3;
  SearchBlock r;
  r.tile = q % tiles;
  r.b = (q / tiles) * 8 + x;
  r.valid = r.b < nb;
  return r;
}
inline unsigned search_grid(int nb, int tiles) { return (unsigned)(8 * ((nb + 7) / 8) * tiles); }

// the mesh of packed row x: the last m with off[m] <= x (off: b + 1 offsets; meshes may be empty: equal offsets)
__device__ __forceinline__ int mesh_of(const long long *__restrict__ off, int b, long long x) {
  int lo = 0, hi = b;  // off[lo] <= x < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// inclusive prefix over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// base + the exclusive prefix of v over the workgroup in thread order (NW waves; base the same in every thread); total = the
// workgroup's sum.  part: NW values of LDS.  A caller that scans in passes hands the running sum in as base and adds total to it.
template <int NW, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T *part, T &total, T base = 0) {
  const T incl = wave_incl_scan(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // (part may still be read by the pass, or the call, before)
  if ((threadIdx.x & 63) == 63) part[w] = incl;
  __syncthreads();
  T before = base, sum = 0;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const T p = part[q];
    before += (q < w) ? p : 0;
    sum += p;
  }
  total = sum;
  return before + incl - v;
}

// Workgroup max / min, for element types whose op gives the same bits in any order (integers; fminf / fmaxf of floats, which drop
// a NaN).  In two halves, so that a caller with several values pays ONE barrier between them:
//   wave_reduce(v, op)         op over the 64 lanes, partners lane ^ 32, 16, ..., 1; every lane holds the result
//   fold_slots<NW>(slots, op)  op over slots[0 .. NW) in index order
// block_reduce is the two around the barrier for one value; slots (NW values of LDS) must not be in use by a call before.
struct MaxOf {
  template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }  // integers
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct MinOf {
  __device__ float operator()(float a, float b) const { return fminf(a, b); }
};

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
  return v;
}

template <int NW, typename T, typename Op>
__device__ __forceinline__ T fold_slots(const T *slots, Op op) {
  T v = slots[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) v = op(v, slots[q]);
  return v;
}

template <int NW, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T *slots, Op op) {
  v = wave_reduce(v, op);
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  return fold_slots<NW>(slots, op);
}

}  // namespace
