// marching_cubes.hip -- indexed triangle meshes from a batch of scalar grids (the step behind dpsr.hip: the reference calls
// skimage.measure.marching_cubes on the host, once per grid: pointnet2/dpsr_utils/utils.py mc_from_psr).
//
// phi (b,r,r,r) f32, flat index (i r + j) r + k, 2 <= r <= 256.  A grid point is INSIDE iff phi < level (a NaN is outside).
//
//   vertices  one per grid edge whose two ends differ in that predicate, owned by the edge's lower-index end p:
//                 t = (level - a) / (b - a)      a = phi[p], b = phi[p + e_axis], fp32, contraction off (build.py)
//                 vertex = p + t e_axis          in grid-index units
//   normals   g(q) = central difference of phi at grid point q, one-sided on the border (numpy.gradient's rule):
//                 g_d(q) = (phi[q + e_d] - phi[q - e_d]) * 0.5   inside,   phi[q + e_d] - phi[q]  or  phi[q] - phi[q - e_d]  on the border
//                 g = g(p) + t (g(p + e_axis) - g(p));   normal = -g / |g|  (down the gradient, skimage's convention);  |g| = 0 -> 0
//   faces     every cell emits the triangles of its 8-bit case from marching_cubes_table.h (tools/gen_mc_table.py derives it and
//             states the numbering); (v1 - v0) x (v2 - v0) points toward increasing phi
//
// A BRICK is BI x BJ x BK grid points, one 512-thread workgroup, one thread per point: the thread owns the three edges that leave
// its point in the positive directions and the cell whose lowest corner its point is.  The brick's samples and a halo (one point
// below, two above: the far end of an edge needs its own central difference) are staged in LDS, with indices clamped to the grid,
// which is what turns the central difference into the one-sided one on the border.
//
//   1. count   per brick: owned vertices, triangles                                       mc_brick_kernel<COUNT>
//   2. scan    per grid, ONE workgroup: exclusive prefix of the brick counts in brick order, in place; totals      mc_scan_kernel
//   3. bases   one workgroup: exclusive prefix of the grids' totals = each grid's first row in the outputs         mc_bases_kernel
//   4. verts   the bricks that own a vertex, again; vertex id = brick offset + in-workgroup prefix in thread order, axis order
//              within a thread; writes vertices, normals and, per grid point of the brick, (id of its first owned vertex |
//              crossed-axis mask << 28)                                                    mc_brick_kernel<VERTS>
//   5. faces   the bricks that own a triangle, again; triangle row = brick offset + in-workgroup prefix; vertex ids from the
//              volume of pass 4                                                            mc_brick_kernel<FACES>
//
// No atomics at all: every id is a fixed-order prefix, so the output order is a function of the grid alone, a grid's mesh is
// bit-identical at any batch size and position (ids are local to the grid), and repeated runs are bit-equal.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_hip.h"
#include "kernel_util.h"
#include "launch.h"
#include "marching_cubes_table.h"

namespace {

constexpr int BI = 4, BJ = 8, BK = 16;            // brick, in grid points (k is the contiguous axis)
constexpr int NTB = BI * BJ * BK;                 // 512 threads
constexpr int TI = BI + 3, TJ = BJ + 3, TK = BK + 3;  // staged tile: brick origin - 1 ... brick end + 1
constexpr int NWAVE = NTB / 64;
constexpr int SCAN_NT = 1024;
constexpr int MC_RMAX = 256;
constexpr unsigned ID_MASK = 0x0fffffffu;         // 3 * 256^3 < 2^28
static_assert(MC_MAX_TRIS * NTB < 65536 && 3 * NTB < 65536, "the packed in-workgroup prefix holds 16 bits per count");

enum { COUNT = 0, VERTS = 1, FACES = 2 };

struct Dims {
  int r, nbi, nbj, nbk;  // grid size, bricks per axis
};

inline Dims dims_of(int r) { return Dims{r, (r + BI - 1) / BI, (r + BJ - 1) / BJ, (r + BK - 1) / BK}; }

template <int MODE>
__global__ __launch_bounds__(NTB) void mc_brick_kernel(Dims d, int nbricks, const float *__restrict__ phi, float level,
                                                       int *__restrict__ counts, const long long *__restrict__ totals,
                                                       float *__restrict__ verts, float *__restrict__ normals,
                                                       int *__restrict__ faces, unsigned *__restrict__ ids) {
  __shared__ float tile[TI * TJ * TK];
  __shared__ int part[NWAVE];
  const int r = d.r;
  const int g = blockIdx.x / nbricks, brick = blockIdx.x % nbricks;
  const int oi = (brick / (d.nbj * d.nbk)) * BI, oj = ((brick / d.nbk) % d.nbj) * BJ, ok = (brick % d.nbk) * BK;
  int *cnt = counts + ((size_t)g * nbricks + brick) * 2;
  if (MODE != COUNT) {
    // A brick that owns no vertex (no triangle) has nothing to write and leaves before it stages anything: most bricks of a grid.
    // Its points' words of the id volume stay unwritten and are never read -- the face pass reads the word of a crossed edge's
    // lower end only, and the brick of that point owns the edge's vertex.
    const int which = MODE == FACES ? 1 : 0;
    const int next = brick + 1 < nbricks ? cnt[2 + which] : (int)totals[g * 4 + which];
    if (next == cnt[which]) return;
  }
  const size_t r3 = (size_t)r * r * r;
  const float *pg = phi + (size_t)g * r3;
  for (int x = threadIdx.x; x < TI * TJ * TK; x += NTB) {
    const int tk = x % TK, tj = (x / TK) % TJ, ti = x / (TK * TJ);
    const int gi = min(max(oi - 1 + ti, 0), r - 1), gj = min(max(oj - 1 + tj, 0), r - 1), gk = min(max(ok - 1 + tk, 0), r - 1);
    tile[x] = pg[((size_t)gi * r + gj) * r + gk];
  }
  __syncthreads();

  const int lk = threadIdx.x % BK, lj = (threadIdx.x / BK) % BJ, li = threadIdx.x / (BK * BJ);
  const int gi = oi + li, gj = oj + lj, gk = ok + lk;
  const int t0 = ((li + 1) * TJ + (lj + 1)) * TK + (lk + 1);  // this thread's point in the tile
  constexpr int STEP[3] = {TJ * TK, TK, 1};
  const bool in_grid = gi < r && gj < r && gk < r;
  const bool in0 = tile[t0] < level;
  const int gc[3] = {gi, gj, gk};
  unsigned mask = 0;  // bit a: the edge from this point along axis a exists and is crossed
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (in_grid && gc[a] < r - 1 && ((tile[t0 + STEP[a]] < level) != in0)) mask |= 1u << a;
  const int nv = __popc(mask);
  int cs = 0, nt = 0;
  if (MODE != VERTS && gi < r - 1 && gj < r - 1 && gk < r - 1) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      cs |= (tile[t0 + ((c >> 2) & 1) * STEP[0] + ((c >> 1) & 1) * STEP[1] + (c & 1) * STEP[2]] < level) ? (1 << c) : 0;
    nt = MC_NTRI[cs];
  }
  int total;
  const int before = block_excl_scan<NWAVE>(nv | (nt << 16), part, total);

  if (MODE == COUNT) {
    if (threadIdx.x == 0) {
      cnt[0] = total & 0xffff;
      cnt[1] = total >> 16;
    }
  } else if (MODE == VERTS) {
    if (!in_grid) return;
    const unsigned first = (unsigned)(cnt[0] + (before & 0xffff));  // local to the grid
    ids[(size_t)g * r3 + ((size_t)gi * r + gj) * r + gk] = first | (mask << 28);
    if (!mask) return;
    const long long row0 = totals[g * 4 + 2] + first;
    const float a0 = tile[t0];
    // central differences of a tile point; the tile's clamped loads make them one-sided on the border
    auto grad = [&](int t, const int (&q)[3], float (&out)[3]) {
#pragma unroll
      for (int x = 0; x < 3; ++x)
        out[x] = (tile[t + STEP[x]] - tile[t - STEP[x]]) * ((q[x] > 0 && q[x] < r - 1) ? 0.5f : 1.0f);
    };
    float g0[3];
    grad(t0, gc, g0);
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(mask & (1u << a))) continue;
      const float b0 = tile[t0 + STEP[a]];
      const float t = (level - a0) / (b0 - a0);
      int q[3] = {gi, gj, gk};
      q[a] += 1;
      float g1[3], n[3];
      grad(t0 + STEP[a], q, g1);
#pragma unroll
      for (int x = 0; x < 3; ++x) n[x] = g0[x] + t * (g1[x] - g0[x]);
      const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      float *v = verts + (row0 + k) * 3, *nn = normals + (row0 + k) * 3;
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        v[x] = (float)gc[x] + (x == a ? t : 0.0f);
        nn[x] = len > 0.0f ? -n[x] / len : 0.0f;
      }
      ++k;
    }
  } else {
    if (!nt) return;
    const long long row0 = totals[g * 4 + 3] + cnt[1] + (before >> 16);
    const unsigned *idg = ids + (size_t)g * r3;
    for (int t = 0; t < nt; ++t) {
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const int e = MC_TRI[cs][t * 3 + x];
        const int c = MC_EDGE_CORNER[e], a = e >> 2;
        const unsigned w = idg[((size_t)(gi + ((c >> 2) & 1)) * r + (gj + ((c >> 1) & 1))) * r + (gk + (c & 1))];
        faces[(row0 + t) * 3 + x] = (int)((w & ID_MASK) + __popc((w >> 28) & ((1u << a) - 1u)));
      }
    }
  }
}

// one workgroup per grid: the brick counts (nbricks,2) become their exclusive prefix in brick order; totals[g] = (V, F, ., .)
__global__ __launch_bounds__(SCAN_NT) void mc_scan_kernel(int nbricks, int *__restrict__ counts, long long *__restrict__ totals) {
  __shared__ int part[SCAN_NT / 64];
  int *cnt = counts + (size_t)blockIdx.x * nbricks * 2;
  int run_v = 0, run_t = 0;
  for (int base = 0; base < nbricks; base += SCAN_NT) {
    const int x = base + threadIdx.x;
    const int v = x < nbricks ? cnt[x * 2] : 0, t = x < nbricks ? cnt[x * 2 + 1] : 0;
    int tot_v, tot_t;
    const int ev = block_excl_scan<SCAN_NT / 64>(v, part, tot_v);
    const int et = block_excl_scan<SCAN_NT / 64>(t, part, tot_t);
    if (x < nbricks) {
      cnt[x * 2] = run_v + ev;
      cnt[x * 2 + 1] = run_t + et;
    }
    run_v += tot_v;
    run_t += tot_t;
  }
  if (threadIdx.x == 0) {
    totals[blockIdx.x * 4 + 0] = run_v;
    totals[blockIdx.x * 4 + 1] = run_t;
  }
}

// one workgroup: totals[g][2], [3] = the sums of V and F over the grids before g.  Every thread sums a run of grids, thread 0
// chains the 256 runs, every thread writes its run.
__global__ __launch_bounds__(256) void mc_bases_kernel(int b, long long *__restrict__ totals) {
  __shared__ long long sv[256], sf[256];
  const int per = (b + 255) / 256;
  const int lo = min(threadIdx.x * per, b), hi = min(lo + per, b);
  long long v = 0, f = 0;
  for (int g = lo; g < hi; ++g) {
    v += totals[g * 4 + 0];
    f += totals[g * 4 + 1];
  }
  sv[threadIdx.x] = v;
  sf[threadIdx.x] = f;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long av = 0, af = 0;
    for (int q = 0; q < 256; ++q) {
      const long long cv = sv[q], cf = sf[q];
      sv[q] = av;
      sf[q] = af;
      av += cv;
      af += cf;
    }
  }
  __syncthreads();
  v = sv[threadIdx.x];
  f = sf[threadIdx.x];
  for (int g = lo; g < hi; ++g) {
    totals[g * 4 + 2] = v;
    totals[g * 4 + 3] = f;
    v += totals[g * 4 + 0];
    f += totals[g * 4 + 1];
  }
}

// 1 ok, 0 nothing to do, -2 bad arguments
int mc_args(int b, int r, bool null_ptr, long long *nblk, int *nbricks) {
  if (r < 2 || r > MC_RMAX || b < 0) return -2;
  if (b == 0) return 0;
  if (null_ptr) return -2;
  const Dims d = dims_of(r);
  *nbricks = d.nbi * d.nbj * d.nbk;
  *nblk = (long long)b * *nbricks;
  return (*nblk <= 0x7fffffffLL) ? 1 : -2;
}

}  // namespace

extern "C" {

int slide_mc_bricks(int r) {
  if (r < 2 || r > MC_RMAX) return -2;
  const Dims d = dims_of(r);
  return d.nbi * d.nbj * d.nbk;
}

int slide_mc_count(int b, int r, const float *phi, float level, int *counts_ws, long long *totals, slide_stream_t stream) {
  long long nblk = 0;
  int nbricks = 0;
  const int st = mc_args(b, r, !phi || !counts_ws || !totals, &nblk, &nbricks);
  if (st != 1) return st;
  hipStream_t s = (hipStream_t)stream;
  mc_brick_kernel<COUNT><<<(unsigned)nblk, NTB, 0, s>>>(dims_of(r), nbricks, phi, level, counts_ws, nullptr, nullptr, nullptr,
                                                        nullptr, nullptr);
  mc_scan_kernel<<<(unsigned)b, SCAN_NT, 0, s>>>(nbricks, counts_ws, totals);
  mc_bases_kernel<<<1, 256, 0, s>>>(b, totals);
  return LAUNCH_STATUS();
}

int slide_mc_emit(int b, int r, const float *phi, float level, const int *counts_ws, const long long *totals, float *verts,
                  float *normals, int *faces, int *ws, slide_stream_t stream) {
  long long nblk = 0;
  int nbricks = 0;
  const int st = mc_args(b, r, !phi || !counts_ws || !totals || !verts || !normals || !faces || !ws, &nblk, &nbricks);
  if (st != 1) return st;
  hipStream_t s = (hipStream_t)stream;
  int *cnt = const_cast<int *>(counts_ws);  // (read only in these two modes)
  mc_brick_kernel<VERTS><<<(unsigned)nblk, NTB, 0, s>>>(dims_of(r), nbricks, phi, level, cnt, totals, verts, normals, nullptr,
                                                        (unsigned *)ws);
  mc_brick_kernel<FACES><<<(unsigned)nblk, NTB, 0, s>>>(dims_of(r), nbricks, phi, level, cnt, totals, nullptr, nullptr, faces,
                                                        (unsigned *)ws);
  return LAUNCH_STATUS();
}

}  // extern "C"
