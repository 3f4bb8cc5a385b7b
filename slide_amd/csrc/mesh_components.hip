// mesh_components.hip -- connected components of a batch of triangle meshes, per-component counts, selection (largest / all above a
// size) and an order-preserving compaction: the mesh clean-up behind marching_cubes.hip (the reference's verts_on_largest_mesh calls
// igl connected_components and trimesh split on the host, one mesh at a time: pointnet2/dpsr_utils/utils.py:352-375).
//
// The batch is PACKED as in mesh_sample.hip: faces (sum F, 3) int32 with vertex indices LOCAL to the mesh, voff / foff (b + 1) int64.
// Everything is integer arithmetic; vertex coordinates are only copied.  The definition (graph, root, cid, counts, selection,
// compaction, refusal) is written out in include/slide_hip.h Part 8.
//
// Labelling.  L[v] = v, then ROUNDS of two launches until a round lowers no label:
//   hook   a thread per face: m = min of the three labels and of THEIR labels; integer atomicMin of m into the three vertices and into
//          the three labels' rows (only where m is below the value read: the value read is an upper bound of the row's value)
//   jump   a thread per vertex: L[v] = L[L[.. L[v]]], at most JUMP_HOPS steps.  L[v] is stored by thread v alone.
// Why no in-launch visibility is needed: labels only decrease, are vertex indices of the same component, and are bounded below by
// the component's root.  A plain load that returns another workgroup's older value (another CU's L1 line, another XCD's L2) returns an
// older UPPER bound; using it costs progress, not correctness.  A round in which no thread lowered anything performed no store, so all
// its loads were fresh; then every face has three equal labels and L[L[v]] = L[v], so L is constant on a component, and as L[root] =
// root that constant is the root.  The fixed point is unique: the result does not depend on order, batch or position.
// Cap: launch boundaries order memory, so by induction a vertex at graph distance d from its root holds the root after round d; the
// caller passes max_rounds = (largest V) + 1, which always suffices, and gets -5 beyond it.
// `state` = {refusal flag, last round that lowered a label}; one atomicMax per workgroup that lowered something (and only when the
// word does not hold the round yet).  The host reads both words once per `group` rounds.
//
// Counts: cnt_v[root]++, cnt_f[root of the face's first index]++ with int32 atomic adds, aggregated over the lanes of a wave that
// share a root (a mesh's big component would otherwise take every lane's add on one address).
// Per mesh, ONE workgroup of SCAN_NT threads, in passes of SCAN_TILE elements (SCAN_ITEMS consecutive ones per thread, then
// kernel_util.h block_excl_scan, as mesh_cdf_kernel): rank of the roots (cid), C, counts by cid; selection by a maximum over the key
// (size << 32 | 2^31 - 1 - root); exclusive scans of the vertex and face keep flags.  Nothing assumes that V fits in LDS.
// Compaction: one launch over vertices and faces.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/slide_hip.h"
#include "kernel_util.h"
#include "launch.h"

namespace {

constexpr int CC_NT = 256;                          // per-face / per-vertex launches
constexpr int JUMP_HOPS = 8;
constexpr int SCAN_NT = 1024;                       // one workgroup per mesh
constexpr int SCAN_ITEMS = 4;                       // consecutive elements per thread
constexpr int SCAN_WAVE_SPAN = 64 * SCAN_ITEMS;     // 256 per wave
constexpr int SCAN_TILE = SCAN_NT * SCAN_ITEMS;     // 4096 per pass
constexpr int ST_ROUND_CAP = -5;

typedef unsigned long long u64;

__device__ __forceinline__ bool in_range(int i, long long nv) { return i >= 0 && i < nv; }

__global__ __launch_bounds__(CC_NT) void cc_init_kernel(int b, long long nv, const long long *__restrict__ voff, int *__restrict__ L,
                                                        int *__restrict__ state) {
  const long long x = (long long)blockIdx.x * CC_NT + threadIdx.x;
  if (x == 0) state[0] = state[1] = 0;
  if (x >= nv) return;
  L[x] = (int)(x - voff[mesh_of(voff, b, x)]);
}

// the workgroup's threads that lowered a label report the round, once
__device__ __forceinline__ void report_round(bool lowered, int *state, int round) {
  if (__syncthreads_or(lowered) && threadIdx.x == 0 && __hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != round)
    atomicMax(&state[1], round);
}

__global__ __launch_bounds__(CC_NT) void cc_hook_kernel(int b, long long nf, const int *__restrict__ faces,
                                                        const long long *__restrict__ voff, const long long *__restrict__ foff, int *L,
                                                        int *state, int round) {
  const long long f = (long long)blockIdx.x * CC_NT + threadIdx.x;
  bool lowered = false;
  if (f < nf) {
    const int m = mesh_of(foff, b, f);
    const long long v0 = voff[m], nv = voff[m + 1] - v0;
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (!in_range(i0, nv) || !in_range(i1, nv) || !in_range(i2, nv)) {
      atomicOr(&state[0], 1);  // refused before any index is used; the face joins nothing
    } else {
      int *l = L + v0;
      // labels are vertex indices of this mesh: in [0, nv) by construction (cc_init_kernel, minima of such values)
      const int a0 = l[i0], a1 = l[i1], a2 = l[i2];
      const int g0 = l[a0], g1 = l[a1], g2 = l[a2];
      const int mn = min(min(min(a0, a1), a2), min(min(g0, g1), g2));
      if (mn < a0) { atomicMin(&l[i0], mn); lowered = true; }
      if (mn < a1) { atomicMin(&l[i1], mn); lowered = true; }
      if (mn < a2) { atomicMin(&l[i2], mn); lowered = true; }
      if (mn < g0) { atomicMin(&l[a0], mn); lowered = true; }
      if (mn < g1) { atomicMin(&l[a1], mn); lowered = true; }
      if (mn < g2) { atomicMin(&l[a2], mn); lowered = true; }
    }
  }
  report_round(lowered, state, round);
}

__global__ __launch_bounds__(CC_NT) void cc_jump_kernel(int b, long long nv, const long long *__restrict__ voff, int *L, int *state,
                                                        int round) {
  const long long x = (long long)blockIdx.x * CC_NT + threadIdx.x;
  bool lowered = false;
  if (x < nv) {
    const long long v0 = voff[mesh_of(voff, b, x)];
    const int *l = L + v0;
    const int first = L[x];
    int p = first;
#pragma unroll 1
    for (int k = 0; k < JUMP_HOPS; ++k) {
      const int q = l[p];  // (q <= p: a label never exceeds its row's index)
      if (q == p) break;
      p = q;
    }
    if (p < first) {
      L[x] = p;  // row x has no other writer in this launch
      lowered = true;
    }
  }
  report_round(lowered, state, round);
}

// cnt[key] += (the number of lanes of the wave that hold `key`), one add per distinct key; key < 0: the lane has nothing to add
__device__ __forceinline__ void wave_count(int *__restrict__ cnt, long long key) {
  const int lane = threadIdx.x & 63;
  u64 left = __ballot(key >= 0);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const long long k = __shfl(key, leader, 64);
    const u64 same = __ballot(key == k) & left;
    if (lane == leader) atomicAdd(&cnt[k], (int)__popcll(same));
    left &= ~same;
  }
}

// a thread per vertex, then a thread per face
__global__ __launch_bounds__(CC_NT) void cc_count_kernel(int b, long long nv, long long nf, const int *__restrict__ faces,
                                                         const long long *__restrict__ voff, const long long *__restrict__ foff,
                                                         const int *__restrict__ L, int *__restrict__ cnt_v, int *__restrict__ cnt_f) {
  const long long x = (long long)blockIdx.x * CC_NT + threadIdx.x;  // (nv is padded to whole workgroups by the launch: a wave is all vertices or all faces)
  const long long nvp = (nv + CC_NT - 1) / CC_NT * CC_NT;
  if (x < nvp) {
    long long key = -1;
    if (x < nv) key = voff[mesh_of(voff, b, x)] + L[x];
    wave_count(cnt_v, key);
  } else {
    const long long f = x - nvp;
    long long key = -1;
    if (f < nf) {
      const int m = mesh_of(foff, b, f);
      const long long v0 = voff[m], n = voff[m + 1] - v0;
      const int i0 = faces[f * 3];
      if (in_range(i0, n)) key = v0 + L[v0 + i0];
    }
    wave_count(cnt_f, key);
  }
}

__global__ __launch_bounds__(SCAN_NT) void cc_rank_kernel(const long long *__restrict__ voff, const int *__restrict__ L,
                                                          const int *__restrict__ cnt_v, const int *__restrict__ cnt_f, int *rank,
                                                          int *__restrict__ cid, int *__restrict__ nverts, int *__restrict__ nfaces,
                                                          int *__restrict__ totals) {
  __shared__ int part[SCAN_NT / 64];
  const int m = blockIdx.x;
  const long long v0 = voff[m], nv = voff[m + 1] - v0;
  const int *l = L + v0;
  int run = 0;
  for (long long base = 0; base < nv; base += SCAN_TILE) {
    const long long x0 = base + (long long)threadIdx.x * SCAN_ITEMS;
    bool root[SCAN_ITEMS];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      root[k] = (x0 + k < nv) && l[x0 + k] == x0 + k;
      sum += root[k];
    }
    int total;  // c: the number of flagged elements of the mesh in front of this thread's SCAN_ITEMS
    int c = block_excl_scan<SCAN_NT / 64>(sum, part, total, run);
    run += total;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
      if (root[k]) {
        rank[v0 + x0 + k] = c;
        nverts[v0 + c] = cnt_v[v0 + x0 + k];
        nfaces[v0 + c] = cnt_f[v0 + x0 + k];
        ++c;
      }
  }
  if (threadIdx.x == 0) totals[m * 4 + 2] = run;
  __syncthreads();  // the workgroup's own stores to rank, read below by its other threads
  for (long long v = threadIdx.x; v < nv; v += SCAN_NT) cid[v0 + v] = rank[v0 + l[v]];
}

__global__ __launch_bounds__(SCAN_NT) void cc_select_kernel(const int *__restrict__ faces, const long long *__restrict__ voff,
                                                            const long long *__restrict__ foff, const int *__restrict__ L,
                                                            const int *__restrict__ cnt_v, const int *__restrict__ cnt_f, int by,
                                                            long long min_size, int keep_all, int *vnew, int *__restrict__ fnew,
                                                            int *__restrict__ totals) {
  __shared__ int part[SCAN_NT / 64];
  __shared__ u64 wbest[SCAN_NT / 64];
  const int m = blockIdx.x;
  const long long v0 = voff[m], nv = voff[m + 1] - v0, f0 = foff[m], nf = foff[m + 1] - f0;
  const int *l = L + v0;
  // a component is a candidate when it has a face and its size reaches min_size
  auto candidate_size = [&](int r) -> long long {
    const int nfc = cnt_f[v0 + r];
    const long long size = by ? nfc : cnt_v[v0 + r];
    return (nfc >= 1 && size >= min_size) ? size : -1;
  };
  // 1. the largest candidate, ties to the lowest root (= the lowest cid)
  int best_root = -1;
  if (!keep_all) {
    u64 best = 0;
    for (long long v = threadIdx.x; v < nv; v += SCAN_NT)
      if (l[v] == v) {
        const long long size = candidate_size((int)v);
        if (size >= 1) best = max(best, ((u64)size << 32) | (u64)(0x7fffffff - (int)v));
      }
    best = block_reduce<SCAN_NT / 64>(best, wbest, MaxOf());
    if (best) best_root = 0x7fffffff - (int)(best & 0xffffffffu);
  }
  // 2. kept vertices
  int run = 0;
  for (long long base = 0; base < nv; base += SCAN_TILE) {
    const long long x0 = base + (long long)threadIdx.x * SCAN_ITEMS;
    bool keep[SCAN_ITEMS];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      keep[k] = false;
      if (x0 + k < nv) {
        const int r = l[x0 + k];
        keep[k] = keep_all ? candidate_size(r) >= 0 : r == best_root;
      }
      sum += keep[k];
    }
    int total;  // c: the number of flagged elements of the mesh in front of this thread's SCAN_ITEMS
    int c = block_excl_scan<SCAN_NT / 64>(sum, part, total, run);
    run += total;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
      if (x0 + k < nv) vnew[v0 + x0 + k] = keep[k] ? c++ : -1;
  }
  const int kept_v = run;
  __syncthreads();  // the workgroup's own stores to vnew, read below by its other threads
  // 3. kept faces: those whose first vertex is kept
  run = 0;
  for (long long base = 0; base < nf; base += SCAN_TILE) {
    const long long x0 = base + (long long)threadIdx.x * SCAN_ITEMS;
    bool keep[SCAN_ITEMS];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      keep[k] = false;
      if (x0 + k < nf) {
        const int i0 = faces[(f0 + x0 + k) * 3];
        keep[k] = in_range(i0, nv) && vnew[v0 + i0] >= 0;
      }
      sum += keep[k];
    }
    int total;  // c: the number of flagged elements of the mesh in front of this thread's SCAN_ITEMS
    int c = block_excl_scan<SCAN_NT / 64>(sum, part, total, run);
    run += total;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
      if (x0 + k < nf) fnew[f0 + x0 + k] = keep[k] ? c++ : -1;
  }
  if (threadIdx.x == 0) {
    totals[m * 4 + 0] = kept_v;
    totals[m * 4 + 1] = run;
    totals[m * 4 + 3] = best_root;
  }
}

// a thread per vertex, then a thread per face; rows are copied as 32-bit words (a NaN keeps its bits)
__global__ __launch_bounds__(CC_NT) void cc_compact_kernel(int b, long long nv, long long nf, const uint32_t *__restrict__ verts,
                                                           const uint32_t *__restrict__ normals, const int *__restrict__ faces,
                                                           const long long *__restrict__ voff, const long long *__restrict__ foff,
                                                           const int *__restrict__ vnew, const int *__restrict__ fnew,
                                                           const long long *__restrict__ ovoff, const long long *__restrict__ ofoff,
                                                           uint32_t *__restrict__ out_verts, uint32_t *__restrict__ out_normals,
                                                           int *__restrict__ out_faces, int *__restrict__ vert_idx) {
  const long long x = (long long)blockIdx.x * CC_NT + threadIdx.x;
  if (x < nv) {
    const int j = vnew[x];
    if (j < 0) return;
    const int m = mesh_of(voff, b, x);
    const long long o = ovoff[m] + j;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      out_verts[o * 3 + k] = verts[x * 3 + k];
      if (normals) out_normals[o * 3 + k] = normals[x * 3 + k];
    }
    vert_idx[o] = (int)(x - voff[m]);
  } else if (x - nv < nf) {
    const long long f = x - nv;
    const int j = fnew[f];
    if (j < 0) return;
    const int m = mesh_of(foff, b, f);
    const long long v0 = voff[m], n = voff[m + 1] - v0, o = ofoff[m] + j;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int i = faces[f * 3 + k];
      out_faces[o * 3 + k] = in_range(i, n) ? vnew[v0 + i] : -1;  // (a kept face of labelled meshes has all three in range and kept)
    }
  }
}

bool counts_ok(int b, long long nv, long long nf) {
  return b >= 0 && b <= 65535 && nv >= 0 && nf >= 0 && nv <= 0x7fffffffLL && nf <= 0x7fffffffLL;
}

unsigned blocks(long long n) { return (unsigned)((n + CC_NT - 1) / CC_NT); }

}  // namespace

extern "C" {

int slide_mesh_cc_span(int level) { return level == 0 ? CC_NT : level == 1 ? SCAN_WAVE_SPAN : level == 2 ? SCAN_TILE : -2; }

int slide_mesh_cc_label(int b, long long nv, long long nf, const int *faces, const long long *voff, const long long *foff, int *labels,
                        int *state, int group, int max_rounds, int *info, slide_stream_t stream) {
  if (!counts_ok(b, nv, nf) || group < 1 || max_rounds < 1) return -2;
  if (info) info[0] = info[1] = info[2] = info[3] = 0;
  if (b == 0 || nv == 0) return 0;
  if (!voff || !foff || !labels || !state || !info || (nf > 0 && !faces)) return -2;
  hipStream_t s = (hipStream_t)stream;
  cc_init_kernel<<<blocks(nv), CC_NT, 0, s>>>(b, nv, voff, labels, state);
  if (nf == 0) return LAUNCH_STATUS();  // every vertex is its own component
  int round = 0, reads = 0;
  for (;;) {
    if (round >= max_rounds) {
      info[2] = reads;
      info[3] = round;
      return ST_ROUND_CAP;
    }
    const int n = group < max_rounds - round ? group : max_rounds - round;
    for (int k = 0; k < n; ++k) {
      ++round;
      cc_hook_kernel<<<blocks(nf), CC_NT, 0, s>>>(b, nf, faces, voff, foff, labels, state, round);
      cc_jump_kernel<<<blocks(nv), CC_NT, 0, s>>>(b, nv, voff, labels, state, round);
    }
    int st = LAUNCH_STATUS();
    if (st) return st;
    int host[2] = {0, 0};
    st = (int)hipMemcpyAsync(host, state, sizeof(host), hipMemcpyDeviceToHost, s);
    if (!st) st = (int)hipStreamSynchronize(s);
    if (st) return st;
    ++reads;
    info[0] = host[0];
    info[1] = host[1];
    info[2] = reads;
    info[3] = round;
    if (host[0] || host[1] < round) return 0;  // refused, or the last round lowered nothing: the fixed point
  }
}

int slide_mesh_cc_stats(int b, long long nv, long long nf, const int *faces, const long long *voff, const long long *foff,
                        const int *labels, int *cnt_v, int *cnt_f, int *rank, int *cid, int *nverts, int *nfaces, int *totals,
                        slide_stream_t stream) {
  if (!counts_ok(b, nv, nf)) return -2;
  if (b == 0 || nv == 0) return 0;
  if (!voff || !foff || !labels || !cnt_v || !cnt_f || !rank || !cid || !nverts || !nfaces || !totals || (nf > 0 && !faces)) return -2;
  hipStream_t s = (hipStream_t)stream;
  int st = (int)hipMemsetAsync(cnt_v, 0, (size_t)nv * sizeof(int), s);
  if (!st) st = (int)hipMemsetAsync(cnt_f, 0, (size_t)nv * sizeof(int), s);
  if (st) return st;
  cc_count_kernel<<<blocks(nv) + blocks(nf), CC_NT, 0, s>>>(b, nv, nf, faces, voff, foff, labels, cnt_v, cnt_f);
  cc_rank_kernel<<<(unsigned)b, SCAN_NT, 0, s>>>(voff, labels, cnt_v, cnt_f, rank, cid, nverts, nfaces, totals);
  return LAUNCH_STATUS();
}

int slide_mesh_cc_select(int b, long long nv, long long nf, const int *faces, const long long *voff, const long long *foff,
                         const int *labels, const int *cnt_v, const int *cnt_f, int by, long long min_size, int keep_all, int *vnew,
                         int *fnew, int *totals, slide_stream_t stream) {
  if (!counts_ok(b, nv, nf) || by < 0 || by > 1) return -2;
  if (b == 0 || nv == 0) return 0;
  if (!voff || !foff || !labels || !cnt_v || !cnt_f || !vnew || !totals || (nf > 0 && (!faces || !fnew))) return -2;
  cc_select_kernel<<<(unsigned)b, SCAN_NT, 0, (hipStream_t)stream>>>(faces, voff, foff, labels, cnt_v, cnt_f, by, min_size, keep_all,
                                                                     vnew, fnew, totals);
  return LAUNCH_STATUS();
}

int slide_mesh_cc_compact(int b, long long nv, long long nf, const float *verts, const float *normals, const int *faces,
                          const long long *voff, const long long *foff, const int *vnew, const int *fnew, const long long *ovoff,
                          const long long *ofoff, float *out_verts, float *out_normals, int *out_faces, int *vert_idx,
                          slide_stream_t stream) {
  if (!counts_ok(b, nv, nf)) return -2;
  if (b == 0 || nv == 0) return 0;
  if (!verts || !voff || !foff || !vnew || !ovoff || !ofoff || !out_verts || !vert_idx) return -2;
  if ((normals != nullptr) != (out_normals != nullptr)) return -2;
  if (nf > 0 && (!faces || !fnew || !out_faces)) return -2;
  cc_compact_kernel<<<blocks(nv + nf), CC_NT, 0, (hipStream_t)stream>>>(
      b, nv, nf, reinterpret_cast<const uint32_t *>(verts), reinterpret_cast<const uint32_t *>(normals), faces, voff, foff, vnew, fnew,
      ovoff, ofoff, reinterpret_cast<uint32_t *>(out_verts), reinterpret_cast<uint32_t *>(out_normals), out_faces, vert_idx);
  return LAUNCH_STATUS();
}

}  // extern "C"
