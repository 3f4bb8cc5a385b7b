// mesh_sample.hip -- area-weighted point samples from a batch of triangle meshes (the step behind marching_cubes.hip: the reference
// calls pytorch3d.ops.sample_points_from_meshes once per mesh: pointnet2/dpsr_evaluation.py batch_mc_from_psr).
//
// The batch is PACKED, as marching_cubes returns it: verts (sum V, 3) f32, faces (sum F, 3) int32 with vertex indices LOCAL to the
// mesh, optional vertex normals (sum V, 3) f32, voff / foff (b + 1) int64 = every mesh's first row in verts / faces (voff[b] = sum V,
// foff[b] = sum F).  All arithmetic is fp32 with contraction off (build.py) unless it says double or integer.
//
//   face vector   n_f = (v1 - v0) x (v2 - v0), every component a*b - c*d as two products and one subtraction
//   face area     area_f = 0.5f * sqrtf(n.n),  n.n = (nx*nx + ny*ny) + nz*nz
//   refused face  a vertex index outside [0, V) of its mesh (tested BEFORE it is used: flag |= 1) or a non-finite coordinate of
//                 a referenced vertex (flag |= 2): area_f = 0
//   amax          the largest finite area of the mesh (a maximum: exact, order-free)
//   quantised     q_f = (uint64) floor((double)area_f * 2^32 / (double)amax); 0 for a zero or non-finite area or amax = 0.
//                 q_f <= 2^32
//   cdf           cdf_f = q_0 + ... + q_f within the mesh (INCLUSIVE), uint64: integers, so any scan order gives the same bits;
//                 total = cdf_{F-1} < 2^63 for any int32 face count.  The only bias: faces smaller than amax 2^-32 are never drawn.
//   draw          sample s of mesh m takes four 32-bit words (c0, c1, c2, c3): the explicit `words` (b, S, 4) when given, else ONE
//                 Philox4x32-10 call (ddpm_update.h philox_round) with key (seed_lo, seed_hi) and counter
//                 (s, mesh_id[m], stream_id, 0x13198A2E); mesh_id[m] = m when no ids are given.  A mesh's samples are a function
//                 of (mesh, seed, mesh_id, stream_id, s) alone -- not of the batch, the position or the chunk.
//   face          r = c0 << 32 | c1;  t = mulhi64(r, total) in [0, total);  face = the number of cdf entries <= t (upper bound):
//                 a face with q = 0 is never chosen
//   weights       u = ((float)(c2 >> 8) + 0.5f) * 2^-24, v likewise from c3 (the uniform of philox_normal: fp32, so it lies in
//                 (0, 1] -- the sum rounds to even from 2^23 on);  su = sqrtf(u), w0 = 1 - su, w1 = su * (1 - v), w2 = su * v
//                 (pytorch3d's barycentric weights; all three >= 0)
//   point         p = (w0*v0 + w1*v1) + w2*v2 per coordinate
//   normal        face mode:   n_f / max(|n_f|, FLT_EPSILON), |n_f| = sqrtf(n.n) as above (what pytorch3d returns)
//                 vertex mode: g = (w0*g0 + w1*g1) + w2*g2 of the three vertex normals, then g / max(|g|, FLT_EPSILON)
//   empty mesh    F = 0 or total = 0: points and normals are 0, face_idx is -1 and valid[m] = 0 (else 1)
//
// Launches.   1. mesh_area_kernel   a thread per face of the batch: areas, flag
//             2. mesh_cdf_kernel    ONE workgroup per mesh: the maximum, then quantise + scan in tiles of CDF_TILE faces,
//                                   CDF_ITEMS consecutive faces per thread (a wave spans CDF_WAVE_SPAN)
//             3. mesh_sample_kernel a thread per sample: Philox, binary search of the mesh's cdf, three vertex gathers
// The only atomic is the integer OR into the flag word of a refused face.  Repeated runs are bit-equal.
//
// The search is ceil(log2 F) dependent 8-byte loads on a table that stays in L2 (a 128^3 sphere: up to 0.8 MB per mesh).  Staging
// a coarse level of the table in LDS was NOT built: the search and the gathers' misses together are 0.046 ms of a 32-mesh batch's
// 20480-sample launch (profiles/mesh_sampling.md).
#include "ddpm_update.h"
#include "../../include/slide_hip.h"
#include "kernel_util.h"
#include "launch.h"

namespace {

constexpr int AREA_NT = 256;
constexpr int CDF_NT = 1024;                       // one workgroup per mesh
constexpr int CDF_ITEMS = 4;                       // consecutive faces per thread
constexpr int CDF_WAVE_SPAN = 64 * CDF_ITEMS;      // 256 faces per wave
constexpr int CDF_TILE = CDF_NT * CDF_ITEMS;       // 4096 faces per pass of the workgroup
constexpr int SAMPLE_NT = 256;
constexpr uint32_t MESH_PHILOX_K = 0x13198A2Eu;    // (philox_normal's is 0x85A308D3)
constexpr float MESH_EPS = 1.1920928955078125e-07f;  // FLT_EPSILON

typedef unsigned long long u64;

__device__ __forceinline__ bool finite3(const float *p) {
  return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY;  // (a NaN compares false)
}

// n = (b - a) x (c - a)
__device__ __forceinline__ void face_vector(const float *a, const float *b, const float *c, float (&n)[3]) {
#pragma clang fp contract(off)
  const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  n[0] = e1y * e2z - e1z * e2y;
  n[1] = e1z * e2x - e1x * e2z;
  n[2] = e1x * e2y - e1y * e2x;
}

__device__ __forceinline__ float length3(const float (&n)[3]) {
#pragma clang fp contract(off)
  return sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
}

__global__ __launch_bounds__(AREA_NT) void mesh_area_kernel(int b, long long nf, const float *__restrict__ verts,
                                                            const int *__restrict__ faces, const long long *__restrict__ voff,
                                                            const long long *__restrict__ foff, float *__restrict__ areas,
                                                            int *__restrict__ flag) {
#pragma clang fp contract(off)
  const long long f = (long long)blockIdx.x * AREA_NT + threadIdx.x;
  if (f >= nf) return;
  const int m = mesh_of(foff, b, f);
  const long long v0 = voff[m], nv = voff[m + 1] - v0;
  const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  float area = 0.0f;
  int bad = 0;
  if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
    bad = 1;
  } else {
    const float *a = verts + (v0 + i0) * 3, *bb = verts + (v0 + i1) * 3, *c = verts + (v0 + i2) * 3;
    if (!finite3(a) || !finite3(bb) || !finite3(c)) {
      bad = 2;
    } else {
      float n[3];
      face_vector(a, bb, c, n);
      area = 0.5f * length3(n);
    }
  }
  areas[f] = area;
  if (bad) atomicOr(flag, bad);
}

// q of one area; scale = (double)amax, 0 when the mesh has no positive finite area
__device__ __forceinline__ u64 quantise(float area, double amax) {
  if (!(area > 0.0f) || !(area < INFINITY) || !(amax > 0.0)) return 0;
  return (u64)((double)area * 4294967296.0 / amax);  // (a positive value: the conversion truncates = floor)
}

__global__ __launch_bounds__(CDF_NT) void mesh_cdf_kernel(const long long *__restrict__ foff, const float *__restrict__ areas,
                                                          u64 *__restrict__ cdf) {
  __shared__ u64 part[CDF_NT / 64];
  __shared__ unsigned wmax[CDF_NT / 64];
  const long long f0 = foff[blockIdx.x], nf = foff[blockIdx.x + 1] - f0;
  if (nf <= 0) return;
  const float *ar = areas + f0;
  u64 *out = cdf + f0;

  // 1. the largest finite area.  Areas are >= 0, and non-negative floats order like their bit patterns.
  unsigned mx = 0;
  for (long long x = threadIdx.x; x < nf; x += CDF_NT) {
    const float a = ar[x];
    if (a < INFINITY) mx = max(mx, __float_as_uint(a));
  }
  const double amax = (double)__uint_as_float(block_reduce<CDF_NT / 64>(mx, wmax, MaxOf()));

  // 2. quantise and scan, CDF_TILE faces per pass
  u64 run = 0;
  for (long long base = 0; base < nf; base += CDF_TILE) {
    const long long x0 = base + (long long)threadIdx.x * CDF_ITEMS;
    u64 q[CDF_ITEMS];
    u64 sum = 0;
#pragma unroll
    for (int k = 0; k < CDF_ITEMS; ++k) {
      q[k] = (x0 + k < nf) ? quantise(ar[x0 + k], amax) : 0;
      sum += q[k];
    }
    // kernel_util.h block_excl_scan<CDF_NT / 64>(sum, part, total, run), written out: through the helper (any inlined form of
    // it) the register allocator takes 80 VGPRs for this kernel instead of 66 and the resource table drops from 7 to 6 waves/SIMD
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u64 incl = wave_incl_scan(sum);
    __syncthreads();  // (part is still read by the pass before)
    if (lane == 63) part[w] = incl;
    __syncthreads();
    u64 before = run, total = 0;
#pragma unroll
    for (int k = 0; k < CDF_NT / 64; ++k) {
      const u64 p = part[k];
      before += (k < w) ? p : 0;
      total += p;
    }
    u64 acc = before + incl - sum;
#pragma unroll
    for (int k = 0; k < CDF_ITEMS; ++k) {
      acc += q[k];
      if (x0 + k < nf) out[x0 + k] = acc;
    }
    run += total;
  }
}

template <bool VERTEX_NORMALS>
__global__ __launch_bounds__(SAMPLE_NT) void mesh_sample_kernel(int S, const float *__restrict__ verts, const int *__restrict__ faces,
                                                                const float *__restrict__ vnormals,
                                                                const long long *__restrict__ voff,
                                                                const long long *__restrict__ foff, const u64 *__restrict__ cdf,
                                                                uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_id,
                                                                const int *__restrict__ mesh_ids, const uint32_t *__restrict__ words,
                                                                float *__restrict__ points, float *__restrict__ normals,
                                                                int *__restrict__ face_idx, int *__restrict__ valid) {
#pragma clang fp contract(off)
  const int m = blockIdx.y, s = blockIdx.x * SAMPLE_NT + threadIdx.x;
  if (s >= S) return;
  const long long f0 = foff[m], nf = foff[m + 1] - f0;
  const u64 *c = cdf + f0;
  const u64 total = nf > 0 ? c[nf - 1] : 0;
  const size_t row = (size_t)m * S + s;
  if (s == 0) valid[m] = total ? 1 : 0;
  auto nothing = [&](int face) {
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      points[row * 3 + x] = 0.0f;
      if (normals) normals[row * 3 + x] = 0.0f;
    }
    if (face_idx) face_idx[row] = face;
  };
  if (!total) return nothing(-1);
  uint32_t c0, c1, c2, c3;
  if (words) {
    const uint4 wd = reinterpret_cast<const uint4 *>(words)[row];
    c0 = wd.x; c1 = wd.y; c2 = wd.z; c3 = wd.w;
  } else {
    c0 = (uint32_t)s; c1 = (uint32_t)(mesh_ids ? mesh_ids[m] : m); c2 = stream_id; c3 = MESH_PHILOX_K;
    uint32_t k0 = seed_lo, k1 = seed_hi;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      philox_round(c0, c1, c2, c3, k0, k1);
      k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
  }
  const u64 t = __umul64hi(((u64)c0 << 32) | c1, total);
  // the number of entries <= t; t < total = c[nf - 1], so the answer is at most nf - 1
  long long lo = 0, hi = nf - 1;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (c[mid] <= t) lo = mid + 1;
    else hi = mid;
  }
  const long long f = f0 + lo;
  const long long v0 = voff[m], nv = voff[m + 1] - v0;
  // A chosen face has q > 0, so mesh_area_kernel found its indices in range and its vertices finite -- when cdf was made from these
  // arrays.  The indices are tested again all the same: a table from elsewhere must not turn into a read out of bounds.
  const int j0 = faces[f * 3], j1 = faces[f * 3 + 1], j2 = faces[f * 3 + 2];
  if (j0 < 0 || j0 >= nv || j1 < 0 || j1 >= nv || j2 < 0 || j2 >= nv) return nothing((int)lo);
  const long long i0 = v0 + j0, i1 = v0 + j1, i2 = v0 + j2;
  const float *a = verts + i0 * 3, *b = verts + i1 * 3, *d = verts + i2 * 3;
  const float A[3] = {a[0], a[1], a[2]}, B[3] = {b[0], b[1], b[2]}, D[3] = {d[0], d[1], d[2]};
  const float u = ((float)(c2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float v = ((float)(c3 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float su = sqrtf(u);
  const float w0 = 1.0f - su, w1 = su * (1.0f - v), w2 = su * v;
#pragma unroll
  for (int x = 0; x < 3; ++x) points[row * 3 + x] = (w0 * A[x] + w1 * B[x]) + w2 * D[x];
  if (normals) {
    float n[3];
    if (VERTEX_NORMALS) {
      const float *ga = vnormals + i0 * 3, *gb = vnormals + i1 * 3, *gd = vnormals + i2 * 3;
#pragma unroll
      for (int x = 0; x < 3; ++x) n[x] = (w0 * ga[x] + w1 * gb[x]) + w2 * gd[x];
    } else {
      face_vector(A, B, D, n);
    }
    const float len = fmaxf(length3(n), MESH_EPS);
#pragma unroll
    for (int x = 0; x < 3; ++x) normals[row * 3 + x] = n[x] / len;
  }
  if (face_idx) face_idx[row] = (int)lo;
}

}  // namespace

extern "C" {

int slide_mesh_cdf_span(int level) {
  return level == 0 ? CDF_ITEMS : level == 1 ? CDF_WAVE_SPAN : level == 2 ? CDF_TILE : -2;
}

int slide_mesh_face_cdf(int b, long long nf, const float *verts, const int *faces, const long long *voff, const long long *foff,
                        float *areas, unsigned long long *cdf, int *flag, slide_stream_t stream) {
  if (b < 0 || nf < 0 || nf > 0x7fffffffLL) return -2;
  if (b == 0 || nf == 0) return 0;
  if (!verts || !faces || !voff || !foff || !areas || !cdf || !flag) return -2;
  hipStream_t s = (hipStream_t)stream;
  mesh_area_kernel<<<(unsigned)((nf + AREA_NT - 1) / AREA_NT), AREA_NT, 0, s>>>(b, nf, verts, faces, voff, foff, areas, flag);
  mesh_cdf_kernel<<<(unsigned)b, CDF_NT, 0, s>>>(foff, areas, cdf);
  return LAUNCH_STATUS();
}

int slide_mesh_sample(int b, int s, const float *verts, const int *faces, const float *vnormals, const long long *voff,
                      const long long *foff, const unsigned long long *cdf, int seed_lo, int seed_hi, int stream_id,
                      const int *mesh_ids, const unsigned *words, int vertex_normals, float *points, float *normals, int *face_idx,
                      int *valid, slide_stream_t stream) {
  if (b < 0 || s < 0 || b > 65535) return -2;
  if (b == 0 || s == 0) return 0;
  if (!verts || !faces || !voff || !foff || !cdf || !points || !valid) return -2;
  if (vertex_normals && (!vnormals || !normals)) return -2;
  const dim3 grid((unsigned)((s + SAMPLE_NT - 1) / SAMPLE_NT), (unsigned)b);
  hipStream_t st = (hipStream_t)stream;
  if (vertex_normals)
    mesh_sample_kernel<true><<<grid, SAMPLE_NT, 0, st>>>(s, verts, faces, vnormals, voff, foff, cdf, (uint32_t)seed_lo,
                                                         (uint32_t)seed_hi, (uint32_t)stream_id, mesh_ids, words, points, normals,
                                                         face_idx, valid);
  else
    mesh_sample_kernel<false><<<grid, SAMPLE_NT, 0, st>>>(s, verts, faces, nullptr, voff, foff, cdf, (uint32_t)seed_lo,
                                                          (uint32_t)seed_hi, (uint32_t)stream_id, mesh_ids, words, points, normals,
                                                          face_idx, valid);
  return LAUNCH_STATUS();
}

}  // extern "C"
