// emd_pairwise.hip -- the all-pairs approximate Earth Mover's Distance behind metrics_point_cloud.emd and the EMD keys of
// metrics_point_cloud.generation_metrics (the reference's PyTorchEMD approxmatch + matchcost, forward only).
//
// For one ordered pair, xyz1 (n points) against xyz2 (m points), d(k, l) the squared distance:
//   multiL, multiR = (1, n / m) if n >= m else (m / n, 1);  remainL[k] = multiL, remainR[l] = multiR, cost = 0
//   for level = -4^7, -4^6, ..., -4^-1, 0                                                                     (ten levels)
//     A: ratioL[k] = remainL[k] / (1e-9 + sum_l exp(level d(k,l)) remainR[l])
//     B: sumr[l]   = remainR[l] sum_k exp(level d(k,l)) ratioL[k]
//        ratioR[l] = min(remainR[l] / (sumr[l] + 1e-9), 1) remainR[l];  remainR[l] = max(0, remainR[l] - sumr[l])
//     C: w(k,l) = exp(level d(k,l)) ratioL[k] ratioR[l];  cost += sum_kl d(k,l) w(k,l);  remainL[k] = max(0, remainL[k] - sum_l w(k,l))
// The reference stores w into a (m, n) match matrix per pair (16 MB at 2048 points) and sums d * match in a second kernel.  Here the
// match is never built: ONE 256-thread workgroup owns one ordered pair, keeps the four mass vectors in LDS for all ten levels and
// adds d * w into the cost in sweep C itself.  The three sweeps are one routine: a thread holds OWN points of one cloud in
// registers (8 per thread at 2048 points) and walks the OTHER cloud, staged per tile of 512 points as three coordinate planes
// plus one weight plane (remainR for A, ratioL for B, ratioR for C) and read back four points per step (every lane the same
// address: a broadcast).  exp(level d) is the hardware's base-2 exponential of (level log2 e) d in float, one constant per level;
// d is computed by one recipe whichever cloud is "own", so all three sweeps see the same bits of it.
// The mass vectors, the staged weights and the sums over exp * weight are DOUBLE.  The auction subtracts what it has matched from
// what remained (remainR - sumr, remainL - sum w) and divides by sums that one neighbour dominates: where 1e-5 of a point's mass
// is left, one float rounding of a sum near 1 moves that remainder by 0.5 %, the next level's ratioL follows it, and the cost
// moves by up to 6e-6 (|cost| + S) -- in float the kernel, like a float numpy evaluation, misses the float64 result by that much
// on one pair in a few hundred.  With the exponentials in float and the sums in double it stays within 2e-7.  Clouds with
// p + q > 9600, whose double vectors do not fit 160 KB of LDS, run the same code with float vectors (up to p + q = 19456).
// The cost itself (sum d * exp * ratioR, times ratioL[k] once per tile: ratioL[k] is a factor of a whole row of w) runs in float
// partials per tile, is promoted to double between tiles and finished by one LDS tree: no atomics, and an entry depends on
// nothing but its two clouds (not on m, n, the pair's position, or the paired / matrix form).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_hip.h"
#include "kernel_util.h"
#include "launch.h"

namespace {

constexpr int EM_NT = 256;    // threads per workgroup
constexpr int EM_TILE = 512;  // points of the other cloud per LDS tile: x, y, z planes (float) and one weight plane
constexpr int EM_CH = 4;      // points per step (the tile is padded to a multiple of it with weight-0 points)
constexpr int EM_LEVELS = 10;
constexpr int EM_LDS_MAX = 160 * 1024;

// V = double (the default) or float (clouds whose double vectors do not fit the LDS): the type of the four mass vectors, of the
// staged weight plane and of the sums over exp * weight
template <typename V>
__host__ __device__ constexpr size_t emd_lds_bytes(int p, int q) {
  return sizeof(float) * 3 * (size_t)EM_TILE + sizeof(V) * ((size_t)EM_TILE + 2 * ((size_t)p + q));
}

template <typename V>
struct EmdLds {
  float (*tile)[EM_TILE];   // [x, y, z]
  V *wt;                    // the staged weights
  V *remainL, *ratioL;      // per point of xyz1
  V *remainR, *ratioR;      // per point of xyz2
};

__device__ __forceinline__ float fma_v(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fma_v(double a, double b, double c) { return fma(a, b, c); }

enum { SWEEP_A = 0, SWEEP_B = 1, SWEEP_C = 2 };

// One pass of one sweep: own points o0 + r * 256 + tid (r < KPT) of `own` (no points, stride so) against all of `oth` (nt points,
// stride st) with the weights w (LDS, one per point of oth).  c = level * log2(e).
//   A (own = xyz1, w = remainR): writes ratioL        B (own = xyz2, w = ratioL): writes ratioR, remainR
//   C (own = xyz1, w = ratioR):  adds to cost, writes remainL
// No sweep writes the vector it stages, and a thread writes only its own points' slots; the barrier in front of the next staging
// loop orders those writes before any other thread reads them.
template <typename V, int KPT, int SWEEP>
__device__ __forceinline__ void sweep_pass(const float *__restrict__ own, int o0, int no, int so, const float *__restrict__ oth, int nt,
                                           int st, const V *w, float c, const EmdLds<V> &s, int tid, double &cost) {
  float ax[KPT], ay[KPT], az[KPT], rl[KPT];
  V s0[KPT];
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int i = o0 + r * EM_NT + tid;
    ax[r] = ay[r] = az[r] = 0.f;
    s0[r] = (V)0;
    rl[r] = 0.f;
    if (i < no) {
      const float *a = own + (size_t)i * so;
      ax[r] = a[0]; ay[r] = a[1]; az[r] = a[2];
      if (SWEEP == SWEEP_C) rl[r] = (float)s.ratioL[i];
    }
  }
  for (int t0 = 0; t0 < nt; t0 += EM_TILE) {
    const int tn = min(EM_TILE, nt - t0);
    const int tnp = (tn + EM_CH - 1) / EM_CH * EM_CH;
    __syncthreads();
    for (int p = tid; p < tnp; p += EM_NT) {
      float bx = 0.f, by = 0.f, bz = 0.f;  // padding: weight 0 at a finite distance
      V bw = (V)0;
      if (p < tn) {
        const float *b = oth + (size_t)(t0 + p) * st;
        bx = b[0]; by = b[1]; bz = b[2];
        bw = w[t0 + p];
      }
      s.tile[0][p] = bx; s.tile[1][p] = by; s.tile[2][p] = bz; s.wt[p] = bw;
    }
    __syncthreads();
    float s1[KPT];
#pragma unroll
    for (int r = 0; r < KPT; ++r) s1[r] = 0.f;
    for (int k0 = 0; k0 < tnp; k0 += EM_CH) {
      const float4 bx = *reinterpret_cast<const float4 *>(&s.tile[0][k0]);
      const float4 by = *reinterpret_cast<const float4 *>(&s.tile[1][k0]);
      const float4 bz = *reinterpret_cast<const float4 *>(&s.tile[2][k0]);
      const V w0 = s.wt[k0], w1 = s.wt[k0 + 1], w2 = s.wt[k0 + 2], w3 = s.wt[k0 + 3];
      const float f0 = (float)w0, f1 = (float)w1, f2 = (float)w2, f3 = (float)w3;  // sweep C's cost runs in float
#pragma unroll
      for (int r = 0; r < KPT; ++r) {
#define EM_STEP(u, wv, wf)                                             \
  {                                                                    \
    const float d = sqdist3(ax[r], ay[r], az[r], bx.u, by.u, bz.u);    \
    const float e = __builtin_amdgcn_exp2f(c * d);                     \
    s0[r] = fma_v((V)e, wv, s0[r]);                                    \
    if (SWEEP == SWEEP_C) s1[r] = fmaf(d, e * wf, s1[r]);              \
  }
        EM_STEP(x, w0, f0) EM_STEP(y, w1, f1) EM_STEP(z, w2, f2) EM_STEP(w, w3, f3)
#undef EM_STEP
      }
    }
    if (SWEEP == SWEEP_C) {  // this tile's share of the cost: ratioL[k] is a factor of row k of w
      float part = 0.f;
#pragma unroll
      for (int r = 0; r < KPT; ++r) part = fmaf(rl[r], s1[r], part);
      cost += (double)part;
    }
  }
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int i = o0 + r * EM_NT + tid;
    if (i < no) {
      if (SWEEP == SWEEP_A) {
        s.ratioL[i] = s.remainL[i] / ((V)1e-9 + s0[r]);
      } else if (SWEEP == SWEEP_B) {
        const V rem = s.remainR[i], sumr = rem * s0[r], x = rem / (sumr + (V)1e-9);
        s.ratioR[i] = (x < (V)1 ? x : (V)1) * rem;
        const V left = rem - sumr;
        s.remainR[i] = left > (V)0 ? left : (V)0;
      } else {
        const V left = s.remainL[i] - s.ratioL[i] * s0[r];
        s.remainL[i] = left > (V)0 ? left : (V)0;
      }
    }
  }
}

// One sweep over all own points: passes of 256 * KPT points, KPT the smallest of 1, 2, 4, 8 that covers what remains.
template <typename V, int SWEEP>
__device__ __forceinline__ void sweep(const float *__restrict__ own, int no, int so, const float *__restrict__ oth, int nt, int st,
                                      const V *w, float c, const EmdLds<V> &s, int tid, double &cost) {
  int o0 = 0;
  for (; no - o0 > 4 * EM_NT; o0 += 8 * EM_NT) sweep_pass<V, 8, SWEEP>(own, o0, no, so, oth, nt, st, w, c, s, tid, cost);
  const int left = no - o0;
  if (left > 2 * EM_NT) sweep_pass<V, 4, SWEEP>(own, o0, no, so, oth, nt, st, w, c, s, tid, cost);
  else if (left > EM_NT) sweep_pass<V, 2, SWEEP>(own, o0, no, so, oth, nt, st, w, c, s, tid, cost);
  else if (left > 0) sweep_pass<V, 1, SWEEP>(own, o0, no, so, oth, nt, st, w, c, s, tid, cost);
}

// x (m, p, *) with a point stride of sx floats, y (n, q, *) with sy; out (m, n), or (m) in the paired form.  Matrix form: the
// XCD-aware block map of chamfer_pairwise.hip -- block L runs on XCD L % 8 and takes j = 8 k + L % 8, consecutive blocks of an XCD
// take consecutive i: the workgroups that share y[j] share an L2.  Paired form: block L is pair (L, L).
template <typename V>
__global__ __launch_bounds__(EM_NT) void emd_pairwise_kernel(int m, int n, int p, int q, const float *__restrict__ x, int sx,
                                                             const float *__restrict__ y, int sy, int paired, float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int L = blockIdx.x, tid = threadIdx.x;
  int i, j;
  if (paired) {
    i = j = L;
  } else {
    const int g = L >> 3;
    i = g % m;
    j = (g / m) * 8 + (L & 7);
    if (j >= n) return;
  }
  EmdLds<V> s;
  s.tile = reinterpret_cast<float(*)[EM_TILE]>(lds);
  s.wt = reinterpret_cast<V *>(lds + 3 * EM_TILE);
  s.remainL = s.wt + EM_TILE;
  s.ratioL = s.remainL + p;
  s.remainR = s.ratioL + p;
  s.ratioR = s.remainR + q;
  const float *x1 = x + (size_t)i * p * sx;
  const float *x2 = y + (size_t)j * q * sy;
  const V multiL = p >= q ? (V)1 : (V)(q / p), multiR = p >= q ? (V)(p / q) : (V)1;
  for (int k = tid; k < p; k += EM_NT) s.remainL[k] = multiL;
  for (int l = tid; l < q; l += EM_NT) s.remainR[l] = multiR;
  double cost = 0.0;
  float level = -16384.f;  // -4^7
  for (int it = 0; it < EM_LEVELS; ++it, level *= 0.25f) {
    const float c = it == EM_LEVELS - 1 ? 0.f : level * 1.44269504088896340736f;
    sweep<V, SWEEP_A>(x1, p, sx, x2, q, sy, s.remainR, c, s, tid, cost);
    sweep<V, SWEEP_B>(x2, q, sy, x1, p, sx, s.ratioL, c, s, tid, cost);
    sweep<V, SWEEP_C>(x1, p, sx, x2, q, sy, s.ratioR, c, s, tid, cost);
  }
  __syncthreads();  // the last tile is no longer read: its space holds the tree (256 doubles in the 6 KB of coordinate planes)
  double *red = reinterpret_cast<double *>(lds);
  red[tid] = cost;
  __syncthreads();
  for (int h = EM_NT / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[paired ? (size_t)i : (size_t)i * n + j] = (float)red[0];
}

template <typename V>
int launch_emd(int64_t grid, size_t lds, hipStream_t stream, int m, int n, int p, int q, const float *x, int sx, const float *y, int sy,
               int paired, float *out) {
  allow_dynamic_lds<&emd_pairwise_kernel<V>>(EM_LDS_MAX);
  hipLaunchKernelGGL(emd_pairwise_kernel<V>, dim3((unsigned)grid), dim3(EM_NT), lds, stream, m, n, p, q, x, sx, y, sy, paired, out);
  return LAUNCH_STATUS();
}

}  // namespace

extern "C" {

int slide_emd_pairwise(int m, int n, int p, int q, const float *x, int sx, const float *y, int sy, int paired, float *out,
                       slide_stream_t stream) {
  if (sx < 3 || sy < 3) return -2;
  if (paired && m != n) return -2;
  if (m <= 0 || n <= 0 || p <= 0 || q <= 0) return 0;
  if (emd_lds_bytes<float>(p, q) > (size_t)EM_LDS_MAX) return -2;
  const int64_t grid = paired ? (int64_t)m : (int64_t)8 * ((n + 7) / 8) * m;
  if (grid > 0x7fffffffLL) return -2;
  // double mass vectors while they fit (p + q <= 9600), float beyond
  if (emd_lds_bytes<double>(p, q) <= (size_t)EM_LDS_MAX)
    return launch_emd<double>(grid, emd_lds_bytes<double>(p, q), (hipStream_t)stream, m, n, p, q, x, sx, y, sy, paired ? 1 : 0, out);
  return launch_emd<float>(grid, emd_lds_bytes<float>(p, q), (hipStream_t)stream, m, n, p, q, x, sx, y, sy, paired ? 1 : 0, out);
}

}  // extern "C"
