// dpsr.hip -- differentiable Poisson surface reconstruction, the forward: oriented points -> the Poisson indicator grid (the
// backward is dpsr_bwd.hip)
// (pointnet2/dpsr_utils/dpsr.py: DPSR.forward; the reference's pointnet2/dpsr_utils/dpsr.py + utils.py, where torch index
// arithmetic, scatter_add_, torch.fft.rfftn / irfftn and fancy-index gathers do this work).
//
//   1. rasterize   every point adds w_c * value to the 8 corners of its cell                      point_rasterize_kernel
//   2. r2c         3-D real FFT, half spectrum (k3 <= r/2)                                         fft_r2c_axis3 + 2 x fft_strided
//   3. solve       Phi = sum_d(-i omega_d G S_d) / (-|omega|^2 + 1e-6), bin (0,0,0) = 0            dpsr_spectral_kernel
//   4. c2r         inverse c2c on axes 1, 2 of the half spectrum, Hermitian extension + c2c axis 3 2 x fft_strided + fft_c2r_axis3
//   5. interp      trilinear gather of phi at the points, fixed-order per-sample mean              grid_interp_kernel, dpsr_coef_kernel
//   6. finish      phi = -(phi - offset) / |phi[0,0,0] - offset| * 0.5                             dpsr_finish_kernel
//
// Cell arithmetic (steps 1 and 5), in float with contraction off (build.py: -ffp-contract=off), the reference's own expressions:
//     cs = 1.0f / r;  q = p / cs;  ind0 = floor(q);  ind1 = fmod(ceil(q), r)   (periodic wrap of the last cell)
//     corner positions ind0 * cs and (ind0 + 1) * cs (NOT ind1 * cs);  weight = prod_axes |p - opposite corner| / cs
//   corner c = 4 b0 + 2 b1 + b2 takes ind1 / the position ind0 * cs as its opposite on the axes whose bit is set.  A point on a
//   lattice plane has ind0 == ind1: both corners are the same cell, with weights 1 and 0.
//
// The rasterizer accumulates in 64-bit fixed point: llrint(fl(w * v) * 2^32) added with integer atomics.  Integer addition is exact
// and order-independent: the grid is bit-reproducible and a sample's grid does not depend on its batch (the argument of
// occupancy_grid.hip).  |w * v| < 2^20 keeps a contribution below 2^52; the quantum is 2^-32 (2.3e-10) per contribution.  A
// non-finite coordinate or value, a coordinate outside [0, 1) and |v| >= 2^20 set bit 0 of *flag; the point is left out.
//
// The line FFT is a radix-2 Stockham autosort in LDS (two buffers, log2 r passes), a tile of T lines per 256-thread workgroup,
// r in {16, 32, 64, 128, 256}.  Twiddles: a table of r/2 complex floats, each rounded once from double sincospi.  The passes along
// axes 1 and 2 take tiles of ADJACENT lines, so global accesses stay contiguous along axis 3.  The first forward pass reads the
// fixed-point grid (times 2^-32) or a float grid and writes k3 <= r/2; the last inverse pass extends every axis-3 line
//     full[0] = Re Y[0], full[r/2] = Re Y[r/2], full[k] = Y[k], full[r - k] = conj Y[k]
// (what a c2r transform does: the imaginary parts of bins 0 and r/2 are dropped per line), transforms and writes the real part
// times 1 / r^3 (a power of two: exact).  This is numpy's / torch's irfftn; a full c2c with fftfreq on all axes is NOT.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_hip.h"
#include "dpsr_cell.h"  // NT, the fixed-point scale, cell_of, log2_fft, blocks_ok / blocks_of

namespace {

constexpr int FFT_TILE = 2048;                       // complex elements of one LDS buffer
constexpr int FFT_RMAX = 256;

// ------------------------------------------------------------------------------------------------------------ rasterize
template <int NF>
__global__ __launch_bounds__(NT) void point_rasterize_kernel(long long total, int n, int r, const float *__restrict__ pts,
                                                             const float *__restrict__ vals, long long *__restrict__ grid,
                                                             int *__restrict__ flag) {
  const long long g = (long long)blockIdx.x * NT + threadIdx.x;
  if (g >= total) return;
  const long long s = g / n;
  const float *p = pts + g * 3;
  float v[NF];
  bool ok = true;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    v[f] = vals[g * NF + f];
    ok = ok && (fabsf(v[f]) < VAL_MAX);  // (NaN and inf fail)
  }
  int idx[8];
  float w[8];
  ok = cell_of(p[0], p[1], p[2], r, idx, w) && ok;
  if (!ok) {
    atomicOr(flag, 1);
    return;
  }
  const long long r3 = (long long)r * r * r;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    unsigned long long *comp = (unsigned long long *)(grid + (s * NF + f) * r3);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const long long q = llrint((double)(w[c] * v[f]) * FIX_ONE);
      if (q != 0) atomicAdd(comp + idx[c], (unsigned long long)q);
    }
  }
}

__global__ __launch_bounds__(NT) void fixed_to_float_kernel(long long total, const long long *__restrict__ in, float *__restrict__ out) {
  const long long g = (long long)blockIdx.x * NT + threadIdx.x;
  if (g < total) out[g] = (float)in[g] * FIX_INV;
}

// ------------------------------------------------------------------------------------------------------------ interp
__global__ __launch_bounds__(NT) void grid_interp_kernel(long long total, int n, int C, int r, const float *__restrict__ grid,
                                                         const float *__restrict__ pts, float *__restrict__ out, int *__restrict__ flag) {
  const long long g = (long long)blockIdx.x * NT + threadIdx.x;
  if (g >= total) return;
  const long long s = g / n;
  const float *p = pts + g * 3;
  int idx[8];
  float w[8];
  if (!cell_of(p[0], p[1], p[2], r, idx, w)) {
    atomicOr(flag, 1);
    for (int ch = 0; ch < C; ++ch) out[g * C + ch] = 0.0f;
    return;
  }
  const float *base = grid + s * ((long long)r * r * r) * C;
  for (int ch = 0; ch < C; ++ch) {
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) acc = acc + base[(long long)idx[c] * C + ch] * w[c];
    out[g * C + ch] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------------ line FFT
__device__ __forceinline__ void twiddle_table(float2 *tw, int r) {
  for (int m = threadIdx.x; m < (r >> 1); m += NT) {
    double s, c;
    sincospi(-2.0 * (double)m / (double)r, &s, &c);
    tw[m] = make_float2((float)c, (float)s);  // exp(-2 pi i m / r)
  }
}

// log2 r radix-2 Stockham passes over a tile of (1 << lgT) lines; element i of line t sits at t * r + i (LINE_MAJOR: the
// lines are contiguous in memory) or at i * T + t (the tile's lines are adjacent in memory).  Returns the buffer with the result.
template <bool LINE_MAJOR>
__device__ __forceinline__ float2 *fft_tile(float2 *a, float2 *b, const float2 *tw, int lgT, int lg, bool inverse) {
  const int r = 1 << lg, half = r >> 1, T = 1 << lgT;
  const int work = T * half;
  for (int s = 0; s < lg; ++s) {
    const int p = 1 << s;
    for (int wi = threadIdx.x; wi < work; wi += NT) {
      const int t = LINE_MAJOR ? (wi >> (lg - 1)) : (wi & (T - 1));
      const int i = LINE_MAJOR ? (wi & (half - 1)) : (wi >> lgT);
      const int k = i & (p - 1);
      const int j = ((i - k) << 1) + k;
      float2 wv = tw[k * (half >> s)];
      if (inverse) wv.y = -wv.y;
      const int ia = LINE_MAJOR ? t * r + i : i * T + t;
      const int ib = LINE_MAJOR ? ia + half : ia + half * T;
      const int oa = LINE_MAJOR ? t * r + j : j * T + t;
      const int ob = LINE_MAJOR ? oa + p : oa + p * T;
      const float2 u0 = a[ia], x1 = a[ib];
      const float2 u1 = make_float2(wv.x * x1.x - wv.y * x1.y, wv.x * x1.y + wv.y * x1.x);
      b[oa] = make_float2(u0.x + u1.x, u0.y + u1.y);
      b[ob] = make_float2(u0.x - u1.x, u0.y - u1.y);
    }
    __syncthreads();
    float2 *tmp = a;
    a = b;
    b = tmp;
  }
  return a;
}

// forward along axis 3: real lines (fixed point or float) -> bins 0 .. r/2.  One workgroup: T = 1 << lgT consecutive lines.
template <bool FIXED>
__global__ __launch_bounds__(NT) void fft_r2c_axis3_kernel(const void *__restrict__ in, float2 *__restrict__ spec, int lg, int lgT) {
  __shared__ float2 sa[FFT_TILE], sb[FFT_TILE], tw[FFT_RMAX / 2];
  const int r = 1 << lg, h = (r >> 1) + 1, T = 1 << lgT;
  const long long line0 = (long long)blockIdx.x * T;
  twiddle_table(tw, r);
  for (int e = threadIdx.x; e < T * r; e += NT) {
    const long long g = line0 * r + e;
    const float v = FIXED ? (float)((const long long *)in)[g] * FIX_INV : ((const float *)in)[g];
    sa[e] = make_float2(v, 0.0f);
  }
  __syncthreads();
  const float2 *res = fft_tile<true>(sa, sb, tw, lgT, lg, false);
  for (int e = threadIdx.x; e < T * h; e += NT) {
    const int t = e / h, k = e - t * h;
    spec[(line0 + t) * h + k] = res[t * r + k];
  }
}

// c2c in place along the middle axis of an (outer, r, inner) complex array; one workgroup: T adjacent inner positions
__global__ __launch_bounds__(NT) void fft_strided_kernel(float2 *__restrict__ x, int inner, int tiles, int lg, int lgT, int inverse) {
  __shared__ float2 sa[FFT_TILE], sb[FFT_TILE], tw[FFT_RMAX / 2];
  const int r = 1 << lg, T = 1 << lgT;
  const long long o = blockIdx.x / tiles;
  const int m0 = (int)(blockIdx.x - o * tiles) * T;
  float2 *base = x + o * r * (long long)inner + m0;
  twiddle_table(tw, r);
  for (int e = threadIdx.x; e < T * r; e += NT) {
    const int t = e & (T - 1), i = e >> lgT;
    sa[e] = (m0 + t < inner) ? base[(long long)i * inner + t] : make_float2(0.0f, 0.0f);
  }
  __syncthreads();
  const float2 *res = fft_tile<false>(sa, sb, tw, lgT, lg, inverse != 0);
  for (int e = threadIdx.x; e < T * r; e += NT) {
    const int t = e & (T - 1), i = e >> lgT;
    if (m0 + t < inner) base[(long long)i * inner + t] = res[e];
  }
}

// inverse along axis 3: Hermitian extension of bins 0 .. r/2, inverse c2c, real part times `scale`
__global__ __launch_bounds__(NT) void fft_c2r_axis3_kernel(const float2 *__restrict__ spec, float *__restrict__ out, int lg, int lgT,
                                                           float scale) {
  __shared__ float2 sa[FFT_TILE], sb[FFT_TILE], tw[FFT_RMAX / 2];
  const int r = 1 << lg, half = r >> 1, h = half + 1, T = 1 << lgT;
  const long long line0 = (long long)blockIdx.x * T;
  twiddle_table(tw, r);
  for (int e = threadIdx.x; e < T * r; e += NT) {
    const int t = e >> lg, k = e & (r - 1);
    const float2 *line = spec + (line0 + t) * h;
    float2 y;
    if (k <= half) {
      y = line[k];
      if (k == 0 || k == half) y.y = 0.0f;
    } else {
      y = line[r - k];
      y.y = -y.y;
    }
    sa[e] = y;
  }
  __syncthreads();
  const float2 *res = fft_tile<true>(sa, sb, tw, lgT, lg, true);
  for (int e = threadIdx.x; e < T * r; e += NT) out[line0 * r + e] = res[e].x * scale;
}

// ------------------------------------------------------------------------------------------------------------ spectral solve
// spec (nb, 3, r, r, h) -> phis (nb, r, r, h); omega_d = fl(k_d * fl(2 pi)), k from fftfreq on axes 1, 2 and rfftfreq on axis 3
__global__ __launch_bounds__(NT) void dpsr_spectral_kernel(long long total, int r, const float2 *__restrict__ spec,
                                                           const float *__restrict__ G, float2 *__restrict__ phis) {
  const long long g = (long long)blockIdx.x * NT + threadIdx.x;
  if (g >= total) return;
  const int half = r >> 1, h = half + 1;
  const long long per = (long long)r * r * h;
  const long long s = g / per, rem = g - s * per;
  const int k3 = (int)(rem % h);
  const int j = (int)((rem / h) % r);
  const int i = (int)(rem / ((long long)h * r));
  const float two_pi = 6.283185307179586f;
  const float w0 = (float)(i < half ? i : i - r) * two_pi;
  const float w1 = (float)(j < half ? j : j - r) * two_pi;
  const float w2 = (float)k3 * two_pi;
  const float gk = G[rem];
  const float2 *c = spec + s * 3 * per + rem;
  const float2 s0 = c[0], s1 = c[per], s2 = c[2 * per];
  // N_ = S * G;  -img(N_) = (im, -re);  times omega, summed over the components in order
  const float dre = ((s0.y * gk) * w0 + (s1.y * gk) * w1) + (s2.y * gk) * w2;
  const float dim = ((-(s0.x * gk)) * w0 + (-(s1.x * gk)) * w1) + (-(s2.x * gk)) * w2;
  const float den = -((w0 * w0 + w1 * w1) + w2 * w2) + 1e-6f;
  phis[g] = rem == 0 ? make_float2(0.0f, 0.0f) : make_float2(dre / den, dim / den);
}

// ------------------------------------------------------------------------------------------------------------ shift and scale
// one workgroup per sample: coef[2 s] = offset = mean_n fv (0 without shift), coef[2 s + 1] = |phi[s,0,0,0] - offset|.
// Fixed order: every thread sums its strided share in double, then a tree over LDS.
__global__ __launch_bounds__(NT) void dpsr_coef_kernel(int n, long long r3, const float *__restrict__ fv, const float *__restrict__ phi,
                                                       int shift, float *__restrict__ coef) {
  __shared__ double part[NT];
  const long long s = blockIdx.x;
  double acc = 0.0;
  if (shift)
    for (int i = threadIdx.x; i < n; i += NT) acc += (double)fv[s * n + i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int st = NT / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float off = shift ? (float)(part[0] / (double)n) : 0.0f;
    coef[2 * s] = off;
    coef[2 * s + 1] = fabsf(phi[s * r3] - off);
  }
}

__global__ __launch_bounds__(NT) void dpsr_finish_kernel(long long total, long long r3, const float *__restrict__ coef, int scale,
                                                         float *__restrict__ phi) {
  const long long g = (long long)blockIdx.x * NT + threadIdx.x;
  if (g >= total) return;
  const long long s = g / r3;
  float v = phi[g] - coef[2 * s];
  if (scale) v = (-v) / coef[2 * s + 1] * 0.5f;
  phi[g] = v;
}

// ------------------------------------------------------------------------------------------------------------ host side
inline int tile_log2(int lg) {  // T = min(FFT_TILE / r, 32) lines
  const int lgT = 11 - lg;
  return lgT > 5 ? 5 : lgT;
}

int strided_pass(float2 *x, long long outer, long long inner, int lg, int inverse, hipStream_t st) {
  const int lgT = tile_log2(lg);
  const long long tiles = (inner + (1 << lgT) - 1) >> lgT;
  if (inner > 0x7fffffffLL || !blocks_ok(outer * tiles)) return -2;
  hipLaunchKernelGGL(fft_strided_kernel, dim3((unsigned)(outer * tiles)), dim3(NT), 0, st, x, (int)inner, (int)tiles, lg, lgT, inverse);
  return LAUNCH_STATUS();
}

}  // namespace

extern "C" {

int slide_point_rasterize(int b, int n, int nf, int r, const float *pts, const float *vals, long long *grid, int *flag,
                          slide_stream_t stream) {
  if ((nf != 1 && nf != 3) || r < 2 || r > GRID_RMAX || b < 0 || n < 0) return -2;
  if (b == 0 || n == 0) return 0;
  const long long total = (long long)b * n;
  if (!pts || !vals || !grid || !flag || !blocks_ok((total + NT - 1) / NT)) return -2;
  if (nf == 1)
    hipLaunchKernelGGL(point_rasterize_kernel<1>, dim3(blocks_of(total)), dim3(NT), 0, (hipStream_t)stream, total, n, r, pts, vals, grid, flag);
  else
    hipLaunchKernelGGL(point_rasterize_kernel<3>, dim3(blocks_of(total)), dim3(NT), 0, (hipStream_t)stream, total, n, r, pts, vals, grid, flag);
  return LAUNCH_STATUS();
}

int slide_grid_fixed_to_float(long long count, const long long *grid, float *out, slide_stream_t stream) {
  if (count < 0) return -2;
  if (count == 0) return 0;
  if (!grid || !out || !blocks_ok((count + NT - 1) / NT)) return -2;
  hipLaunchKernelGGL(fixed_to_float_kernel, dim3(blocks_of(count)), dim3(NT), 0, (hipStream_t)stream, count, grid, out);
  return LAUNCH_STATUS();
}

int slide_grid_interp(int b, int n, int c, int r, const float *grid, const float *pts, float *out, int *flag, slide_stream_t stream) {
  if (c < 1 || r < 2 || r > GRID_RMAX || b < 0 || n < 0) return -2;
  if (b == 0 || n == 0) return 0;
  const long long total = (long long)b * n;
  if (!grid || !pts || !out || !flag || !blocks_ok((total + NT - 1) / NT)) return -2;
  hipLaunchKernelGGL(grid_interp_kernel, dim3(blocks_of(total)), dim3(NT), 0, (hipStream_t)stream, total, n, c, r, grid, pts, out, flag);
  return LAUNCH_STATUS();
}

int slide_fft3_r2c(int nb, int r, const void *in, int fixed_point, float *spec, slide_stream_t stream) {
  const int lg = log2_fft(r);
  if (lg < 0 || nb < 0) return -2;
  if (nb == 0) return 0;
  if (!in || !spec) return -2;
  const int lgT = tile_log2(lg), h = r / 2 + 1;
  const long long lines = (long long)nb * r * r;  // (a multiple of the tile: r * r >= 256)
  if (!blocks_ok(lines >> lgT)) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (fixed_point)
    hipLaunchKernelGGL(fft_r2c_axis3_kernel<true>, dim3((unsigned)(lines >> lgT)), dim3(NT), 0, st, in, (float2 *)spec, lg, lgT);
  else
    hipLaunchKernelGGL(fft_r2c_axis3_kernel<false>, dim3((unsigned)(lines >> lgT)), dim3(NT), 0, st, in, (float2 *)spec, lg, lgT);
  int rc = LAUNCH_STATUS();
  if (rc) return rc;
  rc = strided_pass((float2 *)spec, (long long)nb * r, h, lg, 0, st);  // axis 2
  if (rc) return rc;
  return strided_pass((float2 *)spec, nb, (long long)r * h, lg, 0, st);  // axis 1
}

int slide_fft3_c2r(int nb, int r, float *spec, float *out, slide_stream_t stream) {
  const int lg = log2_fft(r);
  if (lg < 0 || nb < 0) return -2;
  if (nb == 0) return 0;
  if (!spec || !out) return -2;
  const int lgT = tile_log2(lg), h = r / 2 + 1;
  const long long lines = (long long)nb * r * r;
  if (!blocks_ok(lines >> lgT)) return -2;
  hipStream_t st = (hipStream_t)stream;
  int rc = strided_pass((float2 *)spec, nb, (long long)r * h, lg, 1, st);  // axis 1
  if (rc) return rc;
  rc = strided_pass((float2 *)spec, (long long)nb * r, h, lg, 1, st);  // axis 2
  if (rc) return rc;
  const float scale = 1.0f / ((float)r * (float)r * (float)r);
  hipLaunchKernelGGL(fft_c2r_axis3_kernel, dim3((unsigned)(lines >> lgT)), dim3(NT), 0, st, (const float2 *)spec, out, lg, lgT, scale);
  return LAUNCH_STATUS();
}

int slide_dpsr_spectral(int b, int r, const float *spec, const float *g, float *phis, slide_stream_t stream) {
  if (log2_fft(r) < 0 || b < 0) return -2;
  if (b == 0) return 0;
  const long long total = (long long)b * r * r * (r / 2 + 1);
  if (!spec || !g || !phis || !blocks_ok((total + NT - 1) / NT)) return -2;
  hipLaunchKernelGGL(dpsr_spectral_kernel, dim3(blocks_of(total)), dim3(NT), 0, (hipStream_t)stream, total, r, (const float2 *)spec, g,
                     (float2 *)phis);
  return LAUNCH_STATUS();
}

int slide_dpsr_finish(int b, int n, int r, const float *fv, int shift, int scale, float *coef, float *phi, slide_stream_t stream) {
  if (r < 2 || r > GRID_RMAX || b < 0 || n < 0 || (shift && n == 0)) return -2;
  if (b == 0 || (!shift && !scale)) return 0;
  const long long r3 = (long long)r * r * r, total = r3 * b;
  if (!coef || !phi || (shift && !fv) || !blocks_ok((total + NT - 1) / NT)) return -2;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dpsr_coef_kernel, dim3((unsigned)b), dim3(NT), 0, st, n, r3, fv, (const float *)phi, shift, coef);
  int rc = LAUNCH_STATUS();
  if (rc) return rc;
  hipLaunchKernelGGL(dpsr_finish_kernel, dim3(blocks_of(total)), dim3(NT), 0, st, total, r3, (const float *)coef, scale, phi);
  return LAUNCH_STATUS();
}

int slide_dpsr_grid(int b, int n, int r, const float *pts, const float *normals, const float *g, int shift, int scale,
                    long long *ws_grid, float *ws_spec, float *ws_phis, float *ws_fv, float *ws_coef, float *phi, int *flag,
                    slide_stream_t stream) {
  if (log2_fft(r) < 0 || b < 0 || n <= 0) return -2;
  if (b == 0) return 0;
  if (!pts || !normals || !g || !ws_grid || !ws_spec || !ws_phis || !ws_fv || !ws_coef || !phi || !flag) return -2;
  const long long r3 = (long long)r * r * r;
  int rc = (int)hipMemsetAsync(ws_grid, 0, (size_t)(3 * r3 * b) * sizeof(long long), (hipStream_t)stream);
  if (rc) return rc;
  if ((rc = slide_point_rasterize(b, n, 3, r, pts, normals, ws_grid, flag, stream))) return rc;
  if ((rc = slide_fft3_r2c(3 * b, r, ws_grid, 1, ws_spec, stream))) return rc;
  if ((rc = slide_dpsr_spectral(b, r, ws_spec, g, ws_phis, stream))) return rc;
  if ((rc = slide_fft3_c2r(b, r, ws_phis, phi, stream))) return rc;
  if (!shift && !scale) return 0;
  if (shift && (rc = slide_grid_interp(b, n, 1, r, phi, pts, ws_fv, flag, stream))) return rc;
  return slide_dpsr_finish(b, n, r, ws_fv, shift, scale, ws_coef, phi, stream);
}

}  // extern "C"
