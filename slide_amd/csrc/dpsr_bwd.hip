// dpsr_bwd.hip -- the backward of DPSR (dpsr.hip): g = dL/dphi -> dL/dV, dL/dN of the oriented points.  With phi the forward's
// output, coef = (off, a = |fv0|) per sample as dpsr_finish wrote them, s = pre - off (pre: the grid before shift and scale):
//
//   1. sums      per sample sum g and sum g phi over the r^3 cells, fixed order                   dpsr_bwd_partial_kernel, dpsr_bwd_final_kernel
//   2. dpre      finish and shift, elementwise.  With scale: ds = -0.5 g / a, da = -sum(g phi) / a,
//                ds[0,0,0] += sign(fv0) da (sign(fv0) = -sign(phi[0,0,0])); without: ds = g.
//                With shift: off = mean_n fv_n, so every point's dfv = -sum(ds) / n and
//                dpre = ds + dfv W, W = rasterize(V, 1) the trilinear density (fixed point, exact:
//                the existing rasterizer; dfv itself is far below its 2^-32 quantum)                dpsr_bwd_dpre_kernel
//   3. r2c       Y = rfftn(dpre)                                                                   dpsr.hip: slide_fft3_r2c
//   4. adjoint   dRas_d = conj(m_d) Y = +i omega_d G Y / (-|omega|^2 + 1e-6), bin (0,0,0) = 0         dpsr_spectral_adj_kernel
//   5. c2r       dras_d = irfftn(dRas_d), three grids per sample                                   dpsr.hip: slide_fft3_c2r
//   6. points    dN_{n,d} = sum_c w_c dras_d[idx_c]
//                dV_n = sum_c (dw_c/dV_n) (sum_d N_{n,d} dras_d[idx_c] + dfv pre[idx_c]),
//                pre = phi + off without scale and -2 a phi + off with it: the unshifted grid is not kept.  (off may NOT be
//                left out: sum_c dw_c/dV is 0 only off the lattice planes, where sign(0) = 0 drops a term)   dpsr_bwd_points_kernel
//
// Step 4 on the half spectrum followed by the c2r IS the adjoint of the forward's solve (r2c, multiply, c2r): with wt_k = 1 on
// the k3 = 0 and k3 = r/2 planes and 2 elsewhere, <g, irfftn Y> = (1/N) Re sum_k wt_k conj(G_k) Y_k, applied twice; a full c2c
// adjoint with fftfreq on all axes is NOT.
//
// Weights: a per-axis factor is |p - corner| / cs, its derivative sign(p - corner) * r with sign(0) = 0 (torch.abs's
// subgradient): -r for the factor of corner bit 0, +r for that of bit 1 except on a lattice plane, where it is 0.  floor, ceil
// and fmod carry no gradient.
//
// The sums run in double: per-thread strided shares, a tree over LDS, then one workgroup per sample over the partials of its
// SUM_SPAN-cell workgroups in the same manner.  No float atomics anywhere in this file (the one integer atomicOr raises the flag
// of a rejected point): every result is bit-reproducible and a sample's gradients do not depend on the batch, its position or
// the chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slide_hip.h"
#include "dpsr_cell.h"

namespace {

constexpr int SUM_SPAN = 4096;  // cells per workgroup of the first sum stage (16 per thread)

// ------------------------------------------------------------------------------------------------------------ sums
__device__ __forceinline__ void tree2(double (&pa)[NT], double (&pb)[NT], double a, double b) {
  pa[threadIdx.x] = a;
  pb[threadIdx.x] = b;
  __syncthreads();
  for (int st = NT / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      pa[threadIdx.x] += pa[threadIdx.x + st];
      pb[threadIdx.x] += pb[threadIdx.x + st];
    }
    __syncthreads();
  }
}

// workgroup (s, k): cells [k SUM_SPAN, (k + 1) SUM_SPAN) of sample s -> part[s * nbps + k] = (sum g, sum g phi)
__global__ __launch_bounds__(NT) void dpsr_bwd_partial_kernel(long long r3, int nbps, const float *__restrict__ g,
                                                              const float *__restrict__ phi, double2 *__restrict__ part) {
  __shared__ double pa[NT], pb[NT];
  const long long s = blockIdx.x / nbps;
  const long long c0 = (long long)(blockIdx.x - s * nbps) * SUM_SPAN;
  const long long end = c0 + SUM_SPAN < r3 ? c0 + SUM_SPAN : r3;
  double a = 0.0, b = 0.0;
  for (long long c = c0 + threadIdx.x; c < end; c += NT) {
    const double gv = (double)g[s * r3 + c];
    a += gv;
    b += gv * (double)phi[s * r3 + c];
  }
  tree2(pa, pb, a, b);
  if (threadIdx.x == 0) part[blockIdx.x] = make_double2(pa[0], pb[0]);
}

// workgroup s: the nbps partials of sample s -> sums[s] = (sum g, sum g phi)
__global__ __launch_bounds__(NT) void dpsr_bwd_final_kernel(int nbps, const double2 *__restrict__ part, double2 *__restrict__ sums) {
  __shared__ double pa[NT], pb[NT];
  const long long s = blockIdx.x;
  double a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < nbps; k += NT) {
    const double2 v = part[s * nbps + k];
    a += v.x;
    b += v.y;
  }
  tree2(pa, pb, a, b);
  if (threadIdx.x == 0) sums[s] = make_double2(pa[0], pb[0]);
}

// ------------------------------------------------------------------------------------------------------------ finish and shift
// the scalars of a sample, from its sums, in double, each rounded once: c0 = sign(fv0) da, the term of cell 0 (0 without scale);
// dfv = -sum(ds) / n, every point's gradient of the offset (0 without shift).  dpre and points call it on the same inputs.
__device__ __forceinline__ void sample_scalars(double2 sm, float a32, float phi0, int n, int shift, int scale, float &c0, float &dfv) {
  double sum_ds = sm.x;
  c0 = 0.0f;
  if (scale) {
    const double a = (double)a32;
    const double sgn = phi0 > 0.0f ? -1.0 : (phi0 < 0.0f ? 1.0 : 0.0);  // sign(fv0) = -sign(phi[0,0,0])
    const double t = sgn * (-sm.y / a);
    c0 = (float)t;
    sum_ds = -0.5 * sm.x / a + t;
  }
  dfv = shift ? (float)(-sum_ds / (double)n) : 0.0f;
}

__global__ __launch_bounds__(NT) void dpsr_bwd_dpre_kernel(long long total, long long r3, int n, const float *__restrict__ g,
                                                           const float *__restrict__ phi, const double2 *__restrict__ sums,
                                                           const float *__restrict__ coef, const long long *__restrict__ wfix, int shift,
                                                           int scale, float *__restrict__ dpre) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const long long s = i / r3;
  float v = g[i];
  if (shift || scale) {
    const float a = coef[2 * s + 1];
    float c0, dfv;
    sample_scalars(sums[s], a, phi[s * r3], n, shift, scale, c0, dfv);
    if (scale) {
      v = (v * -0.5f) / a;
      if (i == s * r3) v = v + c0;
    }
    if (shift) v = v + dfv * ((float)wfix[i] * FIX_INV);
  }
  dpre[i] = v;
}

// ------------------------------------------------------------------------------------------------------------ adjoint solve
// y (nb, r, r, h) -> out (nb, 3, r, r, h); omega, G and den exactly as dpsr_spectral_kernel forms them
__global__ __launch_bounds__(NT) void dpsr_spectral_adj_kernel(long long total, int r, const float2 *__restrict__ y,
                                                               const float *__restrict__ G, float2 *__restrict__ out) {
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
  const float2 v = y[g];
  const float den = -((w0 * w0 + w1 * w1) + w2 * w2) + 1e-6f;
  // i Y = (-im, re);  times G, times omega_d, over den
  const float re = -(v.y * gk), im = v.x * gk;
  float2 *o = out + s * 3 * per + rem;
  const bool zero = rem == 0;
  o[0] = zero ? make_float2(0.0f, 0.0f) : make_float2((re * w0) / den, (im * w0) / den);
  o[per] = zero ? make_float2(0.0f, 0.0f) : make_float2((re * w1) / den, (im * w1) / den);
  o[2 * per] = zero ? make_float2(0.0f, 0.0f) : make_float2((re * w2) / den, (im * w2) / den);
}

// ------------------------------------------------------------------------------------------------------------ points
__device__ __forceinline__ float sign_of(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

// one thread per point: the 8 corners of the three dras grids (and of phi with SHIFT) -> dV (3), dN (3); either may be NULL
template <bool SHIFT>
__global__ __launch_bounds__(NT) void dpsr_bwd_points_kernel(long long total, int n, int r, const float *__restrict__ pts,
                                                             const float *__restrict__ normals, const float *__restrict__ dras,
                                                             const float *__restrict__ phi, const double2 *__restrict__ sums,
                                                             const float *__restrict__ coef, int scale, float *__restrict__ dV,
                                                             float *__restrict__ dN, int *__restrict__ flag) {
  const long long g = (long long)blockIdx.x * NT + threadIdx.x;
  if (g >= total) return;
  const long long s = g / n;
  const long long r3 = (long long)r * r * r;
  const float fr = (float)r;
  const float cs = 1.0f / fr;
  int i0[3], i1[3];
  float wa[3], wb[3], da[3], db[3];
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {  // cell_of's expressions, per axis, with the derivative of every factor
    const float p = pts[g * 3 + d];
    ok = ok && (p >= 0.0f) && (p < 1.0f);
    const float q = p / cs;
    const float f0 = floorf(q);
    i0[d] = (int)f0;
    i1[d] = (int)fmodf(ceilf(q), fr);
    ok = ok && (i0[d] < r);
    const float ea = p - (f0 + 1.0f) * cs, eb = p - f0 * cs;
    wa[d] = fabsf(ea) / cs;
    wb[d] = fabsf(eb) / cs;
    da[d] = sign_of(ea) / cs;
    db[d] = sign_of(eb) / cs;
  }
  if (!ok) {
    atomicOr(flag, 1);
    for (int d = 0; d < 3; ++d) {
      if (dV) dV[g * 3 + d] = 0.0f;
      if (dN) dN[g * 3 + d] = 0.0f;
    }
    return;
  }
  float dfv = 0.0f, sfac = 1.0f, off = 0.0f;  // pre = sfac phi + off: sfac = -2 a with scale
  if (SHIFT) {
    const float a = coef[2 * s + 1];
    float c0;
    sample_scalars(sums[s], a, phi[s * r3], n, 1, scale, c0, dfv);
    if (scale) sfac = -2.0f * a;
    off = coef[2 * s];
  }
  const float n0 = normals[g * 3], n1 = normals[g * 3 + 1], n2 = normals[g * 3 + 2];
  const float *base = dras + s * 3 * r3;
  float vx = 0.0f, vy = 0.0f, vz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int b0 = c >> 2, b1 = (c >> 1) & 1, b2 = c & 1;
    const int idx = ((b0 ? i1[0] : i0[0]) * r + (b1 ? i1[1] : i0[1])) * r + (b2 ? i1[2] : i0[2]);
    const float w0 = b0 ? wb[0] : wa[0], w1 = b1 ? wb[1] : wa[1], w2 = b2 ? wb[2] : wa[2];
    const float d0 = b0 ? db[0] : da[0], d1 = b1 ? db[1] : da[1], d2 = b2 ? db[2] : da[2];
    const float r0 = base[idx], r1 = base[r3 + idx], r2 = base[2 * r3 + idx];
    const float w = (w0 * w1) * w2;
    nx = nx + w * r0;
    ny = ny + w * r1;
    nz = nz + w * r2;
    float q = (n0 * r0 + n1 * r1) + n2 * r2;
    if (SHIFT) q = q + dfv * (sfac * phi[s * r3 + idx] + off);
    vx = vx + ((d0 * w1) * w2) * q;
    vy = vy + ((w0 * d1) * w2) * q;
    vz = vz + ((w0 * w1) * d2) * q;
  }
  if (dV) {
    dV[g * 3] = vx;
    dV[g * 3 + 1] = vy;
    dV[g * 3 + 2] = vz;
  }
  if (dN) {
    dN[g * 3] = nx;
    dN[g * 3 + 1] = ny;
    dN[g * 3 + 2] = nz;
  }
}

inline long long sum_blocks(int r) { return ((long long)r * r * r + SUM_SPAN - 1) / SUM_SPAN; }

}  // namespace

extern "C" {

int slide_dpsr_bwd_sums(int b, int r, const float *gout, const float *phi, double *ws_part, double *sums, slide_stream_t stream) {
  if (r < 2 || r > GRID_RMAX || b < 0) return -2;
  if (b == 0) return 0;
  const long long nbps = sum_blocks(r);
  if (!gout || !phi || !ws_part || !sums || !blocks_ok(nbps * b)) return -2;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dpsr_bwd_partial_kernel, dim3((unsigned)(nbps * b)), dim3(NT), 0, st, (long long)r * r * r, (int)nbps, gout, phi,
                     (double2 *)ws_part);
  int rc = LAUNCH_STATUS();
  if (rc) return rc;
  hipLaunchKernelGGL(dpsr_bwd_final_kernel, dim3((unsigned)b), dim3(NT), 0, st, (int)nbps, (const double2 *)ws_part, (double2 *)sums);
  return LAUNCH_STATUS();
}

int slide_dpsr_bwd_dpre(int b, int n, int r, const float *gout, const float *phi, const double *sums, const float *coef,
                        const long long *w, int shift, int scale, float *dpre, slide_stream_t stream) {
  if (r < 2 || r > GRID_RMAX || b < 0 || n < 0 || (shift && n == 0)) return -2;
  if (b == 0) return 0;
  const long long r3 = (long long)r * r * r, total = r3 * b;
  if (!gout || !dpre || ((shift || scale) && (!phi || !sums || !coef)) || (shift && !w) || !blocks_ok((total + NT - 1) / NT)) return -2;
  hipLaunchKernelGGL(dpsr_bwd_dpre_kernel, dim3(blocks_of(total)), dim3(NT), 0, (hipStream_t)stream, total, r3, n, gout, phi,
                     (const double2 *)sums, coef, w, shift, scale, dpre);
  return LAUNCH_STATUS();
}

int slide_dpsr_spectral_adj(int b, int r, const float *spec, const float *g, float *out, slide_stream_t stream) {
  if (log2_fft(r) < 0 || b < 0) return -2;
  if (b == 0) return 0;
  const long long total = (long long)b * r * r * (r / 2 + 1);
  if (!spec || !g || !out || !blocks_ok((total + NT - 1) / NT)) return -2;
  hipLaunchKernelGGL(dpsr_spectral_adj_kernel, dim3(blocks_of(total)), dim3(NT), 0, (hipStream_t)stream, total, r, (const float2 *)spec, g,
                     (float2 *)out);
  return LAUNCH_STATUS();
}

int slide_dpsr_bwd_points(int b, int n, int r, const float *pts, const float *normals, const float *dras, const float *phi,
                          const double *sums, const float *coef, int shift, int scale, float *dv, float *dn, int *flag,
                          slide_stream_t stream) {
  if (r < 2 || r > GRID_RMAX || b < 0 || n < 0) return -2;
  if (b == 0 || n == 0 || (!dv && !dn)) return 0;
  const long long total = (long long)b * n;
  if (!pts || !normals || !dras || !flag || (shift && (!phi || !sums || !coef)) || !blocks_ok((total + NT - 1) / NT)) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (shift)
    hipLaunchKernelGGL(dpsr_bwd_points_kernel<true>, dim3(blocks_of(total)), dim3(NT), 0, st, total, n, r, pts, normals, dras, phi,
                       (const double2 *)sums, coef, scale, dv, dn, flag);
  else
    hipLaunchKernelGGL(dpsr_bwd_points_kernel<false>, dim3(blocks_of(total)), dim3(NT), 0, st, total, n, r, pts, normals, dras, phi,
                       (const double2 *)sums, coef, scale, dv, dn, flag);
  return LAUNCH_STATUS();
}

int slide_dpsr_grid_bwd(int b, int n, int r, const float *pts, const float *normals, const float *g, const float *phi, const float *coef,
                        const float *gout, int shift, int scale, long long *ws_w, float *ws_ones, float *ws_dpre, float *ws_spec,
                        float *ws_spec3, float *ws_dras, double *ws_part, double *ws_sums, float *dv, float *dn, int *flag,
                        slide_stream_t stream) {
  if (log2_fft(r) < 0 || b < 0 || n <= 0) return -2;
  if (b == 0 || (!dv && !dn)) return 0;
  if (!pts || !normals || !g || !phi || !gout || !ws_dpre || !ws_spec || !ws_spec3 || !ws_dras || !flag) return -2;
  if ((shift || scale) && (!coef || !ws_part || !ws_sums)) return -2;
  if (shift && (!ws_w || !ws_ones)) return -2;
  const long long r3 = (long long)r * r * r;
  // every step's grid, before the first launch: the largest elementwise launch covers 3 b r^3 cells (the c2r's, which also exceeds
  // the spectra, the FFT tiles and the sum partials), the per-point launches b n
  if (!blocks_ok((3 * r3 * b + NT - 1) / NT) || !blocks_ok(((long long)b * n + NT - 1) / NT)) return -2;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (shift || scale)
    if ((rc = slide_dpsr_bwd_sums(b, r, gout, phi, ws_part, ws_sums, stream))) return rc;
  if (shift) {
    if ((rc = (int)hipMemsetAsync(ws_w, 0, (size_t)(r3 * b) * sizeof(long long), st))) return rc;
    if ((rc = (int)hipMemsetD32Async((hipDeviceptr_t)ws_ones, 0x3f800000, (size_t)b * n, st))) return rc;  // 1.0f
    if ((rc = slide_point_rasterize(b, n, 1, r, pts, ws_ones, ws_w, flag, stream))) return rc;
  }
  if ((rc = slide_dpsr_bwd_dpre(b, n, r, gout, phi, ws_sums, coef, ws_w, shift, scale, ws_dpre, stream))) return rc;
  if ((rc = slide_fft3_r2c(b, r, ws_dpre, 0, ws_spec, stream))) return rc;
  if ((rc = slide_dpsr_spectral_adj(b, r, ws_spec, g, ws_spec3, stream))) return rc;
  if ((rc = slide_fft3_c2r(3 * b, r, ws_spec3, ws_dras, stream))) return rc;
  return slide_dpsr_bwd_points(b, n, r, pts, normals, ws_dras, phi, ws_sums, coef, shift, scale, dv, dn, flag, stream);
}

}  // extern "C"
