// refine_front.hip -- what the reference does around its refinement network before DPSR sees a cloud: mirror the cloud across a plane
// through its centroid and tag the halves (pointnet2/data_utils/mirror_partial.py:8-52), split every point into its children
// (models/point_upsample_module.py:4-46), normalise them to the ShapeNet-PSR box or the dataset scale and clamp them into DPSR's cube
// (dpsr_evaluation.py:22-32, 74-82).  The definition -- every expression in the order it is rounded -- is written out in
// include/slide_hip.h Part 9; this file is compiled with -ffp-contract=off and divides with `/` (correctly rounded under hipcc's
// default), so the outputs equal the reference's bit for bit.
//
// slide_mirror_concat   centre launch: one workgroup per sample, double sums in a fixed order (a thread's rows ascending, an LDS
//                       tree); row launch: a thread per output row.
// slide_refine_to_dpsr  A thread owns one OUTPUT row (a child, or a `mid` row of the include_center form) and computes its six
//                       channels from X's row and six consecutive displacements (three 8-byte loads).  Launch 1 stores every
//                       tile's minimum / maximum (wave shuffles, then LDS, plain stores to partials[sample][tile]); launch 2
//                       recomputes the row -- cheaper than a round trip of 24 bytes per row -- reduces the sample's partials in every
//                       workgroup and transforms.  Minimum and maximum are exact in any order, so nothing depends on the schedule.
// Flags: the first launch of an entry point resets flag[0..1]; only the second launch sets bits (integer atomicOr / atomicMax), so
// the reset and the bits are ordered by the launch boundary.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/slide_hip.h"
#include "kernel_util.h"
#include "launch.h"

namespace {

constexpr int RF_NT = 256;  // threads = output rows per tile
constexpr int RF_WAVES = RF_NT / 64;
constexpr int ST_LDX = -3, ST_DW = -4, ST_CENTER = -5, ST_FACTOR = -6;

__device__ __forceinline__ void raise_flag(int *flag, int bits, int sample) {
  atomicOr(&flag[0], bits);
  atomicMax(&flag[1], sample + 1);
}

// ------------------------------------------------------------------------------------------------------------ mirror
__global__ __launch_bounds__(RF_NT) void mirror_center_kernel(int n, int c, const float *__restrict__ x, float *__restrict__ center,
                                                              int *__restrict__ flag) {
  __shared__ double part[3][RF_NT];
  const int s = blockIdx.x, t = threadIdx.x;
  if (s == 0 && t == 0) flag[0] = flag[1] = 0;
  const float *xs = x + (size_t)s * n * c;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i = t; i < n; i += RF_NT) {
    a0 += (double)xs[(size_t)i * c];
    a1 += (double)xs[(size_t)i * c + 1];
    a2 += (double)xs[(size_t)i * c + 2];
  }
  part[0][t] = a0;
  part[1][t] = a1;
  part[2][t] = a2;
  __syncthreads();
  for (int d = RF_NT / 2; d >= 1; d >>= 1) {
    if (t < d) {
      part[0][t] += part[0][t + d];
      part[1][t] += part[1][t + d];
      part[2][t] += part[2][t + d];
    }
    __syncthreads();
  }
  if (t < 3) center[s * 3 + t] = (float)(part[t][0] / (double)n);
}

__global__ __launch_bounds__(RF_NT) void mirror_rows_kernel(int b, int n, int c, const float *__restrict__ x, int axis, int label,
                                                            const int *__restrict__ perm, const float *__restrict__ center,
                                                            float *__restrict__ out, int *flag) {
  const long long gid = (long long)blockIdx.x * RF_NT + threadIdx.x;
  const long long n2 = 2LL * n;
  if (gid >= (long long)b * n2) return;
  const int s = (int)(gid / n2);
  const int j = (int)(gid - (long long)s * n2);
  const int co = c + label;
  float *o = out + (size_t)gid * co;
  int src = j;
  if (perm) {
    src = perm[j];
    if (src < 0 || src >= n2) {  // tested before it addresses anything
      raise_flag(flag, 1, s);
      for (int k = 0; k < co; ++k) o[k] = 0.f;
      return;
    }
  }
  const bool mirrored = src >= n;
  const float *row = x + ((size_t)s * n + (mirrored ? src - n : src)) * c;
  if (!mirrored) {
    for (int k = 0; k < c; ++k) o[k] = row[k];
  } else {
    for (int k = 0; k < 3; ++k) {
      const float ck = center[s * 3 + k];
      float m = row[k] - ck;
      if (k == axis) m = -m;
      o[k] = m + ck;
    }
    for (int k = 3; k < c; ++k) o[k] = (c >= 6 && k == axis + 3) ? -row[k] : row[k];
  }
  if (label) o[c] = mirrored ? -1.f : 1.f;
}

// ------------------------------------------------------------------------------------------------------------ refine
struct RefineArgs {
  const float *X, *disp;
  int m, ldx, dw, rows, kp, first, with_mid;
  long long R;  // output rows per sample
  float g, s;
};

// the six channels of output row o of sample `smp` (o < R)
__device__ __forceinline__ void refine_row(const RefineArgs &a, int smp, long long o, float (&ch)[6]) {
  const long long nchild = (long long)a.rows * a.kp;
  const bool is_mid = o >= nchild;  // (only with with_mid)
  const int n = is_mid ? (int)(o - nchild) : (int)(o / a.kp);
  const int j = is_mid ? 0 : (int)(o - (long long)n * a.kp);
  const float *xr = a.X + ((size_t)smp * a.m + n) * a.ldx;
  const float *dr = a.disp + ((size_t)smp * a.m + n) * a.dw;
  float base[6];
  if (a.ldx == 6) {
    const float2 *x2 = reinterpret_cast<const float2 *>(xr);  // rows of 24 bytes from an 8-byte aligned base (checked by the launcher)
    const float2 p0 = x2[0], p1 = x2[1], p2 = x2[2];
    base[0] = p0.x; base[1] = p0.y; base[2] = p1.x; base[3] = p1.y; base[4] = p2.x; base[5] = p2.y;
  } else {
#pragma unroll
    for (int c = 0; c < 6; ++c) base[c] = xr[c];
  }
  if (a.first) {
    const float2 *d2 = reinterpret_cast<const float2 *>(dr);
    const float2 q0 = d2[0], q1 = d2[1], q2 = d2[2];
    const float cd[6] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y};
#pragma unroll
    for (int c = 0; c < 6; ++c) base[c] = base[c] + cd[c] * a.s;
    dr += 6;
  }
  if (is_mid) {
#pragma unroll
    for (int c = 0; c < 6; ++c) ch[c] = base[c];
    return;
  }
  const float2 *d2 = reinterpret_cast<const float2 *>(dr + (size_t)j * 6);  // dw and 6 j are even: 8-byte aligned
  const float2 q0 = d2[0], q1 = d2[1], q2 = d2[2];
  const float d[6] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y};
#pragma unroll
  for (int c = 0; c < 6; ++c) ch[c] = base[c] + (d[c] * a.g) * a.s;
}

// the waves' minima / maxima of xyz into red[0 .. 3) / red[3 .. 6), behind ONE barrier; slot row r < 3 folds with MinOf, the others
// with MaxOf (kernel_util.h: fminf / fmaxf, which drop a NaN)
__device__ __forceinline__ void minmax_to_slots(const float (&mn)[3], const float (&mx)[3], float (*red)[RF_WAVES]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = wave_reduce(mn[k], MinOf()), hi = wave_reduce(mx[k], MaxOf());
    if ((threadIdx.x & 63) == 0) {
      red[k][threadIdx.x >> 6] = lo;
      red[3 + k][threadIdx.x >> 6] = hi;
    }
  }
  __syncthreads();
}
__device__ __forceinline__ float fold_minmax_row(const float (*red)[RF_WAVES], int r) {
  return r < 3 ? fold_slots<RF_WAVES>(red[r], MinOf()) : fold_slots<RF_WAVES>(red[r], MaxOf());
}

// grid (tiles, b): partials[smp][tile] = {min xyz, max xyz} of the tile's rows
__global__ __launch_bounds__(RF_NT) void refine_minmax_kernel(RefineArgs a, float *__restrict__ partials, int *__restrict__ flag) {
  __shared__ float red[6][RF_WAVES];
  const int smp = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  if (smp == 0 && tile == 0 && t == 0) flag[0] = flag[1] = 0;
  const long long o = (long long)tile * RF_NT + t;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (o < a.R) {
    float ch[6];
    refine_row(a, smp, o, ch);
#pragma unroll
    for (int k = 0; k < 3; ++k) mn[k] = mx[k] = ch[k];  // (fminf / fmaxf below drop a NaN; launch 2 reports it)
  }
  minmax_to_slots(mn, mx, red);
  if (t < 6) partials[((size_t)smp * gridDim.x + tile) * 6 + t] = fold_minmax_row(red, t);
}

// grid (tiles, b): every workgroup reduces its sample's partials (written by the launch before), then transforms its tile
__global__ __launch_bounds__(RF_NT) void refine_apply_kernel(RefineArgs a, int mode, float scale, const float *__restrict__ partials,
                                                             float *__restrict__ points, float *__restrict__ normals,
                                                             float *__restrict__ bbox, int *flag) {
  __shared__ float red[6][RF_WAVES];
  const int smp = blockIdx.y, tile = blockIdx.x, t = threadIdx.x, tiles = gridDim.x;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  const float *ps = partials + (size_t)smp * tiles * 6;
  for (int q = t; q < tiles; q += RF_NT) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      mn[k] = fminf(mn[k], ps[(size_t)q * 6 + k]);
      mx[k] = fmaxf(mx[k], ps[(size_t)q * 6 + 3 + k]);
    }
  }
  minmax_to_slots(mn, mx, red);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mn[k] = fold_slots<RF_WAVES>(red[k], MinOf());
    mx[k] = fold_slots<RF_WAVES>(red[3 + k], MaxOf());
  }
  if (tile == 0 && t < 6) bbox[smp * 6 + t] = fold_minmax_row(red, t);
  float ctr[3], L = 0.f;
  if (mode == 0) {
    float len[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ctr[k] = (mx[k] + mn[k]) / 2.f;
      len[k] = mx[k] - mn[k];
    }
    L = fmaxf(fmaxf(len[0], len[1]), len[2]);
    if (tile == 0 && t == 0 && !(L > 0.f || L < 0.f)) raise_flag(flag, 2, smp);  // 0, or NaN from an all-NaN sample
  }
  const long long o = (long long)tile * RF_NT + t;
  if (o >= a.R) return;
  float ch[6];
  refine_row(a, smp, o, ch);
  if (!(isfinite(ch[0]) && isfinite(ch[1]) && isfinite(ch[2]))) raise_flag(flag, 1, smp);
  const size_t row = ((size_t)smp * a.R + o) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float p;
    if (mode == 0) p = (ch[k] - ctr[k]) / L * 0.99f;
    else p = ch[k] / scale / 2.f;
    p = p / 1.2f + 0.5f;
    points[row + k] = fminf(fmaxf(p, 0.f), 0.99f);
    normals[row + k] = ch[3 + k];
  }
}

}  // namespace

extern "C" {

int slide_refine_span(int level) { return level == 0 ? RF_NT : -2; }

int slide_mirror_concat(int b, int n, int c, const float *x, int axis, int attach_label, const int *perm, float *out, float *center,
                        int *flag, slide_stream_t stream) {
  if (b < 0 || b > 65535 || n < 0 || c < 3 || axis < 0 || axis > 2 || n > 0x3fffffff) return -2;
  if (b == 0 || n == 0) return 0;
  if (!x || !out || !center || !flag) return -2;
  hipStream_t s = (hipStream_t)stream;
  mirror_center_kernel<<<(unsigned)b, RF_NT, 0, s>>>(n, c, x, center, flag);
  const long long total = (long long)b * 2 * n;
  const long long blocks = (total + RF_NT - 1) / RF_NT;
  if (blocks > 0x7fffffffLL) return -2;
  mirror_rows_kernel<<<(unsigned)blocks, RF_NT, 0, s>>>(b, n, c, x, axis, attach_label ? 1 : 0, perm, center, out, flag);
  return LAUNCH_STATUS();
}

int slide_refine_to_dpsr(int b, int m, int ldx, int dw, int rows, const float *X, const float *disp, int factor, int first_refine,
                         int include_center, float out_scale, int mode, float scale, float *points, float *normals, float *bbox,
                         float *partials, int *flag, slide_stream_t stream) {
  if (b < 0 || b > 65535 || m < 0 || rows < 0 || rows > m || mode < 0 || mode > 1) return -2;
  if (ldx != 6 && ldx != 7) return ST_LDX;
  if (factor < 1) return ST_FACTOR;
  if (include_center && !first_refine) return ST_CENTER;
  const int kp = include_center ? factor - 1 : factor;
  if ((long long)dw != 6LL * (first_refine ? kp + 1 : kp)) return ST_DW;
  const long long R = (long long)rows * kp + (include_center ? rows : 0);
  if (b == 0 || R == 0) return 0;
  if (!X || !disp || !points || !normals || !bbox || !partials || !flag) return -2;
  if (((uintptr_t)disp & 7) || (ldx == 6 && ((uintptr_t)X & 7))) return -2;
  const long long tiles = (R + RF_NT - 1) / RF_NT;
  if (tiles > 0x7fffffffLL) return -2;
  RefineArgs a;
  a.X = X;
  a.disp = disp;
  a.m = m;
  a.ldx = ldx;
  a.dw = dw;
  a.rows = rows;
  a.kp = kp;
  a.first = first_refine ? 1 : 0;
  a.with_mid = include_center ? 1 : 0;
  a.R = R;
  a.g = (float)(1.0 / sqrt((double)factor));
  a.s = out_scale;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles, (unsigned)b);
  refine_minmax_kernel<<<grid, RF_NT, 0, s>>>(a, partials, flag);
  refine_apply_kernel<<<grid, RF_NT, 0, s>>>(a, mode, scale, partials, points, normals, bbox, flag);
  return LAUNCH_STATUS();
}

}  // extern "C"
