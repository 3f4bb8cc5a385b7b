// dpsr_cell.h -- what dpsr.hip (forward) and dpsr_bwd.hip (backward) share: the launch constants, the fixed-point scale and the
// cell arithmetic of a point.  Both files are built with -ffp-contract=off; the expressions below are the reference's own
// (dpsr.hip's header comment), and the backward differentiates exactly these.
#ifndef SLIDE_DPSR_CELL_H
#define SLIDE_DPSR_CELL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"

namespace {

constexpr int NT = 256;
constexpr double FIX_ONE = 4294967296.0;             // 2^32
constexpr float FIX_INV = 2.3283064365386963e-10f;   // 2^-32
constexpr float VAL_MAX = 1048576.0f;                // 2^20
constexpr int GRID_RMAX = 1024;                      // r^3 stays within 2^30

// the cell of a point: flat indices and weights of its 8 corners; false when a coordinate is not in [0, 1)
__device__ __forceinline__ bool cell_of(float px, float py, float pz, int r, int (&idx)[8], float (&w)[8]) {
  const float p[3] = {px, py, pz};
  const float fr = (float)r;
  const float cs = 1.0f / fr;
  int i0[3], i1[3];
  float wa[3], wb[3];
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ok = ok && (p[d] >= 0.0f) && (p[d] < 1.0f);  // (a NaN fails both)
    const float q = p[d] / cs;
    const float f0 = floorf(q);
    i0[d] = (int)f0;
    i1[d] = (int)fmodf(ceilf(q), fr);
    ok = ok && (i0[d] < r);  // (p / cs can round up to r when r is no power of two)
    wa[d] = fabsf(p[d] - (f0 + 1.0f) * cs) / cs;  // corner bit 0: the opposite corner is (ind0 + 1) * cs
    wb[d] = fabsf(p[d] - f0 * cs) / cs;           // corner bit 1: the opposite corner is ind0 * cs
  }
  if (!ok) return false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int b0 = c >> 2, b1 = (c >> 1) & 1, b2 = c & 1;
    idx[c] = ((b0 ? i1[0] : i0[0]) * r + (b1 ? i1[1] : i0[1])) * r + (b2 ? i1[2] : i0[2]);
    w[c] = ((b0 ? wb[0] : wa[0]) * (b1 ? wb[1] : wa[1])) * (b2 ? wb[2] : wa[2]);
  }
  return true;
}

inline int log2_fft(int r) {
  for (int lg = 4; lg <= 8; ++lg)
    if (r == (1 << lg)) return lg;
  return -1;
}

inline bool blocks_ok(long long nblk) { return nblk > 0 && nblk <= 0x7fffffffLL; }

inline unsigned blocks_of(long long total) { return (unsigned)((total + NT - 1) / NT); }

}  // namespace

#endif
