// attn_tail.h -- what the fused fp16 attention tails share (SLIDE_OP_ATTN_TAIL): the argument block and how an op fills it.
// Included by attn_tail.hip (register-X and ring forms) and experiments/attn_tail_variants.hip (wide and eight-wave forms).
#pragma once
#include <cstdlib>

#include "gemm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ attention tail
// The end of an AttentionModule (attention.py:90-95) as ONE launch: scores S = W5 . u + b5, values
// V = ReLU(GN(Wv . mo + bv)), out[point] = sum_k softmax_k(S) * V -- instead of two GEMMs that write S and V
// ([rows][C] each) and a third kernel that reads them back.  MFMA operands are SWAPPED with respect to gemm_glds_kernel
// (A = X rows, B = W rows): a lane then owns ONE channel and its registers run over rows, so GroupNorm statistics
// and the softmax over a point's K neighbours are register loops plus one exchange between the lane halves, and
// neither S nor V ever leaves the registers.  Tile: 256 rows x 64 channels, four waves x 64 rows; K = 2^(NPXL-4)
// neighbours per point (16 rows of a 256-row sample, 8 of a 128-row one).
struct AttnTailArgs {
  const void *X1, *W1, *X2, *W2;  // scores: u [rows][x1_ld] . W5 [C][k1];  values: mo [rows][x2_ld] . Wv [C][k2]
  const float *vec;               // [bias_s | bias_v | gamma | beta], n_cob * 32 floats each
  void *out;                      // [rows >> (NPXL - 4)][out_ld] fp16
  void *out_cm;                   // optional second copy, chunk-major [c / 32][rows >> (NPXL - 4)][32]
  void *out2;                     // optional copy of the first out2_n channels into another per-point buffer [..][out2_ld]
  int out2_ld, out2_n;
  int rows, x1_ld, k1, x2_ld, k2, n_cob, gs, n_norm, out_ld;
  unsigned long long *dbg;        // optional per-workgroup timeline (instrumented builds)
  int abl;                        // timing ablations of attn_tail8_kernel (tools only): 1 no DMA, 2 no fragment reads, 3 no MFMA
  int w_cm;                       // both weight matrices are chunk-major [k / 32][n_cob * 32][32] (u / mo are when their ld is 32)
  int x_fm;                       // u / mo are FRAGMENT-major (SLIDE_F_OUT_FM, include/slide_engine.h; register-X kernel only)
  float inv_count;
};

// SLIDE_OP_ATTN_TAIL (include/slide_engine.h) -> AttnTailArgs; 0 or the status of a malformed op
inline int attn_tail_args_from_op(const SlideOp &o, AttnTailArgs &a) {
  a.X1 = o.p[0]; a.W1 = o.p[1]; a.X2 = o.p[2]; a.W2 = o.p[3]; a.out = o.p[4]; a.vec = (const float *)o.p[5];
  a.out_cm = o.p[6];
  a.dbg = (unsigned long long *)o.p[8];
  a.out2 = o.p[7]; a.out2_ld = (int)o.f[2]; a.out2_n = (int)o.f[3];
  a.rows = o.i[0]; a.x1_ld = o.i[1]; a.k1 = o.i[2]; a.x2_ld = o.i[3]; a.k2 = o.i[4]; a.n_cob = o.i[5];
  a.gs = o.i[7]; a.n_norm = o.i[8]; a.out_ld = o.i[9];
  a.inv_count = o.f[0];
  a.w_cm = ((int)o.f[1] & 1) != 0;
  a.x_fm = ((int)o.f[1] & 16) != 0;
  static const int tail_abl = [] { const char *e = getenv("SLIDE_TAIL_ABL"); return e ? atoi(e) : 0; }();
  a.abl = tail_abl;
  if (a.k1 % 32 || a.k2 % 32 || a.rows <= 0 || a.n_cob <= 0) return -3;
  return 0;
}

}  // namespace
