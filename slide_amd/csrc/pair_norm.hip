// pair_norm.hip -- the pair-table pass of the pair decomposition as a launch of its own (SLIDE_OP_PAIR_NORM):
// turns the per-point products into the tables (a, b) the generated-X GEMMs read, GroupNorm statistics over the sample's pairs folded
// in (device body: pair_norm.h).  The product library runs it with FLOAT tables, for the split-arithmetic plans; the fp16 plans
// run SLIDE_OP_PAIR_FIRST (gemm_ring.hip), and their two forms of this op are in experiments/pair_norm_variants.hip.
#include "gemm_common.h"
#include "launch.h"
#include "pair_norm.h"

// version 2 with FLOAT tables (i[4] == 1): the pair-table pass of the split-arithmetic plans (product build)
static int launch_pair_norm2_f32(const SlideOp &o, hipStream_t s) {
  const int B = o.i[0], ld = o.i[1], K = o.i[2];
  if (B <= 0 || ld <= 0 || ld % 32 || ld > 2048) return -3;
  const SlideGnFin *fin = (const SlideGnFin *)o.p[12];
  // (512-thread workgroups: 256 registers per thread -- with 1024 the 16 x 16 pair loop over two 16-entry register tables spills)
  const int npass = (ld + 511) / 512, nthr = ((ld + npass - 1) / npass + 63) / 64 * 64;
  const dim3 grid(B), blk(nthr < 512 ? nthr : 512);
  if (K == 16)
    hipLaunchKernelGGL((pair_norm2_kernel<false, float, 512>), grid, blk, 0, s, ld, (const float *)o.p[0], (const float *)o.p[1],
                       (const float *)o.p[2], (const float *)o.p[3], (const SlideEpi *)o.p[4], (float *)o.p[5], (float *)o.p[6],
                       (const int *)nullptr, (const float *)nullptr, (const float *)nullptr, (const float *)nullptr,
                       (float *)nullptr, fin);
  else if (K == 8) {
    if (!o.p[7] || !o.p[8] || !o.p[9] || !o.p[10] || !o.p[11]) return -3;
    allow_dynamic_lds<&pair_norm2_kernel<true, float, 512>>(16 * 513 * 4);
    hipLaunchKernelGGL((pair_norm2_kernel<true, float, 512>), grid, blk, (size_t)16 * 513 * 4, s, ld, (const float *)o.p[0],
                       (const float *)o.p[1], (const float *)o.p[2], (const float *)o.p[3], (const SlideEpi *)o.p[4],
                       (float *)o.p[5], (float *)o.p[6], (const int *)o.p[7], (const float *)o.p[8], (const float *)o.p[9],
                       (const float *)o.p[10], (float *)o.p[11], fin);
  } else return -5;
  return (int)hipGetLastError();
}

int slide_launch_pair_norm(const SlideOp &o, hipStream_t s) {
  if (o.i[3] == 2 && o.i[4] == 1) return launch_pair_norm2_f32(o, s);
#ifdef SLIDE_EXPERIMENTS
  return slide_launch_pair_norm_variants(o, s);
#else
  return SLIDE_ST_EXPERIMENT;
#endif
}
