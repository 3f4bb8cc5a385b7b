// launch.h -- what crosses translation units inside the library (internal: not part of the C ABI under include/): the launch
// entry points that one .hip defines and another calls, the experiments-only status, LAUNCH_STATUS() of every file that launches
// by itself, and the per-device first-use helper of the dynamic-LDS limit.  Every .hip that defines or calls one of these functions includes this header, so a drifted signature fails
// to compile in the defining file (the library is also linked with --no-undefined: a forgotten source fails the link).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/slide_engine.h"

struct GemmArgs;  // gemm_common.h

// what an entry point returns after its last launch: 0, or the HIP error of a launch that was refused
#define LAUNCH_STATUS() ((int)hipGetLastError())

// Status of an op whose kernel only exists in the EXPERIMENTS build (slide_amd/build.py: libslide_hip_exp.so, -DSLIDE_EXPERIMENTS):
// the opt-in variants that lost their A/Bs (X-stationary tiles, per-point layer chains, head + update launch, wide / eight-wave
// attention tails, 128- / 32-channel and 64-deep ring tiles, the round-2 plan's gathered first layers, the register-staged fp16
// GEMM, the per-point stage, the pair-table pass on fp16 tables).  The product library carries only what a default plan dispatches.
#define SLIDE_ST_EXPERIMENT (-20)

// gemm_ring.hip: SLIDE_OP_GEMM, SLIDE_OP_PAIR_FIRST, SLIDE_OP_GEMM_ATTEND
int slide_launch_gemm(const SlideOp &o, hipStream_t s);
int slide_launch_pair_first(const SlideOp &o, hipStream_t s);
int slide_launch_gemm_attend(const SlideOp &o, hipStream_t s);
// attn_tail.hip: the fused attention tails (fp16): register-X and ring form (argument block: attn_tail.h)
int slide_launch_attn_tail(const SlideOp &o, hipStream_t s);
// attn_tail_split.hip: the fused attention tail in split arithmetic (float rows)
int slide_launch_attn_tail_split(const SlideOp &o, hipStream_t s);
// rows_ops.hip: the row-major ops of the module path
int slide_launch_rows_op(const SlideOp &o, hipStream_t s);
// point_chain.hip
int slide_launch_point_chain(const SlideOp &o, hipStream_t s);
// gemm_gx.hip: generated-X GEMM of the pair decomposition (fp16 tables)
int slide_launch_gemm_gx(const SlideOp &o, hipStream_t s);
int slide_launch_gemm_gx_dual(const SlideOp &o, hipStream_t s);
// gemm_gxs.hip: the same in split arithmetic (float tables)
int slide_launch_gemm_gxs(const SlideOp &o, hipStream_t s);
int slide_launch_gemm_gxs_dual(const SlideOp *pr, hipStream_t s);
// pair_norm.hip: the pair-table pass as a launch of its own (float tables; device body: pair_norm.h)
int slide_launch_pair_norm(const SlideOp &o, hipStream_t s);
// sa_chain.hip: the fused Mlp chain of an SA block, alone and with the attention's per-point query GEMM
int slide_launch_sa_chain(const SlideOp &o, hipStream_t s);
int slide_launch_sa_chain_p(const SlideOp &o, hipStream_t s);
// experiments/block_body.hip (called in the experiments build only)
int slide_launch_block_body(const SlideOp &o, hipStream_t s);
#ifdef SLIDE_EXPERIMENTS
// experiments/gemm_xs.hip: X-stationary kernel (-8: the X tile does not fit the LDS, -4: no such instantiation)
int slide_launch_gemm_xs(const GemmArgs &a, int npxl, int cbw, bool aff, bool gat, int want_occ, hipStream_t s);
// experiments/gemm_chain.hip
int slide_launch_gemm_chain(const SlideOp &o, hipStream_t s);
// experiments/pp_stage.hip: the per-point stage of the split position plan
int slide_launch_pp_stage(const SlideOp &o, hipStream_t s);
// experiments/pair_norm_variants.hip: the pair-table pass on fp16 tables (every SLIDE_OP_PAIR_NORM that pair_norm.hip does not run)
int slide_launch_pair_norm_variants(const SlideOp &o, hipStream_t s);
// experiments/attn_tail_variants.hip: eight-wave (tail8_on) and wide tails; attn_tail.hip offers every op to it first and goes
// on with its own forms when the answer is SLIDE_ST_NOT_A_VARIANT
#define SLIDE_ST_NOT_A_VARIANT (-21)
int slide_launch_attn_tail_variants(const SlideOp &o, bool tail8_on, hipStream_t s);
#endif

// hipFuncSetAttribute is per device: the "already raised the dynamic-LDS limit" flags are kept per device so that one
// process may drive plans on several GPUs (first use of a kernel on each device must still happen outside stream capture
// and from one thread, as for any lazily initialised runtime state)
constexpr int SLIDE_MAX_DEVICES = 64;
inline int current_device_slot() {
  int d = 0;
  (void)hipGetDevice(&d);
  return d >= 0 && d < SLIDE_MAX_DEVICES ? d : 0;
}

// once per (kernel, device): raise the kernel's dynamic-LDS limit.  Kernel is the address of a __global__ function or of one
// instantiation of a kernel template (allow_dynamic_lds<&k<3, true>>(bytes)): each gets its own flags.
template <auto Kernel>
inline void allow_dynamic_lds(int bytes) {
  static bool done[SLIDE_MAX_DEVICES] = {};
  bool &set = done[current_device_slot()];
  if (!set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    set = true;
  }
}
