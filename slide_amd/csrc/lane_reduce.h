// lane_reduce.h -- sums of MANY per-lane fp32 values over the lanes of a 16-lane row / a 32-lane half wave, by a transposing
// ("halving") butterfly.  An all-reduce of NV values costs NV log L cross-lane adds although a GroupNorm epilogue keeps each
// total in ONE place; here a lane keeps half of its values at every level and receives the partner's contribution for those,
// so the levels cost NV/2 + NV/4 + ... pairs and a row of 16 lanes ends up holding 16 DIFFERENT totals.
//
// LEVEL ORDER.  The partner lanes are those of lane_group_sum (gemm_common.h) / half_wave_sum_hi (gemm_gx.hip), in their
// order: lane ^ 1, lane ^ 2, lane ^ 4, lane ^ 8, then the two rows of a half wave.  (The all-reduces use row_half_mirror and
// row_mirror at the third and fourth level; there every lane of a quad / an octet holds the same partial, so the mirror
// partner and the xor partner carry the same number.)  Every addition therefore has the two operands it has in the all-reduce
// and the totals are bit-identical to it: fp32 addition is commutative.
//
// WHERE A TOTAL LANDS.  Values are numbered i < NV.  Level k (k = 0 .. 4) pairs the values whose numbers differ in bit
// log2(NV) - 1 - k; the lane with bit k clear keeps the value with that bit clear.  After lane_row_sums a lane holds NV / 16
// registers, after lane_half_sums NV / 32: register j is the total of value lane_reduce_index<NV>(lane) + j (the row total
// of value lane_reduce_row_index<NV>(lane) + j for lane_row_sums).  With fewer values than lanes (NV < 16, or NV < 32 for the
// half wave) the last levels are plain all-reduce steps: the lanes beyond the first NV hold copies of the same totals.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int lr_log2(int n) { return n <= 1 ? 0 : 1 + lr_log2(n >> 1); }

// registers a lane holds after lane_row_sums / lane_half_sums of NV values
constexpr int lane_row_regs(int nv) { return nv >= 16 ? nv / 16 : 1; }
constexpr int lane_half_regs(int nv) { return nv >= 32 ? nv / 32 : 1; }

template <int NV, int LEVELS>
__device__ __forceinline__ int lr_index(int lane) {
  constexpr int NBITS = lr_log2(NV), NL = NBITS < LEVELS ? NBITS : LEVELS;
  return (int)(__builtin_bitreverse32((unsigned)lane) >> (32 - NL)) << (NBITS - NL);
}
template <int NV> __device__ __forceinline__ int lane_reduce_row_index(int lane) { return lr_index<NV, 4>(lane); }
template <int NV> __device__ __forceinline__ int lane_reduce_index(int lane) { return lr_index<NV, 5>(lane); }

// v + (v of the quad_perm partner): the builtin pair folds into one v_add_f32_dpp
template <int CTRL>
__device__ __forceinline__ float lr_quad_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// levels 0 / 1 (lane ^ 1, lane ^ 2) on w[0 .. N): both values of a pair take their partner's contribution, the lane keeps its
// own of the two -- three instructions per pair, and no select in front of a DPP read (the two-state VALU -> DPP hazard)
template <int N, int CTRL>
__device__ __forceinline__ void lr_quad_level(float *w, bool upper) {
  if constexpr (N == 1) {
    w[0] = lr_quad_add<CTRL>(w[0]);
  } else {
#pragma unroll
    for (int p = 0; p < N / 2; ++p) {
      const float a = lr_quad_add<CTRL>(w[p]), b = lr_quad_add<CTRL>(w[p + N / 2]);
      w[p] = upper ? b : a;
    }
  }
}

// levels 2 / 3 (lane ^ 4, lane ^ 8): the kept value is chosen by the DPP bank mask, two fused adds per pair into ONE register.
// The compiler pads no hazard inside an asm statement: each opens with the two wait states between a VALU write of an
// operand and a DPP read of it; inside, no instruction reads what another one wrote.
#define LR_PAIR(A, B, SH, M_LO, M_HI)                                                      \
  "v_add_f32_dpp " A ", " A ", " A " row_shl:" SH " row_mask:0xf bank_mask:" M_LO "\n\t" \
  "v_add_f32_dpp " A ", " B ", " B " row_shr:" SH " row_mask:0xf bank_mask:" M_HI "\n\t"
#define LR_LEVEL(SH, M_LO, M_HI)                                                                                              \
  if constexpr (N == 16)                                                                                                      \
    asm("s_nop 1\n\t" LR_PAIR("%0", "%8", SH, M_LO, M_HI) LR_PAIR("%1", "%9", SH, M_LO, M_HI)                                \
        LR_PAIR("%2", "%10", SH, M_LO, M_HI) LR_PAIR("%3", "%11", SH, M_LO, M_HI) LR_PAIR("%4", "%12", SH, M_LO, M_HI)     \
        LR_PAIR("%5", "%13", SH, M_LO, M_HI) LR_PAIR("%6", "%14", SH, M_LO, M_HI) LR_PAIR("%7", "%15", SH, M_LO, M_HI)     \
        : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7])                    \
        : "v"(w[8]), "v"(w[9]), "v"(w[10]), "v"(w[11]), "v"(w[12]), "v"(w[13]), "v"(w[14]), "v"(w[15]));                    \
  else if constexpr (N == 8)                                                                                                  \
    asm("s_nop 1\n\t" LR_PAIR("%0", "%4", SH, M_LO, M_HI) LR_PAIR("%1", "%5", SH, M_LO, M_HI)                                \
        LR_PAIR("%2", "%6", SH, M_LO, M_HI) LR_PAIR("%3", "%7", SH, M_LO, M_HI)                                              \
        : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]) : "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7]));                     \
  else if constexpr (N == 4)                                                                                                  \
    asm("s_nop 1\n\t" LR_PAIR("%0", "%2", SH, M_LO, M_HI) LR_PAIR("%1", "%3", SH, M_LO, M_HI)                                \
        : "+v"(w[0]), "+v"(w[1]) : "v"(w[2]), "v"(w[3]));                                                                    \
  else if constexpr (N == 2)                                                                                                  \
    asm("s_nop 1\n\t" LR_PAIR("%0", "%1", SH, M_LO, M_HI) : "+v"(w[0]) : "v"(w[1]))

template <int N>
__device__ __forceinline__ void lr_level2(float *w) {  // lane ^ 4
  static_assert(N == 1 || N == 2 || N == 4 || N == 8 || N == 16, "");
  if constexpr (N == 1) {  // all-reduce step: the sum goes to a second register, the lower banks' results must not feed the upper
    float r;
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %0, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xa"
        : "=&v"(r) : "v"(w[0]));
    w[0] = r;
  } else {
    LR_LEVEL("4", "0x5", "0xa");
  }
}
template <int N>
__device__ __forceinline__ void lr_level3(float *w) {  // lane ^ 8
  static_assert(N == 1 || N == 2 || N == 4 || N == 8, "");
  if constexpr (N == 1) {
    asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf" : "+v"(w[0]));
  } else {
    LR_LEVEL("8", "0x3", "0xc");
  }
}
#undef LR_LEVEL
#undef LR_PAIR

// the two rows of each half wave: NR row totals in w -> row 0 + row 1 in w[0 .. max(NR / 2, 1)); v_permlane16_swap trades the
// odd rows of its first operand for the even rows of its second, a fifth transposing level
template <int NR>
__device__ __forceinline__ void lane_row_pair_sums(float *w) {
  static_assert(NR == 1 || NR == 2 || NR == 4, "");
  if constexpr (NR == 4) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3\n\ts_nop 1"
        : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
    w[0] += w[2]; w[1] += w[3];
  } else if constexpr (NR == 2) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(w[0]), "+v"(w[1]));
    w[0] += w[1];
  } else {
    float o;
    asm("v_mov_b32 %1, %0\n\ts_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(w[0]), "=&v"(o));
    w[0] += o;
  }
}

// ONE level on the N values a lane holds at it: w[0 .. N) -> w[0 .. max(N / 2, 1)).  A caller that forms its values in batches
// runs the first levels per batch, so that few values are live at a time (the SA chain's statistics, sa_chain.hip), and the
// later levels on what the batches leave; the value numbering is that of running every level on all values at once.
template <int LEVEL, int N>
__device__ __forceinline__ void lane_sum_level(float *w, int lane) {
  static_assert(LEVEL >= 0 && LEVEL <= 4, "");
  if constexpr (LEVEL == 0) lr_quad_level<N, 0xB1>(w, lane & 1);
  else if constexpr (LEVEL == 1) lr_quad_level<N, 0x4E>(w, lane & 2);
  else if constexpr (LEVEL == 2) lr_level2<N>(w);
  else if constexpr (LEVEL == 3) lr_level3<N>(w);
  else lane_row_pair_sums<N>(w);
}

// NV values in v -> the row totals in v[0 .. lane_row_regs(NV)); lane: the caller's lane number (0 .. 63)
template <int NV>
__device__ __forceinline__ void lane_row_sums(float (&v)[NV], int lane) {
  static_assert(NV == 4 || NV == 8 || NV == 16 || NV == 32 || NV == 64, "");
  lane_sum_level<0, NV>(v, lane);
  lane_sum_level<1, NV / 2>(v, lane);
  lane_sum_level<2, (NV >= 8 ? NV / 4 : 1)>(v, lane);
  lane_sum_level<3, (NV >= 16 ? NV / 8 : 1)>(v, lane);
}

// NV values in v -> the half-wave totals in v[0 .. lane_half_regs(NV))
template <int NV>
__device__ __forceinline__ void lane_half_sums(float (&v)[NV], int lane) {
  lane_row_sums<NV>(v, lane);
  lane_sum_level<4, lane_row_regs(NV)>(v, lane);
}

}  // namespace
