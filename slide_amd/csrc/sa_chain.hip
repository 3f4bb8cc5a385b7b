// sa_chain.hip -- the fused Mlp chain of an SA block (SLIDE_OP_SA_CHAIN, SLIDE_OP_SA_CHAIN_P; fp16): the two
// layers that follow the pair decomposition's first layer, whose input is generated from the pair tables as in gemm_gx.hip.
#include <cstdlib>

#include "gemm_common.h"
#include "gemm_small.h"
#include "lane_reduce.h"
#include "launch.h"

namespace {

// ================================================================================================ fused SA Mlp chain
// second_mlp -> rest_mlp of an SA block's Mlp_plus_t_emb (pointnet2_modules.py:119-176) in ONE launch, one workgroup per
// sample (16 x 16 rows, natural neighbour order), eight waves x 32 rows:
//   stage 1: h2 = relu(GN(W1 . h1 + b1)) + class-embedding vector, h1 GENERATED from the pair tables (mode 0 of gemm_gx.hip);
//            every wave owns ALL n1 channels of its 32 rows, so after the GroupNorm (statistics across the waves through
//            LDS) its accumulators, converted to fp16 and re-paired with v_permlane32_swap, ARE the MFMA B fragments of
//   stage 2: mo = relu(GN(W2 . h2 + b2)) + pair residual, in slabs of 256 channels, stored chunk-major for the attention tail.
// h2 never exists in memory; one weight ring (16 KB chunk images of 256 channels x 32 K) streams W1 then the slabs of W2 and
// keeps running ahead across the epilogues.  GroupNorm group sizes 4 / 8 / 16 (widths 128 / 256 / 512).
struct F1Args {
  const void *ta, *tb, *ra, *rb;  // fp16 pair tables [B*16][t_ld]: first_mlp columns (pre-normalised), res_connect columns
  const void *W1, *W2;            // chunk-major [k1/32][n1][32], [n1/32][n2][32]
  const float *vec1, *vec2;       // [bias | gamma | beta][n]
  const float *add0;              // h1 add vector (t-embedding): add0[idx * add0_stride + b * add0_bs + k] or NULL
  const int *add0_idx;
  const float *add1;              // h2 add vector (class embedding): add1[b * add1_bs + c] or NULL
  void *out;                      // mo, chunk-major [n2/32][B*256][32] fp16
  unsigned long long *dbg;
  int B, t_ld, k1, n1, n2, gs1, gs2, add0_stride, add0_bs, add1_bs;
  float inv1, inv2;
  int out_fm;  // round 6: out is fragment-major (SLIDE_F_OUT_FM)
  int nsplit;  // round 6: workgroups per sample (1 | 2): each takes n2 / 256 / nsplit of the stage-2 slabs (stage 1 is computed by all)
};

// workgroup barrier that orders LDS traffic only: __syncthreads() would also drain the VM counter, i.e. wait for the weight
// ring's DMA in flight (and for the epilogue's own stores)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int NB1>  // 32-channel blocks of h2 (4 or 8)
__device__ __forceinline__ void sa_chain_body(const F1Args &a, const int bid) {
  using T = _Float16;
  constexpr int NB2 = 8;                       // blocks per stage-2 slab
  constexpr int CH_B = 256 * 64, STAGE_B = 2 * CH_B, NST = 2;
  constexpr int NR = 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // SLAB SPLIT (round 6): with few samples per launch (one 8-wave workgroup per sample: 88 of 256 CUs at bench.py's sub-batch size)
  // a sample's stage-2 slabs go to nsplit workgroups -- each repeats stage 1 (a third of the chain's FLOPs at n2 = 512) and runs
  // its own slabs: 1.5x the matrix work per sample on twice the CUs, a shorter critical path for the chain that waits on this launch
  const int b = bid / a.nsplit, sl0 = (bid % a.nsplit) * ((a.n2 >> 8) / a.nsplit);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, col = lane & 31;
  const int nk1 = a.k1 >> 5, nk2 = (NB1 * 32) >> 5, nslab = (a.n2 >> 8) / a.nsplit;
  const int nchunks = nk1 + nslab * nk2, nks = nchunks >> 1;  // (nk1, nk2 even)
  unsigned char *const ring = smem_raw;
  float *const vec1_l = reinterpret_cast<float *>(smem_raw + (size_t)NST * STAGE_B);  // [3][n1]
  float *const vec2_l = vec1_l + 3 * a.n1;                                            // [3][n2]
  float *const add1_l = vec2_l + 3 * a.n2;                                            // [n1]
  float *const red = add1_l + a.n1;                                                   // [8 waves][2 halves][64 values]
  float *const gsh = red + 8 * 8 * 2 * 4 * 2;                                         // [8 cb][2][32]
  T *const add0_l = reinterpret_cast<T *>(gsh + 8 * 2 * 32);                          // [k1] fp16
  unsigned char *const ta_l = reinterpret_cast<unsigned char *>(add0_l + a.k1);
  const int tab_b = (a.k1 >> 3) * NR * 16;
  unsigned char *const tb_l = ta_l + tab_b;
  unsigned char *const ra_l = tb_l + tab_b;                 // res_connect tables, same image: [piece][16 rows][16 B]
  unsigned char *const rb_l = ra_l + (a.n2 >> 3) * NR * 16;
#ifdef SLIDE_TIMELINE
  if (a.dbg && tid == 0) a.dbg[(size_t)b * 16 + 0] = wall_clock64();
#define F1_STAMP(k) do { if (a.dbg && tid == 0) a.dbg[(size_t)b * 16 + (k)] = wall_clock64(); } while (0)
#else
#define F1_STAMP(k) do { } while (0)
#endif

  // ---- pair tables by LDS-DMA: [piece][16 rows][16 B]; one instruction = 4 pieces x 16 rows
  {
    const int r = lane & 15, pl = lane >> 4;
    const size_t grow = ((size_t)b * 16 + r) * a.t_ld;
    const int nins = (a.k1 >> 3) / 4;
    for (int i = wave; i < 2 * nins; i += 8) {
      const int t = i >= nins, ii = t ? i - nins : i;
      const T *src = reinterpret_cast<const T *>(t ? a.tb : a.ta) + grow + (ii * 4 + pl) * 8;
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)src,
                                       (__attribute__((address_space(3))) void *)((t ? tb_l : ta_l) + ii * 1024), 16, 0, 0);
    }
    const int rins = (a.n2 >> 3) / 4;
    for (int i = wave; i < 2 * rins; i += 8) {
      const int t = i >= rins, ii = t ? i - rins : i;
      const T *src = reinterpret_cast<const T *>(t ? a.rb : a.ra) + grow + (ii * 4 + pl) * 8;
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)src,
                                       (__attribute__((address_space(3))) void *)((t ? rb_l : ra_l) + ii * 1024), 16, 0, 0);
    }
  }
  // ---- weight ring: chunk g = W1 chunk g (g < nk1) or chunk (g - nk1) % nk2 of slab (g - nk1) / nk2 of W2; image [256][64 B]
  // 16 DMA instructions per chunk, 2 per wave: instruction j * 8 + wave carries image rows 16 (j * 8 + wave) ..
  int wtrow[2], wpiece[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    wtrow[j] = 16 * (j * 8 + wave) + (lane >> 2);
    wpiece[j] = (lane & 3) ^ ((wtrow[j] >> 2) & 3);
  }
  auto issue = [&](int st) __attribute__((always_inline)) {
    unsigned char *dst = ring + (size_t)(st % NST) * STAGE_B;
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const int g = st * 2 + c2;
      const T *base;
      int nrow, kc, r0;
      if (g < nk1) { base = reinterpret_cast<const T *>(a.W1); nrow = a.n1; kc = g; r0 = 0; }
      else {
        const int h = g - nk1, sl = h / nk2;
        base = reinterpret_cast<const T *>(a.W2); nrow = a.n2; kc = h - sl * nk2; r0 = (sl0 + sl) * 256;
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int row = r0 + wtrow[j];
        row = row < nrow ? row : nrow - 1;  // (stage 1 with n1 = 128: the image's upper half is never read)
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)(base + ((size_t)kc * nrow + row) * 32 + wpiece[j] * 8),
                                         (__attribute__((address_space(3))) void *)(dst + c2 * CH_B + (j * 8 + wave) * 1024),
                                         16, 0, 0);
      }
    }
  };
  issue(0);
  // ---- vectors.  PROLOGUE ORDER (round 6): the table DMAs and the first ring stage above are in flight before anything waits; the fp32
  // vectors go by LDS-DMA as well (four bytes per lane), only the t-embedding row (fp16 in LDS, behind a device-side row index) takes
  // plain loads -- one memory round trip + the index instead of four in a row (timeline "prologue": 1.8 - 2.3 us, and the first stage's
  // wait behind it)
  {
    const int w64 = wave * 64;
    auto dma4 = [&](const float *src, float *dst, int n) __attribute__((always_inline)) {
      for (int i0 = w64; i0 < n; i0 += 512)
        if (i0 + lane < n)
          __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)(src + i0 + lane), (__attribute__((address_space(3))) void *)(dst + i0), 4, 0, 0);
    };
    dma4(a.vec1, vec1_l, 3 * a.n1);
    dma4(a.vec2, vec2_l, 3 * a.n2);
    if (a.add1) dma4(a.add1 + (size_t)b * a.add1_bs, add1_l, a.n1);
    else for (int i = tid; i < a.n1; i += 512) add1_l[i] = 0.f;
  }
  {
    const float *addp = a.add0;
    if (addp && a.add0_idx) addp += (size_t)a.add0_idx[0] * a.add0_stride;
    for (int i = tid; i < a.k1; i += 512) add0_l[i] = (T)(addp ? addp[(size_t)b * a.add0_bs + i] : 0.f);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  F1_STAMP(14);
  // stage st must have landed before anyone reads it (NST = 2: nothing else is in flight)
  auto stage_ready = [&](int st) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (st + 1 < nks) issue(st + 1);  // overwrites the stage consumed at st - 1
  };

  // this wave's 32 rows: points 2 wave, 2 wave + 1; neighbour q = col & 15
  const int aoff = (half * NR + (col & 15)) * 16, boff = (half * NR + 2 * wave + (col >> 4)) * 16;
  int wrow[NB2], wkey[NB2];
#pragma unroll
  for (int cb = 0; cb < NB2; ++cb) {
    const int trow = cb * 32 + col;
    wrow[cb] = trow * 64; wkey[cb] = (trow >> 2) & 3;
  }

  // ================================================================================================ stage 1
  // accumulators start from the bias: the LDS reads land in the accumulator registers, the epilogue has no bias pass
  auto init_acc = [&](auto nb_tag, f32x16 *v, const float *bias_l) __attribute__((always_inline)) {
    constexpr int NB = decltype(nb_tag)::value;
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bia = *reinterpret_cast<const float4 *>(bias_l + cb * 32 + 8 * q + 4 * half);
        v[cb][4 * q] = bia.x; v[cb][4 * q + 1] = bia.y; v[cb][4 * q + 2] = bia.z; v[cb][4 * q + 3] = bia.w;
      }
  };
  f32x16 acc1[NB1];
  struct Step1 { f16x8 af[NB1], av, bv; int kb; };
  auto load1 = [&](Step1 &o, const unsigned char *sb, int c2, int st2, int kc) __attribute__((always_inline)) {
    const int piece = st2 * 2 + half;
#pragma unroll
    for (int cb = 0; cb < NB1; ++cb)
      o.af[cb] = *reinterpret_cast<const f16x8 *>(sb + c2 * CH_B + wrow[cb] + ((piece ^ wkey[cb]) << 4));
    const int pb = (kc * 4 + st2 * 2) * NR * 16;
    o.kb = (kc * 32 + st2 * 16 + half * 8) * 2;
    o.av = *reinterpret_cast<const f16x8 *>(ta_l + pb + aoff);
    o.bv = *reinterpret_cast<const f16x8 *>(tb_l + pb + boff);
  };
  auto compute1 = [&](const Step1 &o) __attribute__((always_inline)) {
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const f16x8 v0 = *reinterpret_cast<const f16x8 *>(reinterpret_cast<const unsigned char *>(add0_l) + o.kb);
    const f16x8 bf = __builtin_elementwise_max(o.av + o.bv, zero) + v0;
#pragma unroll
    for (int cb = 0; cb < NB1; ++cb) acc1[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(o.af[cb], bf, acc1[cb], 0, 0, 0);
  };
  const int nks1 = nk1 >> 1;
  {
    Step1 cur, nxt;
    stage_ready(0);  // (its barrier publishes the vectors staged above)
    init_acc(std::integral_constant<int, NB1>(), acc1, vec1_l);
    load1(cur, ring, 0, 0, 0);
    for (int st = 0; st < nks1; ++st) {
      const unsigned char *sb = ring + (size_t)(st % NST) * STAGE_B;
      load1(nxt, sb, 0, 1, st * 2);
      compute1(cur);
      load1(cur, sb, 1, 0, st * 2 + 1);
      compute1(nxt);
      load1(nxt, sb, 1, 1, st * 2 + 1);
      compute1(cur);
      if (st + 1 < nks1) {
        stage_ready(st + 1);
        load1(cur, ring + (size_t)((st + 1) % NST) * STAGE_B, 0, 0, st * 2 + 2);
      }
      compute1(nxt);
    }
  }
  F1_STAMP(1);
  // (the ring runs one stage ahead: stage_ready(s) issued stage s + 1, so the first chunks of W2 land under the epilogue below)

  // GroupNorm of a stage: acc blocks v[NB] (D layout: reg r -> channel (r & 3) + 8 (r >> 2) + 4 half of the block, lane col ->
  // row; bias included since the accumulator init); statistics over the sample's 256 rows x gs channels.  Leaves per-channel
  // scale / shift in gsh.  Written on register PAIRS (packed fp32 VALU ops): these epilogues are VALU-issue bound.
  // The sums over the wave's 32 rows go through the transposing lane reduction (lane_reduce.h): value q (NB * 2) + 2 cb + {0: sum,
  // 1: sum of squares} of channel quad q (its pair of quads for groups of 16, folded BEFORE the reduction) of block cb.  The
  // accumulators and stage 2's B fragments leave some forty registers, so the values are formed two quads at a time and the
  // levels that pair the quads of a block, then blocks cb and cb + NB / 2, run as soon as their operands exist, each step
  // behind a scheduling barrier: a dozen values are live at a time, not 64.  The last levels run on the NB values left; every
  // lane then holds one or two totals of its half wave and all 64 store them at once: red[wave][half][value].
  auto stats_reduce = [&](auto nb_tag, auto fold_tag, const f32x16 *v) __attribute__((always_inline)) {
    constexpr int NB = decltype(nb_tag)::value, NQ = decltype(fold_tag)::value ? 2 : 4, NV = NB * NQ * 2;
    // {sum, sum of squares} of quads qa and qb of a block over the lane's 16 channels x 1 row -> o[0 .. 4)
    auto quad_pair = [&](const f32x16 &a, int qa, int qb, float *o) __attribute__((always_inline)) {
      f32x2 t[2], tt[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int q = k ? qb : qa;
        const f32x2 lo = {a[4 * q], a[4 * q + 1]}, hi = {a[4 * q + 2], a[4 * q + 3]};
        t[k] = lo + hi;
        tt[k] = __builtin_elementwise_fma(hi, hi, lo * lo);
      }
      o[0] = t[0][0]; o[1] = tt[0][0]; o[2] = t[1][0]; o[3] = tt[1][0];
      // o += the upper halves: written out, or the compiler packs pairs of these adds and spends three register moves on each
      // pair.  (A DPP add reads these next, two wait states behind a VALU write: the compiler pads an asm statement's outputs.)
      asm("v_add_f32 %0, %0, %4\n\tv_add_f32 %1, %1, %5\n\tv_add_f32 %2, %2, %6\n\tv_add_f32 %3, %3, %7"
          : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]) : "v"(t[0][1]), "v"(tt[0][1]), "v"(t[1][1]), "v"(tt[1][1]));
    };
    // the two values a block leaves after the levels inside it
    auto block_sums = [&](const f32x16 &a, float *o) __attribute__((always_inline)) {
      float w[4], x[4];
      if constexpr (NQ == 2) {
        quad_pair(a, 0, 1, w);
        o[0] = w[0] + w[2]; o[1] = w[1] + w[3];
        __builtin_amdgcn_sched_barrier(0);
        quad_pair(a, 2, 3, x);
        o[2] = x[0] + x[2]; o[3] = x[1] + x[3];
        lane_sum_level<0, 4>(o, lane);
      } else {
        quad_pair(a, 0, 2, w);
        lane_sum_level<0, 4>(w, lane);
        __builtin_amdgcn_sched_barrier(0);
        quad_pair(a, 1, 3, x);
        lane_sum_level<0, 4>(x, lane);
        o[0] = w[0]; o[1] = w[1]; o[2] = x[0]; o[3] = x[1];
        lane_sum_level<1, 4>(o, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    float p[NB];
#pragma unroll
    for (int k = 0; k < NB / 2; ++k) {
      float w[4], x[4];
      block_sums(v[k], w);
      block_sums(v[k + NB / 2], x);
      w[2] = x[0]; w[3] = x[1];
      lane_sum_level<(NQ == 2 ? 1 : 2), 4>(w, lane);
      p[2 * k] = w[0]; p[2 * k + 1] = w[1];
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (NQ == 2) {
      lane_sum_level<2, NB>(p, lane);
      lane_sum_level<3, NB / 2>(p, lane);
      lane_sum_level<4, (NB == 8 ? 2 : 1)>(p, lane);
    } else {
      lane_sum_level<3, NB>(p, lane);
      lane_sum_level<4, NB / 2>(p, lane);
    }
    float *dst = red + (wave * 2 + half) * 64 + lane_reduce_index<NV>(lane);
    if constexpr (lane_half_regs(NV) == 2) *reinterpret_cast<f32x2 *>(dst) = f32x2{p[0], p[1]};
    else *dst = p[0];
  };
  auto group_stats = [&](auto nb_tag, f32x16 *v, const float *vec_l, int cb_base, int n, int gs, float inv_count) __attribute__((always_inline)) {
    constexpr int NB = decltype(nb_tag)::value;
    if (gs == 16) stats_reduce(nb_tag, std::true_type(), v);
    else stats_reduce(nb_tag, std::false_type(), v);
    lds_barrier();
    // one wave per channel block: channel c = lane (lower half), sums its group's partials over the 8 waves
    if (wave < NB && half == 0) {
      const int cb = wave, c = col, q = c >> 3, hh = (c >> 2) & 1;
      f32x2 t = {0.f, 0.f};
      const int vi = (gs == 16 ? q >> 1 : q) * (NB * 2) + 2 * cb;  // the group's value number (stats_reduce)
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        const float *pw = red + w * 128 + vi;
        if (gs == 4) t += *reinterpret_cast<const f32x2 *>(pw + hh * 64);
        else t += *reinterpret_cast<const f32x2 *>(pw) + *reinterpret_cast<const f32x2 *>(pw + 64);
      }
      const float mean = t[0] * inv_count;
      const float var = fmaxf(t[1] * inv_count - mean * mean, 0.f);
      const float g = vec_l[n + (cb_base + cb) * 32 + c] * __builtin_amdgcn_rsqf(var + GN_EPS);
      gsh[(cb * 2 + 0) * 32 + c] = g;
      gsh[(cb * 2 + 1) * 32 + c] = vec_l[2 * n + (cb_base + cb) * 32 + c] - mean * g;
    }
    lds_barrier();
  };
  // normalise block cb (fp32, packed), convert to fp16, ReLU on the packed halves, [+ addp: 16 fp32 per lane in the D layout's
  // channel order], and re-pair between the lane halves: o[p] = the 8 consecutive channels 16 p + 8 half of the lane's row
  auto norm_pack = [&](const f32x16 &v, int cb, const float *addp, f16x8 (&o)[2]) __attribute__((always_inline)) {
    uint32_t u[8];
    const f16x2 zero2 = {0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 g = *reinterpret_cast<const float4 *>(gsh + (cb * 2 + 0) * 32 + 8 * q + 4 * half);
      const float4 sh = *reinterpret_cast<const float4 *>(gsh + (cb * 2 + 1) * 32 + 8 * q + 4 * half);
      f32x2 lo = __builtin_elementwise_fma(f32x2{v[4 * q], v[4 * q + 1]}, f32x2{g.x, g.y}, f32x2{sh.x, sh.y});
      f32x2 hi = __builtin_elementwise_fma(f32x2{v[4 * q + 2], v[4 * q + 3]}, f32x2{g.z, g.w}, f32x2{sh.z, sh.w});
      f16x2 l2 = __builtin_elementwise_max(__builtin_convertvector(lo, f16x2), zero2);
      f16x2 h2 = __builtin_elementwise_max(__builtin_convertvector(hi, f16x2), zero2);
      if (addp) {
        const float4 ad = *reinterpret_cast<const float4 *>(addp + 8 * q + 4 * half);
        l2 += __builtin_convertvector(f32x2{ad.x, ad.y}, f16x2);
        h2 += __builtin_convertvector(f32x2{ad.z, ad.w}, f16x2);
      }
      u[2 * q] = __builtin_bit_cast(uint32_t, l2);
      u[2 * q + 1] = __builtin_bit_cast(uint32_t, h2);
    }
    // quads 2p (u[4p], u[4p+1]) <-> 2p + 1 (u[4p+2], u[4p+3]) across the lane halves: four swaps behind one hazard pad
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %2\n\tv_permlane32_swap_b32 %1, %3\n\t"
                 "v_permlane32_swap_b32 %4, %6\n\tv_permlane32_swap_b32 %5, %7\n\ts_nop 1"
                 : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]), "+v"(u[6]), "+v"(u[7]));
    o[0] = __builtin_bit_cast(f16x8, u32x4{u[0], u[1], u[2], u[3]});
    o[1] = __builtin_bit_cast(f16x8, u32x4{u[4], u[5], u[6], u[7]});
  };

  group_stats(std::integral_constant<int, NB1>(), acc1, vec1_l, 0, a.n1, a.gs1, a.inv1);
  f16x8 h2b[2 * NB1];  // B fragments of stage 2: K block kb of 16 channels, this lane's row
#pragma unroll
  for (int cb = 0; cb < NB1; ++cb) {
    f16x8 o[2];
    norm_pack(acc1[cb], cb, add1_l + cb * 32, o);
    h2b[2 * cb] = o[0]; h2b[2 * cb + 1] = o[1];
  }
  F1_STAMP(2);

  // ================================================================================================ stage 2
  const size_t R = (size_t)a.B * 256;
  const int row = b * 256 + wave * 32 + col;
  const int raoff = (col & 15) * 16, rboff = (2 * wave + (col >> 4)) * 16;  // this lane's rows inside a piece of the residual tables
  for (int sli = 0; sli < nslab; ++sli) {
    const int sl = sl0 + sli;  // the slab's position in the layer; sli: its position in this workgroup's ring sequence
    f32x16 acc2[NB2];
    init_acc(std::integral_constant<int, NB2>(), acc2, vec2_l + sl * 256);
    const int st0 = nks1 + sli * (nk2 >> 1);  // first ring stage of this slab
    f16x8 afc[NB2], afn[NB2];
    auto loadw = [&](f16x8 (&o)[NB2], const unsigned char *sb, int c2, int st2) __attribute__((always_inline)) {
      const int piece = st2 * 2 + half;
#pragma unroll
      for (int cb = 0; cb < NB2; ++cb)
        o[cb] = *reinterpret_cast<const f16x8 *>(sb + c2 * CH_B + wrow[cb] + ((piece ^ wkey[cb]) << 4));
    };
    stage_ready(st0);
    loadw(afc, ring + (size_t)(st0 % NST) * STAGE_B, 0, 0);
#pragma unroll
    for (int s2 = 0; s2 < NB1 / 2; ++s2) {  // ring stages of the slab: 4 K steps of 16 each (K blocks 4 s2 .. 4 s2 + 3)
      const unsigned char *sb = ring + (size_t)((st0 + s2) % NST) * STAGE_B;
      loadw(afn, sb, 0, 1);
#pragma unroll
      for (int cb = 0; cb < NB2; ++cb) acc2[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afc[cb], h2b[4 * s2], acc2[cb], 0, 0, 0);
      loadw(afc, sb, 1, 0);
#pragma unroll
      for (int cb = 0; cb < NB2; ++cb) acc2[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afn[cb], h2b[4 * s2 + 1], acc2[cb], 0, 0, 0);
      loadw(afn, sb, 1, 1);
#pragma unroll
      for (int cb = 0; cb < NB2; ++cb) acc2[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afc[cb], h2b[4 * s2 + 2], acc2[cb], 0, 0, 0);
      if (s2 + 1 < NB1 / 2) {
        stage_ready(st0 + s2 + 1);
        loadw(afc, ring + (size_t)((st0 + s2 + 1) % NST) * STAGE_B, 0, 0);
      }
#pragma unroll
      for (int cb = 0; cb < NB2; ++cb) acc2[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afn[cb], h2b[4 * s2 + 3], acc2[cb], 0, 0, 0);
    }
    F1_STAMP(3 + 3 * sli);
    group_stats(std::integral_constant<int, NB2>(), acc2, vec2_l, sl * NB2, a.n2, a.gs2, a.inv2);
    F1_STAMP(4 + 3 * sli);
#pragma unroll
    for (int cb = 0; cb < NB2; ++cb) {
      const int cg = sl * 256 + cb * 32;
      f16x8 ra4[2], rb4[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int pc = ((cg + 16 * p) >> 3) + half;  // 16-byte piece of channels cg + 16 p + 8 half ..
        ra4[p] = *reinterpret_cast<const f16x8 *>(ra_l + pc * NR * 16 + raoff);
        rb4[p] = *reinterpret_cast<const f16x8 *>(rb_l + pc * NR * 16 + rboff);
      }
      f16x8 o[2];
      norm_pack(acc2[cb], cb, nullptr, o);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const f16x8 y = o[p] + (ra4[p] + rb4[p]);
        // (chunk-major rows, or FRAGMENT-major: SLIDE_F_OUT_FM, include/slide_engine.h -- 1 KB of consecutive memory per instruction)
        const size_t o16 = a.out_fm ? (size_t)(row & ~31) * 32 + p * 512 + half * 256 + (row & 31) * 8 : (size_t)row * 32 + 16 * p + 8 * half;
        *reinterpret_cast<u32x4 *>(reinterpret_cast<T *>(a.out) + (size_t)(cg >> 5) * R * 32 + o16) = __builtin_bit_cast(u32x4, y);
      }
    }
    F1_STAMP(5 + 3 * sli);
  }
#ifdef SLIDE_TIMELINE
  if (a.dbg) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    F1_STAMP(15);
  }
#endif
}

template <int NB1>
__global__ __launch_bounds__(512, 2) void sa_chain_kernel(F1Args a) {
  sa_chain_body<NB1>(a, blockIdx.x);
}

// The fused Mlp chain of an SA block AND the per-point query GEMM of its attention (weight_conv.2's query half with the joint
// GroupNorm finalisation: gemm_small.h, AFF form) in ONE launch (SLIDE_OP_SA_CHAIN_P): both depend on the block's pair tables
// only and nothing on each other.  Blocks [0, grid_sa) run the chain (eight waves); the others run one 64 x 64 tile of the
// query GEMM on their first four waves (the other four exit).  The query GEMM's ~10 us launch + gap disappear under the chain.
template <int NB1>
__global__ __launch_bounds__(512, 2) void sa_chain_p_kernel(F1Args a, GemmArgs g, int grid_sa) {
  if ((int)blockIdx.x < grid_sa) {
    sa_chain_body<NB1>(a, blockIdx.x);
    return;
  }
  if (threadIdx.x >= 256) return;
  small_body<2, true, 0>(g, PairArgs(), (int)blockIdx.x - grid_sa);
}

}  // namespace

// SLIDE_OP_SA_CHAIN (include/slide_engine.h)
static int sa_args_from_op(const SlideOp &o, F1Args &a, size_t &shm) {
  a = F1Args();
  a.ta = o.p[0]; a.tb = o.p[1]; a.ra = o.p[2]; a.rb = o.p[3]; a.W1 = o.p[4]; a.W2 = o.p[5];
  a.vec1 = (const float *)o.p[6]; a.vec2 = (const float *)o.p[7];
  a.add0 = (const float *)o.p[8]; a.add0_idx = (const int *)o.p[9]; a.add1 = (const float *)o.p[10]; a.out = o.p[11];
  a.dbg = (unsigned long long *)o.p[12];
  a.B = o.i[0]; a.t_ld = o.i[1]; a.k1 = o.i[2]; a.n1 = o.i[3]; a.n2 = o.i[4]; a.gs1 = o.i[5]; a.gs2 = o.i[6];
  a.add0_stride = o.i[7]; a.add0_bs = o.i[8]; a.add1_bs = o.i[9];
  a.inv1 = o.f[0]; a.inv2 = o.f[1];
  a.out_fm = o.f[2] != 0.f;
  // OPT-IN (SLIDE_SA_SPLIT_MAX=<samples>: two workgroups per sample for launches of at most that many samples).  Measured in bench.py's
  // arrangement (tools/ab/r06_split.sh, three alternating pairs, --steps 300): 379.1 shapes/s with the split at 88 samples per launch
  // against 387.5 without -- the launch itself gets shorter, but the arrangement is bound by CU-time, not by this launch's latency,
  // and the repeated stage 1 is 1.33x the chain's matrix work.
  static const bool no_split = getenv("SLIDE_SA_SPLIT") && getenv("SLIDE_SA_SPLIT")[0] == '0';
  static const int split_max = getenv("SLIDE_SA_SPLIT_MAX") ? atoi(getenv("SLIDE_SA_SPLIT_MAX")) : 0;
  a.nsplit = (!no_split && (a.n2 >> 8) % 2 == 0 && a.B <= split_max) ? 2 : 1;
  if (a.B <= 0 || a.k1 % 64 || a.k1 <= 0 || (a.n1 != 128 && a.n1 != 256) || a.n2 % 256 || a.n2 <= 0 || a.t_ld % 8) return -3;
  auto okgs = [](int g) { return g == 4 || g == 8 || g == 16; };
  if (!okgs(a.gs1) || !okgs(a.gs2)) return -3;
  shm = (size_t)2 * 32768 + (size_t)(3 * a.n1 + 3 * a.n2 + a.n1 + 8 * 8 * 2 * 4 * 2 + 8 * 2 * 32) * 4 +
        (size_t)a.k1 * 2 + (size_t)2 * (a.k1 >> 3) * 16 * 16 + (size_t)2 * (a.n2 >> 3) * 16 * 16 + 64;
  if (shm > 160 * 1024) return -8;
  return 0;
}

// SLIDE_OP_SA_CHAIN_P: p[0] = HOST pointer to two SlideOp: the SLIDE_OP_SA_CHAIN and the SLIDE_OP_GEMM of the per-point query
// layer (16 rows per sample, fp16, input affine + statistics finalisation: the small-launch kernel's AFF form)
int slide_launch_sa_chain_p(const SlideOp &o, hipStream_t s) {
  const SlideOp *pr = (const SlideOp *)o.p[0];
  if (!pr || pr[0].kind != SLIDE_OP_SA_CHAIN || pr[1].kind != SLIDE_OP_GEMM) return -3;
  F1Args a;
  size_t shm_sa = 0;
  const int st = sa_args_from_op(pr[0], a, shm_sa);
  if (st != 0) return st;
  const SlideOp &q = pr[1];
  GemmArgs g = GemmArgs();
  g.X = q.p[0]; g.W = q.p[1]; g.epi = (const SlideEpi *)q.p[2];
  g.in_scale = (const float *)q.p[3]; g.in_shift = (const float *)q.p[4];
  g.gn_fin = (const SlideGnFin *)q.p[6];
  g.aff_tps = 1;
  g.rows = q.i[0]; g.x_ld = q.i[1]; g.k_pad = q.i[2]; g.n_cob = q.i[3]; g.in_bs = q.i[5];
  resolve_epi(g);
  if (q.i[4] != 4 || q.i[6] != SLIDE_PREC_F16 || (q.i[8] & 6) || !g.in_scale || !g.in_shift || q.p[8] || q.p[9] ||
      q.p[10] || q.p[11] || g.k_pad % 32 || g.x_ld % 8 || g.rows != a.B * 16 || g.n_cob <= 0)
    return -3;
  const int grid_p = ((g.rows + 63) / 64) * ((g.n_cob + 1) / 2);
  const size_t shm_p = (size_t)4 * 2 * 6144 + 2 * (sizeof(SlideEpi) + 96 * 4) + 32 + (size_t)4 * 2 * g.k_pad * 2 + 1024;
  const size_t shm = shm_sa > shm_p ? shm_sa : shm_p;
  if (a.n1 == 128) {
    allow_dynamic_lds<&sa_chain_p_kernel<4>>(160 * 1024);
    hipLaunchKernelGGL((sa_chain_p_kernel<4>), dim3(a.B * a.nsplit + grid_p), dim3(512), shm, s, a, g, a.B * a.nsplit);
  } else {
    allow_dynamic_lds<&sa_chain_p_kernel<8>>(160 * 1024);
    hipLaunchKernelGGL((sa_chain_p_kernel<8>), dim3(a.B * a.nsplit + grid_p), dim3(512), shm, s, a, g, a.B * a.nsplit);
  }
  return (int)hipGetLastError();
}

int slide_launch_sa_chain(const SlideOp &o, hipStream_t s) {
  F1Args a;
  size_t shm = 0;
  const int ast = sa_args_from_op(o, a, shm);
  if (ast != 0) return ast;
  if (a.n1 == 128) {
    allow_dynamic_lds<&sa_chain_kernel<4>>(160 * 1024);
    hipLaunchKernelGGL((sa_chain_kernel<4>), dim3(a.B * a.nsplit), dim3(512), shm, s, a);
  } else {
    allow_dynamic_lds<&sa_chain_kernel<8>>(160 * 1024);
    hipLaunchKernelGGL((sa_chain_kernel<8>), dim3(a.B * a.nsplit), dim3(512), shm, s, a);
  }
  return (int)hipGetLastError();
}
