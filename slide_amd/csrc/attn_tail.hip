// attn_tail.hip -- the fused attention tails of the latent-DDPM denoiser for gfx950 (SLIDE_OP_ATTN_TAIL, fp16;
// include/slide_engine.h; the split-arithmetic tail is in gemm_gxs.hip).
#include "gemm_common.h"
#include "launch.h"

#include <cstdlib>

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

__device__ __forceinline__ float other_half(float x) {  // value of lane ^ 32
  uint32_t a = __float_as_uint(x), b = a;
  lane32_swap(a, b);  // a = [x.lo | x.lo in the upper lanes], b = [x.hi in the lower lanes | x.hi]
  return __uint_as_float((threadIdx.x & 32) ? a : b);
}

// The epilogue of the fused attention tail on the two accumulator sets (values: bias, GroupNorm over the sample, ReLU; scores: bias,
// soft-max over a point's K rows; weighted sum, one row out per point).  vec_lds: [bias_s | bias_v | gamma | beta] of the tile's 64
// channels of THIS wave (vstride floats apart), red: 2 KB of scratch shared by the waves of one channel group, wave: the row wave
// (rows 64 wave ..); vectors / scratch must be visible / free on entry (the callers end their K loops with a workgroup barrier).
template <int NPXL>
__device__ __forceinline__ void attn_tail_finish(const AttnTailArgs &a, f32x16 (&sacc)[2][2], f32x16 (&vacc)[2][2], const float *vec_lds,
                                                 int vstride, float *red, int row0, int cob0, int wave) {
  // Round 6: the per-workgroup timeline (tools/ab/op_timeline.py) put 4.4 - 6.1 us of a tail workgroup's 11 - 21 us into this epilogue,
  // VALU-issue-bound (~1340 issue slots per wave).  Rewritten on register PAIRS (accumulator registers 2 i, 2 i + 1 are rows of one
  // point: v_pk_add / v_pk_fma_f32), log2(e) folded into the score bias step (exp2 of a difference: no multiply per value), one
  // v_rcp per output instead of an IEEE division, ONE lane-half exchange for numerator and denominator together, store addresses as
  // scalar base + one per-lane offset.
  using T = _Float16;
  constexpr int CBW = 2;
  constexpr int KLOG = NPXL - 4, KN = 1 << KLOG, GPB = 32 / KN;
  constexpr int WPS = (1 << NPXL) / 64;
  constexpr float LOG2E = 1.44269504088896340736f;
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  auto pr = [](const f32x16 &v, int i) __attribute__((always_inline)) { return f32x2{v[2 * i], v[2 * i + 1]}; };

  // ---- values: bias, GroupNorm over the sample (rows of WPS waves x the gs adjacent channel lanes), ReLU
  // red: [wave][cb][32 channels][sum, sumsq]
  const float *b_s = vec_lds, *b_v = vec_lds + vstride, *gam = vec_lds + 2 * vstride, *bet = vec_lds + 3 * vstride;
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const float bv = b_v[cb * 32 + col];
    const f32x2 bv2 = {bv, bv};
    f32x2 s2 = {0.f, 0.f}, ss2 = {0.f, 0.f};
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x2 x = pr(vacc[cb][rb], i) + bv2;
        vacc[cb][rb][2 * i] = x[0]; vacc[cb][rb][2 * i + 1] = x[1];
        s2 += x;
        ss2 = __builtin_elementwise_fma(x, x, ss2);
      }
    float s = s2[0] + s2[1], ss = ss2[0] + ss2[1];
    s += other_half(s);
    ss += other_half(ss);
    if (half == 0) *reinterpret_cast<f32x2 *>(red + ((wave * CBW + cb) * 32 + col) * 2) = f32x2{s, ss};
  }
  __syncthreads();
  const int w0 = (wave / WPS) * WPS;
  // output row of the wave's first point: scalar base + the lane's channel (bytes)
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const int pt0 = (row0 + wave_s * 64) >> KLOG, npts = a.rows >> KLOG;
  const uint32_t lofs = (uint32_t)col * 2;
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    f32x2 t = {0.f, 0.f};
#pragma unroll
    for (int w = 0; w < WPS; ++w) t += *reinterpret_cast<const f32x2 *>(red + (((w0 + w) * CBW + cb) * 32 + col) * 2);
    float s = t[0], ss = t[1];
    // the gs channels of a group sit in gs adjacent lanes (physical GroupNorm layout: power-of-two runs)
    if (a.gs >= 2) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0xB1, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0xB1, 0xF, 0xF, true)); }
    if (a.gs >= 4) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x4E, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x4E, 0xF, 0xF, true)); }
    if (a.gs >= 8) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x141, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x141, 0xF, 0xF, true)); }
    if (a.gs >= 16) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x140, 0xF, 0xF, true));
                      ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x140, 0xF, 0xF, true)); }
    if (a.gs >= 32) { s += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(s), 0x401F));
                      ss += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(ss), 0x401F)); }
    const float mean = s * a.inv_count;
    const float var = fmaxf(ss * a.inv_count - mean * mean, 0.f);
    float g = gam[cb * 32 + col] * __builtin_amdgcn_rsqf(var + GN_EPS);
    float bt = bet[cb * 32 + col] - mean * g;
    if ((cob0 + cb) * 32 + col >= a.n_norm) { g = 1.f; bt = 0.f; }
    const float bsl = b_s[cb * 32 + col] * LOG2E;
    const f32x2 g2 = {g, g}, bt2 = {bt, bt}, bs2 = {bsl, bsl}, l2 = {LOG2E, LOG2E};
    const bool cb_ok = cob0 + cb < a.n_cob;  // (uniform)
    // ---- softmax over the K neighbour rows of every point (base 2: the scores carry log2 e), weighted sum of the values, one row out per point
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int pg = 0; pg < GPB; ++pg) {
        // rows of point pg inside the 32-row block: 16 -> regs 8pg .. 8pg+7 (both halves); 8 -> regs 4pg .. 4pg+3
        constexpr int PPG = 8 / GPB;  // register pairs per point
        f32x2 sc[PPG], vv[PPG];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < PPG; ++j) {
          sc[j] = __builtin_elementwise_fma(pr(sacc[cb][rb], pg * PPG + j), l2, bs2);
          vv[j] = __builtin_elementwise_fma(pr(vacc[cb][rb], pg * PPG + j), g2, bt2);
          vv[j][0] = fmaxf(vv[j][0], 0.f); vv[j][1] = fmaxf(vv[j][1], 0.f);
          m = fmaxf(m, fmaxf(sc[j][0], sc[j][1]));
        }
        m = fmaxf(m, other_half(m));
        const f32x2 m2 = {m, m};
        f32x2 den2 = {0.f, 0.f}, num2 = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < PPG; ++j) {
          const f32x2 d = sc[j] - m2;
          const f32x2 e = {__builtin_amdgcn_exp2f(d[0]), __builtin_amdgcn_exp2f(d[1])};
          den2 += e;
          num2 = __builtin_elementwise_fma(e, vv[j], num2);
        }
        // one exchange for both sums: afterwards the LOWER lanes hold (num.lo, num.hi), the upper lanes (den.lo, den.hi); the upper
        // lanes' total (den) then comes down with a second exchange
        uint32_t un = __float_as_uint(num2[0] + num2[1]), ud = __float_as_uint(den2[0] + den2[1]);
        lane32_swap(un, ud);
        const float tot = __uint_as_float(un) + __uint_as_float(ud);  // lower lanes: numerator, upper lanes: denominator
        uint32_t ua = __float_as_uint(tot), ub = ua;
        lane32_swap(ua, ub);  // ub (lower lanes) = the upper lanes' tot
        const int pidx = rb * GPB + pg;  // point of the wave
        if (half == 0 && pt0 + pidx < npts && cb_ok) {
          const T v = (T)(tot * __builtin_amdgcn_rcpf(__uint_as_float(ub)));
          const int ch = (cob0 + cb) * 32;
          *reinterpret_cast<T *>(reinterpret_cast<char *>(reinterpret_cast<T *>(a.out) + (size_t)(pt0 + pidx) * a.out_ld + ch) + lofs) = v;
          // chunk-major copy of the per-point table for the next block's gather-on-load GEMM
          if (a.out_cm)
            *reinterpret_cast<T *>(reinterpret_cast<char *>(reinterpret_cast<T *>(a.out_cm) + ((size_t)(cob0 + cb) * npts + pt0 + pidx) * 32) + lofs) = v;
          // second copy into the columns of a later concatenation buffer (the skip input of an FP block's second Mlp)
          if (a.out2 && ch + col < a.out2_n)
            *reinterpret_cast<T *>(reinterpret_cast<char *>(reinterpret_cast<T *>(a.out2) + (size_t)(pt0 + pidx) * a.out2_ld + ch) + lofs) = v;
        }
      }
  }
}

#ifndef SLIDE_ATTN_NST
#define SLIDE_ATTN_NST 3  // ring stages of the fused attention tail
#endif
template <int NPXL, int NST>
__device__ __forceinline__ void attn_tail_body(const AttnTailArgs &a) {
  using T = _Float16;
  constexpr int CBW = 2, RT = TM + 64, STAGE_B = RT * 64, LPW = RT / 16 / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + CBW - 1) / CBW;
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr * TM >= a.rows) return;
  const int row0 = tr * TM, cob0 = tc * CBW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  float *const vec_lds = reinterpret_cast<float *>(smem_raw + (size_t)NST * STAGE_B);  // [4 vectors][CBW*32]
  for (int i = tid; i < 4 * CBW * 32; i += 256) {
    const int which = i / (CBW * 32), c = i - which * (CBW * 32), gc = cob0 * 32 + c;
    vec_lds[i] = gc < a.n_cob * 32 ? a.vec[(size_t)which * a.n_cob * 32 + gc] : 0.f;
  }
  int wrow[CBW], wkey[CBW], xrow[2], xkey[2];
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const int trow = TM + cb * 32 + col;
    wrow[cb] = trow * 64; wkey[cb] = (trow >> 2) & 3;
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int trow = wave * 64 + rb * 32 + col;
    xrow[rb] = trow * 64; xkey[rb] = (trow >> 2) & 3;
  }
  // one LDS-DMA ring GEMM: acc[cb][rb] = D[row][channel] (lane: channel col of block cb; reg r: row (r&3)+8(r>>2)+4 half)
  auto run = [&](const void *Xp, const void *Wp, int x_ld, int k_pad, f32x16 (&acc)[CBW][2]) __attribute__((always_inline)) {
    // chunk-major operands as in glds_tile: X when x_ld == 32, the weights when a.w_cm
    const size_t x_cs = x_ld == 32 ? (size_t)a.rows * 32 : 32;
    const size_t w_cs = a.w_cm ? (size_t)a.n_cob * 32 * 32 : 32;
    const int w_ld = a.w_cm ? 32 : k_pad;
    const T *gp[LPW];
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int trow = 16 * (j * 4 + wave) + (lane >> 2);
      const int piece = (lane & 3) ^ ((trow >> 2) & 3);
      if (trow < TM) {
        int grow = row0 + trow;
        grow = grow < a.rows ? grow : a.rows - 1;
        gp[j] = reinterpret_cast<const T *>(Xp) + (size_t)grow * x_ld + piece * 8;
      } else {
        int gco = cob0 * 32 + (trow - TM);
        gco = gco < a.n_cob * 32 ? gco : a.n_cob * 32 - 1;
        gp[j] = reinterpret_cast<const T *>(Wp) + (size_t)gco * w_ld + piece * 8;
      }
    }
    auto issue = [&](int kc, int st) {
#pragma unroll
      for (int j = 0; j < LPW; ++j)
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)(gp[j] + (size_t)kc * (j < TM / 64 ? x_cs : w_cs)),
                                         (__attribute__((address_space(3))) void *)(smem_raw + (size_t)st * STAGE_B +
                                                                                    (j * 4 + wave) * 1024),
                                         16, 0, 0);
    };
#pragma unroll
    for (int i = 0; i < CBW; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int nk = k_pad / 32;
#pragma unroll
    for (int s0 = 0; s0 < NST - 1; ++s0)
      if (s0 < nk) issue(s0, s0);
    for (int kc = 0; kc < nk; ++kc) {
      if (kc + NST - 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * LPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kc + NST - 1 < nk) issue(kc + NST - 1, (kc + NST - 1) % NST);
      const unsigned char *sb = smem_raw + (size_t)(kc % NST) * STAGE_B;
#pragma unroll
      for (int st2 = 0; st2 < 2; ++st2) {
        f16x8 wf[CBW], xf[2];
        const int piece = st2 * 2 + half;
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) wf[cb] = *reinterpret_cast<const f16x8 *>(sb + wrow[cb] + ((piece ^ wkey[cb]) << 4));
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) xf[rb] = *reinterpret_cast<const f16x8 *>(sb + xrow[rb] + ((piece ^ xkey[rb]) << 4));
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xf[rb], wf[cb], acc[cb][rb], 0, 0, 0);  // rows x channels
      }
    }
    __syncthreads();  // ring drained and free (also orders the staged vectors before their first use)
  };
  f32x16 sacc[CBW][2], vacc[CBW][2];
  run(a.X1, a.W1, a.x1_ld, a.k1, sacc);
  run(a.X2, a.W2, a.x2_ld, a.k2, vacc);
  attn_tail_finish<NPXL>(a, sacc, vacc, vec_lds, CBW * 32, reinterpret_cast<float *>(smem_raw), row0, cob0, wave);
}

// REGISTER-X form (round 5; the default, SLIDE_TAIL_RX=0 restores the ring form above).  16 KB of a 20 KB ring stage is the X tile,
// which no two waves share -- a wave's MFMAs read only its own 64 rows.  Here a wave loads ITS X fragments straight into registers
// (chunk-major u / mo: a 32-row block of one chunk is 2 KB contiguous, a lane's 16 bytes are its MFMA A fragment as stored) RXD chunks
// ahead, and only the weights (64 channels x 32 k = 4 KB per chunk, read by all four waves) go through an LDS-DMA ring of RXD + 1
// stages: 23 KB of LDS per workgroup instead of 61, a quarter of the ds_reads, RXD - 1 ... RXD chunks in flight per workgroup instead
// of two.  ONE pipeline over both contractions, values first (their chunk count must be a multiple of RXD -- the launcher checks --
// so that the register slot of a chunk is a compile-time index), then scores.  Measured (tools/ab/r05_tailrx.sh): the feature step's two
// SA tails 67.0 -> 64.4 us stand-alone, 378.9 -> 382.6 shapes/s in the arrangement (three alternating pairs) -- the deeper prefetch
// buys little: the tile's fill rate (~58 GB/s per CU, round 3's ablations) is a throughput cap, not a latency one.
constexpr int RXD = 4;
// WC = 2 (eight waves, tile 256 rows x 128 channels: wave (wr, wc) owns rows 64 wr .. and the channel half wc, a row block's fragments
// are requested by two waves) was measured and is not instantiated: 76.5 us per feature step's two SA tails against 64.4 (WC = 1) and
// 67.0 (ring form) -- the second request is not free, and one eight-wave workgroup per CU overlaps less than two of four.
// FM (round 6): u / mo FRAGMENT-major -- inside a 32-row group the chunk's 2 KB are [k16 step][k half][row][8 halves], i.e. the two
// A fragments of the group as the wave's lanes hold them: each global_load_dwordx4 below then reads 1 KB of consecutive memory instead
// of 32 B from each of 32 rows 64 B apart (the request-bound pattern; tools/lds_fill.hip XP vs XF: 28 -> 44-49 B/clk/CU into VGPRs).
template <int NPXL, int WC, bool FM>
__device__ __forceinline__ void attn_tail_rx_body(const AttnTailArgs &a) {
  using T = _Float16;
  constexpr int CBW = 2, CBWT = CBW * WC, NSTW = RXD + 1, WSTAGE = 64 * WC * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + CBWT - 1) / CBWT;
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr * TM >= a.rows) return;
  const int row0 = tr * TM, cob0 = tc * CBWT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int wr = wave & 3, wc = wave >> 2;
  float *const vec_lds = reinterpret_cast<float *>(smem_raw + (size_t)NSTW * WSTAGE);  // [4 vectors][CBWT*32]
  float *const red = vec_lds + 4 * CBWT * 32;                                          // [wc][4 row waves][CBW][32][2]
  // the tile's four vectors go to LDS by LDS-DMA (wave w: vector w, 64 floats) -- through registers the ds_write's wait was a full
  // memory round trip BEFORE the first chunk load could issue (~1 us of every workgroup: "primed" in tools/ab/op_timeline.py); as the
  // oldest loads of the pipeline they have landed with chunk 0 and the first step's barrier publishes them.  (Channels past n_cob * 32
  // read a valid address: their values are never stored and never mix with valid channels -- GroupNorm groups lie inside a block.)
  static_assert(WC == 1, "vector staging: one LDS-DMA instruction per wave covers the tile's 64 channels");
  {
    int gc = cob0 * 32 + lane;
    gc = gc < a.n_cob * 32 ? gc : a.n_cob * 32 - 1;
    __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)(a.vec + (size_t)wave * a.n_cob * 32 + gc),
                                     (__attribute__((address_space(3))) void *)(vec_lds + wave * 64), 4, 0, 0);
  }
  // weights: wave w stages channels 16 w .. 16 w + 15 of the tile (one 1 KB piece per chunk); fragments: lane = channel, swizzled pieces
  const int wch = 16 * wave + (lane >> 2);
  int gco = cob0 * 32 + wch;
  gco = gco < a.n_cob * 32 ? gco : a.n_cob * 32 - 1;
  const int wpiece = (lane & 3) ^ ((wch >> 2) & 3);
  const size_t w_cs = a.w_cm ? (size_t)a.n_cob * 32 * 32 : 32;
  const T *const w2p = reinterpret_cast<const T *>(a.W2) + (size_t)gco * (a.w_cm ? 32 : a.k2) + wpiece * 8;
  const T *const w1p = reinterpret_cast<const T *>(a.W1) + (size_t)gco * (a.w_cm ? 32 : a.k1) + wpiece * 8;
  int wrow[CBW], wkey[CBW];
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const int trow = wc * 64 + cb * 32 + col;
    wrow[cb] = trow * 64; wkey[cb] = (trow >> 2) & 3;
  }
  // X: lane (col, half) of row block rb reads row  row0 + 64 wave + 32 rb + col,  k pieces  2 st2 + half  of the chunk
  const size_t x2_cs = a.x2_ld == 32 ? (size_t)a.rows * 32 : 32, x1_cs = a.x1_ld == 32 ? (size_t)a.rows * 32 : 32;
  const T *x2p[2], *x1p[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    int grow = row0 + wr * 64 + rb * 32 + col;
    grow = grow < a.rows ? grow : a.rows - 1;
    const size_t fmo = (size_t)(grow & ~31) * 32 + half * 256 + (grow & 31) * 8;
    x2p[rb] = reinterpret_cast<const T *>(a.X2) + (FM ? fmo : (size_t)grow * a.x2_ld + half * 8);
    x1p[rb] = reinterpret_cast<const T *>(a.X1) + (FM ? fmo : (size_t)grow * a.x1_ld + half * 8);
  }
  const int nk2 = a.k2 / 32, total = nk2 + a.k1 / 32;
  f16x8 xq[RXD][2][2];
  // EVERY chunk slot issues its five loads, also past the last chunk (there: all lanes read one valid address -- a broadcast, next to no
  // traffic -- and nobody consumes the result): with unconditional issues the number of loads behind a chunk's is the constant
  // 5 (RXD - 1), for the manual wait below and for the compiler's own wait-count insertion alike (a conditional issue made it fall
  // back to vmcnt(0) at every use, which serialises the pipeline).
  // FM: every address is SCALAR base + one per-lane 32-bit offset (lane * 16 bytes: a fragment is 1 KB in lane order; the second k16
  // step, the second row group are immediate offsets when the group exists) -- the chunk-major form below spends ~10 VALU
  // instructions per load on 64-bit pointer arithmetic, ~50 per chunk against the chunk's 8 MFMAs (32 clocks each): as much issue
  // time as the matrix work itself.  Idle slots (past the last chunk) read one address in all lanes (offset 0 of chunk 0).
  const int wr_s = __builtin_amdgcn_readfirstlane(wr), ngrp = a.rows >> 5;
  const int g0u = (row0 >> 5) + wr_s * 2, g0 = g0u < ngrp ? g0u : ngrp - 1, g1 = g0u + 1 < ngrp ? g0u + 1 : ngrp - 1;
  const uint64_t xg0 = (uint64_t)g0 * 2048, xg1 = (uint64_t)g1 * 2048, xcsb = (uint64_t)a.rows * 64;  // bytes
  const uint32_t lane16 = lane * 16, woff = (uint32_t)(gco * 32 + wpiece * 8) * 2;
  auto issue_fm = [&](int c, f16x8 (&x)[2][2]) __attribute__((always_inline)) {
    const bool live = c < total;
    const int cl = live ? c : 0;
    const bool second = cl >= nk2;
    const int kc = second ? cl - nk2 : cl;
    const uint32_t vo = live ? lane16 : 0u, vw = live ? woff : 0u;
    const uint64_t xb = reinterpret_cast<uint64_t>(second ? a.X1 : a.X2) + (uint64_t)kc * xcsb, b0 = xb + xg0, b1 = xb + xg1;
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(x[0][0]) : "v"(vo), "s"(b0) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(x[0][1]) : "v"(vo), "s"(b0) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(x[1][0]) : "v"(vo), "s"(b1) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(x[1][1]) : "v"(vo), "s"(b1) : "memory");
    const uint64_t wb = reinterpret_cast<uint64_t>(second ? a.W1 : a.W2) + (uint64_t)kc * (w_cs * 2);
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const GLOBAL_AS void *>(wb + vw),
                                     (__attribute__((address_space(3))) void *)(smem_raw + (size_t)(c % NSTW) * WSTAGE + wave * 1024), 16, 0, 0);
  };
  auto issue = [&](int c, f16x8 (&x)[2][2]) __attribute__((always_inline)) {
    if constexpr (FM) { issue_fm(c, x); return; }
    // (branch-free: an idle slot's addresses collapse onto `dummy` through a mask, not through a select the compiler could turn into
    //  control flow -- every path through the pipeline must carry the same loads)
    const bool second = c >= nk2;
    const int kc = second ? c - nk2 : c;
    const uint64_t mask = c < total ? ~0ull : 0ull;
    const uint64_t dummy = reinterpret_cast<uint64_t>(a.vec);
    const uint64_t wp = dummy + ((reinterpret_cast<uint64_t>((second ? w1p : w2p) + (size_t)kc * w_cs) - dummy) & mask);
    const size_t xo = (size_t)kc * (second ? x1_cs : x2_cs);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const uint64_t xp = dummy + ((reinterpret_cast<uint64_t>((second ? x1p[rb] : x2p[rb]) + xo) - dummy) & mask);
      // (asm: hipcc's wait-count insertion answers ANY register load pending beside an LDS-DMA load with vmcnt(0) -- the two may
      //  return out of order for all it knows -- which drains the pipeline once per round; these loads are waited for by hand)
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(x[rb][0]) : "v"(xp) : "memory");
      if constexpr (FM) asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(x[rb][1]) : "v"(xp) : "memory");
      else asm volatile("global_load_dwordx4 %0, %1, off offset:32" : "=v"(x[rb][1]) : "v"(xp) : "memory");
    }
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const GLOBAL_AS void *>(wp),
                                     (__attribute__((address_space(3))) void *)(smem_raw + (size_t)(c % NSTW) * WSTAGE + wave * 1024), 16, 0, 0);
  };
  f32x16 sacc[CBW][2], vacc[CBW][2];
#pragma unroll
  for (int i = 0; i < CBW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[i][j][r] = 0.f; vacc[i][j][r] = 0.f; }
  SLIDE_STAMP(a, 0);
#pragma unroll
  for (int j = 0; j < RXD; ++j) issue(j, xq[j]);
  SLIDE_STAMP(a, 1);
  auto step = [&](int c, f16x8 (&x)[2][2], f32x16 (&acc)[CBW][2]) __attribute__((always_inline)) {
    // chunk c's loads have landed when only those of chunks c + 1 .. c + RXD - 1 are outstanding (the operands tie the fragments'
    // uses to this wait)
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(x[0][0]), "+v"(x[0][1]), "+v"(x[1][0]), "+v"(x[1][1]) : "n"((RXD - 1) * 5) : "memory");
    __builtin_amdgcn_s_barrier();  // every wave's piece of W chunk c has landed; W stage (c - 1) % NSTW is free
    const unsigned char *sb = smem_raw + (size_t)(c % NSTW) * WSTAGE;
#pragma unroll
    for (int st2 = 0; st2 < 2; ++st2) {
      f16x8 wf[CBW];
      const int piece = st2 * 2 + half;
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb) wf[cb] = *reinterpret_cast<const f16x8 *>(sb + wrow[cb] + ((piece ^ wkey[cb]) << 4));
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[rb][st2], wf[cb], acc[cb][rb], 0, 0, 0);  // rows x channels
    }
    issue(c + RXD, x);
  };
  for (int c0 = 0; c0 < nk2; c0 += RXD) {
#pragma unroll
    for (int j = 0; j < RXD; ++j) step(c0 + j, xq[j], vacc);
    if (c0 == 0) SLIDE_STAMP(a, 2);
  }
  SLIDE_STAMP(a, 3);
  for (int c0 = nk2; c0 < total; c0 += RXD) {  // (leaves from the middle of a round after the last chunk: no path re-joins the pipeline)
#pragma unroll
    for (int j = 0; j < RXD; ++j) {
      step(c0 + j, xq[j], sacc);
      if (c0 + j + 1 >= total) break;
    }
  }
  // the idle slots' loads: their registers stay reserved until they have landed
#pragma unroll
  for (int j = 0; j < RXD; ++j)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(xq[j][0][0]), "+v"(xq[j][0][1]), "+v"(xq[j][1][0]), "+v"(xq[j][1][1]) :: "memory");
  SLIDE_STAMP(a, 4);
  __syncthreads();  // (orders the staged vectors before their first use)
  SLIDE_STAMP(a, 5);
  attn_tail_finish<NPXL>(a, sacc, vacc, vec_lds + wc * 64, CBWT * 32, red + wc * (4 * CBW * 32 * 2), row0, cob0 + wc * CBW, wr);
  SLIDE_STAMP(a, 6);
#ifdef SLIDE_TIMELINE
  if (a.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); SLIDE_STAMP(a, 7); }
#endif
}

// WIDE form (round 3): 256 rows x 128 channels on the same four waves.  Per MFMA the tile moves 1.1 KB through the LDS instead
// of 1.6 KB (X fragments feed four channel blocks, an X chunk is written once per 128 channels) -- the 64-channel tile's K
// loop is LDS-bandwidth-bound at ~60 % of the matrix pipe -- and a sample's u / mo tiles are read from L2
// by half as many workgroups.  128 accumulator registers hold ONE contraction at a time: VALUES first (GroupNorm statistics,
// normalise, ReLU, packed to fp16: 64 registers), then the SCORES into the same accumulators, then the soft-max weighted sum.
template <int NPXL, int NST>
__device__ __forceinline__ void attn_tail_wide_body(const AttnTailArgs &a) {
  using T = _Float16;
  constexpr int CBW = 4, RT = TM + 32 * CBW, STAGE_B = RT * 64, LPW = RT / 16 / 4;
  constexpr int KLOG = NPXL - 4, KN = 1 << KLOG, GPB = 32 / KN;  // neighbours per point, points per 32-row block
  constexpr int WPS = (1 << NPXL) / 64;                            // waves per sample
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + CBW - 1) / CBW;
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr * TM >= a.rows) return;
  const int row0 = tr * TM, cob0 = tc * CBW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  float *const vec_lds = reinterpret_cast<float *>(smem_raw + (size_t)NST * STAGE_B);  // [4 vectors][CBW*32]
  for (int i = tid; i < 4 * CBW * 32; i += 256) {
    const int which = i / (CBW * 32), c = i - which * (CBW * 32), gc = cob0 * 32 + c;
    vec_lds[i] = gc < a.n_cob * 32 ? a.vec[(size_t)which * a.n_cob * 32 + gc] : 0.f;
  }
  int wrow[CBW], wkey[CBW], xrow[2], xkey[2];
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const int trow = TM + cb * 32 + col;
    wrow[cb] = trow * 64; wkey[cb] = (trow >> 2) & 3;
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int trow = wave * 64 + rb * 32 + col;
    xrow[rb] = trow * 64; xkey[rb] = (trow >> 2) & 3;
  }
  // one LDS-DMA ring GEMM: acc[cb][rb] = D[row][channel] (lane: channel col of block cb; reg r: row (r&3)+8(r>>2)+4 half)
  auto run = [&](const void *Xp, const void *Wp, int x_ld, int k_pad, f32x16 (&acc)[CBW][2]) __attribute__((always_inline)) {
    // chunk-major operands as in glds_tile: X when x_ld == 32, the weights when a.w_cm
    const size_t x_cs = x_ld == 32 ? (size_t)a.rows * 32 : 32;
    const size_t w_cs = a.w_cm ? (size_t)a.n_cob * 32 * 32 : 32;
    const int w_ld = a.w_cm ? 32 : k_pad;
    const T *gp[LPW];
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int trow = 16 * (j * 4 + wave) + (lane >> 2);
      const int piece = (lane & 3) ^ ((trow >> 2) & 3);
      if (trow < TM) {
        int grow = row0 + trow;
        grow = grow < a.rows ? grow : a.rows - 1;
        gp[j] = reinterpret_cast<const T *>(Xp) + (size_t)grow * x_ld + piece * 8;
      } else {
        int gco = cob0 * 32 + (trow - TM);
        gco = gco < a.n_cob * 32 ? gco : a.n_cob * 32 - 1;
        gp[j] = reinterpret_cast<const T *>(Wp) + (size_t)gco * w_ld + piece * 8;
      }
    }
    auto issue = [&](int kc, int st) {
#pragma unroll
      for (int j = 0; j < LPW; ++j)
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)(gp[j] + (size_t)kc * (j < TM / 64 ? x_cs : w_cs)),
                                         (__attribute__((address_space(3))) void *)(smem_raw + (size_t)st * STAGE_B +
                                                                                    (j * 4 + wave) * 1024),
                                         16, 0, 0);
    };
#pragma unroll
    for (int i = 0; i < CBW; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int nk = k_pad / 32;
#pragma unroll
    for (int s0 = 0; s0 < NST - 1; ++s0)
      if (s0 < nk) issue(s0, s0);
    for (int kc = 0; kc < nk; ++kc) {
      if (kc + NST - 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * LPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kc + NST - 1 < nk) issue(kc + NST - 1, (kc + NST - 1) % NST);
      const unsigned char *sb = smem_raw + (size_t)(kc % NST) * STAGE_B;
#pragma unroll
      for (int st2 = 0; st2 < 2; ++st2) {
        f16x8 wf[CBW], xf[2];
        const int piece = st2 * 2 + half;
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) wf[cb] = *reinterpret_cast<const f16x8 *>(sb + wrow[cb] + ((piece ^ wkey[cb]) << 4));
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) xf[rb] = *reinterpret_cast<const f16x8 *>(sb + xrow[rb] + ((piece ^ xkey[rb]) << 4));
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xf[rb], wf[cb], acc[cb][rb], 0, 0, 0);  // rows x channels
      }
    }
    __syncthreads();  // ring drained and free (also orders the staged vectors before their first use)
  };
  f32x16 acc[CBW][2];
  run(a.X2, a.W2, a.x2_ld, a.k2, acc);  // values first

  // ---- values: bias, GroupNorm over the sample (rows of WPS waves x the gs adjacent channel lanes), ReLU, packed to fp16
  float *const red = reinterpret_cast<float *>(smem_raw);  // [wave][cb][32 channels][sum, sumsq]
  const float *b_s = vec_lds, *b_v = vec_lds + CBW * 32, *gam = vec_lds + 2 * CBW * 32, *bet = vec_lds + 3 * CBW * 32;
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const float bv = b_v[cb * 32 + col];
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float x = acc[cb][rb][r] + bv;
        acc[cb][rb][r] = x;
        s += x;
        ss = fmaf(x, x, ss);
      }
    s += other_half(s);
    ss += other_half(ss);
    if (half == 0) *reinterpret_cast<f32x2 *>(red + ((wave * CBW + cb) * 32 + col) * 2) = f32x2{s, ss};
  }
  __syncthreads();
  const int w0 = (wave / WPS) * WPS;
  f16x2 vp[CBW][2][8];  // relu(GN(values)) of this lane's channel, rows (2 j, 2 j + 1) of the block
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    f32x2 t = {0.f, 0.f};
#pragma unroll
    for (int w = 0; w < WPS; ++w) t += *reinterpret_cast<const f32x2 *>(red + (((w0 + w) * CBW + cb) * 32 + col) * 2);
    float s = t[0], ss = t[1];
    if (a.gs >= 2) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0xB1, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0xB1, 0xF, 0xF, true)); }
    if (a.gs >= 4) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x4E, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x4E, 0xF, 0xF, true)); }
    if (a.gs >= 8) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x141, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x141, 0xF, 0xF, true)); }
    if (a.gs >= 16) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x140, 0xF, 0xF, true));
                      ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x140, 0xF, 0xF, true)); }
    if (a.gs >= 32) { s += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(s), 0x401F));
                      ss += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(ss), 0x401F)); }
    const float mean = s * a.inv_count;
    const float var = fmaxf(ss * a.inv_count - mean * mean, 0.f);
    float g = gam[cb * 32 + col] * __builtin_amdgcn_rsqf(var + GN_EPS);
    float bt = bet[cb * 32 + col] - mean * g;
    if ((cob0 + cb) * 32 + col >= a.n_norm) { g = 1.f; bt = 0.f; }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        vp[cb][rb][j] = f16x2{(T)fmaxf(fmaf(acc[cb][rb][2 * j], g, bt), 0.f), (T)fmaxf(fmaf(acc[cb][rb][2 * j + 1], g, bt), 0.f)};
  }
  __syncthreads();  // every wave has read the statistics: the ring area is free for the score contraction
  run(a.X1, a.W1, a.x1_ld, a.k1, acc);  // scores into the same accumulators
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const float bs = b_s[cb * 32 + col];
    // ---- softmax over the K neighbour rows of every point, weighted sum of the values, one row out per point
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int pg = 0; pg < GPB; ++pg) {
        constexpr int RPG = 16 / GPB;
        float sc[RPG], vv[RPG];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < RPG; ++j) {
          sc[j] = acc[cb][rb][pg * RPG + j] + bs;
          vv[j] = (float)vp[cb][rb][(pg * RPG + j) >> 1][(pg * RPG + j) & 1];
          m = fmaxf(m, sc[j]);
        }
        m = fmaxf(m, other_half(m));
        float den = 0.f, num = 0.f;
#pragma unroll
        for (int j = 0; j < RPG; ++j) {
          const float e = __expf(sc[j] - m);
          den += e;
          num = fmaf(e, vv[j], num);
        }
        den += other_half(den);
        num += other_half(num);
        const int rbase = row0 + wave * 64 + rb * 32 + pg * KN;
        if (half == 0 && rbase < a.rows && cob0 + cb < a.n_cob) {
          const T v = (T)(num / den);
          reinterpret_cast<T *>(a.out)[(size_t)(rbase >> KLOG) * a.out_ld + (cob0 + cb) * 32 + col] = v;
          if (a.out_cm)
            reinterpret_cast<T *>(a.out_cm)[((size_t)(cob0 + cb) * (a.rows >> KLOG) + (rbase >> KLOG)) * 32 + col] = v;
          if (a.out2 && (cob0 + cb) * 32 + col < a.out2_n)
            reinterpret_cast<T *>(a.out2)[(size_t)(rbase >> KLOG) * a.out2_ld + (cob0 + cb) * 32 + col] = v;
        }
      }
  }
}

template <int NPXL>
__global__ __launch_bounds__(256, 1) void attn_tail_wide_kernel(AttnTailArgs a) {
  attn_tail_wide_body<NPXL, 3>(a);
}

template <int NPXL>
__global__ __launch_bounds__(256, 2) void attn_tail_kernel(AttnTailArgs a) {
  attn_tail_body<NPXL, SLIDE_ATTN_NST>(a);
}

template <int NPXL, bool FM>
__global__ __launch_bounds__(256, 2) void attn_tail_rx_kernel(AttnTailArgs a) {
  attn_tail_rx_body<NPXL, 1, FM>(a);
}

// the same tile on a TWO-stage ring (41 KB) inside the 168-register budget: three workgroups per CU instead of two
template <int NPXL>
__global__ __launch_bounds__(256, 3) void attn_tail_occ3_kernel(AttnTailArgs a) {
  attn_tail_body<NPXL, 2>(a);
}

// Eight-wave form of the fused attention tail (round 3): tile 256 rows x 128 channels -- wave (wr, wc) owns rows 64 wr .. and the
// channel half wc, so an X chunk is fetched once per 128 channels (24 KB of L2 -> LDS per 2 MFLOP instead of 20 KB per 1) --,
// ring stages 64 deep (two chunk images: one barrier per 16 MFMAs of a wave), ONE continuous ring over the chunks of both
// GEMMs (no drain between the score and the value contraction), fragment reads of the next 16-deep step issued before the
// current step's MFMAs.  Same arithmetic, same epilogue as attn_tail_kernel; used when the layer has at least eight blocks.
template <int NPXL>
__global__ __launch_bounds__(512, 2) void attn_tail8_kernel(AttnTailArgs a) {
  using T = _Float16;
  constexpr int CBW = 2, NST = 3, RT = TM + 128, CH_B = RT * 64, STAGE_B = 2 * CH_B, LPW = RT / 16 / 8;  // 3 DMA / wave / chunk
  constexpr int KLOG = NPXL - 4, KN = 1 << KLOG, GPB = 32 / KN;
  constexpr int WPS = (1 << NPXL) / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + 3) / 4;
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr * TM >= a.rows) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), wave = wv & 3, wc = wv >> 2;
  const int half = lane >> 5, col = lane & 31;
  const int row0 = tr * TM, cobt = tc * 4, cob0 = cobt + wc * CBW;
  SLIDE_STAMP(a, 0);
  float *const vec_lds = reinterpret_cast<float *>(smem_raw + (size_t)NST * STAGE_B);  // [4 vectors][4 * 32]
  for (int i = tid; i < 4 * 128; i += 512) {
    const int which = i >> 7, c = i & 127, gc = cobt * 32 + c;
    vec_lds[i] = gc < a.n_cob * 32 ? a.vec[(size_t)which * a.n_cob * 32 + gc] : 0.f;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int wrow[CBW], wkey[CBW], xrow[2], xkey[2];
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const int trow = TM + (wc * CBW + cb) * 32 + col;
    wrow[cb] = trow * 64; wkey[cb] = (trow >> 2) & 3;
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int trow = wave * 64 + rb * 32 + col;
    xrow[rb] = trow * 64; xkey[rb] = (trow >> 2) & 3;
  }
  const int nk1 = a.k1 >> 5, nk2 = a.k2 >> 5, nkt = nk1 + nk2, nks = (nkt + 1) >> 1;
  // this lane's source piece of the wave's three DMA instructions per chunk, for both GEMMs
  const T *gp[2][LPW];
  size_t cs[2][LPW];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const void *Xp = g ? a.X2 : a.X1, *Wp = g ? a.W2 : a.W1;
    const int x_ld = g ? a.x2_ld : a.x1_ld, k_pad = g ? a.k2 : a.k1;
    const size_t x_cs = x_ld == 32 ? (size_t)a.rows * 32 : 32;
    const size_t w_cs = a.w_cm ? (size_t)a.n_cob * 32 * 32 : 32;
    const int w_ld = a.w_cm ? 32 : k_pad;
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int trow = 16 * (j * 8 + wv) + (lane >> 2);
      const int piece = (lane & 3) ^ ((trow >> 2) & 3);
      if (trow < TM) {
        int grow = row0 + trow;
        grow = grow < a.rows ? grow : a.rows - 1;
        gp[g][j] = reinterpret_cast<const T *>(Xp) + (size_t)grow * x_ld + piece * 8;
        cs[g][j] = x_cs;
      } else {
        int gco = cobt * 32 + (trow - TM);
        gco = gco < a.n_cob * 32 ? gco : a.n_cob * 32 - 1;
        gp[g][j] = reinterpret_cast<const T *>(Wp) + (size_t)gco * w_ld + piece * 8;
        cs[g][j] = w_cs;
      }
    }
  }
  auto issue = [&](int st) __attribute__((always_inline)) {
    unsigned char *dst = smem_raw + (size_t)(st % NST) * STAGE_B;
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      int h = st * 2 + c2;
      h = h < nkt ? h : nkt - 1;  // odd total: the last image is a dummy (never read)
      const int g = h >= nk1, kc = g ? h - nk1 : h;
#pragma unroll
      for (int j = 0; j < LPW; ++j)
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)((g ? gp[1][j] : gp[0][j]) + (size_t)kc * (g ? cs[1][j] : cs[0][j])),
                                         (__attribute__((address_space(3))) void *)(dst + c2 * CH_B + (j * 8 + wv) * 1024), 16, 0, 0);
    }
  };
  // stage st must have landed; the next one (2 * LPW instructions per wave) stays in flight: with ONE workgroup per CU the
  // bytes in flight are what the L2 -> LDS rate hangs on (two-stage ring: 1.26 us per 48 KB stage, DMA-latency bound)
  auto stage_ready = [&](int st) __attribute__((always_inline)) {
    if (st + 1 < nks) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (st + 2 < nks && a.abl != 1) issue(st + 2);  // overwrites the stage consumed at st - 1
  };
  f32x16 sacc[CBW][2], vacc[CBW][2];
#pragma unroll
  for (int i = 0; i < CBW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[i][j][r] = 0.f; vacc[i][j][r] = 0.f; }
  struct Frag { f16x8 wf[CBW], xf[2]; };
  auto loadf = [&](Frag &o, const unsigned char *sb, int st2) __attribute__((always_inline)) {
    if (a.abl == 2 && sb != smem_raw) return;
    const int piece = st2 * 2 + half;
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb) o.wf[cb] = *reinterpret_cast<const f16x8 *>(sb + wrow[cb] + ((piece ^ wkey[cb]) << 4));
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) o.xf[rb] = *reinterpret_cast<const f16x8 *>(sb + xrow[rb] + ((piece ^ xkey[rb]) << 4));
  };
  auto mma = [&](const Frag &o, f32x16 (&acc)[CBW][2]) __attribute__((always_inline)) {
    if (a.abl == 3) { asm volatile("" :: "v"(o.xf[0]), "v"(o.xf[1]), "v"(o.wf[0]), "v"(o.wf[1])); return; }
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
        acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(o.xf[rb], o.wf[cb], acc[cb][rb], 0, 0, 0);  // rows x channels
  };
  issue(0);
  if (nks > 1) issue(1);
  SLIDE_STAMP(a, 1);
  stage_ready(0);
  SLIDE_STAMP(a, 2);
  Frag cur, nxt;
  loadf(cur, smem_raw, 0);
  // (nk1, nk2 even: a ring stage never straddles the two GEMMs, each accumulator set has its own loop)
  auto run = [&](int st_lo, int st_hi, f32x16 (&acc)[CBW][2]) __attribute__((always_inline)) {
    for (int st = st_lo; st < st_hi; ++st) {
      const unsigned char *sb = smem_raw + (size_t)(st % NST) * STAGE_B;
      loadf(nxt, sb, 1);
      mma(cur, acc);
      loadf(cur, sb + CH_B, 0);
      mma(nxt, acc);
      loadf(nxt, sb + CH_B, 1);
      mma(cur, acc);
      if (st + 1 < nks) {
        stage_ready(st + 1);
        loadf(cur, smem_raw + (size_t)((st + 1) % NST) * STAGE_B, 0);
      }
      mma(nxt, acc);
    }
  };
  run(0, nk1 >> 1, sacc);
  SLIDE_STAMP(a, 3);
  run(nk1 >> 1, nks, vacc);
  SLIDE_STAMP(a, 4);
  __syncthreads();  // ring drained and free

  // ---- values: bias, GroupNorm over the sample (rows of WPS waves x the gs adjacent channel lanes), ReLU
  float *const red = reinterpret_cast<float *>(smem_raw);  // [wave 0..7][cb][32 channels][sum, sumsq]
  const float *b_s = vec_lds + wc * 64, *b_v = vec_lds + 128 + wc * 64, *gam = vec_lds + 256 + wc * 64, *bet = vec_lds + 384 + wc * 64;
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const float bv = b_v[cb * 32 + col];
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float x = vacc[cb][rb][r] + bv;
        vacc[cb][rb][r] = x;
        s += x;
        ss = fmaf(x, x, ss);
      }
    s += other_half(s);
    ss += other_half(ss);
    if (half == 0) *reinterpret_cast<f32x2 *>(red + ((wv * CBW + cb) * 32 + col) * 2) = f32x2{s, ss};
  }
  __syncthreads();
  SLIDE_STAMP(a, 5);
  const int w0 = wc * 4 + (wave / WPS) * WPS;
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    f32x2 t = {0.f, 0.f};
#pragma unroll
    for (int w = 0; w < WPS; ++w) t += *reinterpret_cast<const f32x2 *>(red + (((w0 + w) * CBW + cb) * 32 + col) * 2);
    float s = t[0], ss = t[1];
    if (a.gs >= 2) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0xB1, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0xB1, 0xF, 0xF, true)); }
    if (a.gs >= 4) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x4E, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x4E, 0xF, 0xF, true)); }
    if (a.gs >= 8) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x141, 0xF, 0xF, true));
                     ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x141, 0xF, 0xF, true)); }
    if (a.gs >= 16) { s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x140, 0xF, 0xF, true));
                      ss += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(ss), 0x140, 0xF, 0xF, true)); }
    if (a.gs >= 32) { s += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(s), 0x401F));
                      ss += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(ss), 0x401F)); }
    const float mean = s * a.inv_count;
    const float var = fmaxf(ss * a.inv_count - mean * mean, 0.f);
    float g = gam[cb * 32 + col] * __builtin_amdgcn_rsqf(var + GN_EPS);
    float bt = bet[cb * 32 + col] - mean * g;
    if ((cob0 + cb) * 32 + col >= a.n_norm) { g = 1.f; bt = 0.f; }
    const float bs = b_s[cb * 32 + col];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int pg = 0; pg < GPB; ++pg) {
        constexpr int RPG = 16 / GPB;
        float sc[RPG], vv[RPG];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < RPG; ++j) {
          sc[j] = sacc[cb][rb][pg * RPG + j] + bs;
          vv[j] = fmaxf(fmaf(vacc[cb][rb][pg * RPG + j], g, bt), 0.f);
          m = fmaxf(m, sc[j]);
        }
        m = fmaxf(m, other_half(m));
        float den = 0.f, num = 0.f;
#pragma unroll
        for (int j = 0; j < RPG; ++j) {
          const float e = __expf(sc[j] - m);
          den += e;
          num = fmaf(e, vv[j], num);
        }
        den += other_half(den);
        num += other_half(num);
        const int rbase = row0 + wave * 64 + rb * 32 + pg * KN;
        if (half == 0 && rbase < a.rows && cob0 + cb < a.n_cob) {
          const T v = (T)(num / den);
          reinterpret_cast<T *>(a.out)[(size_t)(rbase >> KLOG) * a.out_ld + (cob0 + cb) * 32 + col] = v;
          if (a.out_cm)
            reinterpret_cast<T *>(a.out_cm)[((size_t)(cob0 + cb) * (a.rows >> KLOG) + (rbase >> KLOG)) * 32 + col] = v;
          if (a.out2 && (cob0 + cb) * 32 + col < a.out2_n)
            reinterpret_cast<T *>(a.out2)[(size_t)(rbase >> KLOG) * a.out2_ld + (cob0 + cb) * 32 + col] = v;
        }
      }
  }
  SLIDE_STAMP(a, 6);
#ifdef SLIDE_TIMELINE
  if (a.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); SLIDE_STAMP(a, 7); }
#endif
}

int run_attn_tail(const SlideOp &o, hipStream_t s) {
  AttnTailArgs a;
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
  const int npxl = o.i[6];
  if (a.k1 % 32 || a.k2 % 32 || a.rows <= 0 || a.n_cob <= 0) return -3;
  const int ntr8 = (a.rows + TM - 1) / TM;
  // (opt-in, SLIDE_TAIL8=1: measured equal to the four-wave form for one chain and 2 % slower with four chains in flight --
  //  both forms are bound by the per-CU L2 -> LDS fill rate of the non-resident u / mo tiles)
  static const bool tail8_on = [] { const char *e = getenv("SLIDE_TAIL8"); return e && e[0] == '1'; }();
  const int ntc = (a.n_cob + 1) / 2, ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
#ifndef SLIDE_EXPERIMENTS
  (void)ntr8;
  if (tail8_on || ((int)o.f[1] & 6)) return SLIDE_ST_EXPERIMENT;  // eight-wave / wide / three-workgroup tails
#else
  if (tail8_on && a.n_cob >= 8 && (npxl == 7 || npxl == 8) && a.k1 % 64 == 0 && a.k2 % 64 == 0) {  // eight-wave 256 x 128 tiles (see attn_tail8_kernel)
    const size_t shm8 = (size_t)3 * 2 * (TM + 128) * 64 + 4 * 128 * 4 + 64;
    const int grid8 = ((ntr8 + 7) / 8) * 8 * ((a.n_cob + 3) / 4);
    if (npxl == 8) {
      allow_dynamic_lds<&attn_tail8_kernel<8>>(160 * 1024);
      hipLaunchKernelGGL(attn_tail8_kernel<8>, dim3(grid8), dim3(512), shm8, s, a);
    } else {
      allow_dynamic_lds<&attn_tail8_kernel<7>>(160 * 1024);
      hipLaunchKernelGGL(attn_tail8_kernel<7>, dim3(grid8), dim3(512), shm8, s, a);
    }
    return (int)hipGetLastError();
  }
  if (((int)o.f[1] & 4) && npxl == 8 && a.n_cob % 4 == 0) {  // plan knob SLIDE_TAIL_WIDE: 256 x 128 tiles (attn_tail_wide_kernel)
    const int ntc4 = a.n_cob / 4;
    const int grid4 = ((ntr8 + 7) / 8) * 8 * ntc4;
    const size_t shm4 = (size_t)3 * (TM + 128) * 64 + 4 * 4 * 32 * 4 + 64;
    allow_dynamic_lds<&attn_tail_wide_kernel<8>>(80 * 1024);
    hipLaunchKernelGGL(attn_tail_wide_kernel<8>, dim3(grid4), dim3(256), shm4, s, a);
    return (int)hipGetLastError();
  }
  const bool tail_occ3 = ((int)o.f[1] & 2) != 0;  // (plan knob SLIDE_TAIL_OCC3: two-stage ring, three workgroups per CU)
  if (tail_occ3 && (npxl == 7 || npxl == 8)) {
    const size_t shm3 = (size_t)2 * (TM + 64) * 64 + 4 * 2 * 32 * 4 + 64;
    if (npxl == 8) hipLaunchKernelGGL(attn_tail_occ3_kernel<8>, dim3(grid), dim3(256), shm3, s, a);
    else hipLaunchKernelGGL(attn_tail_occ3_kernel<7>, dim3(grid), dim3(256), shm3, s, a);
    return (int)hipGetLastError();
  }
#endif
  static const int tail_rx = [] { const char *e = getenv("SLIDE_TAIL_RX"); return e ? atoi(e) : 1; }();
  if (tail_rx && (npxl == 7 || npxl == 8) && (a.k2 / 32) % RXD == 0) {  // X fragments through registers (attn_tail_rx_kernel)
    const size_t shmr = (size_t)(RXD + 1) * 64 * 64 + 4 * 2 * 32 * 4 + 4 * 2 * 32 * 2 * 4;
    if (a.x_fm) {
      if (a.x1_ld != 32 || a.x2_ld != 32 || a.rows % 32 || !a.w_cm) return -3;
      if (npxl == 8) hipLaunchKernelGGL((attn_tail_rx_kernel<8, true>), dim3(grid), dim3(256), shmr, s, a);
      else hipLaunchKernelGGL((attn_tail_rx_kernel<7, true>), dim3(grid), dim3(256), shmr, s, a);
      return (int)hipGetLastError();
    }
    if (npxl == 8) hipLaunchKernelGGL((attn_tail_rx_kernel<8, false>), dim3(grid), dim3(256), shmr, s, a);
    else hipLaunchKernelGGL((attn_tail_rx_kernel<7, false>), dim3(grid), dim3(256), shmr, s, a);
    return (int)hipGetLastError();
  }
  if (a.x_fm) return -3;  // fragment-major u / mo: only the register-X kernel reads that layout
  const size_t shm = (size_t)SLIDE_ATTN_NST * (TM + 64) * 64 + 4 * 2 * 32 * 4 + 64;
  if (npxl == 8) {
    allow_dynamic_lds<&attn_tail_kernel<8>>(80 * 1024);
    hipLaunchKernelGGL(attn_tail_kernel<8>, dim3(grid), dim3(256), shm, s, a);
  } else if (npxl == 7) {
    allow_dynamic_lds<&attn_tail_kernel<7>>(80 * 1024);
    hipLaunchKernelGGL(attn_tail_kernel<7>, dim3(grid), dim3(256), shm, s, a);
  } else return -4;
  return (int)hipGetLastError();
}

}  // namespace

int slide_launch_attn_tail(const SlideOp &o, hipStream_t s) { return run_attn_tail(o, s); }
