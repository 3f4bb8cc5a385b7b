// attn_tail.hip -- the fused attention tails of the latent-DDPM denoiser for gfx950 (SLIDE_OP_ATTN_TAIL, fp16;
// include/slide_engine.h): the shared epilogue, the ring form and the register-X form, which are what a default plan
// launches (the ring form on two stages, three workgroups per CU, is an experiments-build launch).  The argument block is in
// attn_tail.h; the wide and eight-wave forms are in experiments/attn_tail_variants.hip; the split-arithmetic tail is in
// attn_tail_split.hip.
#include "attn_tail.h"
#include "launch.h"

namespace {

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

template <int NPXL>
__global__ __launch_bounds__(256, 2) void attn_tail_kernel(AttnTailArgs a) {
  attn_tail_body<NPXL, SLIDE_ATTN_NST>(a);
}

template <int NPXL, bool FM>
__global__ __launch_bounds__(256, 2) void attn_tail_rx_kernel(AttnTailArgs a) {
  attn_tail_rx_body<NPXL, 1, FM>(a);
}

// the same tile on a TWO-stage ring (41 KB) inside the 168-register budget: three workgroups per CU instead of two (plan knob
// SLIDE_TAIL_OCC3; launched by the experiments build only.  It stays beside the other users of attn_tail_finish: the compiler
// propagates the epilogue's arguments across its callers before it inlines, so this kernel's code depends on which callers share
// its translation unit -- profiles/kernel_split.md)
template <int NPXL>
__global__ __launch_bounds__(256, 3) void attn_tail_occ3_kernel(AttnTailArgs a) {
  attn_tail_body<NPXL, 2>(a);
}

int run_attn_tail(const SlideOp &o, hipStream_t s) {
  AttnTailArgs a;
  const int ast = attn_tail_args_from_op(o, a);
  if (ast != 0) return ast;
  const int npxl = o.i[6];
  // (opt-in, SLIDE_TAIL8=1: measured equal to the four-wave form for one chain and 2 % slower with four chains in flight --
  //  both forms are bound by the per-CU L2 -> LDS fill rate of the non-resident u / mo tiles)
  static const bool tail8_on = [] { const char *e = getenv("SLIDE_TAIL8"); return e && e[0] == '1'; }();
  const int ntc = (a.n_cob + 1) / 2, ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
#ifndef SLIDE_EXPERIMENTS
  if (tail8_on || ((int)o.f[1] & 6)) return SLIDE_ST_EXPERIMENT;  // eight-wave / wide / three-workgroup tails
#else
  // eight-wave and wide tails first (experiments/attn_tail_variants.hip); an op neither of them takes goes on below
  const int vst = slide_launch_attn_tail_variants(o, tail8_on, s);
  if (vst != SLIDE_ST_NOT_A_VARIANT) return vst;
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
