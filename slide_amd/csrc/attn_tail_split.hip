// attn_tail_split.hip -- the fused attention tail of the SPLIT-arithmetic plans (SLIDE_OP_ATTN_TAIL with f[1] bit 3; round 5,
// DESIGN.md section 5): float rows, float weights split into fp16 terms on the way to LDS like gemm_gxs.hip's operands.  The fp16
// tails are in attn_tail.hip.
#include "gemm_common.h"
#include "launch.h"

namespace {

// ------------------------------------------------------------------------------------------------ split attention tail
// The end of an AttentionModule (attention.py:86-95) on FLOAT rows in the split arithmetic, ONE launch: values V = relu(GN(Wv mo + bv))
// first (accumulators -> GroupNorm statistics over the sample -> normalised in place: 64 registers), then scores S = W5 u + b5 into a
// second accumulator set, soft-max over a point's K neighbours and the weighted sum -- S and V (2 x rows x C x 4 B, written and read
// back by the three-launch form: 134 MB per step at the position net's SA1) never leave the registers.  Operand roles are SWAPPED
// (A = X rows, B = W rows) as in attn_tail_kernel (attn_tail.hip): a lane owns one channel and its registers run over the rows.
// Tile 256 rows x 64 channels, four waves x 64 rows; one LDS stage of five fp16 planes [X hi | X lo | W hi | 2^11 W hi | W lo].
struct TailSArgs {
  const float *X1, *W1, *X2, *W2;  // scores: u [rows][x1_ld] . W5 [n_cob*32][k1];  values: mo [rows][x2_ld] . Wv [n_cob*32][k2]
  const float *vec;                // [bias_s | bias_v | gamma | beta], n_cob * 32 floats each
  float *out;                      // [rows >> (NPXL - 4)][out_ld]
  float *out2;                     // optional copy of the first out2_n channels into another per-point buffer [..][out2_ld]
  int out2_ld, out2_n;
  int rows, x1_ld, k1, x2_ld, k2, n_cob, gs, n_norm, out_ld;
  float inv_count;
};

template <int NPXL>
__global__ __launch_bounds__(256, 2) void attn_tail_split_kernel(TailSArgs a) {
  constexpr int CBW = 2, TN = 64;
  constexpr int LDK = TileT<SLIDE_PREC_SPLIT>::LDK;
  constexpr int XP = 8, WP = 2;
  constexpr int KLOG = NPXL - 4, KN = 1 << KLOG, GPB = 32 / KN;  // neighbours per point, points per 32-row block
  constexpr int WPS = (1 << NPXL) / 64;                            // waves per sample
  constexpr int STAGE = (2 * TM + 3 * TN) * LDK;                   // halves
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  _Float16 *const Xh = reinterpret_cast<_Float16 *>(smem_raw);
  _Float16 *const Xl = Xh + TM * LDK, *const Wh = Xl + TM * LDK, *const Ws = Wh + TN * LDK, *const Wl = Ws + TN * LDK;
  const int ntc = (a.n_cob + CBW - 1) / CBW;
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr * TM >= a.rows) return;
  const int row0 = tr * TM, cob0 = tc * CBW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int l_row = tid >> 3, l_c = (tid & 7) * 4;
  float *const vec_lds = reinterpret_cast<float *>(smem_raw + (size_t)STAGE * 2);  // [4 vectors][CBW*32]
  for (int i = tid; i < 4 * CBW * 32; i += 256) {
    const int which = i / (CBW * 32), c = i - which * (CBW * 32), gc = cob0 * 32 + c;
    vec_lds[i] = gc < a.n_cob * 32 ? a.vec[(size_t)which * a.n_cob * 32 + gc] : 0.f;
  }
  // one split contraction: acc[cb][rb] = D[row][channel] (lane: channel col of block cb; reg r: row (r&3) + 8 (r>>2) + 4 half)
  auto run = [&](const float *Xp, const float *Wp, int x_ld, int k_pad, f32x16 (&acc)[CBW][2]) __attribute__((always_inline)) {
    float4 xr[XP], wr[WP];
    auto load_chunk = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < XP; ++p) {
        int grow = row0 + p * 32 + l_row;
        grow = grow < a.rows ? grow : a.rows - 1;
        xr[p] = *reinterpret_cast<const float4 *>(Xp + (size_t)grow * x_ld + kc * BK + l_c);
      }
#pragma unroll
      for (int p = 0; p < WP; ++p) {
        int gco = cob0 * 32 + p * 32 + l_row;
        gco = gco < a.n_cob * 32 ? gco : a.n_cob * 32 - 1;  // (channels beyond the matrix are never stored)
        wr[p] = *reinterpret_cast<const float4 *>(Wp + (size_t)gco * k_pad + kc * BK + l_c);
      }
    };
    auto store_chunk = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < XP; ++p) {
        f16x4 hi, lo;
        split4(xr[p], hi, lo);
        *reinterpret_cast<f16x4 *>(Xh + (p * 32 + l_row) * LDK + l_c) = hi;
        *reinterpret_cast<f16x4 *>(Xl + (p * 32 + l_row) * LDK + l_c) = lo;
      }
#pragma unroll
      for (int p = 0; p < WP; ++p) {
        f16x4 hi, hs, lo;
        gxs_split4w(wr[p], hi, hs, lo);
        *reinterpret_cast<f16x4 *>(Wh + (p * 32 + l_row) * LDK + l_c) = hi;
        *reinterpret_cast<f16x4 *>(Ws + (p * 32 + l_row) * LDK + l_c) = hs;
        *reinterpret_cast<f16x4 *>(Wl + (p * 32 + l_row) * LDK + l_c) = lo;
      }
    };
#pragma unroll
    for (int i = 0; i < CBW; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int nk = k_pad / BK;
    load_chunk(0);
    store_chunk();
    __syncthreads();
    for (int kc = 0; kc < nk; ++kc) {
      if (kc + 1 < nk) load_chunk(kc + 1);
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        f16x8 xh[2], xl[2], wh[CBW], ws[CBW], wl[CBW];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          xh[rb] = *reinterpret_cast<const f16x8 *>(Xh + (wave * 64 + rb * 32 + col) * LDK + st * 16 + half * 8);
          xl[rb] = *reinterpret_cast<const f16x8 *>(Xl + (wave * 64 + rb * 32 + col) * LDK + st * 16 + half * 8);
        }
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) {
          wh[cb] = *reinterpret_cast<const f16x8 *>(Wh + (cb * 32 + col) * LDK + st * 16 + half * 8);
          ws[cb] = *reinterpret_cast<const f16x8 *>(Ws + (cb * 32 + col) * LDK + st * 16 + half * 8);
          wl[cb] = *reinterpret_cast<const f16x8 *>(Wl + (cb * 32 + col) * LDK + st * 16 + half * 8);
        }
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) {  // rows x channels
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[rb], ws[cb], acc[cb][rb], 0, 0, 0);
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl[rb], wh[cb], acc[cb][rb], 0, 0, 0);
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[rb], wl[cb], acc[cb][rb], 0, 0, 0);
          }
      }
      __syncthreads();  // every wave is done reading the stage
      if (kc + 1 < nk) {
        store_chunk();
        __syncthreads();
      }
    }
#pragma unroll
    for (int i = 0; i < CBW; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] *= 1.f / 2048.f;
  };
  f32x16 vacc[CBW][2], sacc[CBW][2];
  run(a.X2, a.W2, a.x2_ld, a.k2, vacc);  // values first

  // ---- values: bias, GroupNorm over the sample (rows of WPS waves x the gs adjacent channel lanes), ReLU -- in place
  float *const red = reinterpret_cast<float *>(smem_raw);  // [wave][cb][32 channels][sum, sumsq] (the stage is free: run() ends on a barrier)
  const float *b_s = vec_lds, *b_v = vec_lds + CBW * 32, *gam = vec_lds + 2 * CBW * 32, *bet = vec_lds + 3 * CBW * 32;
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const float bv = b_v[cb * 32 + col];
    const f32x2 bv2 = {bv, bv};
    f32x2 s2 = {0.f, 0.f}, ss2 = {0.f, 0.f};  // (register pairs: v_pk_add / v_pk_fma_f32)
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x2 x = f32x2{vacc[cb][rb][2 * i], vacc[cb][rb][2 * i + 1]} + bv2;
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
    const f32x2 g2 = {g, g}, bt2 = {bt, bt};
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x2 v = __builtin_elementwise_fma(f32x2{vacc[cb][rb][2 * i], vacc[cb][rb][2 * i + 1]}, g2, bt2);
        vacc[cb][rb][2 * i] = fmaxf(v[0], 0.f); vacc[cb][rb][2 * i + 1] = fmaxf(v[1], 0.f);
      }
  }
  __syncthreads();  // every wave has read the statistics: the stage is free for the score contraction
  run(a.X1, a.W1, a.x1_ld, a.k1, sacc);
  // ---- base-2 soft-max over the K neighbour rows of every point, weighted sum of the values, one row out per point.  Round 6: written
  // like attn_tail_finish (attn_tail.hip) -- register pairs (v_pk_fma / v_pk_add_f32), log2 e folded into the bias step and v_exp_f32 on
  // the difference (libm's expf cost ~25 instructions per value here), v_rcp instead of an IEEE division (1 ulp), one lane-half
  // exchange for numerator and denominator together.  The scores' rounding (one fma at magnitude |s| log2 e) stays at a few 1e-6 of a
  // soft-max weight: fp32-grade (position forwards vs the fp32 mode: bench.py parity, tests/test_hip_engine.py).
  constexpr float LOG2E = 1.44269504088896340736f;
  auto pr = [](const f32x16 &v, int i) __attribute__((always_inline)) { return f32x2{v[2 * i], v[2 * i + 1]}; };
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const int pt0 = (row0 + wave_s * 64) >> KLOG, npts = a.rows >> KLOG;
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const float bsl = b_s[cb * 32 + col] * LOG2E;
    const f32x2 bs2 = {bsl, bsl}, l2 = {LOG2E, LOG2E};
    const bool cb_ok = cob0 + cb < a.n_cob;  // (uniform)
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int pg = 0; pg < GPB; ++pg) {
        // rows of point pg inside the 32-row block: 16 -> regs 8pg .. 8pg+7 (both halves); 8 -> regs 4pg .. 4pg+3
        constexpr int PPG = 8 / GPB;  // register pairs per point
        f32x2 sc[PPG];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < PPG; ++j) {
          sc[j] = __builtin_elementwise_fma(pr(sacc[cb][rb], pg * PPG + j), l2, bs2);
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
          num2 = __builtin_elementwise_fma(e, pr(vacc[cb][rb], pg * PPG + j), num2);
        }
        uint32_t un = __float_as_uint(num2[0] + num2[1]), ud = __float_as_uint(den2[0] + den2[1]);
        lane32_swap(un, ud);
        const float tot = __uint_as_float(un) + __uint_as_float(ud);  // lower lanes: numerator, upper lanes: denominator
        uint32_t ua = __float_as_uint(tot), ub = ua;
        lane32_swap(ua, ub);  // ub (lower lanes) = the upper lanes' tot
        const int pidx = rb * GPB + pg;  // point of the wave
        if (half == 0 && pt0 + pidx < npts && cb_ok) {
          const float v = tot * __builtin_amdgcn_rcpf(__uint_as_float(ub));
          a.out[(size_t)(pt0 + pidx) * a.out_ld + (cob0 + cb) * 32 + col] = v;
          // second copy into the columns of a later concatenation buffer (the skip input of an FP block's second Mlp)
          if (a.out2 && (cob0 + cb) * 32 + col < a.out2_n)
            a.out2[(size_t)(pt0 + pidx) * a.out2_ld + (cob0 + cb) * 32 + col] = v;
        }
      }
  }
}

}  // namespace

// SLIDE_OP_ATTN_TAIL with f[1] bit 3: float rows, float row-major weights, float output (split arithmetic)
int slide_launch_attn_tail_split(const SlideOp &o, hipStream_t s) {
  TailSArgs a;
  a.X1 = (const float *)o.p[0]; a.W1 = (const float *)o.p[1]; a.X2 = (const float *)o.p[2]; a.W2 = (const float *)o.p[3];
  a.out = (float *)o.p[4]; a.vec = (const float *)o.p[5];
  a.out2 = (float *)o.p[7]; a.out2_ld = (int)o.f[2]; a.out2_n = (int)o.f[3];
  a.rows = o.i[0]; a.x1_ld = o.i[1]; a.k1 = o.i[2]; a.x2_ld = o.i[3]; a.k2 = o.i[4]; a.n_cob = o.i[5];
  a.gs = o.i[7]; a.n_norm = o.i[8]; a.out_ld = o.i[9];
  a.inv_count = o.f[0];
  const int npxl = o.i[6];
  if (a.k1 % 32 || a.k2 % 32 || a.k1 <= 0 || a.k2 <= 0 || a.rows <= 0 || a.n_cob <= 0 || a.x1_ld % 4 || a.x2_ld % 4) return -3;
  if ((uintptr_t)a.X1 % 16 || (uintptr_t)a.X2 % 16 || (uintptr_t)a.W1 % 16 || (uintptr_t)a.W2 % 16 || !a.out || !a.vec) return -3;
  constexpr int LDK = TileT<SLIDE_PREC_SPLIT>::LDK;
  const size_t shm = (size_t)(2 * TM + 3 * 64) * LDK * 2 + 4 * 2 * 32 * 4 + 64;
  const int ntc = (a.n_cob + 1) / 2, ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
  if (npxl == 8) hipLaunchKernelGGL(attn_tail_split_kernel<8>, dim3(grid), dim3(256), shm, s, a);
  else if (npxl == 7) hipLaunchKernelGGL(attn_tail_split_kernel<7>, dim3(grid), dim3(256), shm, s, a);
  else return -4;
  return (int)hipGetLastError();
}
