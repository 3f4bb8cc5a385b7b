// gemm_ring.hip -- the GEMM kernels of the fused latent-DDPM denoiser for gfx950: the register-staged fp32 / split / fp16
// kernel, the LDS-DMA ring kernels and the small-launch kernels, with their launchers (SLIDE_OP_GEMM, SLIDE_OP_PAIR_FIRST,
// SLIDE_OP_GEMM_ATTEND; include/slide_engine.h).
//
// Data layout: every activation is a channel-minor fp32 matrix [B*npx][ld] in HBM (npx = 256 for the
// set-abstraction blocks: 16 points x 16 neighbours; 128 for the kNN-feature-propagation blocks; 16 for
// per-point tensors).  A 1x1 convolution is D[co][row] = sum_k W[co][k] X[row][k] on the matrix cores:
//   * fp32 mode: v_mfma_f32_32x32x2_f32  (bit-exact fp32 fma chain; parity mode)
//   * fp16 mode: v_mfma_f32_32x32x16_f16 (fp16 operands, fp32 accumulate; throughput mode)
// W is the A operand (rows = output channels), X the B operand (columns = points), so each lane ends up
// with 4 consecutive channels of one point -> 16-byte channel-minor stores, and the 16 neighbours of a point
// sit in 16 adjacent lanes.  One workgroup (4 waves, 64-wide) owns 256 rows = whole samples, so the
// GroupNorm statistics of a sample never leave the workgroup: bias, ReLU, GroupNorm, t-embedding /
// class-embedding add and the residual are all applied in the epilogue.
#include "gemm_common.h"
#include "gemm_small.h"
#include "launch.h"

namespace {

// (split mode: its two stages of four fp16 planes take 102 KB of LDS -- one workgroup per CU anyway, so it may use the whole
//  register file: the second accumulator set of the cross products does not fit 256 registers next to the 16-row epilogue)
template <int PREC, int NPXL, int CBW, bool PAIRRES = false>
__global__ __launch_bounds__(256, (PREC == SLIDE_PREC_SPLIT && NPXL == 4) ? 1 : 2) void gemm_kernel(GemmArgs a) {
  using T = typename TileT<PREC>::T;
  constexpr int LDK = TileT<PREC>::LDK;
  constexpr int EPL = TileT<PREC>::EPL;   // elements per 16-byte load
  constexpr int TPR = BK / EPL;           // threads per tile row
  constexpr int RPP = 256 / TPR;          // rows per pass
  constexpr int TN = 32 * CBW;
  constexpr int XP = TM / RPP, WP = TN / RPP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr bool SPLIT = PREC == SLIDE_PREC_SPLIT;
  // LDS element type of a stage: T, or (split mode) _Float16 with two planes per operand tile: [X hi | W hi | X lo | W lo]
  using TS = typename std::conditional<SPLIT, _Float16, T>::type;
  TS *const sbase = reinterpret_cast<TS *>(smem_raw);
  constexpr int STAGE = (SPLIT ? 2 : 1) * (TM + TN) * LDK;
  // split mode keeps ONE stage in LDS (51 KB: two workgroups per CU; the next chunk waits in registers, as in the other modes,
  // at the price of a second barrier per chunk)
  constexpr int NSTG = SPLIT ? 1 : 2;
  // consumer-side affine of the fp32 / split modes on 128- / 256-row samples: the tile's one or two samples' scale / shift vectors
  // are staged ONCE in LDS ([sample][scale | shift][k_pad] floats behind the epilogue tables) and applied when a chunk is written to
  // its stage -- loading them per X row (two more global loads per 16 bytes of X) made these launches 2x slower than their plain twins
  constexpr bool AFF_LDS = PREC != SLIDE_PREC_F16 && NPXL >= 7;
  constexpr int AFF_NS = TM >> (NPXL >= 7 ? NPXL : 7);

  const int ntc = (a.n_cob + CBW - 1) / CBW;
  const int ntr = (a.rows + TM - 1) / TM;
  // XCD-aware mapping: workgroup id % 8 picks the XCD (observed dispatch rule); all channel tiles of one
  // row tile share that XCD's L2, so the X panel is fetched from HBM once.
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr >= ntr) return;
  const int row0 = tr * TM, cob0 = tc * CBW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const T *X = reinterpret_cast<const T *>(a.X);
  const T *W = reinterpret_cast<const T *>(a.W);

  f32x16 acc[CBW][2];
  f32x16 acc2[SPLIT ? CBW : 1][2];  // split mode: the two cross products hi*lo + lo*hi (scaled by 2^11), folded in at the end
#pragma unroll
  for (int i = 0; i < CBW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[i][j][r] = 0.f;
        if (SPLIT) acc2[SPLIT ? i : 0][j][r] = 0.f;
      }

  float4 xr[XP], wr[WP];  // raw 16-byte pieces in flight
  const int l_row = tid / TPR, l_c = (tid % TPR) * EPL;

  auto load_chunk = [&](int kc) {
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const int grow = row0 + p * RPP + l_row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (grow < a.rows) {
        v = *reinterpret_cast<const float4 *>(X + (size_t)grow * a.x_ld + kc * BK + l_c);
        if (a.in_scale && !AFF_LDS) {  // consumer-side GroupNorm affine (only the attention weight_conv.2 GEMMs)
          const size_t o = (size_t)(grow >> NPXL) * a.in_bs + kc * BK + l_c;
          if (PREC != SLIDE_PREC_F16) {
            const float4 sc = *reinterpret_cast<const float4 *>(a.in_scale + o);
            const float4 sh = *reinterpret_cast<const float4 *>(a.in_shift + o);
            v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
          } else {
            f16x8 h = *reinterpret_cast<f16x8 *>(&v);
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = (_Float16)((float)h[j] * a.in_scale[o + j] + a.in_shift[o + j]);
            v = *reinterpret_cast<float4 *>(&h);
          }
        }
      }
      xr[p] = v;
    }
#pragma unroll
    for (int p = 0; p < WP; ++p) {
      const int gco = cob0 * 32 + p * RPP + l_row;
      wr[p] = gco < a.n_cob * 32 ? *reinterpret_cast<const float4 *>(W + (size_t)gco * a.k_pad + kc * BK + l_c)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  const float *aff_lds = nullptr;  // set below (behind the epilogue tables)
  auto store_chunk = [&](int s, int kc) {
    TS *Xs = sbase + s * STAGE;
    TS *Ws = Xs + TM * LDK;
    if constexpr (AFF_LDS) {
      if (a.in_scale) {
#pragma unroll
        for (int p = 0; p < XP; ++p) {
          const int trow = p * RPP + l_row;
          if (row0 + trow < a.rows) {
            const float *ap = aff_lds + (size_t)((trow >> NPXL) * 2) * a.k_pad + kc * BK + l_c;
            const float4 sc = *reinterpret_cast<const float4 *>(ap), sh = *reinterpret_cast<const float4 *>(ap + a.k_pad);
            float4 &v = xr[p];
            v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
          }
        }
      }
    }
    if constexpr (SPLIT) {
      _Float16 *Xl = Xs + (TM + TN) * LDK, *Wl = Xl + TM * LDK;
#pragma unroll
      for (int p = 0; p < XP; ++p) {
        f16x4 hi, lo;
        split4(xr[p], hi, lo);
        *reinterpret_cast<f16x4 *>(Xs + (p * RPP + l_row) * LDK + l_c) = hi;
        *reinterpret_cast<f16x4 *>(Xl + (p * RPP + l_row) * LDK + l_c) = lo;
      }
#pragma unroll
      for (int p = 0; p < WP; ++p) {
        f16x4 hi, lo;
        split4(wr[p], hi, lo);
        *reinterpret_cast<f16x4 *>(Ws + (p * RPP + l_row) * LDK + l_c) = hi;
        *reinterpret_cast<f16x4 *>(Wl + (p * RPP + l_row) * LDK + l_c) = lo;
      }
    } else {
#pragma unroll
      for (int p = 0; p < XP; ++p) *reinterpret_cast<float4 *>(Xs + (p * RPP + l_row) * LDK + l_c) = xr[p];
#pragma unroll
      for (int p = 0; p < WP; ++p) *reinterpret_cast<float4 *>(Ws + (p * RPP + l_row) * LDK + l_c) = wr[p];
    }
  };
  auto compute = [&](int s) {
    const TS *Xs = sbase + s * STAGE;
    const TS *Ws = Xs + TM * LDK;
    if constexpr (SPLIT) {
      const _Float16 *Xl = Xs + (TM + TN) * LDK, *Wl = Xl + TM * LDK;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        f16x8 ah[CBW], al[CBW], bh[2], bl[2];
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) {
          ah[cb] = *reinterpret_cast<const f16x8 *>(Ws + (cb * 32 + col) * LDK + st * 16 + half * 8);
          al[cb] = *reinterpret_cast<const f16x8 *>(Wl + (cb * 32 + col) * LDK + st * 16 + half * 8);
        }
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          bh[rb] = *reinterpret_cast<const f16x8 *>(Xs + (wave * 64 + rb * 32 + col) * LDK + st * 16 + half * 8);
          bl[rb] = *reinterpret_cast<const f16x8 *>(Xl + (wave * 64 + rb * 32 + col) * LDK + st * 16 + half * 8);
        }
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) {
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cb], bh[rb], acc[cb][rb], 0, 0, 0);
            acc2[SPLIT ? cb : 0][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cb], bl[rb], acc2[SPLIT ? cb : 0][rb], 0, 0, 0);
            acc2[SPLIT ? cb : 0][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[cb], bh[rb], acc2[SPLIT ? cb : 0][rb], 0, 0, 0);
          }
      }
    } else if (PREC == SLIDE_PREC_F32) {
      const float *Xf = reinterpret_cast<const float *>(Xs);
      const float *Wf = reinterpret_cast<const float *>(Ws);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4 af[CBW], bf[2];
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb)
          af[cb] = *reinterpret_cast<const float4 *>(Wf + (cb * 32 + col) * LDK + q * 8 + half * 4);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          bf[rb] = *reinterpret_cast<const float4 *>(Xf + (wave * 64 + rb * 32 + col) * LDK + q * 8 + half * 4);
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) {
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cb].x, bf[rb].x, acc[cb][rb], 0, 0, 0);
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cb].y, bf[rb].y, acc[cb][rb], 0, 0, 0);
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cb].z, bf[rb].z, acc[cb][rb], 0, 0, 0);
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cb].w, bf[rb].w, acc[cb][rb], 0, 0, 0);
          }
      }
    } else {
      const _Float16 *Xh = reinterpret_cast<const _Float16 *>(Xs);
      const _Float16 *Wh = reinterpret_cast<const _Float16 *>(Ws);
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        f16x8 af[CBW], bf[2];
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb)
          af[cb] = *reinterpret_cast<const f16x8 *>(Wh + (cb * 32 + col) * LDK + st * 16 + half * 8);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          bf[rb] = *reinterpret_cast<const f16x8 *>(Xh + (wave * 64 + rb * 32 + col) * LDK + st * 16 + half * 8);
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
            acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[cb], bf[rb], acc[cb][rb], 0, 0, 0);
      }
    }
  };

  uint32_t *const epi_lds = reinterpret_cast<uint32_t *>(smem_raw + NSTG * (size_t)STAGE * sizeof(TS));
  float *const vec_lds = reinterpret_cast<float *>(epi_lds + CBW * EPI_DW + (CBW * EPI_DW) % 4);
  stage_epilogue_tables<CBW>(a, cob0, tid, epi_lds, vec_lds);
  if constexpr (AFF_LDS) {
    if (a.in_scale) {
      float *al = vec_lds + CBW * 96;
      const int nb = a.rows >> NPXL;
      for (int i = tid * 4; i < AFF_NS * a.k_pad; i += 1024) {
        const int sm = i / a.k_pad, k = i - sm * a.k_pad;
        int b = (row0 >> NPXL) + sm;
        b = b < nb ? b : nb - 1;
        *reinterpret_cast<float4 *>(al + (size_t)(sm * 2 + 0) * a.k_pad + k) = *reinterpret_cast<const float4 *>(a.in_scale + (size_t)b * a.in_bs + k);
        *reinterpret_cast<float4 *>(al + (size_t)(sm * 2 + 1) * a.k_pad + k) = *reinterpret_cast<const float4 *>(a.in_shift + (size_t)b * a.in_bs + k);
      }
      aff_lds = al;
      __syncthreads();
    }
  }

  const int nk = a.k_pad / BK;
#ifdef SLIDE_STAGGER
  const int koff = (tc * 5 + tr * 3) % nk;
#define KIDX(k) (((k) + koff) % nk)
#else
#define KIDX(k) (k)
#endif
  load_chunk(KIDX(0));
  store_chunk(0, KIDX(0));
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    if (kc + 1 < nk) load_chunk(KIDX(kc + 1));
    compute(kc & (NSTG - 1));
    if (NSTG == 1) __syncthreads();  // every wave is done reading the stage before it is overwritten
    if (kc + 1 < nk) store_chunk((kc + 1) & (NSTG - 1), KIDX(kc + 1));
    __syncthreads();
  }
#undef KIDX
  if constexpr (SPLIT) {
#pragma unroll
    for (int i = 0; i < CBW; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = fmaf(acc2[i][j][r], 1.f / 2048.f, acc[i][j][r]);
  }
  // (split mode stores float activations: the fp32 epilogue)
  gemm_epilogue<SPLIT ? SLIDE_PREC_F32 : PREC, NPXL, CBW, 2, PAIRRES>(a, acc, row0, cob0, wave, half, col, epi_lds, vec_lds,
                                                                      reinterpret_cast<float *>(smem_raw));
}

// ------------------------------------------------------------------------------------------------ small split GEMM
// Split-mode GEMM for SMALL launches (the 16-row per-point layers of the fp32-structured plan; the training step's layers at the
// reference's batch 32): tile 64 rows x 64 channels, wave (rb, cb) owns ONE 32x32 block over the whole K.  The 256-row tile of
// gemm_kernel leaves such a launch with a handful of workgroups (1408 rows x 512 channels: 48) whose cost is their own serial
// latency -- here the grid is 4x larger and a workgroup's K loop moves a quarter of the X rows per chunk.  Stage = four fp16
// planes [X hi | W hi | X lo | W lo] of 64 rows (20 KB), double-buffered; three workgroups per CU.  Same split arithmetic
// (hi*hi into one accumulator, hi*lo + lo*hi scaled by 2^11 into a second) and the common epilogue at one block per wave.
template <int NPXL>
__global__ __launch_bounds__(256, 3) void gemm_split_small_kernel(GemmArgs a) {
  constexpr int LDK = TileT<SLIDE_PREC_SPLIT>::LDK;
  constexpr int TR = 64;                       // tile rows = tile channels
  constexpr int PLANE = TR * LDK;              // halves per plane
  constexpr int STAGE = 4 * PLANE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  _Float16 *const sbase = reinterpret_cast<_Float16 *>(smem_raw);
  const int ntc = (a.n_cob + 1) / 2;
  const int tc = blockIdx.x % ntc, tr = blockIdx.x / ntc;
  const int row0 = tr * TR, cob0 = tc * 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int rb = wave >> 1, cb = wave & 1;
  const float *X = reinterpret_cast<const float *>(a.X);
  const float *W = reinterpret_cast<const float *>(a.W);
  f32x16 acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = acc2[r] = 0.f;
  // loads: 8 threads per 32-float row, 32 rows per pass, two passes per operand tile
  const int l_row = tid >> 3, l_c = (tid & 7) * 4;
  constexpr int PD = 3;  // chunks in flight in registers: a lone workgroup's global-load latency hides behind three K steps
  float4 xr[PD][2], wr[PD][2];
  auto load_chunk = [&](int kc, float4 (&xr)[2], float4 (&wr)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int grow = row0 + p * 32 + l_row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (grow < a.rows) {
        v = *reinterpret_cast<const float4 *>(X + (size_t)grow * a.x_ld + kc * BK + l_c);
      }
      xr[p] = v;
      const int gco = cob0 * 32 + p * 32 + l_row;
      wr[p] = gco < a.n_cob * 32 ? *reinterpret_cast<const float4 *>(W + (size_t)gco * a.k_pad + kc * BK + l_c)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  const float *aff_lds = nullptr;  // consumer-side affine: the tile's samples' [scale | shift][k_pad], staged once (set below)
  auto store_chunk = [&](int s, int kc, const float4 (&xr)[2], const float4 (&wr)[2]) __attribute__((always_inline)) {
    _Float16 *Xh = sbase + s * STAGE, *Wh = Xh + PLANE, *Xl = Wh + PLANE, *Wl = Xl + PLANE;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      f16x4 hi, lo;
      float4 v = xr[p];
      if (aff_lds && row0 + p * 32 + l_row < a.rows) {
        const float *ap = aff_lds + (size_t)(((p * 32 + l_row) >> NPXL) * 2) * a.k_pad + kc * BK + l_c;
        const float4 sc = *reinterpret_cast<const float4 *>(ap), sh = *reinterpret_cast<const float4 *>(ap + a.k_pad);
        v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
      }
      split4(v, hi, lo);
      *reinterpret_cast<f16x4 *>(Xh + (p * 32 + l_row) * LDK + l_c) = hi;
      *reinterpret_cast<f16x4 *>(Xl + (p * 32 + l_row) * LDK + l_c) = lo;
      split4(wr[p], hi, lo);
      *reinterpret_cast<f16x4 *>(Wh + (p * 32 + l_row) * LDK + l_c) = hi;
      *reinterpret_cast<f16x4 *>(Wl + (p * 32 + l_row) * LDK + l_c) = lo;
    }
  };
  uint32_t *const epi_lds = reinterpret_cast<uint32_t *>(smem_raw + 2 * (size_t)STAGE * sizeof(_Float16));
  float *const vec_lds = reinterpret_cast<float *>(epi_lds + 2 * EPI_DW + (2 * EPI_DW) % 4);
  SLIDE_STAMP(a, 0);
  stage_epilogue_tables<2>(a, cob0, tid, epi_lds, vec_lds);
  if (a.in_scale) {
    float *al = vec_lds + 2 * 96;
    const int nb = a.rows >> NPXL;
    for (int i = tid * 4; i < (TR >> NPXL) * a.k_pad; i += 1024) {
      const int sm = i / a.k_pad, k = i - sm * a.k_pad;
      int b = (row0 >> NPXL) + sm;
      b = b < nb ? b : nb - 1;
      *reinterpret_cast<float4 *>(al + (size_t)(sm * 2 + 0) * a.k_pad + k) = *reinterpret_cast<const float4 *>(a.in_scale + (size_t)b * a.in_bs + k);
      *reinterpret_cast<float4 *>(al + (size_t)(sm * 2 + 1) * a.k_pad + k) = *reinterpret_cast<const float4 *>(a.in_shift + (size_t)b * a.in_bs + k);
    }
    aff_lds = al;
    __syncthreads();
  }
  const int nk = a.k_pad / BK;
  load_chunk(0, xr[0], wr[0]);
  store_chunk(0, 0, xr[0], wr[0]);
#pragma unroll
  for (int j = 0; j < PD; ++j)
    if (j + 1 < nk) load_chunk(j + 1, xr[j], wr[j]);  // buffer j: chunks j + 1, j + 1 + PD, ...
  __syncthreads();
  SLIDE_STAMP(a, 1);
  for (int kc0 = 0; kc0 < nk; kc0 += PD) {
#pragma unroll
    for (int j = 0; j < PD; ++j) {
      const int kc = kc0 + j;
      if (kc >= nk) break;
      const _Float16 *Xh = sbase + (kc & 1) * STAGE, *Wh = Xh + PLANE, *Xl = Wh + PLANE, *Wl = Xl + PLANE;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const f16x8 ah = *reinterpret_cast<const f16x8 *>(Wh + (cb * 32 + col) * LDK + st * 16 + half * 8);
        const f16x8 al = *reinterpret_cast<const f16x8 *>(Wl + (cb * 32 + col) * LDK + st * 16 + half * 8);
        const f16x8 bh = *reinterpret_cast<const f16x8 *>(Xh + (rb * 32 + col) * LDK + st * 16 + half * 8);
        const f16x8 bl = *reinterpret_cast<const f16x8 *>(Xl + (rb * 32 + col) * LDK + st * 16 + half * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc2, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc2, 0, 0, 0);
      }
      // the other stage: its last readers passed the barrier of chunk kc - 1
      if (kc + 1 < nk) store_chunk((kc + 1) & 1, kc + 1, xr[j], wr[j]);
      __syncthreads();
      if (kc + 1 + PD < nk) load_chunk(kc + 1 + PD, xr[j], wr[j]);
    }
  }
  f32x16 one[1][1];
#pragma unroll
  for (int r = 0; r < 16; ++r) one[0][0][r] = fmaf(acc2[r], 1.f / 2048.f, acc[r]);
  SLIDE_STAMP(a, 2);
  gemm_epilogue<SLIDE_PREC_F32, NPXL, 1, 1>(a, one, row0 + rb * 32, cob0 + cb, 0, half, col, epi_lds + cb * EPI_DW, vec_lds + cb * 96,
                                            nullptr);
  SLIDE_STAMP(a, 5);
#ifdef SLIDE_TIMELINE
  if (a.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); SLIDE_STAMP(a, 6); }
#endif
}

// ------------------------------------------------------------------------------------------------ LDS-DMA GEMM
// fp16 throughput variant of gemm_kernel (no consumer-side affine): the X / W chunks go HBM/L2 -> LDS directly with
// `global_load_lds_dwordx4` (no VGPR staging), NST chunks deep, so many more bytes are in flight per CU than a
// register-staged prefetch allows.  An LDS-DMA instruction writes lane-linearly (base + 16 B x lane), so a stage is an
// unpadded [rows][32] fp16 image (64 B rows) and bank conflicts are avoided by swizzling on the SOURCE side: slot
// (lane & 3) of row r receives the 16-byte piece p = slot ^ ((r >> 2) & 3); fragment reads apply the same XOR
// (conflict-free for ds_read_b128's 16-lane groups).  One raw s_barrier per chunk; counted vmcnt keeps NST-2 chunks in
// flight across it.
// AFF: consumer-side GroupNorm affine (attention weight_conv.2): the per-(sample, channel) scale / shift vectors of the
// workgroup's samples are staged once in LDS (fp16) and applied in fp32 to the X fragments between LDS and MFMA.
// WC = 1: four waves, tile 256 rows x 32*CBW channels.  WC = 2: eight waves, tile 256 rows x 64*CBW channels -- wave
// (wr, wc) owns rows 64*wr.. and channel half wc, so the X chunk is fetched once per 64*CBW channels (less L2 -> LDS
// traffic per MAC, half as many prologues); each channel half runs the 4-wave epilogue on its own LDS tables.
template <int NPXL, int CBW, int NST, int BKT, bool AFF, int WC = 1, bool GAT = false, bool PAIRRES = false, bool ATTN = false>
__device__ __forceinline__ void glds_tile(const GemmArgs &a, unsigned char *smem_raw, const int tr, const int tc) {
  using T = _Float16;
  constexpr int NW = 4 * WC, NT = 256 * WC;  // waves, threads
  constexpr int TN = 32 * CBW * WC;
  // W rows staged per chunk: TN rounded up until the stage splits into whole DMA instructions per wave
  constexpr int TNS = ((TM + TN + 16 * NW - 1) / (16 * NW)) * (16 * NW) - TM;
  constexpr int RT = TM + TNS;             // tile rows per stage (X rows then W rows)
  constexpr int ROWB = BKT * 2;            // bytes per tile row (64 or 128 = one full cache line)
  constexpr int PPR = ROWB / 16;           // 16-byte pieces per row (4 or 8)
  constexpr int RPI = 64 / PPR;            // rows per LDS-DMA instruction (16 or 8)
  constexpr int NI = RT / RPI;             // LDS-DMA instructions per stage
  constexpr int LPW = NI / NW;             // per wave
  constexpr int STAGE_B = RT * ROWB;       // bytes
  constexpr int SWS = BKT == 32 ? 2 : 1;   // swizzle: slot = piece ^ ((row >> SWS) & (PPR - 1))
  static_assert(NI % NW == 0, "tile rows must split evenly over the waves");
  static_assert(!AFF || WC == 1, "the affine variant is four-wave only");

  const int row0 = tr * TM, cob0 = tc * CBW * WC;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wave = wv & 3, wc = wv >> 2;
  const int half = lane >> 5, col = lane & 31;

  SLIDE_STAMP(a, 0);
  // per-lane source pointers of this wave's LPW instructions (chunk 0); out-of-range rows are clamped to a valid row:
  // they only feed accumulator rows / channel blocks that are never stored
  // GAT: the grouped input is never materialised -- the feature columns of row (sample, point, neighbour) are DMA-read
  // straight from the neighbour's row of the point-feature table (per-lane source addresses are free), only the last
  // chunks (coordinate channels) come from a small assembled buffer.  ga[j] serves chunks < g_nsplit, gp[j] the rest.
  // CHUNK-MAJOR operands (BKT == 32): X [k / 32][rows][32] when x_ld == 32, W [k / 32][n_cob * 32][32] when a.w_cm -- the
  // chunk kc of a row is then kc * (rows x 32) elements further instead of kc * 32, and the 16 rows of one DMA instruction
  // are consecutive memory.  x_cs / w_cs: elements between consecutive chunks of one row.
  constexpr int NXI = TM / (RPI * NW);  // instructions j < NXI carry X rows, the rest W rows
  static_assert(TM % (RPI * NW) == 0, "X rows must fill whole DMA instructions");
  const size_t x_cs = (BKT == 32 && a.x_ld == 32) ? (size_t)a.rows * 32 : BKT;
  const size_t w_cs = (BKT == 32 && a.w_cm) ? (size_t)a.n_cob * 32 * 32 : BKT;
  const int w_ld = (BKT == 32 && a.w_cm) ? 32 : a.k_pad;
  // gathered point-feature table: chunk-major [k / 32][samples * 16][32] when g_ldf == 32 -- the sixteen 64-byte pieces an
  // instruction gathers (the neighbours of one point) then lie inside ONE KB instead of sixteen rows
  const size_t g_cs = (GAT && BKT == 32 && a.g_ldf == 32) ? (size_t)(a.rows >> NPXL) * 16 * 32 : BKT;
  const T *gp[LPW];
  const T *ga[GAT ? LPW : 1];
#pragma unroll
  for (int j = 0; j < LPW; ++j) {
    const int trow = RPI * (j * NW + wv) + lane / PPR;
    const int piece = (lane % PPR) ^ ((trow >> SWS) & (PPR - 1));
    if (trow < TM) {
      int grow = row0 + trow;
      grow = grow < a.rows ? grow : a.rows - 1;
      gp[j] = reinterpret_cast<const T *>(a.X) + (size_t)grow * a.x_ld + piece * 8;
      if (GAT) {
        const int smp = grow >> NPXL, pxl = grow & ((1 << NPXL) - 1);
        const int nb = a.gidx[(smp * 16 + (pxl >> a.g_klog2)) * 16 + (pxl & ((1 << a.g_klog2) - 1))];
        ga[j] = reinterpret_cast<const T *>(a.gfeat) + (size_t)(smp * 16 + nb) * a.g_ldf + piece * 8;
        gp[j] -= (size_t)a.g_nsplit * x_cs;  // chunk index kc keeps counting over the whole K
      }
    } else {
      int gco = cob0 * 32 + (trow - TM);
      gco = gco < a.n_cob * 32 ? gco : a.n_cob * 32 - 1;
      gp[j] = reinterpret_cast<const T *>(a.W) + (size_t)gco * w_ld + piece * 8;
      if (GAT) ga[j] = gp[j];
    }
  }
  auto issue = [&](int kc, int st) {
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const T *src = (j < NXI) ? ((GAT && kc < a.g_nsplit) ? ga[GAT ? j : 0] + (size_t)kc * g_cs : gp[j] + (size_t)kc * x_cs)
                               : gp[j] + (size_t)kc * w_cs;
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)src,
                                       (__attribute__((address_space(3))) void *)(smem_raw + (size_t)st * STAGE_B +
                                                                                  (j * NW + wv) * 1024),
                                       16, 0, 0);
    }
  };

  // the ring is primed BEFORE the epilogue tables are staged: the first chunks' L2 latency covers the table reads
  const int nk = a.k_pad / BKT;
#pragma unroll
  for (int s0 = 0; s0 < NST - 1; ++s0)
    if (s0 < nk) issue(s0, s0);
  uint32_t *const epi_lds = reinterpret_cast<uint32_t *>(smem_raw + (size_t)NST * STAGE_B);
  float *const vec_lds = reinterpret_cast<float *>(epi_lds + CBW * WC * EPI_DW + (CBW * WC * EPI_DW) % 4);
  stage_epilogue_tables<CBW * WC, NT>(a, cob0, tid, epi_lds, vec_lds);
  constexpr int NSAMP = (1 << NPXL) >= TM ? 1 : TM >> NPXL;  // samples per workgroup
  _Float16 *const aff_lds = reinterpret_cast<_Float16 *>(vec_lds + CBW * WC * 96);  // [sample][scale | shift | add][k_pad]
  if (AFF) {
    static_assert(!AFF || NPXL >= 6, "the affine variant assumes one sample per wave");
    const int tps = a.aff_tps > 1 ? a.aff_tps : 1;
    const int nb = (a.rows >> NPXL) / tps, n_aff = NSAMP * a.k_pad;
    for (int i0 = tid; i0 < n_aff; i0 += 1024) {  // four elements per trip, their loads issued together
      float sc4[4], sh4[4], ad4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 256 * u < n_aff ? i0 + 256 * u : i0;
        const int sm = i / a.k_pad, k = i - sm * a.k_pad;
        int b = ((row0 >> NPXL) + sm) / tps;
        b = b < nb ? b : nb - 1;
        sc4[u] = a.in_scale[(size_t)b * a.in_bs + k];
        sh4[u] = a.in_shift[(size_t)b * a.in_bs + k];
        ad4[u] = (a.in_add && k < a.add_n) ? a.in_add[(size_t)b * a.add_bs + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 256 * u;
        if (i >= n_aff) break;
        const int sm = i / a.k_pad, k = i - sm * a.k_pad;
        aff_lds[(sm * 3 + 0) * a.k_pad + k] = (_Float16)sc4[u];
        aff_lds[(sm * 3 + 1) * a.k_pad + k] = (_Float16)sh4[u];
        aff_lds[(sm * 3 + 2) * a.k_pad + k] = (_Float16)ad4[u];
      }
    }
  }
  const _Float16 *const aff_w = aff_lds + (size_t)((wave * 64) >> NPXL) * 3 * a.k_pad;  // this wave's sample
  const bool aff_relu = AFF && a.aff_relu;
  const bool aff_add = AFF && a.in_add && a.add_n > 0;  // (the add applies with or without the ReLU)

  f32x16 acc[CBW][2];
#pragma unroll
  for (int i = 0; i < CBW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // row base offsets and swizzle keys of this lane's fragment rows (bytes inside a stage)
  int wrow[CBW], wkey[CBW], xrow[2], xkey[2];
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const int trow = TM + (wc * CBW + cb) * 32 + col;
    wrow[cb] = trow * ROWB; wkey[cb] = (trow >> SWS) & (PPR - 1);
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int trow = wave * 64 + rb * 32 + col;
    xrow[rb] = trow * ROWB; xkey[rb] = (trow >> SWS) & (PPR - 1);
  }

  SLIDE_STAMP(a, 1);
  for (int kc = 0; kc < nk; ++kc) {
    // chunk kc must have landed; up to NST-2 younger chunks may stay in flight (fewer in the tail -> drain)
    if (kc + NST - 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * LPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kc + NST - 1 < nk) issue(kc + NST - 1, (kc + NST - 1) % NST);  // overwrites the stage consumed at kc-1
    const unsigned char *sb = smem_raw + (size_t)(kc % NST) * STAGE_B;
#pragma unroll
    for (int st2 = 0; st2 < BKT / 16; ++st2) {
      f16x8 af[CBW], bf[2];
      const int piece = st2 * 2 + half;
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb) af[cb] = *reinterpret_cast<const f16x8 *>(sb + wrow[cb] + ((piece ^ wkey[cb]) << 4));
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) bf[rb] = *reinterpret_cast<const f16x8 *>(sb + xrow[rb] + ((piece ^ xkey[rb]) << 4));
      if (AFF) {
        const f16x8 sc = *reinterpret_cast<const f16x8 *>(aff_w + kc * BKT + piece * 8);
        const f16x8 sh = *reinterpret_cast<const f16x8 *>(aff_w + a.k_pad + kc * BKT + piece * 8);
        // packed fp16 fma (v_pk_fma_f16, one rounding like the fp32-then-convert form it replaces, 1/6 of the VALU ops).
        // scale / shift / add are fp16 copies of the fp32 vectors (2^-11 relative each): against normalising in fp32 and
        // storing the fp16 result (SLIDE_MODULE_DEFER=0) the GEMM output moves by <= 3e-3 of its L2 norm at |shift| ~ 6 and
        // |add| ~ 50 (tests/test_hip_modules.py::test_deferred_normalisation_matches_the_materialised_path); values beyond
        // fp16's range (65504) do not occur: scale = gamma * rstd <= gamma / sqrt(eps), shift and add are O(activations)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) bf[rb] = __builtin_elementwise_fma(bf[rb], sc, sh);
        if (aff_relu || aff_add) {  // deferred GroupNorm [+ ReLU] [+ embedding add] of the producing layer (module-level path)
          const f16x8 ad = *reinterpret_cast<const f16x8 *>(aff_w + 2 * a.k_pad + kc * BKT + piece * 8);
          const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) bf[rb] = (aff_relu ? __builtin_elementwise_max(bf[rb], zero) : bf[rb]) + ad;
        }
      }
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[cb], bf[rb], acc[cb][rb], 0, 0, 0);
    }
  }
  __syncthreads();  // every wave is done with the tiles before `red` reuses them
  SLIDE_STAMP(a, 2);

  if constexpr (ATTN)
    attend_epilogue<CBW>(a, acc, row0, cob0, wave, half, col, vec_lds, reinterpret_cast<float *>(smem_raw));
  else
    gemm_epilogue<SLIDE_PREC_F16, NPXL, CBW, 2, PAIRRES>(a, acc, row0, cob0 + wc * CBW, wave, half, col, epi_lds + wc * CBW * EPI_DW,
                                             vec_lds + wc * CBW * 96,
                                             reinterpret_cast<float *>(smem_raw) + wc * (256 + 128) * CBW);
  SLIDE_STAMP(a, 5);
#ifdef SLIDE_TIMELINE
  if (a.dbg) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    SLIDE_STAMP(a, 6);
  }
#endif
}

// Scheduler.  a.sched == nullptr: one tile per workgroup (grid = tiles).  Otherwise PERSISTENT: 2 workgroups per CU
// pull tiles from per-XCD counters (tile columns of one row tile stay on one XCD's L2), so workgroups drift out of
// phase instead of all bursting their loads, then all bursting their stores, and there is no last partial round.
// The workgroup in the odd wave slot of a CU starts `stagger` later so that the pair begins half a tile apart.
// sched[0..7] = next tile per XCD, sched[8] = finished workgroups; the last one to finish re-arms the counters.
template <int NPXL, int CBW, int NST, int BKT, bool AFF, bool GAT = false, bool PAIRRES = false>
__global__ __launch_bounds__(256, 2) void gemm_glds_kernel(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + CBW - 1) / CBW;
  const int ntr = (a.rows + TM - 1) / TM;
  const int xcd = blockIdx.x & 7;
  if (!a.sched) {
    const int q0 = blockIdx.x >> 3;
    const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
    if (tr >= ntr) return;
    glds_tile<NPXL, CBW, NST, BKT, AFF, 1, GAT, PAIRRES>(a, smem_raw, tr, tc);
    return;
  }
  const int my_tiles = ((ntr - xcd + 7) / 8) * ntc;  // row tiles tr = xcd, xcd + 8, ...
  volatile int *const s_tile = reinterpret_cast<volatile int *>(smem_raw + a.shm_bytes - 16);
  // a.stagger < 0: STATIC persistent schedule -- workgroup l of an XCD takes tiles l, l + n, l + 2n, ... (no counter):
  // the store drain and the relaunch of a workgroup are overlapped by its next tile's prologue
  const bool fixed = a.stagger < 0;
  int next = blockIdx.x >> 3;
  const int step = gridDim.x >> 3;
  if (a.stagger > 0 && threadIdx.x < 64) {
    const unsigned slot = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 4);  // HW_ID.WAVE_ID
    if (slot & 1) {
      const unsigned long long t0 = wall_clock64();
      while (wall_clock64() - t0 < (unsigned long long)a.stagger) __builtin_amdgcn_s_sleep(32);
    }
  }
  for (;;) {
    int t = next;
    next += step;
    if (!fixed) {
      if (threadIdx.x == 0) *s_tile = atomicAdd(&a.sched[xcd], 1);
      __syncthreads();
      t = __builtin_amdgcn_readfirstlane(*s_tile);
    }
    if (t >= my_tiles) break;
#ifdef SLIDE_TIMELINE
    GemmArgs a2 = a;  // stamps indexed by tile instead of by workgroup
    if (a.dbg) a2.dbg = a.dbg + ((long long)(xcd + 8 * t) - (long long)blockIdx.x) * 16;
    glds_tile<NPXL, CBW, NST, BKT, AFF, 1, GAT, PAIRRES>(a2, smem_raw, (t / ntc) * 8 + xcd, t % ntc);
#else
    glds_tile<NPXL, CBW, NST, BKT, AFF, 1, GAT, PAIRRES>(a, smem_raw, (t / ntc) * 8 + xcd, t % ntc);
#endif
    __syncthreads();  // the epilogue's LDS reads are done before the next tile's tables / DMAs / s_tile land
  }
  if (!fixed && threadIdx.x == 0 && atomicAdd(&a.sched[8], 1) == (int)gridDim.x - 1) {
#pragma unroll
    for (int x = 0; x < 9; ++x) a.sched[x] = 0;
  }
}

// Three workgroups per CU: 64-channel tiles on a two-stage ring (41 KB of LDS) under a 168-VGPR budget -- one more
// resident workgroup to fill the epilogue / prologue bubbles of the other two (opt-in: GemmArgs.stagger == 3).
template <int NPXL, bool AFF, bool GAT, bool PAIRRES = false>
__global__ __launch_bounds__(256, 3) void gemm_glds_occ3_kernel(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + 1) / 2;
  const int ntr = (a.rows + TM - 1) / TM;
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr >= ntr) return;
  glds_tile<NPXL, 2, 2, 32, AFF, 1, GAT, PAIRRES>(a, smem_raw, tr, tc);
}

// SLIDE_OP_GEMM_ATTEND (round 6): the 256 x 64 ring tile with the ATTEND epilogue (gemm_common.h) -- the score GEMM of an
// AttentionModule of the module-level path, its soft-max over the neighbours and the weighted sum of the values in one launch
// (two-stage ring and 126 registers: three workgroups per CU, as gemm_glds_occ3_kernel -- the launch is HBM-bound)
template <bool AFF>
__global__ __launch_bounds__(256, 3) void gemm_attend_kernel(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + 1) / 2;
  const int ntr = (a.rows + TM - 1) / TM;
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr >= ntr) return;
  glds_tile<8, 2, 2, 32, AFF, 1, false, false, true>(a, smem_raw, tr, tc);
}

// eight-wave variant (one tile per workgroup, one workgroup per CU: its deeper ring needs the LDS of two)
template <int NPXL, int CBW, int NST>
__global__ __launch_bounds__(512, 2) void gemm_glds8_kernel(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + 2 * CBW - 1) / (2 * CBW);
  const int ntr = (a.rows + TM - 1) / TM;
  const int xcd = blockIdx.x & 7, q0 = blockIdx.x >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;
  if (tr >= ntr) return;
  glds_tile<NPXL, CBW, NST, 32, false, 2>(a, smem_raw, tr, tc);
}

template <int NST, bool AFF>
__global__ __launch_bounds__(256, 3) void gemm_small_kernel(GemmArgs a) {
  small_body<NST, AFF, 0>(a, PairArgs(), blockIdx.x);
}

// The per-point GEMM of a block's pair decomposition and the pair-table pass (SLIDE_OP_PAIR_NORM version 1) as ONE launch
// (SLIDE_OP_PAIR_FIRST): the products never go through memory.  FP: the 8-neighbour samples of the FP blocks.
template <bool FP>
__global__ __launch_bounds__(256, 3) void pair_first_kernel(GemmArgs a, PairArgs pa) {
  small_body<2, false, FP ? 2 : 1>(a, pa, blockIdx.x);
}

template <int PREC, int NPXL, int CBW, bool PAIRRES = false>
int launch_gemm(const GemmArgs &a, hipStream_t s) {
  constexpr int LDK = TileT<PREC>::LDK;
  // (split mode: two fp16 planes per operand tile)
  const size_t aff = (PREC != SLIDE_PREC_F16 && NPXL >= 7 && a.in_scale) ? (size_t)(TM >> NPXL) * 2 * a.k_pad * 4 : 0;
  const size_t shm = (PREC == SLIDE_PREC_SPLIT ? (size_t)(TM + 32 * CBW) * LDK * 4 : 2 * (size_t)(TM + 32 * CBW) * LDK * sizeof(typename TileT<PREC>::T)) +
                     CBW * (sizeof(SlideEpi) + 96 * 4) + 16 + aff;
  if (shm > 160 * 1024) return -8;
  const int ntc = (a.n_cob + CBW - 1) / CBW, ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
  allow_dynamic_lds<&gemm_kernel<PREC, NPXL, CBW, PAIRRES>>(160 * 1024);
  hipLaunchKernelGGL((gemm_kernel<PREC, NPXL, CBW, PAIRRES>), dim3(grid), dim3(256), shm, s, a);
  return (int)hipGetLastError();
}

int launch_gemm_split_small(const GemmArgs &a, hipStream_t s) {
  constexpr int LDK = TileT<SLIDE_PREC_SPLIT>::LDK;
  const size_t shm = (size_t)2 * 4 * 64 * LDK * 2 + 2 * (sizeof(SlideEpi) + 96 * 4) + 32 + (a.in_scale ? (size_t)4 * 2 * a.k_pad * 4 : 0);
  if (shm > 64 * 1024) return -8;
  const int grid = ((a.rows + 63) / 64) * ((a.n_cob + 1) / 2);
  hipLaunchKernelGGL((gemm_split_small_kernel<4>), dim3(grid), dim3(256), shm, s, a);
  return (int)hipGetLastError();
}

template <int NPXL, int CBW, int NST, int BKT, bool AFF, bool GAT = false, bool PAIRRES = false>
int launch_gemm_glds(const GemmArgs &a, hipStream_t s) {
  constexpr int NSAMP = (1 << NPXL) >= TM ? 1 : TM >> NPXL;
  const size_t shm = (size_t)NST * (TM + (CBW < 2 ? 64 : 32 * CBW)) * BKT * 2 + CBW * (sizeof(SlideEpi) + 96 * 4) + 32 +
                     (AFF ? (size_t)NSAMP * 3 * a.k_pad * 2 : 0);
  if (shm > 80 * 1024 && BKT == 32 && NST <= 3) return -8;  // two workgroups per CU must fit
  if (shm > 160 * 1024) return -8;
  const int ntc = (a.n_cob + CBW - 1) / CBW, ntr = (a.rows + TM - 1) / TM;
  int grid = ((ntr + 7) / 8) * 8 * ntc;
  GemmArgs b = a;
  b.shm_bytes = (int)((shm + 15) & ~(size_t)15);
  if (b.sched && grid > 512 && NST <= 3) grid = 512;  // persistent: two resident workgroups per CU pull the tiles
  else b.sched = nullptr;
  allow_dynamic_lds<&gemm_glds_kernel<NPXL, CBW, NST, BKT, AFF, GAT, PAIRRES>>((NST > 3 || BKT > 32) ? 160 * 1024 : 84 * 1024);
  hipLaunchKernelGGL((gemm_glds_kernel<NPXL, CBW, NST, BKT, AFF, GAT, PAIRRES>), dim3(grid), dim3(256), (size_t)b.shm_bytes, s, b);
  return (int)hipGetLastError();
}

template <int NPXL, bool AFF, bool GAT, bool PAIRRES = false>
int launch_gemm_occ3(const GemmArgs &a, hipStream_t s) {
  constexpr int NSAMP = (1 << NPXL) >= TM ? 1 : TM >> NPXL;
  const size_t shm = (size_t)2 * (TM + 64) * 32 * 2 + 2 * (sizeof(SlideEpi) + 96 * 4) + 32 + (AFF ? (size_t)NSAMP * 3 * a.k_pad * 2 : 0);
  if (shm > 53 * 1024) return -8;  // three workgroups per CU must fit
  const int ntc = (a.n_cob + 1) / 2, ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
  GemmArgs b = a;
  b.shm_bytes = (int)((shm + 15) & ~(size_t)15);
  b.sched = nullptr;
  allow_dynamic_lds<&gemm_glds_occ3_kernel<NPXL, AFF, GAT, PAIRRES>>(53 * 1024);
  hipLaunchKernelGGL((gemm_glds_occ3_kernel<NPXL, AFF, GAT, PAIRRES>), dim3(grid), dim3(256), (size_t)b.shm_bytes, s, b);
  return (int)hipGetLastError();
}

template <int NPXL, int CBW, int NST>
int launch_gemm_glds8(const GemmArgs &a, hipStream_t s) {
  constexpr int TNS8 = ((TM + 64 * CBW + 127) / 128) * 128 - TM;
  const size_t shm = (size_t)NST * (TM + TNS8) * 32 * 2 + 2 * CBW * (sizeof(SlideEpi) + 96 * 4) + 32;
  if (shm > 160 * 1024) return -8;
  const int ntc = (a.n_cob + 2 * CBW - 1) / (2 * CBW), ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
  allow_dynamic_lds<&gemm_glds8_kernel<NPXL, CBW, NST>>(160 * 1024);
  GemmArgs b = a;
  b.sched = nullptr;
  b.shm_bytes = (int)shm;
  hipLaunchKernelGGL((gemm_glds8_kernel<NPXL, CBW, NST>), dim3(grid), dim3(512), shm, s, b);
  return (int)hipGetLastError();
}


template <int NST, bool AFF>
int launch_gemm_small_t(const GemmArgs &a, hipStream_t s) {
  const size_t shm = (size_t)4 * NST * 6144 + 2 * (sizeof(SlideEpi) + 96 * 4) + 32 + (AFF ? (size_t)4 * 2 * a.k_pad * 2 + 1024 : 0);
  const int grid = ((a.rows + 63) / 64) * ((a.n_cob + 1) / 2);
  allow_dynamic_lds<&gemm_small_kernel<NST, AFF>>(128 * 1024);
  hipLaunchKernelGGL((gemm_small_kernel<NST, AFF>), dim3(grid), dim3(256), shm, s, a);
  return (int)hipGetLastError();
}

template <bool FP>
int launch_pair_first_t(const GemmArgs &a, const PairArgs &pa, hipStream_t s) {
  const int grid = ((a.rows + 63) / 64) * ((a.n_cob + 1) / 2);
  // (51 KB -> THREE workgroups per CU: the four samples' coordinates behind the rings; the FP blocks' neighbour / distance / weight
  //  slots wait in registers and land in the dead ring area after the K loop, gemm_small.h)
  const size_t shm = (size_t)4 * 2 * 6144 + 2 * (sizeof(SlideEpi) + 96 * 4) + 32 + 192 * 4;
  allow_dynamic_lds<&pair_first_kernel<FP>>(128 * 1024);
  hipLaunchKernelGGL((pair_first_kernel<FP>), dim3(grid), dim3(256), shm, s, a, pa);
  return (int)hipGetLastError();
}

// SLIDE_OP_PAIR_FIRST (include/slide_engine.h)
int run_pair_first(const SlideOp &o, hipStream_t s) {
  GemmArgs a = GemmArgs();
  a.X = o.p[0]; a.W = o.p[1]; a.epi = (const SlideEpi *)o.p[2];
  a.aff_tps = 1;
  a.rows = o.i[0]; a.x_ld = o.i[1]; a.k_pad = o.i[2]; a.n_cob = o.i[3];
  resolve_epi(a);
  a.dbg = (unsigned long long *)o.p[13];
  PairArgs pa;
  pa.pair_cob0 = o.i[4]; pa.ld = o.i[5];
  pa.xyz = (const float *)o.p[3]; pa.wa = (const float *)o.p[4]; pa.wb = (const float *)o.p[5];
  pa.ta = (_Float16 *)o.p[6]; pa.tb = (_Float16 *)o.p[7];
  pa.nbr = (const int *)o.p[8]; pa.d2t = (const float *)o.p[9]; pa.wt = (const float *)o.p[10];
  pa.vv_in = (const float *)o.p[11]; pa.vv_out = (float *)o.p[12];
  if (a.k_pad % BK || a.x_ld % 8 || a.rows <= 0 || a.n_cob <= 0 || a.rows % 16 || pa.pair_cob0 < 0 || pa.pair_cob0 > a.n_cob ||
      pa.ld != (a.n_cob - pa.pair_cob0) * 32)
    return -3;
  if (o.i[6] == 8) {
    if (!pa.nbr || !pa.d2t || !pa.wt || !pa.vv_in || !pa.vv_out) return -3;
    return launch_pair_first_t<true>(a, pa, s);
  }
  return launch_pair_first_t<false>(a, pa, s);
}

int launch_gemm_small(const GemmArgs &a, hipStream_t s) {
  const int grid = ((a.rows + 63) / 64) * ((a.n_cob + 1) / 2);
  // two stages per wave (64 KB of LDS: the size of the partial-sum exchange) rather than three (96 KB): the workgroup
  // then fits a CU beside two 41 KB GEMM workgroups of the other chains (0.913 vs 0.927 ms/step); a.stagger == 5 keeps
  // three stages on single-round grids, for A/B timing
#ifdef SLIDE_EXPERIMENTS
  const bool three = grid <= 256 && a.stagger == 5;
  if (three) return a.in_scale ? launch_gemm_small_t<3, true>(a, s) : launch_gemm_small_t<3, false>(a, s);
#endif
  (void)grid;
  return a.in_scale ? launch_gemm_small_t<2, true>(a, s) : launch_gemm_small_t<2, false>(a, s);
}

template <bool AFF>
int launch_gemm_attend(const GemmArgs &a, hipStream_t s) {
  const size_t shm = (size_t)2 * (TM + 64) * 32 * 2 + 2 * (sizeof(SlideEpi) + 96 * 4) + 32 + (AFF ? (size_t)3 * a.k_pad * 2 : 0);
  if (shm > 53 * 1024) return -8;  // three workgroups per CU must fit
  const int ntc = (a.n_cob + 1) / 2, ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
  GemmArgs b = a;
  b.shm_bytes = (int)((shm + 15) & ~(size_t)15);
  b.sched = nullptr;
  allow_dynamic_lds<&gemm_attend_kernel<AFF>>(53 * 1024);
  hipLaunchKernelGGL((gemm_attend_kernel<AFF>), dim3(grid), dim3(256), (size_t)b.shm_bytes, s, b);
  return (int)hipGetLastError();
}

// SLIDE_OP_GEMM_ATTEND (include/slide_engine.h)
int run_gemm_attend(const SlideOp &o, hipStream_t s) {
  GemmArgs a = GemmArgs();
  a.X = o.p[0]; a.W = o.p[1]; a.epi = (const SlideEpi *)o.p[2];
  a.in_scale = (const float *)o.p[3]; a.in_shift = (const float *)o.p[4];
  a.aff_tps = 1;
  if (a.in_scale) {
    a.in_add = (const float *)o.p[11];
    a.aff_tps = (int)o.f[1] > 1 ? (int)o.f[1] : 1;
    a.add_bs = (int)o.f[2];
    a.add_n = (int)o.f[3] >> 1;
    a.aff_relu = (int)o.f[3] & 1;
  }
  a.at_V = o.p[5]; a.at_out = o.p[6]; a.at_counts = (const int *)o.p[7]; a.at_vss = (const float *)o.p[8];
  a.rows = o.i[0]; a.x_ld = o.i[1]; a.k_pad = o.i[2]; a.n_cob = o.i[3]; a.in_bs = o.i[5];
  resolve_epi(a);
  const int K = o.i[4];
  a.at_ldv = o.i[6]; a.at_ldo = o.i[7]; a.at_pps = o.i[8] > 0 ? o.i[8] : 1; a.at_vrelu = o.i[9]; a.at_C = o.i[10];
  a.at_klog2 = K == 4 ? 2 : K == 8 ? 3 : K == 16 ? 4 : K == 32 ? 5 : -1;
  if (a.at_klog2 < 0 || a.rows <= 0 || a.rows % K || a.k_pad % BK || a.x_ld % 8 || a.n_cob <= 0 || !a.X || !a.W || !a.epi || !a.at_V ||
      !a.at_out || a.at_ldv % 4 || a.at_ldo % 4 || a.at_ldv < a.n_cob * 32 || a.at_ldo < a.n_cob * 32 || (a.in_scale && !a.in_shift))
    return -3;
  // input affine: the kernel takes the sample of a tile from the tile index (tile / aff_tps, clamped to rows / 256 / aff_tps - 1) --
  // whole tiles and whole samples only (fewer rows than one sample's tiles would clamp to sample -1)
  if (a.in_scale && a.rows % ((long long)TM * a.aff_tps)) return -3;
  return a.in_scale ? launch_gemm_attend<true>(a, s) : launch_gemm_attend<false>(a, s);
}

int run_gemm(const SlideOp &o, hipStream_t s) {
  GemmArgs a;
  a.X = o.p[0]; a.W = o.p[1]; a.epi = (const SlideEpi *)o.p[2];
  a.in_scale = (const float *)o.p[3]; a.in_shift = (const float *)o.p[4];
  // deferred normalisation (no gather): p[11] = add vectors, f[1] = tiles per sample, f[2] = add_bs, f[3] = 2 * add_n + relu
  a.in_add = nullptr; a.aff_relu = 0; a.add_bs = 0; a.add_n = 0; a.aff_tps = 1;
  if (a.in_scale && !o.p[8]) {
    a.in_add = (const float *)o.p[11];
    a.aff_tps = (int)o.f[1] > 1 ? (int)o.f[1] : 1;
    a.add_bs = (int)o.f[2];
    a.add_n = (int)o.f[3] >> 1;
    a.aff_relu = (int)o.f[3] & 1;
  }
  a.dbg = (unsigned long long *)o.p[5];
  a.stagger = (int)(o.f[0] * 100.f);
  a.sched = (int *)o.p[7];
  a.gfeat = o.p[8]; a.gidx = (const int *)o.p[9];
  a.gn_fin = (const SlideGnFin *)o.p[6];
  a.gx_d2 = (const float *)o.p[12]; a.gx_w = (const float *)o.p[13];  // PAIR_NBR residual (with p[9] the neighbour table)
  a.gx_ta = a.gx_tb = nullptr; a.gx_vv = nullptr; a.gx_add_idx = nullptr;
  a.g_nsplit = (int)o.f[1]; a.g_ldf = (int)o.f[2]; a.g_klog2 = (int)o.f[3];
  a.rows = o.i[0]; a.x_ld = o.i[1]; a.k_pad = o.i[2]; a.n_cob = o.i[3]; a.in_bs = o.i[5];
  a.ch_epi = nullptr; a.ch_n_cob = 0;
  resolve_epi(a);
  const int npxl = o.i[4], prec = o.i[6], cbw = o.i[7], glds = o.i[8] & 1;
  a.w_cm = (o.i[8] >> 1) & 1;  // chunk-major weights (ring kernels of the 128 / 256-row samples only)
  if ((o.i[8] >> 2) & 1) {     // a block of this GEMM carries a PAIR residual: the instantiations compiled for it
    if (prec == SLIDE_PREC_SPLIT && !glds && !a.in_scale && !o.p[8] && !o.p[10] && cbw == 2) {  // float tables (round 5)
      if (a.k_pad % BK || a.x_ld % 4 || a.rows <= 0 || a.n_cob <= 0) return -3;
      if (npxl == 8) return launch_gemm<SLIDE_PREC_SPLIT, 8, 2, true>(a, s);
      if (npxl == 7) return launch_gemm<SLIDE_PREC_SPLIT, 7, 2, true>(a, s);
      return -12;
    }
    if (!glds || prec != SLIDE_PREC_F16 || a.in_scale || o.p[8] || o.p[10]) return -12;
    // (two workgroups per CU, 256 registers: the three-workgroup form spills with the pair address arithmetic)
    if (npxl == 8) return launch_gemm_glds<8, 2, 3, 32, false, false, true>(a, s);
    if (npxl == 7) return launch_gemm_glds<7, 2, 3, 32, false, false, true>(a, s);
    return -12;
  }
  if (a.w_cm && (!glds || (npxl != 7 && npxl != 8) || o.p[10] || o.i[9] == 1)) return -11;
  if (a.k_pad % BK || a.x_ld % 8 || a.rows <= 0 || a.n_cob <= 0) return -3;
  // fp16 16-row launches: split-K small-launch kernel, with or without the input affine (i[9] == 3 keeps the 256-row
  // kernels, for A/B timing)
  // (up to 1024 tiles with the statistics finalisation, 8192 without: the wide per-point GEMMs of the pair decomposition --
  //  N = 1056 .. 1568 -- stay on this spill-free kernel instead of the 256-row ring tiles, which spill at 16 rows per sample)
  // (round 4: no tile limit without the finalisation -- a chain of 2048 samples used to fall back to the 256-row ring tiles,
  //  which spill at 16 rows per sample; those are experiments-build kernels now)
  if (prec == SLIDE_PREC_F16 && npxl == 4 && o.i[9] != 3 &&
      (!a.gn_fin || ((a.rows + 63) / 64) * ((a.n_cob + 1) / 2) <= 1024))
    return launch_gemm_small(a, s);
  if (a.gn_fin) return -10;  // only the small-launch kernel finalises statistics
  // X-stationary kernel (SlideOp.p[10] = the weights as MFMA A fragments): one workgroup per row tile computes every
  // column tile from an LDS-resident X.  i[9] == 5 keeps the ring kernels, for A/B timing.
#ifndef SLIDE_EXPERIMENTS
  if (o.p[10]) return SLIDE_ST_EXPERIMENT;
#else
  if (o.p[10] && glds && prec == SLIDE_PREC_F16 && o.i[9] != 5 && (npxl == 8 || npxl == 7) && !(a.gfeat && a.in_scale)) {
    int st = -8;
    const bool aff = a.in_scale != nullptr, gat = a.gfeat != nullptr;
    st = slide_launch_gemm_xs(a, npxl, cbw, aff, gat, o.i[9] >= 11 && o.i[9] <= 13 ? o.i[9] - 10 : 0, s);
    if (st != -8) return st;  // -8: the X tile does not fit the LDS -> ring kernels
  }
#endif
  if (glds) {
    if (prec != SLIDE_PREC_F16) return -7;
#ifndef SLIDE_EXPERIMENTS
    // PRODUCT build: 256 x 64 tiles at three workgroups per CU (plain or with the input affine), the two-workgroup form of the
    // affine tile where its vectors do not fit beside three -- what the default DDPM plans and the module path (decode, encode)
    // dispatch.  Every other ring variant is an experiments-build kernel.
    if (o.i[9] != 0 || cbw != 2 || a.gfeat || a.stagger == 7 || (npxl != 7 && npxl != 8)) return SLIDE_ST_EXPERIMENT;
    {
      int st3 = -8;
      if (npxl == 8) st3 = a.in_scale ? launch_gemm_occ3<8, true, false>(a, s) : launch_gemm_occ3<8, false, false>(a, s);
      else if (!a.in_scale) return SLIDE_ST_EXPERIMENT;  // (128-row samples on stored inputs: the round-2 plan's FP blocks)
      else return launch_gemm_glds<7, 2, 3, 32, true>(a, s);
      if (st3 != -8) return st3;
      if (a.in_scale) return launch_gemm_glds<8, 2, 3, 32, true>(a, s);
      return -4;
    }
#else
    // i[9]: 0 = BK 32, three stages (two workgroups / CU); 1 = BK 64 (full 128-B lines), three stages (one / CU)
    const int wide = o.i[9] == 1 && (a.k_pad % 64 == 0) && !a.in_scale;
#define GCASE(L, C)                                                                                        \
  if (npxl == L && cbw == C)                                                                               \
    return wide ? launch_gemm_glds<L, C, 3, 64, false>(a, s) : launch_gemm_glds<L, C, 3, 32, false>(a, s)
#define ACASE(L, C) if (npxl == L && cbw == C) return launch_gemm_glds<L, C, 3, 32, true>(a, s)
    // launches of at most one workgroup per CU (the 16-row per-point GEMMs) are bound by the latency of their K loop:
    // a 7-stage ring keeps five chunks in flight instead of one
    if (npxl == 4 && cbw == 2 && !a.in_scale && !wide &&
        ((a.rows + TM - 1) / TM) * ((a.n_cob + 1) / 2) <= 256 && a.k_pad >= 128)
      return launch_gemm_glds<4, 2, 7, 32, false>(a, s);
    // wide outputs: eight-wave 256 x 256 tiles when the channel blocks fill them and enough tiles remain for the chip
    if (o.i[9] == 2 && cbw == 4 && !a.in_scale && a.n_cob % 8 == 0 &&
        ((a.rows + TM - 1) / TM) * (a.n_cob / 8) >= 256) {
      if (npxl == 8) return launch_gemm_glds8<8, 4, 4>(a, s);
      if (npxl == 7) return launch_gemm_glds8<7, 4, 4>(a, s);
    }
    // narrow outputs on a grid that does not fill the chip: the same 256 x 64 tile on eight waves (one channel block
    // per wave) halves each wave's epilogue
    if (o.i[9] == 4 && cbw == 2 && !a.in_scale && ((a.rows + TM - 1) / TM) * ((a.n_cob + 1) / 2) <= 512) {
      if (npxl == 8) return launch_gemm_glds8<8, 1, 3>(a, s);
      if (npxl == 7) return launch_gemm_glds8<7, 1, 3>(a, s);
    }
    // 64-channel tiles: three workgroups per CU (two-stage ring of 41 KB, 168-VGPR budget) instead of two on a three-stage
    // ring -- 8-13 % faster per launch at N >= 512 and, with four chains in flight, 2.5 % per step (0.921 vs 0.944 ms)
    // (a.stagger == 7: the two-workgroup form, for A/B timing)
    if (cbw == 2 && !wide && !(a.gfeat && a.in_scale) && a.stagger != 7 && (npxl == 7 || npxl == 8)) {
      int st3 = -8;
#define OCASE(L, A, G) if (npxl == L && (a.in_scale != nullptr) == A && (a.gfeat != nullptr) == G) st3 = launch_gemm_occ3<L, A, G>(a, s)
      OCASE(7, false, false); OCASE(8, false, false); OCASE(7, true, false); OCASE(8, true, false);
      OCASE(7, false, true); OCASE(8, false, true);
#undef OCASE
      if (st3 != -8) return st3;
    }
    if (a.gfeat) {  // gathered grouped input (first GEMM of an SA / FP block)
      if (a.in_scale || wide) return -4;
      if (npxl == 7 && cbw == 2) return launch_gemm_glds<7, 2, 3, 32, false, true>(a, s);
      if (npxl == 8 && cbw == 2) return launch_gemm_glds<8, 2, 3, 32, false, true>(a, s);
      if (npxl == 7 && cbw == 4) return launch_gemm_glds<7, 4, 3, 32, false, true>(a, s);
      if (npxl == 8 && cbw == 4) return launch_gemm_glds<8, 4, 3, 32, false, true>(a, s);
      return -4;
    }
    if (a.in_scale) { ACASE(7, 2); ACASE(8, 2); ACASE(7, 4); ACASE(8, 4); return -4; }
    if (cbw == 1 && !wide) {
      if (npxl == 7) return launch_gemm_glds<7, 1, 3, 32, false>(a, s);
      if (npxl == 8) return launch_gemm_glds<8, 1, 3, 32, false>(a, s);
      return -4;
    }
    GCASE(4, 2); GCASE(7, 2); GCASE(8, 2); GCASE(4, 4); GCASE(7, 4); GCASE(8, 4);
#undef ACASE
#undef GCASE
    return -4;
#endif
  }
  // split mode, 16-row samples (and RAW-epilogue launches that ask for them): 64-row tiles
  // (-8: the input affine's vectors do not fit the small kernel's 64 KB of LDS beside its ring -- k_pad >= 736 -- the 256-row
  //  split tile below applies the affine per X row instead)
  if (prec == SLIDE_PREC_SPLIT && npxl == 4 && cbw == 2 && o.i[9] != 3) {
    const int st = launch_gemm_split_small(a, s);
    if (st != -8) return st;
  }
#define CASE(P, L, C) if (prec == P && npxl == L && cbw == C) return launch_gemm<P, L, C>(a, s)
  CASE(SLIDE_PREC_F32, 4, 2); CASE(SLIDE_PREC_F32, 7, 2); CASE(SLIDE_PREC_F32, 8, 2);
  CASE(SLIDE_PREC_SPLIT, 4, 2); CASE(SLIDE_PREC_SPLIT, 7, 2); CASE(SLIDE_PREC_SPLIT, 8, 2);
#ifdef SLIDE_EXPERIMENTS
  CASE(SLIDE_PREC_F16, 4, 2); CASE(SLIDE_PREC_F16, 7, 2); CASE(SLIDE_PREC_F16, 8, 2);
  CASE(SLIDE_PREC_F16, 4, 4); CASE(SLIDE_PREC_F16, 7, 4); CASE(SLIDE_PREC_F16, 8, 4);
#else
  if (prec == SLIDE_PREC_F16) return SLIDE_ST_EXPERIMENT;  // register-staged fp16 GEMM [SLIDE_GLDS=0]
#endif
#undef CASE
  return -4;
}

}  // namespace

int slide_launch_gemm(const SlideOp &o, hipStream_t s) { return run_gemm(o, s); }
int slide_launch_pair_first(const SlideOp &o, hipStream_t s) { return run_pair_first(o, s); }
int slide_launch_gemm_attend(const SlideOp &o, hipStream_t s) { return run_gemm_attend(o, s); }
