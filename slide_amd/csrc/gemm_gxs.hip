// gemm_gxs.hip -- the generated-X GEMM of the SPLIT-arithmetic pair decomposition (round 5).
//
// The position DDPM has to be fp32-grade (north_star: generated latents within 1e-3; its fp16 plan is 1.5e-3 .. 3.2e-3 off on
// single forwards), and the fp32-structured split plan of round 4 moved ~0.8 GB of K-expanded fp32
// activations per step (batch 256).  The pair decomposition of gemm_gx.hip carried into the split arithmetic:
//   * the per-point tables ta / tb stay FLOAT (pair_norm2_kernel<., float>, pair_norm.hip);
//   * gemm_gxs_kernel is the consumer GEMM of a block's first layer: x(p, j) = max(ta[q] + tb[p] (+ d2 vd + w vw), 0) (+ add |
//     * scale + shift) is GENERATED in fp32 from the two 16-row tables (L1 / L2 resident: 2 x 16 x k_pad x 4 B per sample) while the
//     chunk goes to LDS, split there into two fp16 terms x = hi + 2^-11 lo like the weights, three fp16 MFMAs per product
//     (hi hi + 2^-11 (hi lo + lo hi)) into two fp32 accumulator sets -- the 256- / 128-row first-layer outputs (h1, r, keys:
//     288 channels x 65536 rows x 4 B at the position net's SA1) are never written or read;
//   * attn_tail_split_kernel (attn_tail_split.hip) is the tail of an AttentionModule (attention.py:86-95) on float rows: scores S = W5 u + b5 and values
//     V = relu(GN(Wv mo + bv)) as split contractions with SWAPPED operand roles (a lane owns a channel, its registers run over
//     the rows), soft-max over a point's neighbours and the weighted sum in registers -- S and V never reach memory.
// Reference: pointnet2_ops/pointnet2_utils.py:383-430, :497-524 (grouped inputs), pointnet2_ops/pointnet2_modules.py:119-176
// (Mlp_plus_t_emb), pointnet2_ops/attention.py:70-96.
#include "gemm_common.h"
#include "launch.h"

namespace {

// ------------------------------------------------------------------------------------------------ generated-X split GEMM
// Tile 256 rows (one 16 x 16 sample or two 16 x 8 samples) x 64 channels, four waves x 64 rows, K chunks of 32.  One LDS stage of
// five fp16 planes [X hi | X lo | W hi | 2^11 W hi | W lo] (rows of LDK = 40 halves: 56 KB); the next chunk's table rows and weights wait in
// registers.  Thread (l_row = tid / 8, l_c = 4 (tid % 8)) generates columns l_c .. l_c + 3 of tile rows l_row + 32 p, p = 0 .. 7:
// 16 x 16-row samples run in NATURAL neighbour order, so its eight rows share ONE neighbour row (q = l_row % 16) and touch eight
// centre rows; 16 x 8-row samples look their neighbours up once (nbr table) into a per-tile-row LDS table (offset, d2, w).
// The per-sample vectors (add | scale, shift | vd, vw) are staged once per workgroup in LDS.
// CHAIN (16 x 16-row samples, mode 0; round 5): the layer's output -- h2 = relu(GN(second_mlp(h1))) + class embedding of an SA block,
// at most 64 channels: one column tile -- is NOT stored: the common epilogue leaves it in the accumulators (KEEP), each 32-channel
// block of them IS one K chunk of the next layer (rest_mlp), written as split planes into the dead X stage, and the workgroup runs that
// layer's column tiles with its own epilogue (GroupNorm, ReLU, PAIR residual) -- one launch and one K-expanded round trip less per block.
template <int NPXL, int MODE, bool CHAIN = false>
__device__ __forceinline__ void gemm_gxs_body(const GemmArgs &a, const int bid) {
  constexpr int NPX = 1 << NPXL;
  constexpr bool FP = NPXL == 7;
  constexpr int NSAMP = TM >> NPXL;  // 1 or 2
  constexpr int CBW = 2, TN = 64;
  constexpr int LDK = TileT<SLIDE_PREC_SPLIT>::LDK;
  constexpr int XP = 8, WP = 2;                        // tile rows / weight rows per thread and chunk (32 rows per pass)
  constexpr int NVEC = (MODE ? 2 : 1) + (FP ? 2 : 0);  // float vectors per sample in LDS: [add | scale, shift][vd, vw][k_pad]
  constexpr int STAGE = (2 * TM + 3 * TN) * LDK;       // halves: planes [X hi | X lo | W hi | W hi 2^11 | W lo]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  _Float16 *const Xh = reinterpret_cast<_Float16 *>(smem_raw);
  _Float16 *const Xl = Xh + TM * LDK, *const Wh = Xl + TM * LDK, *const Ws = Wh + TN * LDK, *const Wl = Ws + TN * LDK;
  const int ntc = (a.n_cob + CBW - 1) / CBW;
  const int xcd = bid & 7, q0 = bid >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;  // the column tiles of a row tile share one XCD's L2 (tables + weights)
  if (tr * TM >= a.rows) return;
  const int row0 = tr * TM, cob0 = tc * CBW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, col = lane & 31;
  const int l_row = tid >> 3, l_c = (tid & 7) * 4;
  const float *ta = reinterpret_cast<const float *>(a.gx_ta), *tb = reinterpret_cast<const float *>(a.gx_tb);
  const float *W = reinterpret_cast<const float *>(a.W);
  const int nsm = a.rows >> NPXL, smp0 = row0 >> NPXL;

  uint32_t *const epi_lds = reinterpret_cast<uint32_t *>(smem_raw + (size_t)STAGE * 2);
  float *const vec_lds = reinterpret_cast<float *>(epi_lds + CBW * EPI_DW + (CBW * EPI_DW) % 4);
  float *const vv_l = vec_lds + CBW * 96;  // [sample][NVEC][k_pad]
  SLIDE_STAMP(a, 0);
  stage_epilogue_tables<CBW>(a, cob0, tid, epi_lds, vec_lds);
  // this thread's eight tile rows: neighbour (a) and centre (b) table rows (element offsets: the tables are far below 2^31
  // elements).  16 x 8-row samples: the neighbour's table row and the two per-slot scalars of every tile row live in LDS
  // ([256] x (offset, d2, w): kept in registers they push the kernel over its 256)
  int aoff0 = 0, boff[XP];
  int *const arow_l = reinterpret_cast<int *>(vv_l + (size_t)NSAMP * NVEC * a.k_pad);
  float *const d2_l = reinterpret_cast<float *>(arow_l + TM), *const w_l = d2_l + TM;
#pragma unroll
  for (int p = 0; p < XP; ++p) {
    int row = row0 + p * 32 + l_row;
    row = row < a.rows ? row : a.rows - 1;
    const int smp = row >> NPXL, pxl = row & (NPX - 1);
    if (!FP) {
      if (p == 0) aoff0 = (smp * 16 + (pxl & 15)) * a.gx_ld + l_c;
      boff[p] = (smp * 16 + (pxl >> 4)) * a.gx_ld + l_c;
    } else {
      boff[p] = (smp * 16 + (pxl >> 3)) * a.gx_ld + l_c;
    }
  }
  if (FP) {
    int row = row0 + tid;
    row = row < a.rows ? row : a.rows - 1;
    const int smp = row >> NPXL, pxl = row & (NPX - 1);
    const int slot = (smp * 16 + (pxl >> 3)) * 16 + (pxl & 7);
    arow_l[tid] = (smp * 16 + a.gidx[slot]) * a.gx_ld;
    d2_l[tid] = a.gx_d2[slot];
    w_l[tid] = a.gx_w[slot];
  }

  f32x16 acc[CBW][2];
#pragma unroll
  for (int i = 0; i < CBW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // raw table rows / weight rows of the chunk in flight.  16 x 8-row samples (a gathered neighbour row per tile row: twice the
  // registers) prefetch the first NPRE rows under the MFMAs and fetch the rest at the top of store_chunk, where no MFMA operand
  // is live -- all eight in flight across the MFMAs spills 36 registers
  constexpr int NPRE = FP ? 4 : XP;
  float4 ar[FP ? XP : 1], br[XP], wr[WP];
  auto load_rows = [&](int kc, auto lo_tag, auto hi_tag) __attribute__((always_inline)) {
    constexpr int P0 = decltype(lo_tag)::value, P1 = decltype(hi_tag)::value;
    const int ko = kc * BK;
#pragma unroll
    for (int p = P0; p < P1; ++p) {
      if (FP) ar[FP ? p : 0] = *reinterpret_cast<const float4 *>(ta + arow_l[p * 32 + l_row] + l_c + ko);
      else if (p == 0) ar[0] = *reinterpret_cast<const float4 *>(ta + aoff0 + ko);
      br[p] = *reinterpret_cast<const float4 *>(tb + boff[p] + ko);
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using IP = std::integral_constant<int, NPRE>;
  using IX = std::integral_constant<int, XP>;
  auto load_chunk = [&](int kc) __attribute__((always_inline)) {
    const int ko = kc * BK;
    load_rows(kc, I0(), IP());
#pragma unroll
    for (int p = 0; p < WP; ++p) {
      const int gco = cob0 * 32 + p * 32 + l_row;
      wr[p] = gco < a.n_cob * 32 ? *reinterpret_cast<const float4 *>(W + (size_t)gco * a.k_pad + ko + l_c)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_chunk = [&](int kc) __attribute__((always_inline)) {
    const int ko = kc * BK + l_c;
    if constexpr (NPRE < XP) load_rows(kc, IP(), IX());
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const float *vp = vv_l + (size_t)(FP ? (p >> 2) : 0) * NVEC * a.k_pad + ko;  // (two samples: tile rows 0..127 | 128..255)
      const float4 av = ar[FP ? p : 0], bv = br[p];
      float4 x = make_float4(av.x + bv.x, av.y + bv.y, av.z + bv.z, av.w + bv.w);
      if (FP) {
        const float4 vd = *reinterpret_cast<const float4 *>(vp + (MODE ? 2 : 1) * a.k_pad);
        const float4 vw = *reinterpret_cast<const float4 *>(vp + (MODE ? 3 : 2) * a.k_pad);
        const float d2 = d2_l[p * 32 + l_row], w_ = w_l[p * 32 + l_row];
        x.x = fmaf(w_, vw.x, fmaf(d2, vd.x, x.x)); x.y = fmaf(w_, vw.y, fmaf(d2, vd.y, x.y));
        x.z = fmaf(w_, vw.z, fmaf(d2, vd.z, x.z)); x.w = fmaf(w_, vw.w, fmaf(d2, vd.w, x.w));
      }
      x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f);
      const float4 v0 = *reinterpret_cast<const float4 *>(vp);
      if (MODE) {
        const float4 v1 = *reinterpret_cast<const float4 *>(vp + a.k_pad);
        x.x = fmaf(x.x, v0.x, v1.x); x.y = fmaf(x.y, v0.y, v1.y); x.z = fmaf(x.z, v0.z, v1.z); x.w = fmaf(x.w, v0.w, v1.w);
      } else {
        x.x += v0.x; x.y += v0.y; x.z += v0.z; x.w += v0.w;
      }
      f16x4 hi, lo;
      split4(x, hi, lo);
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
  auto compute = [&](f32x16 (&acc)[CBW][2]) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      f16x8 ah[CBW], as[CBW], al[CBW], bh[2], bl[2];
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb) {
        ah[cb] = *reinterpret_cast<const f16x8 *>(Wh + (cb * 32 + col) * LDK + st * 16 + half * 8);
        as[cb] = *reinterpret_cast<const f16x8 *>(Ws + (cb * 32 + col) * LDK + st * 16 + half * 8);
        al[cb] = *reinterpret_cast<const f16x8 *>(Wl + (cb * 32 + col) * LDK + st * 16 + half * 8);
      }
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        bh[rb] = *reinterpret_cast<const f16x8 *>(Xh + (wave * 64 + rb * 32 + col) * LDK + st * 16 + half * 8);
        bl[rb] = *reinterpret_cast<const f16x8 *>(Xl + (wave * 64 + rb * 32 + col) * LDK + st * 16 + half * 8);
      }
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as[cb], bh[rb], acc[cb][rb], 0, 0, 0);
          acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[cb], bl[rb], acc[cb][rb], 0, 0, 0);
          acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[cb], bh[rb], acc[cb][rb], 0, 0, 0);
        }
    }
  };

  const int nk = a.k_pad / BK;
  // PROLOGUE ORDER (round 6): 16 x 16-row samples (natural neighbour order: no row table) request their first chunk BEFORE the
  // per-sample vectors are staged -- one memory round trip instead of two in front of the first MFMA
  if (!FP) load_chunk(0);
  {
    const float *addp = a.in_add;
    if (MODE == 0 && addp && a.gx_add_idx) addp += (size_t)a.gx_add_idx[0] * a.gx_add_idx_stride;  // row t of a per-timestep table
    for (int i = tid * 4; i < NSAMP * a.k_pad; i += 1024) {
      const int sl = i / a.k_pad, k = i - sl * a.k_pad;
      int smp = smp0 + sl;
      smp = smp < nsm ? smp : nsm - 1;
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0, vd = v0, vw = v0;
      if (MODE == 0) {
        if (addp) v0 = *reinterpret_cast<const float4 *>(addp + (size_t)smp * a.add_bs + k);
      } else {
        v0 = *reinterpret_cast<const float4 *>(a.in_scale + (size_t)smp * a.in_bs + k);
        v1 = *reinterpret_cast<const float4 *>(a.in_shift + (size_t)smp * a.in_bs + k);
      }
      if (FP && a.gx_vv) {
        vd = *reinterpret_cast<const float4 *>(a.gx_vv + (size_t)smp * a.gx_vbs + k);
        vw = *reinterpret_cast<const float4 *>(a.gx_vv + (size_t)smp * a.gx_vbs + (a.gx_vbs >> 1) + k);
      }
      float *dst = vv_l + (size_t)sl * NVEC * a.k_pad + k;
      *reinterpret_cast<float4 *>(dst) = v0;
      if (MODE) *reinterpret_cast<float4 *>(dst + a.k_pad) = v1;
      if (FP) {
        *reinterpret_cast<float4 *>(dst + (MODE ? 2 : 1) * a.k_pad) = vd;
        *reinterpret_cast<float4 *>(dst + (MODE ? 3 : 2) * a.k_pad) = vw;
      }
    }
  }
  SLIDE_STAMP(a, 7);
  if (FP) {
    __syncthreads();  // (the row table is read by load_chunk)
    load_chunk(0);
  }
  __syncthreads();  // the staged vectors and epilogue tables are visible
  store_chunk(0);
  __syncthreads();
  SLIDE_STAMP(a, 1);
  for (int kc = 0; kc < nk; ++kc) {
    if (kc + 1 < nk) load_chunk(kc + 1);
    compute(acc);
    __syncthreads();  // every wave is done reading the stage before it is overwritten
    if (kc + 1 < nk) store_chunk(kc + 1);
    __syncthreads();
  }
  SLIDE_STAMP(a, 2);
#pragma unroll
  for (int i = 0; i < CBW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] *= 1.f / 2048.f;
  if constexpr (CHAIN) {
    // ---- this layer's epilogue with the result kept in `acc` (all its channels sit in this one column tile: cob0 == 0)
    gemm_epilogue<SLIDE_PREC_F32, NPXL, CBW, 2, false, true>(a, acc, row0, cob0, wave, half, col, epi_lds, vec_lds,
                                                             reinterpret_cast<float *>(smem_raw));
    GemmArgs b = a;
    b.W = a.ch_W; b.epi = a.ch_epi; b.vecs = a.ch_vecs; b.n_cob = a.ch_n_cob; b.k_pad = a.ch_k_pad;
    const float *W2 = reinterpret_cast<const float *>(a.ch_W);
    const int nk2 = a.ch_k_pad / BK;  // <= CBW: chunk kc2 of the next layer = channel block kc2 of this one
    for (int tc2 = 0; tc2 < (a.ch_n_cob + CBW - 1) / CBW; ++tc2) {
      __syncthreads();  // the previous epilogue is done with its tables and scratch
      stage_epilogue_tables<CBW>(b, tc2 * CBW, tid, epi_lds, vec_lds);
      f32x16 acc2[CBW][2];
#pragma unroll
      for (int i = 0; i < CBW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc2[i][j][r] = 0.f;
#pragma unroll
      for (int kc2 = 0; kc2 < CBW; ++kc2) {
        if (kc2 >= nk2) break;
        if (kc2) __syncthreads();  // the stage is free again
        // X planes from the accumulators: lane (row, half) holds channels 8 q + 4 half + 0 .. 3 of block kc2
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          const int trow = wave * 64 + rb * 32 + col;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            f16x4 hi, lo;
            split4(make_float4(acc[kc2][rb][4 * q], acc[kc2][rb][4 * q + 1], acc[kc2][rb][4 * q + 2], acc[kc2][rb][4 * q + 3]), hi, lo);
            *reinterpret_cast<f16x4 *>(Xh + trow * LDK + 8 * q + 4 * half) = hi;
            *reinterpret_cast<f16x4 *>(Xl + trow * LDK + 8 * q + 4 * half) = lo;
          }
        }
#pragma unroll
        for (int p = 0; p < WP; ++p) {
          const int gco = tc2 * CBW * 32 + p * 32 + l_row;
          const float4 w4 = gco < a.ch_n_cob * 32 ? *reinterpret_cast<const float4 *>(W2 + (size_t)gco * a.ch_k_pad + kc2 * BK + l_c)
                                                  : make_float4(0.f, 0.f, 0.f, 0.f);
          f16x4 hi, hs, lo;
          gxs_split4w(w4, hi, hs, lo);
          *reinterpret_cast<f16x4 *>(Wh + (p * 32 + l_row) * LDK + l_c) = hi;
          *reinterpret_cast<f16x4 *>(Ws + (p * 32 + l_row) * LDK + l_c) = hs;
          *reinterpret_cast<f16x4 *>(Wl + (p * 32 + l_row) * LDK + l_c) = lo;
        }
        __syncthreads();
        compute(acc2);
      }
      __syncthreads();  // the stage turns into the epilogue's scratch
#pragma unroll
      for (int i = 0; i < CBW; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc2[i][j][r] *= 1.f / 2048.f;
      // (rest_mlp carries no add vector -- the class embedding is added to second_mlp's output: the NOADDV epilogue, whose 16 fewer
      //  registers keep h2 alive across this tile's epilogue without a spill)
      gemm_epilogue<SLIDE_PREC_F32, NPXL, CBW, 2, true, false, true>(b, acc2, row0, tc2 * CBW, wave, half, col, epi_lds, vec_lds,
                                                                     reinterpret_cast<float *>(smem_raw));
    }
    return;
  }
  // float rows: the fp32 epilogue (mode 0 = the Mlp layers: PAIR residual on the float tables)
  gemm_epilogue<SLIDE_PREC_F32, NPXL, CBW, 2, MODE == 0>(a, acc, row0, cob0, wave, half, col, epi_lds, vec_lds,
                                                         reinterpret_cast<float *>(smem_raw));
  SLIDE_STAMP(a, 5);
#ifdef SLIDE_TIMELINE
  if (a.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); SLIDE_STAMP(a, 6); }
#endif
}

template <int NPXL, int MODE>
__global__ __launch_bounds__(256, 2) void gemm_gxs_kernel(GemmArgs a) {
  gemm_gxs_body<NPXL, MODE>(a, blockIdx.x);
}

// the two independent generated-X GEMMs of a block (keys -> u: mode 1; first Mlp layer: mode 0) in ONE launch: they read the same
// pair tables and nothing of each other -- one launch gap instead of two, and their workgroups fill the chip together
template <int NPXL, bool CHAIN = false>
__global__ __launch_bounds__(256, 2) void gemm_gxs_dual_kernel(GemmArgs a1, GemmArgs a0, int grid1) {
  if ((int)blockIdx.x < grid1) gemm_gxs_body<NPXL, 1>(a1, blockIdx.x);
  else gemm_gxs_body<NPXL, 0, CHAIN>(a0, blockIdx.x - grid1);
}

template <int NPXL>
__global__ __launch_bounds__(256, 2) void gemm_gxs_chain_kernel(GemmArgs a) {
  gemm_gxs_body<NPXL, 0, true>(a, blockIdx.x);
}

template <int NPXL, int MODE, bool CHAIN = false>
int launch_gxs(const GemmArgs &a, hipStream_t s) {
  constexpr int LDK = TileT<SLIDE_PREC_SPLIT>::LDK;
  constexpr int NSAMP = TM >> NPXL, NVEC = (MODE ? 2 : 1) + (NPXL == 7 ? 2 : 0);
  const size_t shm = (size_t)(2 * TM + 3 * 64) * LDK * 2 + (2 * EPI_DW + (2 * EPI_DW) % 4 + 2 * 96) * 4 + (size_t)NSAMP * NVEC * a.k_pad * 4 + (NPXL == 7 ? 3 * TM * 4 : 0) + 16;
  if (shm > 80 * 1024) return -8;
  const int ntc = (a.n_cob + 1) / 2, ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
  if constexpr (CHAIN) {
    allow_dynamic_lds<&gemm_gxs_chain_kernel<NPXL>>(80 * 1024);
    hipLaunchKernelGGL((gemm_gxs_chain_kernel<NPXL>), dim3(grid), dim3(256), shm, s, a);
  } else {
    allow_dynamic_lds<&gemm_gxs_kernel<NPXL, MODE>>(80 * 1024);
    hipLaunchKernelGGL((gemm_gxs_kernel<NPXL, MODE>), dim3(grid), dim3(256), shm, s, a);
  }
  return (int)hipGetLastError();
}

}  // namespace

static int gxs_args_from_op(const SlideOp &o, GemmArgs &a) {
  a = GemmArgs();
  a.gx_ta = o.p[0]; a.W = o.p[1]; a.epi = (const SlideEpi *)o.p[2];
  a.in_scale = (const float *)o.p[3]; a.in_shift = (const float *)o.p[4];
  a.gx_tb = o.p[5]; a.in_add = (const float *)o.p[6]; a.gx_add_idx = (const int *)o.p[7];
  a.gidx = (const int *)o.p[8]; a.gx_d2 = (const float *)o.p[9]; a.gx_w = (const float *)o.p[10];
  a.gx_vv = (const float *)o.p[11];
  a.rows = o.i[0]; a.gx_ld = o.i[1]; a.k_pad = o.i[2]; a.n_cob = o.i[3]; a.in_bs = o.i[5];
  a.gx_mode = o.i[6]; a.add_bs = o.i[7]; a.gx_add_idx_stride = o.i[8]; a.gx_vbs = o.i[9];
  a.aff_tps = 1;
  const int npxl = o.i[4];
  if (a.k_pad % 32 || a.k_pad <= 0 || a.gx_ld % 4 || a.rows <= 0 || a.n_cob <= 0 || !a.gx_ta || !a.gx_tb) return -3;
  if ((uintptr_t)a.gx_ta % 16 || (uintptr_t)a.gx_tb % 16 || (uintptr_t)a.W % 16) return -3;
  if (a.gx_mode != 0 && (!a.in_scale || !a.in_shift || (uintptr_t)a.in_scale % 16 || (uintptr_t)a.in_shift % 16 || a.in_bs % 4)) return -3;
  if (a.in_add && ((uintptr_t)a.in_add % 16 || a.add_bs % 4 || a.gx_add_idx_stride % 4)) return -3;
  if (a.gx_vv && ((uintptr_t)a.gx_vv % 16 || a.gx_vbs % 8)) return -3;
  if (npxl == 7 && (!a.gidx || !a.gx_d2 || !a.gx_w)) return -3;
  // chained second layer (p[12] = its float weights, p[13] = its epilogue descriptors, f[1] = its n_cob, f[2] = its k_pad): 16 x 16-row
  // samples, mode 0, every channel of this layer in one 64-channel tile, which is also the next layer's whole K
  a.ch_W = o.p[12]; a.ch_epi = (const SlideEpi *)o.p[13]; a.ch_n_cob = (int)o.f[1]; a.ch_k_pad = (int)o.f[2];
#ifdef SLIDE_TIMELINE
  if (!a.ch_W) { a.dbg = (unsigned long long *)o.p[13]; a.ch_epi = nullptr; }  // (tools/ab/op_timeline.py: stamps of an unchained launch)
#endif
  resolve_epi(a);
  if (a.ch_W && (npxl != 8 || a.gx_mode != 0 || a.n_cob > 2 || !a.ch_epi || a.ch_n_cob <= 0 || a.ch_k_pad != a.n_cob * 32 ||
                 (uintptr_t)a.ch_W % 16))
    return -3;
  return 0;
}

// SLIDE_OP_GEMM_GX with f[0] == 3: float tables, float row-major weights [n_cob*32][k_pad], float outputs (split arithmetic)
int slide_launch_gemm_gxs(const SlideOp &o, hipStream_t s) {
  GemmArgs a;
  const int st = gxs_args_from_op(o, a);
  if (st != 0) return st;
  const int npxl = o.i[4];
  const bool m1 = a.gx_mode != 0;
  if (a.ch_W) return launch_gxs<8, 0, true>(a, s);
  if (npxl == 8) return m1 ? launch_gxs<8, 1>(a, s) : launch_gxs<8, 0>(a, s);
  if (npxl == 7) return m1 ? launch_gxs<7, 1>(a, s) : launch_gxs<7, 0>(a, s);
  return -4;
}

namespace {
template <int NPXL, bool CHAIN = false>
int launch_gxs_dual(const GemmArgs &a1, const GemmArgs &a0, hipStream_t s) {
  constexpr int LDK = TileT<SLIDE_PREC_SPLIT>::LDK;
  constexpr int NSAMP = TM >> NPXL;
  auto lds = [&](const GemmArgs &a, int nvec) {
    return (size_t)(2 * TM + 3 * 64) * LDK * 2 + (2 * EPI_DW + (2 * EPI_DW) % 4 + 2 * 96) * 4 + (size_t)NSAMP * nvec * a.k_pad * 4 +
           (NPXL == 7 ? 3 * TM * 4 : 0) + 16;
  };
  const size_t s1 = lds(a1, 2 + (NPXL == 7 ? 2 : 0)), s0 = lds(a0, 1 + (NPXL == 7 ? 2 : 0));
  const size_t shm = s1 > s0 ? s1 : s0;
  if (shm > 80 * 1024) return -8;
  const int ntr = (a1.rows + TM - 1) / TM;
  const int g1 = ((ntr + 7) / 8) * 8 * ((a1.n_cob + 1) / 2), g0 = ((ntr + 7) / 8) * 8 * ((a0.n_cob + 1) / 2);
  allow_dynamic_lds<&gemm_gxs_dual_kernel<NPXL, CHAIN>>(80 * 1024);
  hipLaunchKernelGGL((gemm_gxs_dual_kernel<NPXL, CHAIN>), dim3(g1 + g0), dim3(256), shm, s, a1, a0, g1);
  return (int)hipGetLastError();
}
}  // namespace

// SLIDE_OP_GEMM_GX_DUAL whose two ops carry f[0] == 3 (mode 1 first, then mode 0; same rows and sample size)
int slide_launch_gemm_gxs_dual(const SlideOp *pr, hipStream_t s) {
  GemmArgs a1, a0;
  int st = gxs_args_from_op(pr[0], a1);
  if (st == 0) st = gxs_args_from_op(pr[1], a0);
  if (st != 0) return st;
  if (a1.gx_mode == 0 || a0.gx_mode != 0 || a1.rows != a0.rows || pr[0].i[4] != pr[1].i[4]) return -3;
  if (pr[0].i[4] == 8) st = a0.ch_W ? launch_gxs_dual<8, true>(a1, a0, s) : launch_gxs_dual<8>(a1, a0, s);
  else if (pr[0].i[4] == 7) st = launch_gxs_dual<7>(a1, a0, s);
  else return -4;
  if (st == -8) {  // (LDS of the dual form does not fit: two launches)
    st = slide_launch_gemm_gxs(pr[0], s);
    if (st == 0) st = slide_launch_gemm_gxs(pr[1], s);
  }
  return st;
}
