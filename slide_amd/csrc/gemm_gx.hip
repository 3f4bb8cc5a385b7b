// gemm_gx.hip -- the generated-X GEMM of the PAIR DECOMPOSITION of the SA / FP blocks' first layers (round 3).
//
// Every SA / FP block of PointNet2CloudCondition starts with 1x1 convolutions over the grouped input
//   row (p, j) = [features of neighbour q | coordinate channels of (q, p)]        (pointnet2_utils.py:383-430, :497-524)
// (first_mlp, res_connect, grouped_feat_conv: pointnet2_modules.py:119-176, attention.py:70-96).  A 1x1 convolution is
// linear, and every coordinate channel is a linear function of xyz[q] and xyz[p], so its output separates:
//   y(p, j) = a[q] + b[p] (+ d2(p, j) vd + w(p, j) vw for group_knn's two per-slot scalars)
// with a[q] = Wf feat[q] + (W_rel + W_abs) xyz[q] + bias and b[p] = (W_ctr - W_rel) xyz[p] -- a 16-row GEMM per sample
// instead of a 256- / 128-row one (1/16 or 1/8 of the MACs: 31 % of the feature denoiser's FLOPs), and, more important,
// the K-expanded first-layer outputs (1056 channels x 256 rows per sample at SA1: the largest tensors of a step) are never
// written to or read from HBM:
//   * the pair-table pass (pair_norm.h, pair_norm.hip) turns the per-point products into the tables (a, b): GroupNorm
//     statistics over the sample's pairs (exact, fp32) are folded INTO the tables (a g + shift, b g), or emitted as sums for the attention's joint GroupNorm;
//   * gemm_gx_kernel is the consumer GEMM of such a layer: a workgroup keeps its sample's tables in LDS and GENERATES the
//     MFMA B fragments (x = max(a[q] + b[p], 0) + t-embedding, or max(.)*scale + shift) between LDS and MFMA -- three packed
//     fp16 VALU ops per fragment register -- while only the weights stream through an LDS-DMA ring;
//   * the res_connect output re-enters as a PAIR residual in the common epilogue (gemm_common.h).
// In the SA blocks every point is a neighbour of every point (K = N = 16) and everything downstream (GroupNorm statistics,
// softmax-weighted sum over the neighbours) is invariant to the neighbour ORDER, so rows run in natural order (q = j): no
// index table, and the a-fragment is shared by all row blocks of a wave.
#include "gemm_common.h"
#include "launch.h"

namespace {

// ------------------------------------------------------------------------------------------------ generated-X GEMM
// Tile: 256 rows (one 16x16 sample, or two 16x8 samples) x 128 channels; four waves, wave w owns rows 64 w .. 64 w + 63 and
// all 128 channels (acc[4][2] = 128 registers).  W: chunk-major [k / 32][n_cob * 32][32]; a ring stage is two 32-deep
// chunk images ([128 rows][64 B], source-side XOR swizzle as in the ring kernels of gemm_ring.hip) = 16 KB; NST stages.
// Tables in LDS: [16-byte piece of the row][table row][8 halves] -- the 16 rows a ds_read_b128 lane group touches for one
// piece are 256 consecutive bytes (conflict-free for any neighbour permutation), filled by LDS-DMA (per-lane source rows).
// The K loop is software-pipelined by hand over its 16-deep steps: the LDS reads of step s + 1 (weight fragments, table
// rows, vectors) are issued before the B fragments of step s are generated and its 8 MFMAs issued, so the reads' latency and
// the packed-fp16 generation of the next fragments run under the matrix pipe's 256 busy cycles; the ring's wait + barrier of
// the next stage sits one step early for the same reason.
template <int NPXL, int NST, int MODE, int CBW>
__device__ __forceinline__ void gemm_gx_body(const GemmArgs &a, const int bid) {
  using T = _Float16;
  constexpr int NPX = 1 << NPXL;
  constexpr bool FP = NPXL == 7;
  constexpr int NSAMP = TM >> NPXL;            // 1 or 2
  constexpr int NR = 16 * NSAMP;               // table rows in LDS
  constexpr int CH_B = 32 * CBW * 64;                      // a weight chunk image: [32 CBW weight rows][64 B]
  constexpr int NJ = CBW / 2;                              // weight DMA instructions per wave and chunk image (16 rows each)
  // the sample's pair tables STREAM with the weights (round 3): a stage also carries, per 32-deep chunk and table, the image
  // [4 sixteen-byte pieces][NR rows][8 halves] = 64 NR bytes -- instead of both tables staged whole before the K loop
  // (2 x 16 x k_pad x 2 B per sample: 69 KB on the FP1 layer, which pinned that launch to one workgroup per CU, and a 2 - 3 us
  // prologue on every workgroup)
  constexpr int TBL_B = 64 * NR;                           // one (chunk, table) image
  constexpr int STAGE_B = 2 * CH_B + 4 * TBL_B;
  constexpr int NTI = NSAMP;                               // table DMA instructions per wave and stage (1 KB each)
  constexpr int NVEC = (MODE ? 2 : 1) + (FP ? 2 : 0);  // fp16 vectors per sample in LDS: [add | scale, shift][vd, vw][k_pad]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ntc = (a.n_cob + CBW - 1) / CBW;
  const int ntr = (a.rows + TM - 1) / TM;
  const int xcd = bid & 7, q0 = bid >> 3;
  const int tc = q0 % ntc, tr = (q0 / ntc) * 8 + xcd;  // the column tiles of a row tile share one XCD's L2 (weights + tables)
  if (tr >= ntr) return;
  const int row0 = tr * TM, cob0 = tc * CBW;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, col = lane & 31;
  const int nk32 = a.k_pad >> 5, nks = (nk32 + 1) >> 1;
  unsigned char *const ring = smem_raw;
  SLIDE_STAMP(a, 0);
  uint32_t *const epi_lds = reinterpret_cast<uint32_t *>(smem_raw + (size_t)NST * STAGE_B);
  float *const vec_lds = reinterpret_cast<float *>(epi_lds + CBW * EPI_DW + (CBW * EPI_DW) % 4);
  T *const vv_l = reinterpret_cast<T *>(vec_lds + CBW * 96);
  const int nsm = a.rows >> NPXL, smp0 = row0 >> NPXL;

  // PROLOGUE ORDER (round 6): descriptor / vector DMAs and the first ring stages are ISSUED before anything waits -- the plain loads
  // below (per-sample vectors, neighbour slots) then share ONE memory round trip with them instead of preceding them (the
  // per-workgroup timeline's "tables" phase: 1.0 - 1.7 us of a 7 - 17 us workgroup; tools/ab/op_timeline.py)
  stage_epilogue_tables<CBW, 256>(a, cob0, tid, epi_lds, vec_lds);
  // ---- table stream: this wave's NTI instructions per stage; instruction id = wave + 4 n -> (chunk of the stage, table, piece half)
  const T *tsrc[NTI];
  int tdst[NTI];
#pragma unroll
  for (int n = 0; n < NTI; ++n) {
    const int id = wave + 4 * n;                       // SA: 0..3 = (c2, t); FP: 0..7 = (c2, t, h)
    const int c2 = FP ? (id >> 2) & 1 : (id >> 1) & 1, t = FP ? (id >> 1) & 1 : id & 1, h = FP ? id & 1 : 0;
    const int piece = FP ? 2 * h + (lane >> 5) : lane >> 4, r = lane & (NR - 1);
    int smp = smp0 + (r >> 4);
    smp = smp < nsm ? smp : nsm - 1;
    tsrc[n] = reinterpret_cast<const T *>(t ? a.gx_tb : a.gx_ta) + ((size_t)smp * 16 + (r & 15)) * a.gx_ld + piece * 8;
    tdst[n] = 2 * CH_B + (c2 * 2 + t) * TBL_B + (FP ? 2 * h * NR * 16 : 0);
  }
  // ---- weight ring: this lane's source piece of the wave's two DMA instructions per 32-deep chunk
  const T *wsrc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int trow = 16 * (j * 4 + wave) + (lane >> 2);
    const int piece = (lane & 3) ^ ((trow >> 2) & 3);
    int gco = cob0 * 32 + trow;
    gco = gco < a.n_cob * 32 ? gco : a.n_cob * 32 - 1;  // rows beyond the matrix: clamp (their channels are never stored)
    wsrc[j] = reinterpret_cast<const T *>(a.W) + (size_t)gco * 32 + piece * 8;
  }
  const size_t w_cs = (size_t)a.n_cob * 32 * 32;  // elements between consecutive chunks
  auto issue = [&](int st) __attribute__((always_inline)) {  // stage st -> slot st % NST (2 NJ DMA instructions per wave)
    unsigned char *dst = ring + (size_t)(st % NST) * STAGE_B;
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      int kc = st * 2 + c2;
      kc = kc < nk32 ? kc : nk32 - 1;  // odd chunk count: the last stage's second image is a dummy (never read)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)(wsrc[j] + (size_t)kc * w_cs),
                                         (__attribute__((address_space(3))) void *)(dst + c2 * CH_B + (j * 4 + wave) * 1024),
                                         16, 0, 0);
    }
#pragma unroll
    for (int n = 0; n < NTI; ++n) {
      int kc = st * 2 + (FP ? n : (wave >> 1));  // the chunk of the stage this instruction serves (id = wave + 4 n)
      kc = kc < nk32 ? kc : nk32 - 1;
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void *)(tsrc[n] + kc * 32),
                                       (__attribute__((address_space(3))) void *)(dst + tdst[n]), 16, 0, 0);
    }
  };
#pragma unroll
  for (int s0 = 0; s0 < NST - 1; ++s0)
    if (s0 < nks) issue(s0);
  // ---- per-sample vectors (plain loads, converted to fp16)
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
      T *dst = vv_l + (size_t)sl * NVEC * a.k_pad + k;
      store4<T>(dst, v0);
      if (MODE) store4<T>(dst + a.k_pad, v1);
      if (FP) {
        store4<T>(dst + (MODE ? 2 : 1) * a.k_pad, vd);
        store4<T>(dst + (MODE ? 3 : 2) * a.k_pad, vw);
      }
    }
  }
  // this lane's two row blocks: table rows of the neighbour (a) and of the centre point (b), per-slot scalars
  int aoff[2], boff[2];
  f16x2 d2s[2], ws[2];
  const int sl_w = FP ? (wave >> 1) : 0;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    int row = row0 + wave * 64 + rb * 32 + col;
    row = row < a.rows ? row : a.rows - 1;
    const int smp = row >> NPXL, pxl = row & (NPX - 1);
    int p, q;
    float d2 = 0.f, w = 0.f;
    if (!FP) { p = pxl >> 4; q = pxl & 15; }
    else {
      p = pxl >> 3;
      const int slot = (smp * 16 + p) * 16 + (pxl & 7);
      q = a.gidx[slot];
      d2 = a.gx_d2[slot]; w = a.gx_w[slot];
    }
    aoff[rb] = (half * NR + sl_w * 16 + q) * 16;
    boff[rb] = (half * NR + sl_w * 16 + p) * 16;
    d2 = fminf(d2, 65504.f);  // (fp16 range: beyond it the conversion gives inf)
    d2s[rb] = f16x2{(T)d2, (T)d2};
    ws[rb] = f16x2{(T)w, (T)w};
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every plain load above has landed (and the primed stages with them)

  SLIDE_STAMP(a, 7);

  const unsigned char *const vbase = reinterpret_cast<const unsigned char *>(vv_l + (size_t)sl_w * NVEC * a.k_pad) + half * 16;
  const int vstr = a.k_pad * 2;  // bytes between the vectors of a sample

  f32x16 acc[CBW][2];
#pragma unroll
  for (int i = 0; i < CBW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  int wrow[CBW], wkey[CBW];
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) {
    const int trow = cb * 32 + col;
    wrow[cb] = trow * 64; wkey[cb] = (trow >> 2) & 3;
  }

  // operands of one 16-deep step: weight fragments + the table rows its B fragments are generated from (the per-channel
  // vectors are uniform reads, fetched where they are used: keeping them out of the double buffer is what fits 256 registers)
  struct Step { f16x8 af[CBW], av[FP ? 2 : 1], bv[2]; int kb; };
  auto load_step = [&](Step &o, const unsigned char *sb, int c2, int st2, int kc) __attribute__((always_inline)) {
    const int piece = st2 * 2 + half;
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb)
      o.af[cb] = *reinterpret_cast<const f16x8 *>(sb + c2 * CH_B + wrow[cb] + ((piece ^ wkey[cb]) << 4));
    const unsigned char *ta_s = sb + 2 * CH_B + (c2 * 2) * TBL_B + st2 * 2 * NR * 16;  // this step's pieces of the a image
    const unsigned char *tb_s = ta_s + TBL_B;
    o.kb = (kc * 32 + st2 * 16) * 2;              // byte offset of this step inside a vector
    o.av[0] = *reinterpret_cast<const f16x8 *>(ta_s + aoff[0]);
    if (FP) o.av[FP ? 1 : 0] = *reinterpret_cast<const f16x8 *>(ta_s + aoff[1]);  // (natural order: q is the same in both blocks)
    o.bv[0] = *reinterpret_cast<const f16x8 *>(tb_s + boff[0]);
    o.bv[1] = *reinterpret_cast<const f16x8 *>(tb_s + boff[1]);
  };
  auto compute_step = [&](const Step &o) __attribute__((always_inline)) {
    const f16x2 zero2 = {0, 0};
    const f16x8 v0 = *reinterpret_cast<const f16x8 *>(vbase + o.kb);
    f16x8 v1, vd, vw;
    if (MODE) v1 = *reinterpret_cast<const f16x8 *>(vbase + vstr + o.kb);
    if (FP) {
      vd = *reinterpret_cast<const f16x8 *>(vbase + (MODE ? 2 : 1) * vstr + o.kb);
      vw = *reinterpret_cast<const f16x8 *>(vbase + (MODE ? 3 : 2) * vstr + o.kb);
    }
    f16x8 bf[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const f16x8 av = o.av[FP ? rb : 0], bv = o.bv[rb];
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // packed fp16 math on register pieces; the per-slot scalars are ONE register each
        f16x2 y = f16x2{av[2 * i], av[2 * i + 1]} + f16x2{bv[2 * i], bv[2 * i + 1]};
        if (FP) {
          y = __builtin_elementwise_fma(d2s[rb], f16x2{vd[2 * i], vd[2 * i + 1]}, y);
          y = __builtin_elementwise_fma(ws[rb], f16x2{vw[2 * i], vw[2 * i + 1]}, y);
        }
        y = __builtin_elementwise_max(y, zero2);
        if (MODE) y = __builtin_elementwise_fma(y, f16x2{v0[2 * i], v0[2 * i + 1]}, f16x2{v1[2 * i], v1[2 * i + 1]});
        else y = y + f16x2{v0[2 * i], v0[2 * i + 1]};
        bf[rb][2 * i] = y[0]; bf[rb][2 * i + 1] = y[1];
      }
    }
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
        acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(o.af[cb], bf[rb], acc[cb][rb], 0, 0, 0);
  };
  // stage st must have landed before anyone reads it; the next one (2 NJ instructions per wave) may stay in flight
  auto stage_ready = [&](int st) __attribute__((always_inline)) {
    if (st + 1 < nks && NST > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NJ + NTI) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // (first pass: also publishes the tables and vectors staged above)
    if (st + NST - 1 < nks) issue(st + NST - 1);  // overwrites the stage consumed at st - 1
  };

  SLIDE_STAMP(a, 1);
  Step cur, nxt;
  stage_ready(0);
  load_step(cur, ring, 0, 0, 0);
  for (int st = 0; st < nks; ++st) {
    const unsigned char *sb = ring + (size_t)(st % NST) * STAGE_B;
    const bool two = st * 2 + 1 < nk32;  // the stage's second 32-deep chunk exists
    // step 0 of chunk 0
    load_step(nxt, sb, 0, 1, st * 2);
    compute_step(cur);
    // step 1 of chunk 0
    if (two) {
      load_step(cur, sb, 1, 0, st * 2 + 1);
      compute_step(nxt);
      load_step(nxt, sb, 1, 1, st * 2 + 1);
      compute_step(cur);
    }
    // last step of the stage: the next stage's barrier and first reads go ahead of its MFMAs
    if (st + 1 < nks) {
      stage_ready(st + 1);
      load_step(cur, ring + (size_t)((st + 1) % NST) * STAGE_B, 0, 0, st * 2 + 2);
    }
    compute_step(nxt);
  }
  __syncthreads();  // every wave is done with the ring before `red` reuses it
  SLIDE_STAMP(a, 2);
  gemm_epilogue<SLIDE_PREC_F16, NPXL, CBW, 2, MODE == 0, false, false, true>(a, acc, row0, cob0, wave, half, col, epi_lds, vec_lds,  // (mode 0 = the Mlp layers: PAIR residual)
                                           reinterpret_cast<float *>(smem_raw));
  SLIDE_STAMP(a, 5);
#ifdef SLIDE_TIMELINE
  if (a.dbg) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    SLIDE_STAMP(a, 6);
  }
#endif
}

template <int NPXL, int NST, int MODE>
__global__ __launch_bounds__(256, 2) void gemm_gx_kernel(GemmArgs a) {
  gemm_gx_body<NPXL, NST, MODE, 4>(a, blockIdx.x);
}

// 256 x 64 tiles inside the 168-register budget (64 accumulator registers, 8 KB ring stages): THREE workgroups per CU and
// twice the workgroups per launch -- the K loops of these layers are short (K = 64 .. 544) and each workgroup spends most of
// its life in the table prologue and the epilogue, which a third resident workgroup overlaps
template <int NPXL, int NST, int MODE>
__global__ __launch_bounds__(256, 3) void gemm_gx_n64_kernel(GemmArgs a) {
  gemm_gx_body<NPXL, NST, MODE, 2>(a, blockIdx.x);
}

// the same 64-channel tile at two workgroups per CU (256 registers: also mode 0 with its PAIR residual): for launches whose
// 128-channel grid does not cover the chip -- the FP blocks at 88 samples: 96 workgroups -- half-size tiles double the
// workgroups in flight and halve each one's K loop and epilogue
template <int NPXL, int NST, int MODE>
__global__ __launch_bounds__(256, 2) void gemm_gx_n64w_kernel(GemmArgs a) {
  gemm_gx_body<NPXL, NST, MODE, 2>(a, blockIdx.x);
}

// TWO independent generated-X GEMMs of one block in ONE launch (SLIDE_OP_GEMM_GX_DUAL): the keys -> u layer (mode 1) and the
// first Mlp layer (mode 0) of an FP block read the same pair tables and nothing of each other; as one grid they cost one
// launch gap instead of two and their workgroups fill the chip together (64-channel tiles, two workgroups per CU)
// FP blocks (NPXL = 7; round 6): THREE workgroups per CU -- a two-stage ring (42 KB with the per-sample vectors of K = 544 instead of 58)
// inside the 168-register budget.  The K loops of these layers are bound by the LDS reads and packed-fp16 generation of their fragments
// (ten ds_read_b128 and ~40 VALU per four MFMAs), their workgroups by prologue and epilogue latency: a third resident workgroup -- of
// this launch or of another chain's -- fills what two leave idle: 415.2 -> 419.7 shapes/s in bench.py's arrangement (four alternating
// pairs in one call, tools/ab/r06_libab.sh dual3).  The mode-0 body (PAIR residual) needs 178 registers when left alone: at 168 the
// compiler parks 15 values in scratch -- addressing terms of the prologue / epilogue and ONE 8-byte reload per ring stage (none in the
// MFMA steps) -- which is the one deliberate exception to the product build's no-spill rule (slide_amd/build.py SPILL_OPT_IN).
template <int NPXL>
constexpr int GX_DUAL_NST = NPXL == 7 ? 2 : 3;
template <int NPXL>
__global__ __launch_bounds__(256, NPXL == 7 ? 3 : 2) void gemm_gx_dual_kernel(GemmArgs a1, GemmArgs a0, int grid1) {
  if ((int)blockIdx.x < grid1) gemm_gx_body<NPXL, GX_DUAL_NST<NPXL>, 1, 2>(a1, blockIdx.x);
  else gemm_gx_body<NPXL, GX_DUAL_NST<NPXL>, 0, 2>(a0, blockIdx.x - grid1);
}

template <int NPXL, int NST, int MODE, int CBW = 4, bool OCC3 = true>
int launch_gx(const GemmArgs &a, hipStream_t s) {
  constexpr int NSAMP = TM >> NPXL, NVEC = (MODE ? 2 : 1) + (NPXL == 7 ? 2 : 0);
  const size_t shm = (size_t)NST * (4096 * CBW + 4 * 64 * 16 * NSAMP) + (CBW * EPI_DW + (CBW * EPI_DW) % 4 + CBW * 96) * 4 +
                     (size_t)NSAMP * NVEC * a.k_pad * 2 + 16;
  // the OCC3 form needs three workgroups per CU, the others two (the tables stream through the ring, so only the per-sample
  // vectors grow with K)
  if (shm > (CBW == 2 && OCC3 ? 53 : 80) * 1024) return -8;
  const int ntc = (a.n_cob + CBW - 1) / CBW, ntr = (a.rows + TM - 1) / TM;
  const int grid = ((ntr + 7) / 8) * 8 * ntc;
  GemmArgs b = a;
  b.shm_bytes = (int)shm;
  if constexpr (CBW == 2 && !OCC3) {
    allow_dynamic_lds<&gemm_gx_n64w_kernel<NPXL, NST, MODE>>(160 * 1024);
    hipLaunchKernelGGL((gemm_gx_n64w_kernel<NPXL, NST, MODE>), dim3(grid), dim3(256), shm, s, b);
  } else if constexpr (CBW == 2) {
    // (red / gsh of the common epilogue live in the dead ring: 256 CBW + 128 CBW floats = 3 KB < the ring)
    allow_dynamic_lds<&gemm_gx_n64_kernel<NPXL, NST, MODE>>(64 * 1024);
    hipLaunchKernelGGL((gemm_gx_n64_kernel<NPXL, NST, MODE>), dim3(grid), dim3(256), shm, s, b);
  } else {
    allow_dynamic_lds<&gemm_gx_kernel<NPXL, NST, MODE>>(160 * 1024);
    hipLaunchKernelGGL((gemm_gx_kernel<NPXL, NST, MODE>), dim3(grid), dim3(256), shm, s, b);
  }
  return (int)hipGetLastError();
}

}  // namespace

static int gx_args_from_op(const SlideOp &o, GemmArgs &a) {
  a = GemmArgs();
  a.gx_ta = o.p[0]; a.W = o.p[1]; a.epi = (const SlideEpi *)o.p[2];
  a.in_scale = (const float *)o.p[3]; a.in_shift = (const float *)o.p[4];
  a.gx_tb = o.p[5]; a.in_add = (const float *)o.p[6]; a.gx_add_idx = (const int *)o.p[7];
  a.gidx = (const int *)o.p[8]; a.gx_d2 = (const float *)o.p[9]; a.gx_w = (const float *)o.p[10];
  a.gx_vv = (const float *)o.p[11];
  a.dbg = (unsigned long long *)o.p[12];
  a.rows = o.i[0]; a.gx_ld = o.i[1]; a.k_pad = o.i[2]; a.n_cob = o.i[3]; a.in_bs = o.i[5];
  a.gx_mode = o.i[6]; a.add_bs = o.i[7]; a.gx_add_idx_stride = o.i[8]; a.gx_vbs = o.i[9];
  a.w_cm = 1; a.x_ld = 32;
  resolve_epi(a);
  const int npxl = o.i[4];
  if (a.k_pad % 32 || a.k_pad <= 0 || a.gx_ld % 8 || a.rows <= 0 || a.n_cob <= 0 || !a.gx_ta || !a.gx_tb) return -3;
  if (a.gx_mode != 0 && (!a.in_scale || !a.in_shift)) return -3;
  if (a.in_add && ((uintptr_t)a.in_add % 16 || a.add_bs % 4 || a.gx_add_idx_stride % 4)) return -3;  // 16-byte vector loads
  if (a.gx_mode != 0 && ((uintptr_t)a.in_scale % 16 || (uintptr_t)a.in_shift % 16 || a.in_bs % 4)) return -3;
  if (a.gx_vv && ((uintptr_t)a.gx_vv % 16 || a.gx_vbs % 8)) return -3;
  if (npxl == 7 && (!a.gidx || !a.gx_d2 || !a.gx_w)) return -3;
  return 0;
}

template <int NPXL>
static int launch_gx_dual(const GemmArgs &a1, const GemmArgs &a0, hipStream_t s) {
  constexpr int NSAMP = TM >> NPXL;
  auto lds = [&](const GemmArgs &a, int nvec) {
    return (size_t)GX_DUAL_NST<NPXL> * (8192 + 4 * 64 * 16 * NSAMP) + (2 * EPI_DW + (2 * EPI_DW) % 4 + 2 * 96) * 4 + (size_t)NSAMP * nvec * a.k_pad * 2 + 16;
  };
  const size_t s1 = lds(a1, 2 + (NPXL == 7 ? 2 : 0)), s0 = lds(a0, 1 + (NPXL == 7 ? 2 : 0));
  const size_t shm = s1 > s0 ? s1 : s0;
  if (shm > (NPXL == 7 ? 53 : 80) * 1024) return -8;  // (three / two workgroups per CU)
  const int ntr = (a1.rows + TM - 1) / TM;
  const int g1 = ((ntr + 7) / 8) * 8 * ((a1.n_cob + 1) / 2), g0 = ((ntr + 7) / 8) * 8 * ((a0.n_cob + 1) / 2);
  allow_dynamic_lds<&gemm_gx_dual_kernel<NPXL>>(160 * 1024);
  GemmArgs b1 = a1, b0 = a0;
  b1.shm_bytes = b0.shm_bytes = (int)shm;
  hipLaunchKernelGGL((gemm_gx_dual_kernel<NPXL>), dim3(g1 + g0), dim3(256), shm, s, b1, b0, g1);
  return (int)hipGetLastError();
}

// SLIDE_OP_GEMM_GX_DUAL: p[0] = HOST pointer to two SlideOp (SLIDE_OP_GEMM_GX: mode 1, then mode 0) of the same block
int slide_launch_gemm_gx_dual(const SlideOp &o, hipStream_t s) {
  const SlideOp *pr = (const SlideOp *)o.p[0];
  if (!pr || pr[0].kind != SLIDE_OP_GEMM_GX || pr[1].kind != SLIDE_OP_GEMM_GX) return -3;
  if ((int)pr[0].f[0] == 3 && (int)pr[1].f[0] == 3) return slide_launch_gemm_gxs_dual(pr, s);
  GemmArgs a1, a0;
  int st = gx_args_from_op(pr[0], a1);
  if (st == 0) st = gx_args_from_op(pr[1], a0);
  if (st != 0) return st;
  if (a1.gx_mode == 0 || a0.gx_mode != 0 || a1.rows != a0.rows || pr[0].i[4] != pr[1].i[4]) return -3;
  if (pr[0].i[4] == 8) st = launch_gx_dual<8>(a1, a0, s);
  else if (pr[0].i[4] == 7) st = launch_gx_dual<7>(a1, a0, s);
  else return -4;
  if (st == -8) {  // (LDS of the dual form does not fit: two launches)
    st = slide_launch_gemm_gx(pr[0], s);
    if (st == 0) st = slide_launch_gemm_gx(pr[1], s);
  }
  return st;
}

int slide_launch_gemm_gx(const SlideOp &o, hipStream_t s) {
  GemmArgs a;
  const int ast = gx_args_from_op(o, a);
  if (ast != 0) return ast;
  const int npxl = o.i[4];
  const bool m1 = a.gx_mode != 0;
  // f[0] != 0 (the plan's default, SLIDE_GX_N64): 256 x 64 tiles, three workgroups per CU (128-channel tiles when the LDS does
  // not fit): measured 385 vs 374 shapes/s in bench.py's arrangement
  // f[0] == 2: the 64-channel tile at two workgroups per CU (both modes; the plan asks for it when the 128-channel grid would
  // leave CUs empty)
  const int n64 = (int)o.f[0];
  // (mode 1 only -- the keys -> u layers: with mode 0's PAIR residual the epilogue does not fit 168 registers)
  int st = -8;
  if (n64 == 1 && m1) {  // 64-channel tiles at three workgroups per CU (a two-stage ring of this form spills at 168 registers)
    if (npxl == 8) st = launch_gx<8, 3, 1, 2>(a, s);
    else if (npxl == 7) st = launch_gx<7, 3, 1, 2>(a, s);
    if (st != -8) return st;
  }
  if (n64 == 2) {
    if (npxl == 8) st = m1 ? launch_gx<8, 3, 1, 2, false>(a, s) : launch_gx<8, 3, 0, 2, false>(a, s);
    else if (npxl == 7) st = m1 ? launch_gx<7, 3, 1, 2, false>(a, s) : launch_gx<7, 3, 0, 2, false>(a, s);
    if (st != -8) return st;
  }
  // 128-channel tiles at two workgroups per CU: three ring stages, else two
  if (npxl == 8) {
    st = m1 ? launch_gx<8, 3, 1>(a, s) : launch_gx<8, 3, 0>(a, s);
    if (st == -8) st = m1 ? launch_gx<8, 2, 1>(a, s) : launch_gx<8, 2, 0>(a, s);
    return st;
  }
  if (npxl == 7) {
    st = m1 ? launch_gx<7, 3, 1>(a, s) : launch_gx<7, 3, 0>(a, s);
    if (st == -8) st = m1 ? launch_gx<7, 2, 1>(a, s) : launch_gx<7, 2, 0>(a, s);
    return st;
  }
  return -4;
}
