"""The case matrix of the pair-decomposition ops, their float64 references, error bounds and mutants -- shared by
tests/test_hip_pair_arith.py (every case on the GPU against the reference; on the CPU every bound against the mutants).

A case is ONE launch (two for the composition cases) emitted by the engine's own emitters, so the host-side packing is under test too:
  op "gx"   SLIDE_OP_GEMM_GX, fp16 tables (csrc/gemm_gx.hip, gemm_gx_body)         DenoiserEngine._gemm(gx=GxArgs)
  op "gxs"  SLIDE_OP_GEMM_GX, float tables, split arithmetic (csrc/gemm_gxs.hip)   DenoiserEngine._gemm(gx=GxArgs, chain=_chained_layer)
  op "sa"   SLIDE_OP_SA_CHAIN (csrc/sa_chain.hip, sa_chain_body)                   DenoiserEngine._sa_chain
  op "pf"   SLIDE_OP_PAIR_FIRST (csrc/gemm_small.h, small_body<., ., PAIR>)        DenoiserEngine._pair_first (fp16 plan)
  op "pn"   SLIDE_OP_PAIR_NORM version 2, float tables (csrc/pair_norm.hip)        DenoiserEngine._pair_first (split plan)
  op "comp" PAIR_FIRST -> mode-0 GEMM_GX against the K-EXPANDED float64 evaluation of the first two layers of a block

branch of the product build's launchers                | cases
  gemm_gx_n64_kernel<8 / 7, 3, 1>                      | gx_n8_m1_n64, gx_n7_m1_n64 (k_pad <= 224 at 128-row samples: 53 KB)
  gemm_gx_n64w_kernel<8, 3, 0 / 1>                     | gx_n8_m0_n64w, gx_n8_m1_n64w (k_pad 4096: the three-per-CU form declines)
  gemm_gx_n64w_kernel<7, 3, 0 / 1>                     | gx_n7_m0_n64w, gx_n7_m1_n64w (k_pad 544 > 224)
  gemm_gx_kernel<8, 3, 0 / 1>   (SLIDE_GX_N64=0)       | gx_n8_m0_w128, gx_n8_m1_w128
  gemm_gx_kernel<8, 2, 0 / 1>   (SLIDE_GX_N64=0)       | gx_n8_m0_w128_2st (k_pad 9152 > 9144), gx_n8_m1_w128_2st (4608 > 4572)
  gemm_gx_kernel<7, 3, 0 / 1>   (SLIDE_GX_N64=0)       | gx_n7_m0_w128 (k_pad 96 <= 480), gx_n7_m1_w128 (64 <= 352)
  gemm_gx_kernel<7, 2, 0 / 1>   (SLIDE_GX_N64=0)       | gx_n7_m0_w128_2st, gx_n7_m1_w128_2st (k_pad 544)
  gemm_gxs_kernel<8 / 7, 0 / 1>                        | gxs_n8_m0, gxs_n8_m1, gxs_n7_m0, gxs_n7_m1
  gemm_gxs_chain_kernel<8>                             | gxs_n8_chain;  gxs_w32 (|w| = 32): the plan raises SlideHipError
  sa_chain_kernel<4> / <8>                             | sa_64_128_256, sa_128_128_512 / sa_192_256_512
  pair_first_kernel<false / true>                      | pf_k16, pf_k16_lead, pf_k16_cluster / pf_k8_knn, pf_k8_same, pf_k8_q15
  pair_norm2_kernel<false / true, float, 512>          | pn_k16_32, pn_k16_544_fin, pn_k16_cluster / pn_k8_32, pn_k8_2048_fin;  pn_2080: -3
                                                       | (ld 32, 544 = two passes of 320 threads, 2048 = the limit, 2080 refused)
  PAIR_FIRST -> GEMM_GX                                | comp_k16, comp_k8
  gemm_gx_dual_kernel<7> (SLIDE_OP_GEMM_GX_DUAL)       | dual_n7 = gx_n7_m1_n64 + gx_n7_m0_n64w in ONE launch through the host-pointer form
  SLIDE_OP_GEMM_GX_DUAL, LDS does not fit              | dual_n7_two_launches = gx_n7_m1_k1568 (gemm_gx_n64w_kernel<7, 3, 1>) + gx_n7_m0_w128_2st:
                                                       | the launcher falls back to the two single launches
  sa_chain_p_kernel<4> (SLIDE_OP_SA_CHAIN_P)           | sa_p_64_128_256 = sa_64_128_256 + the 16-row query GEMM f16_n4_norm_aff of gemm_cases
                                                       | (its B set to the chain's: the launcher wants rows == 16 B)
LDS thresholds (launch_gx, csrc/gemm_gx.hip: shm = NST (4096 CBW + 4096 NSAMP) + (40 CBW + 96 CBW) 4 + 2 NSAMP NVEC k_pad + 16, NSAMP = 1 / 2
samples per tile, NVEC = 1 (mode 0) / 2 (mode 1) + 2 (128-row samples)):  64-channel tiles, three stages: 36864 (49152) + 1104 +
2 NSAMP NVEC k_pad <= 53 KB for the three-per-CU form -> k_pad <= 4076 (256 rows, mode 1), <= 251 (128 rows, mode 1); 128-channel tiles,
three stages: 61440 (73728) + 2192 + ... <= 80 KB -> k_pad <= 9144 / 4572 (256 rows, mode 0 / 1), <= 500 / 375 (128 rows): beyond that two.

HOST-POINTER PAIRS (DUAL, CHAIN_P).  p[0] of the op is a HOST pointer to two SlideOps; every output is held to the float64 reference and
bound its single-launch case already has.  The dual form runs both GEMMs on 64-channel tiles with NST = 2 (128-row samples) / 3 ring
stages: dual_lds() restates launch_gx_dual's LDS, NST (8192 + 4096 NSAMP) + (2 EPI_DW + 192) 4 + 2 NSAMP NVEC k_pad + 16 <= 53 KB (128-row
samples) / 80 KB: at 128-row samples mode 1 fits up to k_pad 1274, so k_pad 1568 is the two-launch fallback.

GENERATED X (fp16; gemm_gx_body::compute_step, sa_chain_body::compute1).  r16 = one rounding to fp16:
  y = r16(ta[q] + tb[p]);  128-row samples: y = r16(d2h vdh + y), y = r16(wh vwh + y) (fp16 FMAs), d2h = r16(min(d2, 65504));
  y = max(y, 0);  mode 0: x = r16(y + addh);  mode 1: x = r16(y scaleh + shifth)    (vdh, vwh, addh, scaleh, shifth: r16 when staged)
The reference evaluates each step in float64 and rounds once.  That is the kernel's value exactly: every operand is a multiple of
2^-24, a product of two a multiple of 2^-48, and every sum stays below 2^5 in magnitude, so float64 (53 bits) holds it exactly -- the
reference CHECKS this on every FMA with an error-free transformation (_fma16).  Magnitudes: tables N(0, 1) (mode 1 "common": a + 30,
shift - 30), d2 in [0, 4), w in [0, 1), vd, vw 0.3 N(0, 1), scale in [0.5, 1.5].  X' carries no tolerance; the contraction has
gemm_cases' bound C_ACC (|X'| . |W|^T + |bias|), and the epilogue steps (NORM / ReLU / PAIR residual / store / STATS) are gemm_cases'.
d2 beyond the fp16 range (the fp16 kernels clamp at 65504, the table pass does not) is NOT tested.

GENERATED X (split; gemm_gxs_body::store_chunk), fp32: x = a + b [, fmaf(d2, vd, x), fmaf(w, vw, x)], max, x + add | fmaf(x, scale,
shift): n = 1 (256-row) or 3 (128-row) roundings before the max, one after.  With S = |ta| + |tb| + |d2 vd| + |w vw|:
  mode 0: xb = (n + 1) u (S + |add|) (1 + 8 u);   mode 1: xb = (n u S |scale| + u (S |scale| + |shift|)) (1 + 8 u)
propagated through |W| beside C_ACC A (gemm_cases.forward(xb=...)).  The chained second layer (gemm_gxs_chain_kernel) takes the first
layer's output bound as its xb: the values stay in accumulators, no store rounding lies between (gemm_cases adds u |y| for an fp32
store there: the register value's own rounding counted twice, 2^-24 |h2| too wide).

SA CHAIN (sa_chain_body).  Stage 1: X' as above (mode 0, natural order), contraction (bias as the accumulators' initial value: one more
term of the fp32 sum, inside C_ACC A), GroupNorm, then norm_pack: n16 = r16(normalised value), max(., 0), h2 = r16(. + r16(add1)).
The reference keeps h2 = max(n, 0) + r16(add1) unrounded; with b1 the bound of n, n16 is within b1' = b1 (1 + 2^-11) + 2^-11 |n| +
2^-25 of it (gemm_cases' fp16 store bound) and h2's fp16 value within xb2 = b1' (1 + 2^-11) + 2^-11 |h2| + 2^-25 -- the roundings can
fall either way, so "h2_unrounded" (stage 2 fed the unrounded h2) is NOT a mutant: the test asserts it stays INSIDE the bound.
Stage 2: xb2 . |W2|^T + C_ACC A2, GroupNorm, o16 = r16(normalised value) -> ReLU, then out = r16(o16 + r16(ra[q] + rb[p])) (packed fp16
adds): the bound of o16 through one more fp16 rounding of the sum.

TABLE PASSES (pair_first's epilogue, gemm_small.h; pair_norm2_body, pair_norm.h).  Per channel c and point p of a sample:
  y = X W^T + bias (PAIR_FIRST: fp16 operands, by = C_ACC A with A = |X| . |W|^T + |bias|; float pass: y is an fp32 INPUT, by = 0)
  a = y + wa . xyz, b = wb . xyz      da = by + 4 u (|y| + sum |wa_i x_i|),  db = 3 u sum |wb_i x_i|   (three products, three adds)
  v(p, j) = a[q] + b[p] (+ d2 vd + w vw), max(., 0) under PRE_RELU:  dv = da[q] + db[p] + 5 u (|a| + |b| + |d2 vd| + |w vw|)
  explicit loop over the n = 16 K pairs (sequential fp32 sums, one FMA per square):
      ds = sum dv + n u sum |v|,  dss = sum (2 |v| dv + dv^2) + n u sum v^2
  closed form (float pass, K = 16, no PRE_RELU): s = 16 (A + B), ss = 16 (A2 + B2) + 2 A B with A = sum a, B = sum b, A2 = sum a^2:
      dA = sum da + 16 u sum |a| (dB likewise), dA2 = sum (2 |a| da + da^2) + 16 u A2,
      ds = 16 (dA + dB) + 2 u |s|,  dss = 16 (dA2 + dB2) + 2 (|A| dB + |B| dA + dA dB) + 4 u (16 (A2 + B2) + 2 |A| |B|)
      -- the last term is what the closed form costs where a and b carry opposite common modes (the displaced cluster): ss is small
      against 16 (A2 + B2) and 2 A B each.
  STATS: (s, ss) x stats_scale, bounds likewise + u.  NORM: the group's sums over gs channels (+ (log2 gs) u), mean m = S inv_count,
  var = max(SS inv_count - m^2, 0), g = gamma rsq(var + eps), sh = beta - m g:
      dm = dS inv + 2 u |m|,  dvar = dSS inv + 2 |m| dm + dm^2 + 3 u (SS inv + m^2),  dg = |g| (0.6 dvar / (var + eps) + 4 u),
      dsh = |m| dg + |g| dm + 3 u (|beta| + |m g|)
  ta = a g + sh, tb = b g, vv = (vd g | vw g):  d(ta) = |g| da + |a| dg + dsh + 2 u (|a g| + |sh|),  d(tb) = |g| db + |b| dg + u |b g|,
  then the store: fp16 d (1 + 2^-11) + 2^-11 |ref| + 2^-25, float d + u |ref|;  d(vv) = |v.| dg + 2 u |v. g|.
  SlideGnFin (joint [query | key] GroupNorm finalised in the launch): group sums S = sum_c csum[c] sequentially over the group's cn
  channels, dS = sum d(csum) + cn u sum |csum|; mean, var as above; rstd = 1 / sqrtf (4 u); scale = gamma rstd, shift = beta - mean scale.

COMPOSITION: the reference is the float64 K-expanded evaluation [feat[q] | rel | abs | centre (| d2 | w)] . W1^T -> GroupNorm over the
sample's K-expanded rows -> ReLU -> + add -> W2; the bound is the consumer's with the producer's table bounds as input uncertainty
(2^-11 |ta| and 2^-11 |tb| SEPARATELY, the cost of storing two fp16 tables), through the consumer's fp16 steps (each 1-Lipschitz in its
inputs up to its own rounding 2^-11 |value|).

Mutants (test_pair_bounds_see_the_mutants): see MUTANT_DOC; a mutant that is the same computation on a case's inputs (the next slot
of a table whose slots all name one neighbour) does not apply there; one below the arithmetic's resolution goes to EXEMPT with the case
of the same kernel that shows it."""
import zlib

import numpy as np

import gemm_cases as G
from gemm_cases import C_ACC, EPI_NORM, EPI_RAW, EPI_STATS, EPS, U, gn_params, r16, r32, ru  # noqa: F401

H = 2.0 ** -11  # fp16 unit roundoff

MUTANT_DOC = {
    "k_tail": "last logical K column ignored", "sample_vec": "add / scale / shift / vv of the neighbouring sample",
    "swap_pq": "ta[p] + tb[q]", "nbr_natural": "q = slot instead of the table", "nbr_next_slot": "the next slot's neighbour",
    "drop_vd": "d2 vd missing", "drop_vw": "w vw missing", "scalars_other_row": "d2 / w of the tile's other row block",
    "relu_after_add": "mode 0: max(y + add, 0)", "affine_before_relu": "mode 1: max(y scale + shift, 0)",
    "drop_whi_xlo": "split: w_hi x_lo dropped", "drop_wlo_xhi": "split: w_lo x_hi dropped",
    "gs_swapped": "SA chain: stage 2 normalised with stage 1's group size", "add1_before_relu": "SA chain: relu(n + add1)",
    "residual_swap_pq": "SA chain: ra[p] + rb[q]",
    "unbiased_var": "variance over n - 1", "count_256_at_K8": "inv_count of the 256-row form at K = 8",
    "stats_ignore_pre_relu": "statistics of the un-rectified values", "closed_form_under_relu": "the closed form where PRE_RELU is set",
    "shift_in_both_tables": "sh added to tb as well", "vv_unscaled": "vv = (vd | vw) without g",
    "norm_tail_channels": "the last C % G channels normalised", "fin_group_of_neighbour": "GnFin: group id off by one at a boundary",
}
NON_MUTANTS = ("h2_unrounded",)


def _p(name, op, prec, npxl, B, K, k_pad, N, epi, kernel, dist="normal", **kw):
    c = dict(name=name, op=op, prec=prec, npxl=npxl, B=B, K=K, k_pad=k_pad, N=N, epi=epi, kernel=kernel, dist=dist, gxmode=0, add=None,
             pre_relu=False, post_relu=False, pair=False, out="rm", coff=0, t_extra=0, nbr="knn", env={}, status=0, raises=False,
             chain=None, add1=False, stats_scale=1.0)
    c.update(kw)
    return c


N64OFF = {"SLIDE_GX_N64": "0"}
GX = [
    _p("gx_n8_m1_n64", "gx", "fp16", 8, 3, 35, 64, 51, EPI_NORM, "gemm_gx_n64_kernel<8, 3, 1>", "common", gxmode=1, post_relu=True),
    _p("gx_n7_m1_n64", "gx", "fp16", 7, 3, 96, 96, 64, EPI_STATS, "gemm_gx_n64_kernel<7, 3, 1>", gxmode=1, stats_scale=0.25, coff=32, t_extra=40),
    _p("gx_n8_m0_n64w", "gx", "fp16", 8, 9, 32, 32, 111, EPI_NORM, "gemm_gx_n64w_kernel<8, 3, 0>", add="plain", post_relu=True, pair=True, out="cm"),
    _p("gx_n8_m1_n64w", "gx", "fp16", 8, 1, 4095, 4096, 32, EPI_RAW, "gemm_gx_n64w_kernel<8, 3, 1>", "small", gxmode=1),
    _p("gx_n7_m0_n64w", "gx", "fp16", 7, 3, 543, 544, 96, EPI_RAW, "gemm_gx_n64w_kernel<7, 3, 0>", add="idx", pair=True, coff=64, t_extra=24),
    _p("gx_n7_m1_n64w", "gx", "fp16", 7, 1, 544, 544, 64, EPI_NORM, "gemm_gx_n64w_kernel<7, 3, 1>", gxmode=1, nbr="same", post_relu=True),
    _p("gx_n8_m0_w128", "gx", "fp16", 8, 3, 96, 96, 111, EPI_NORM, "gemm_gx_kernel<8, 3, 0>", post_relu=True, pair=True, env=N64OFF, coff=8, t_extra=8),
    _p("gx_n8_m1_w128", "gx", "fp16", 8, 9, 35, 64, 32, EPI_STATS, "gemm_gx_kernel<8, 3, 1>", gxmode=1, env=N64OFF),
    _p("gx_n8_m0_w128_2st", "gx", "fp16", 8, 1, 9151, 9152, 32, EPI_RAW, "gemm_gx_kernel<8, 2, 0>", add="plain", env=N64OFF),
    _p("gx_n8_m1_w128_2st", "gx", "fp16", 8, 3, 4608, 4608, 64, EPI_RAW, "gemm_gx_kernel<8, 2, 1>", gxmode=1, env=N64OFF, out="fm"),
    _p("gx_n7_m0_w128", "gx", "fp16", 7, 3, 96, 96, 96, EPI_NORM, "gemm_gx_kernel<7, 3, 0>", add="plain", pair=True, nbr="q15", env=N64OFF, out="fm"),
    _p("gx_n7_m1_w128", "gx", "fp16", 7, 9, 35, 64, 64, EPI_RAW, "gemm_gx_kernel<7, 3, 1>", "common", gxmode=1, env=N64OFF, out="cm"),
    _p("gx_n7_m0_w128_2st", "gx", "fp16", 7, 1, 543, 544, 32, EPI_STATS, "gemm_gx_kernel<7, 2, 0>", "small", add="plain", pre_relu=True, env=N64OFF),
    _p("gx_n7_m1_w128_2st", "gx", "fp16", 7, 3, 544, 544, 51, EPI_NORM, "gemm_gx_kernel<7, 2, 1>", gxmode=1, post_relu=True, env=N64OFF),
    # (beyond the dual form's LDS: the mode-1 half of dual_n7_two_launches)
    _p("gx_n7_m1_k1568", "gx", "fp16", 7, 1, 1568, 1568, 32, EPI_RAW, "gemm_gx_n64w_kernel<7, 3, 1>", gxmode=1),
]
GXS = [
    _p("gxs_n8_m0", "gxs", "split", 8, 3, 35, 64, 111, EPI_NORM, "gemm_gxs_kernel<8, 0>", "bigw", add="idx", post_relu=True, pair=True, coff=8, t_extra=4),
    _p("gxs_n8_m1", "gxs", "split", 8, 9, 96, 96, 32, EPI_STATS, "gemm_gxs_kernel<8, 1>", "common", gxmode=1),
    _p("gxs_n7_m0", "gxs", "split", 7, 3, 543, 544, 96, EPI_RAW, "gemm_gxs_kernel<7, 0>", add="plain", pair=True),
    _p("gxs_n7_m1", "gxs", "split", 7, 1, 32, 32, 64, EPI_NORM, "gemm_gxs_kernel<7, 1>", "small", gxmode=1, post_relu=True, nbr="same"),
    _p("gxs_n8_chain", "gxs", "split", 8, 3, 96, 96, 64, EPI_NORM, "gemm_gxs_chain_kernel<8>", "bigw", add="plain", post_relu=True, add1=True,
       chain=dict(N=111)),
    _p("gxs_w32", "gxs", "split", 8, 1, 32, 32, 32, EPI_RAW, "(none: SlideHipError)", "w32", raises=True),
]
# (k1, n1, n2): group sizes 4 / 8 / 16 across the two stages
SA = [
    _p("sa_64_128_256", "sa", "fp16", 8, 3, 64, 64, 128, EPI_NORM, "sa_chain_kernel<4>", out="cm", chain=dict(N=256)),
    _p("sa_192_256_512", "sa", "fp16", 8, 1, 192, 192, 256, EPI_NORM, "sa_chain_kernel<8>", add="plain", add1=True, out="fm", chain=dict(N=512),
       t_extra=8),
    _p("sa_128_128_512", "sa", "fp16", 8, 9, 128, 128, 128, EPI_NORM, "sa_chain_kernel<4>", add="idx", add1=True, out="cm", chain=dict(N=512)),
]
CASES = GX + GXS + SA
# the host-pointer pair launches (module docstring)
DUAL = [dict(name="dual_n7", m1="gx_n7_m1_n64", m0="gx_n7_m0_n64w", fits=True),
        dict(name="dual_n7_two_launches", m1="gx_n7_m1_k1568", m0="gx_n7_m0_w128_2st", fits=False)]
CHAIN_P = [dict(name="sa_p_64_128_256", sa="sa_64_128_256", q=dict(G.CASE_BY_NAME["f16_n4_norm_aff"], B=3), kernel="sa_chain_p_kernel<4>")]


def dual_lds(c, epi_dw):
    """launch_gx_dual's dynamic LDS of one half (csrc/gemm_gx.hip) and its limit"""
    nsamp = 256 >> c["npxl"]
    nst = 2 if c["npxl"] == 7 else 3
    nvec = (2 if c["gxmode"] else 1) + (2 if c["npxl"] == 7 else 0)
    return nst * (8192 + 4 * 64 * 16 * nsamp) + (2 * epi_dw + (2 * epi_dw) % 4 + 2 * 96) * 4 + nsamp * nvec * c["k_pad"] * 2 + 16, \
        (53 if c["npxl"] == 7 else 80) * 1024
CASE_BY_NAME = {c["name"]: c for c in CASES}
KERNELS = (["gemm_gx_n64_kernel<%d, 3, 1>" % n for n in (7, 8)] + ["gemm_gx_n64w_kernel<%d, 3, %d>" % (n, m) for n in (7, 8) for m in (0, 1)] +
           ["gemm_gx_kernel<%d, %d, %d>" % (n, s, m) for n in (7, 8) for s in (3, 2) for m in (0, 1)] +
           ["gemm_gxs_kernel<%d, %d>" % (n, m) for n in (7, 8) for m in (0, 1)] + ["gemm_gxs_chain_kernel<8>", "sa_chain_kernel<4>",
                                                                                    "sa_chain_kernel<8>"])

# (case, mutant) -> the case of the same kernel where that mutant IS visible
EXEMPT = {}


def mutants(c):
    if c["raises"] or c["status"] != 0:
        return []
    m = []
    if c["op"] in ("gx", "gxs", "sa"):
        has_vec = c["add"] is not None or c["gxmode"] == 1 or c["npxl"] == 7 or c["add1"]
        m.append("k_tail")
        if c["B"] > 1 and has_vec:
            m.append("sample_vec")
        if c["npxl"] == 8:
            m.append("swap_pq")
        else:
            m += ["nbr_natural", "drop_vd", "drop_vw", "scalars_other_row"]
            if c["nbr"] == "knn":  # (a table whose slots all name one neighbour: the next slot is the same computation)
                m.append("nbr_next_slot")
        if c["gxmode"] == 0 and c["add"] is not None:
            m.append("relu_after_add")
        if c["gxmode"] == 1:
            m.append("affine_before_relu")
        if c["prec"] == "split":
            m += ["drop_whi_xlo", "drop_wlo_xhi"]
    if c["op"] == "sa":
        m += ["gs_swapped", "residual_swap_pq"] + (["add1_before_relu"] if c["add1"] else [])
    return m


# ------------------------------------------------------------------------------------------------------------------ inputs
def neighbour_table(rs, kind, pts):
    """[n][16] int32: slots 0..7 the table proper, slots 8..15 OTHER valid indices (a kernel that read them would get wrong numbers)"""
    n = pts.shape[0]
    nbr = np.empty((n, 16), np.int32)
    for s in range(n // 16):
        x = pts[16 * s:16 * s + 16].astype(np.float64)
        order = np.argsort(((x[:, None] - x[None]) ** 2).sum(-1), axis=1, kind="stable")
        for p in range(16):
            if kind == "knn":
                nbr[16 * s + p] = order[p]
            else:
                q = 15 if kind == "q15" else int(rs.randint(16))
                nbr[16 * s + p, :8] = q
                nbr[16 * s + p, 8:] = (q + 1 + np.arange(8)) % 16
    return nbr


def make_data(c):
    """the case's fp32 inputs in logical layouts -- deterministic per case name"""
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    B, K, N, dist = c["B"], c["K"], c["N"], c["dist"]
    nt = B * 16
    sm = np.float32(1e-3 if dist == "small" else 1.0)
    d = dict(ta=f(nt, K) * sm, tb=f(nt, K) * sm, W=f(N, K) / np.float32(np.sqrt(K)), bias=0.5 * f(N) * sm, gamma=1 + 0.2 * f(N), beta=0.2 * f(N))
    if dist == "common":
        d["ta"] = d["ta"] + np.float32(30.0)
    if dist in ("bigw", "w32"):  # single-accumulator split kernels: |w| < 32
        top = 30.0 if dist == "bigw" else 32.0
        d["W"] = rs.uniform(-30.0, 30.0, (N, K)).astype(np.float32)
        d["W"].flat[rs.randint(d["W"].size)] = top
    if c["add"] == "plain":
        d["add"] = f(B, K) * sm
    elif c["add"] == "idx":
        d["add_tab"], d["add_t"] = f(4, B, K) * sm, 2
        d["add"] = d["add_tab"][2]
    if c["gxmode"] == 1:
        d["scale"] = rs.uniform(0.5, 1.5, (B, K)).astype(np.float32)
        d["shift"] = (-(30.0 if dist == "common" else 0.0) + 0.5 * f(B, K) * sm).astype(np.float32)
    if c["npxl"] == 7:
        d["pts"] = f(nt, 3)
        d["nbr"] = neighbour_table(rs, c["nbr"], d["pts"]).reshape(-1)
        d["d2"] = rs.uniform(0, 4, (nt, 16)).astype(np.float32)
        d["w"] = rs.uniform(0, 1, (nt, 16)).astype(np.float32)
        d["d2"][:, 8:], d["w"][:, 8:] = 6e4, 6e4  # slots 8..15 are never read: large FINITE values
        d["vd"], d["vw"] = 0.3 * f(B, K) * sm, 0.3 * f(B, K) * sm
    NR = c["chain"]["N"] if c["chain"] else N
    if c["pair"] or c["chain"]:
        d["rta"], d["rtb"] = f(nt, NR), f(nt, NR)
        if c["npxl"] == 7:
            d["rvd"], d["rvw"] = 0.3 * f(NR), 0.3 * f(NR)
    if c["chain"]:
        n1 = N
        d["W2"] = f(NR, n1) / np.float32(np.sqrt(n1))
        if dist == "bigw":
            d["W2"] = rs.uniform(-30.0, 30.0, (NR, n1)).astype(np.float32)
        d["bias2"], d["gamma2"], d["beta2"] = 0.5 * f(NR), 1 + 0.2 * f(NR), 0.2 * f(NR)
    if c["add1"]:
        d["add1"] = f(B, N)
    return {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------------------ generated X
def _fma16(x, y, z):
    """r16(x y + z) of fp16-valued float64 arrays -- with the proof that float64 evaluated it exactly (TwoSum's error term is 0)"""
    p = x * y
    s = p + z
    bb = s - p
    err = (p - (s - bb)) + (z - bb)
    assert not err.any(), "the float64 evaluation of an fp16 FMA is not exact at these magnitudes"
    return r16(s)


def gen_x(c, d, mutant=None):
    """X' [rows][K] as the kernel generates it, and (split) its bound xb"""
    B, K, npxl = c["B"], c["K"], c["npxl"]
    rows = np.arange(B << npxl)
    smp, pxl = rows >> npxl, rows & ((1 << npxl) - 1)
    h = c["prec"] == "fp16"
    rd = r16 if h else (lambda a: np.asarray(a, np.float64))
    vs = (smp + 1) % B if mutant == "sample_vec" else smp  # the sample whose vectors a row reads
    if npxl == 8:
        p, q = pxl >> 4, pxl & 15
        if mutant == "swap_pq":
            p, q = q, p
    else:
        p, j = pxl >> 3, pxl & 7
        slot = (smp * 16 + p) * 16 + j
        q = d["nbr"][(smp * 16 + p) * 16 + (j + 1) % 8] if mutant == "nbr_next_slot" else j if mutant == "nbr_natural" else d["nbr"][slot]
    ta, tb = rd(d["ta"])[smp * 16 + q], rd(d["tb"])[smp * 16 + p]
    y = rd(ta + tb)
    S = np.abs(ta) + np.abs(tb)
    nr = 1
    if npxl == 7:
        sl = slot
        if mutant == "scalars_other_row":
            r2 = rows ^ 32
            s2, x2 = r2 >> npxl, r2 & 127
            sl = (s2 * 16 + (x2 >> 3)) * 16 + (x2 & 7)
        d2 = d["d2"].reshape(-1)[sl].astype(np.float64)[:, None]
        w = d["w"].reshape(-1)[sl].astype(np.float64)[:, None]
        if h:
            d2 = r16(np.minimum(d2, 65504.0))
        vd, vw = rd(d["vd"])[vs], rd(d["vw"])[vs]
        w = rd(w)
        if mutant != "drop_vd":
            y = _fma16(d2, vd, y) if h else d2 * vd + y
            S = S + np.abs(d2 * vd)
        if mutant != "drop_vw":
            y = _fma16(w, vw, y) if h else w * vw + y
            S = S + np.abs(w * vw)
        nr = 3
    if c["gxmode"] == 0:
        add = rd(d["add"])[vs] if "add" in d else np.zeros((1, K))
        x = np.maximum(rd(y + add), 0) if mutant == "relu_after_add" else rd(np.maximum(y, 0) + add)
        xb = (nr + 1) * U * (S + np.abs(add)) * (1 + 8 * U)
    else:
        sc, sh = rd(d["scale"])[vs], rd(d["shift"])[vs]
        fma = _fma16 if h else (lambda a_, b_, c_: a_ * b_ + c_)
        x = np.maximum(fma(y, sc, sh), 0) if mutant == "affine_before_relu" else fma(np.maximum(y, 0), sc, sh)
        xb = (nr * U * S * np.abs(sc) + U * (S * np.abs(sc) + np.abs(sh))) * (1 + 8 * U)
    return x, (None if h else xb)


def _gemm_case(c, K, N, epi, **kw):
    return G._c(c["name"], c["prec"], c["npxl"], c["B"], K, N, epi, c["kernel"], pre_relu=c["pre_relu"], **kw)


def _res_data(c, d):
    r = dict(ta=d["rta"], tb=d["rtb"])
    if c["npxl"] == 7:
        r.update(nbr=d["nbr"], d2=d["d2"], w=d["w"], vd=d["rvd"], vw=d["rvw"])
    return r


def forward(c, d, mutant=None):
    """float64 reference of a case or of one of its mutants: dict(y, stored, b [, stats, stats_b])"""
    if c["op"] == "sa":
        return sa_forward(c, d, mutant)
    X, xb = gen_x(c, d, mutant)
    gm = mutant if mutant in ("k_tail", "drop_whi_xlo", "drop_wlo_xhi") else None
    pair = ("nbr" if c["npxl"] == 7 else "pair") if c["pair"] else None
    gd = dict(X=X, W=d["W"], bias=d["bias"], gamma=d["gamma"], beta=d["beta"])
    if c["chain"] is None:
        gc = _gemm_case(c, c["K"], c["N"], c["epi"], post_relu=c["post_relu"], pair=pair, stats_scale=c["stats_scale"])
        if pair:
            gd.update(_res_data(c, d))
        return G.forward(gc, gd, mutant=gm, xb=xb)
    # chained second layer (split): h2 stays in the accumulators
    g1 = _gemm_case(c, c["K"], c["N"], EPI_NORM, post_relu=True)
    if c["add1"]:
        gd["addvec"] = d["add1"]
    f1 = G.forward(g1, gd, mutant=gm, xb=xb)
    g2 = _gemm_case(c, c["N"], c["chain"]["N"], EPI_NORM, post_relu=True, pair="pair")
    g2["pre_relu"] = False
    gd2 = dict(X=f1["y"], W=d["W2"], bias=d["bias2"], gamma=d["gamma2"], beta=d["beta2"], **_res_data(c, d))
    return G.forward(g2, gd2, mutant=gm if gm != "k_tail" else None, xb=f1["b"])  # (a dropped cross product: in both contractions)


def sa_forward(c, d, mutant=None):
    B, k1, n1, n2 = c["B"], c["K"], c["N"], c["chain"]["N"]
    X, _ = gen_x(c, d, mutant if mutant in ("swap_pq", "relu_after_add", "sample_vec") else None)
    smp = np.arange(B * 256) >> 8
    g1 = _gemm_case(c, k1, n1, EPI_NORM, post_relu=True)
    f1 = G.forward(g1, dict(X=X, W=d["W"], bias=d["bias"], gamma=d["gamma"], beta=d["beta"]), mutant="k_tail" if mutant == "k_tail" else None)
    n_pos, b1 = f1["y"], f1["b"]  # max(n, 0) and the bound of its fp16 value (gemm_cases' fp16 store = norm_pack's conversion)
    a1 = r16(d["add1"])[(smp + 1) % B if mutant == "sample_vec" else smp] if c["add1"] else 0.0
    if mutant == "add1_before_relu":  # (needs the signed value: recompute without the ReLU)
        g1n = _gemm_case(c, k1, n1, EPI_NORM, post_relu=False)
        h2 = np.maximum(G.forward(g1n, dict(X=X, W=d["W"], bias=d["bias"], gamma=d["gamma"], beta=d["beta"]))["y"] + a1, 0)
    else:
        h2 = n_pos + a1
    xb2 = b1 * (1 + H) + H * np.abs(h2) + 2.0 ** -25
    if mutant == "h2_rounded":  # what the kernel does; the reference keeps h2 unrounded ("h2_unrounded")
        h2 = r16(r16(n_pos) + a1)
    g2 = _gemm_case(c, n1, n2, EPI_NORM, post_relu=True)
    gd2 = dict(X=h2, W=d["W2"], bias=d["bias2"], gamma=d["gamma2"], beta=d["beta2"])
    if mutant == "gs_swapped":
        real, gs1 = G.gn_params, gn_params(n1)[2]
        G.gn_params = lambda N_: (N_ // gs1, N_, gs1)
        try:
            f2 = G.forward(g2, gd2, xb=xb2)
        finally:
            G.gn_params = real
    else:
        f2 = G.forward(g2, gd2, xb=xb2)
    gr = _gemm_case(c, n1, n2, EPI_RAW, pair="pair")
    rd_ = _res_data(c, d)
    if mutant == "residual_swap_pq":
        rd_ = dict(ta=d["rtb"], tb=d["rta"])  # (ta[q] + tb[p] with the tables exchanged is rb[q] + ra[p])
    r = G.pair_residual(gr, rd_)
    y = f2["y"] + r
    b = f2["b"] * (1 + H) + H * np.abs(y) + 2.0 ** -25
    return dict(y=y, stored=r16(r16(f2["y"]) + r), b=b, stats=None, stats_b=None)


# =================================================================================================================== table passes
def _t(name, op, K, B, C, segs, kernel, dist="normal", **kw):
    """segs: (logical width, epilogue mode, PRE_RELU) of the pair segments, in table order"""
    c = dict(name=name, op=op, prec="fp16" if op in ("pf", "comp") else "split", K=K, npxl=7 if K == 8 else 8, B=B, C=C, segs=segs, kernel=kernel,
             dist=dist, lead=None, fin=None, nbr="knn", status=0, raises=False, env={}, ld_claim=None, N2=None, epi2=EPI_NORM)
    c.update(kw)
    return c


R, NM, ST = EPI_RAW, EPI_NORM, EPI_STATS
PF = [
    # res_connect (RAW), first_mlp (NORM, ragged 111), keys (STATS + PRE_RELU): 64 + 160 + 128 = 352 channels > 256
    _t("pf_k16", "pf", 16, 3, 35, ((64, R, False), (111, NM, False), (128, ST, True)), "pair_first_kernel<false>"),
    _t("pf_k16_lead", "pf", 16, 9, 96, ((51, NM, False), (64, ST, False)), "pair_first_kernel<false>", "common", lead=32),
    _t("pf_k16_cluster", "pf", 16, 1, 32, ((128, NM, False), (64, ST, True)), "pair_first_kernel<false>", "cluster"),
    _t("pf_k8_knn", "pf", 8, 3, 96, ((64, R, False), (51, NM, False), (32, ST, True)), "pair_first_kernel<true>", lead=64),
    _t("pf_k8_same", "pf", 8, 1, 35, ((128, NM, False), (111, NM, True)), "pair_first_kernel<true>", "small", nbr="same"),
    _t("pf_k8_q15", "pf", 8, 9, 32, ((64, NM, False), (64, ST, False)), "pair_first_kernel<true>", nbr="q15"),
]
PN = [
    _t("pn_k16_32", "pn", 16, 3, 0, ((32, NM, False),), "pair_norm2_kernel<false, float>"),
    # 64 + 128 + 352 = 544: two equal passes of 320 threads; the keys' sums stay on chip for the joint [96 query | 352 key] GroupNorm
    _t("pn_k16_544_fin", "pn", 16, 3, 0, ((64, R, False), (128, NM, False), (352, ST, True)), "pair_norm2_kernel<false, float>", fin=96),
    _t("pn_k16_cluster", "pn", 16, 1, 0, ((64, NM, False), (32, ST, False)), "pair_norm2_kernel<false, float>", "cluster"),
    _t("pn_k8_32", "pn", 8, 3, 0, ((32, NM, False),), "pair_norm2_kernel<true, float>"),
    _t("pn_k8_2048_fin", "pn", 8, 1, 0, ((512, R, False), (512, NM, True), (1024, ST, True)), "pair_norm2_kernel<true, float>", fin=128),
    _t("pn_2080", "pn", 16, 1, 0, ((32, R, False),), "pair_norm2_kernel<false, float>", status=-3, ld_claim=2080),
]
COMP = [
    _t("comp_k16", "comp", 16, 3, 35, ((64, NM, False),), "gemm_gx_n64w_kernel<8, 3, 0>", N2=51),
    _t("comp_k8", "comp", 8, 3, 96, ((96, NM, False),), "gemm_gx_n64w_kernel<7, 3, 0>", N2=64, epi2=EPI_RAW),
]
CASES += PF + PN + COMP
CASE_BY_NAME.update({c["name"]: c for c in PF + PN + COMP})
KERNELS += ["pair_first_kernel<false>", "pair_first_kernel<true>", "pair_norm2_kernel<false, float>", "pair_norm2_kernel<true, float>"]


def table_mutants(c):
    if c["status"] != 0:
        return []
    m = []
    modes = {s[1] for s in c["segs"]}
    if NM in modes:
        m += ["unbiased_var", "shift_in_both_tables"]
        if c["K"] == 8:
            m += ["count_256_at_K8", "vv_unscaled"]
        if any(s[1] == NM and s[0] % min(32, s[0]) for s in c["segs"]):
            m.append("norm_tail_channels")
    if any(s[2] for s in c["segs"]):
        m.append("stats_ignore_pre_relu")
        if c["op"] == "pn" and c["K"] == 16:
            m.append("closed_form_under_relu")
    if c["fin"]:
        m.append("fin_group_of_neighbour")
    return m


def make_table_data(c):
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    B, C, K, dist = c["B"], c["C"], c["K"], c["dist"]
    nt, ncoord = B * 16, 9 + (2 if K == 8 else 0)
    sm = np.float32(1e-3 if dist == "small" else 1.0)
    d = dict(xyz=f(nt, 3))
    if dist == "cluster":  # a displaced cluster: a and b carry opposite common modes, a[q] + b[p] is small against either
        d["xyz"] = (3.0 + 0.1 * f(nt, 3) / np.sqrt(3.0)).astype(np.float32)
    if C:
        d["feat"] = f(nt, C) * sm + np.float32(30.0 if dist == "common" else 0.0)
    d["segs"] = []
    for (N, mode, _pre) in c["segs"]:
        # coordinate weights on a 2^-10 grid: rel + abs and ctr - rel are then exact in fp32 (the host folds them in fp32)
        wc = np.round(f(N, ncoord) * 1024.0) / 1024.0
        if dist == "cluster":  # first_mlp of a real block: the rel columns dominate, abs and ctr are small -> wa ~ -wb
            wc[:, 3:9] *= 1.0 / 64
        sg = dict(wc=wc.astype(np.float32) * (sm if dist != "cluster" else 1), gamma=1 + 0.2 * f(N), beta=0.2 * f(N))
        sg["wc"] = (np.round(sg["wc"].astype(np.float64) * 2.0 ** 20) / 2.0 ** 20).astype(np.float32)
        if C:
            sg["wf"], sg["bias"] = f(N, C) / np.float32(np.sqrt(C)) * (np.float32(1 / 30.0) if dist == "common" else 1), 0.5 * f(N) * sm
        else:
            sg["y"] = f(nt, N) * sm  # the float pass: y = Wf feat + bias is an fp32 INPUT
        d["segs"].append(sg)
    if K == 8:
        d["nbr"] = neighbour_table(rs, c["nbr"], d["xyz"]).reshape(-1)
        d["d2"] = rs.uniform(0, 4, (nt, 16)).astype(np.float32)  # random positive tables, NOT derived from the coordinates
        d["w"] = rs.uniform(0, 1, (nt, 16)).astype(np.float32)
        d["d2"][:, 8:], d["w"][:, 8:] = 6e4, 6e4
    if c["lead"]:
        d["lead_w"], d["lead_bias"] = f(c["lead"], C) / np.float32(np.sqrt(C)), 0.5 * f(c["lead"])
    if c["fin"]:
        Cq, Ck = c["fin"], c["segs"][-1][0]
        qv = np.maximum(f(B, 16, Cq), 0).astype(np.float64)
        d["qsum"], d["qsq"] = (K * qv.sum(1)).astype(np.float32), (K * (qv * qv).sum(1)).astype(np.float32)
        d["fin_gamma"], d["fin_beta"] = 1 + 0.2 * f(Cq + Ck), 0.2 * f(Cq + Ck)
    if c["op"] == "comp":
        c1, N2 = c["segs"][0][0], c["N2"]
        d["add"] = f(B, c1)
        d["W2"], d["bias2"], d["gamma2"], d["beta2"] = f(N2, c1) / np.float32(np.sqrt(c1)), 0.5 * f(N2), 1 + 0.2 * f(N2), 0.2 * f(N2)
    return d


def _store(c, ref, bnd):
    if c["prec"] == "fp16":
        return r16(ref), bnd * (1 + H) + H * np.abs(ref) + 2.0 ** -25
    return r32(ref), bnd + U * np.abs(ref)


def _norm_fin(S, SS, dS, dSS, inv, unbiased_n=None):
    """mean, var, rstd of sums and their bounds (dm, relative bound of rstd); asserts the first-order regime of the rstd bound"""
    m = S * inv
    var = np.maximum(SS * inv - m * m, 0)
    if unbiased_n:
        var = var * unbiased_n / (unbiased_n - 1)
    dm = dS * inv + 2 * U * np.abs(m)
    dvar = dSS * inv + 2 * np.abs(m) * dm + dm * dm + 3 * U * (SS * inv + m * m)
    x = dvar / (var + EPS)
    assert (x <= 0.3).all(), "the variance bound left the first-order regime of the rstd bound: %.3g" % x.max()
    return m, var, 1 / np.sqrt(var + EPS), dm, 0.6 * x + 4 * U


def table_forward(c, d, mutant=None):
    """float64 pair-form reference of a table pass (or of a mutant): {output name: (ref, stored, bound)}; the unrounded tables in "_ctx" """
    B, C, K = c["B"], c["C"], c["K"]
    pf = c["op"] != "pn"
    x = d["xyz"].astype(np.float64).reshape(B, 16, 3)
    outs, ctx = {}, []
    bi = np.arange(B)[:, None, None]
    if K == 8:
        nb = d["nbr"].reshape(B, 16, 16)[:, :, :8]
        d2, w = (d[k].astype(np.float64).reshape(B, 16, 16)[:, :, :8, None] for k in ("d2", "w"))
    csum_key = None
    for i, ((N, mode, pre), sg) in enumerate(zip(c["segs"], d["segs"])):
        wc = sg["wc"]
        wa = (wc[:, 0:3] + wc[:, 3:6]).astype(np.float32).astype(np.float64)  # the host's fp32 folding
        wb = (wc[:, 6:9] - wc[:, 0:3]).astype(np.float32).astype(np.float64)
        if pf:
            Xf, Wf = r16(d["feat"]), r16(sg["wf"])
            y = (Xf @ Wf.T + sg["bias"]).reshape(B, 16, N)
            by = (C_ACC * (np.abs(Xf) @ np.abs(Wf).T + np.abs(sg["bias"]))).reshape(B, 16, N)
        else:
            y, by = sg["y"].astype(np.float64).reshape(B, 16, N), 0.0
        pa_, pb_ = np.abs(x)[:, :, None, :] * np.abs(wa)[None, None], np.abs(x)[:, :, None, :] * np.abs(wb)[None, None]
        a, b = y + x @ wa.T, x @ wb.T
        da, db = by + 4 * U * (np.abs(y) + pa_.sum(-1)), 3 * U * pb_.sum(-1)
        vd = vw = None
        if K == 16:
            v = a[:, None, :, :] + b[:, :, None, :]
            dv = da[:, None] + db[:, :, None] + 5 * U * (np.abs(a)[:, None] + np.abs(b)[:, :, None])
        else:
            vd, vw = wc[:, 9].astype(np.float64), wc[:, 10].astype(np.float64)
            aq = a[bi, nb]
            v = aq + b[:, :, None, :] + d2 * vd + w * vw
            dv = da[bi, nb] + db[:, :, None] + 5 * U * (np.abs(aq) + np.abs(b)[:, :, None] + np.abs(d2 * vd) + np.abs(w * vw))
        if pre and mutant not in ("stats_ignore_pre_relu", "closed_form_under_relu"):
            v = np.maximum(v, 0)
        n = 16 * K
        s, ss = v.sum((1, 2)), (v * v).sum((1, 2))
        ds = dv.sum((1, 2)) + n * U * np.abs(v).sum((1, 2))
        dss = (2 * np.abs(v) * dv + dv * dv).sum((1, 2)) + n * U * ss
        noab = None
        if not pf and K == 16 and not pre:  # the closed form
            A, Bs, A2, B2 = a.sum(1), b.sum(1), (a * a).sum(1), (b * b).sum(1)
            dA, dB = da.sum(1) + 16 * U * np.abs(a).sum(1), db.sum(1) + 16 * U * np.abs(b).sum(1)
            dA2 = (2 * np.abs(a) * da + da * da).sum(1) + 16 * U * A2
            dB2 = (2 * np.abs(b) * db + db * db).sum(1) + 16 * U * B2
            ds = 16 * (dA + dB) + 2 * U * np.abs(s)
            noab = 16 * (dA2 + dB2) + 4 * U * ss  # (what a bound without the |A| |B| terms would say)
            dss = 16 * (dA2 + dB2) + 2 * (np.abs(A) * dB + np.abs(Bs) * dA + dA * dB) + 4 * U * (16 * (A2 + B2) + 2 * np.abs(A) * np.abs(Bs))
        g, sh, dg, dsh = np.ones((B, N)), np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N))
        if mode == ST:
            sc = 1.0  # (stats_scale of the keys; the per-point queries carry K)
            if c["fin"] and i == len(c["segs"]) - 1:
                csum_key = (s * sc, ss * sc, ds * sc + U * np.abs(s), dss * sc + U * ss)
            else:
                outs["sum%d" % i] = (s * sc,) + (r32(s * sc), ds * sc + U * np.abs(s))
                outs["sq%d" % i] = (ss * sc,) + (r32(ss * sc), dss * sc + U * ss)
        elif mode == NM:
            G_, n_norm, gs = gn_params(N)
            gsp = 1
            while gsp < gs:
                gsp *= 2
            lg = np.log2(gsp)
            grp = lambda t: t[:, :n_norm].reshape(B, G_, gs).sum(2)
            S, SS = grp(s), grp(ss)
            dS, dSS = grp(ds) + lg * U * grp(np.abs(s)), grp(dss) + lg * U * SS
            cnt = gs * (256 if mutant == "count_256_at_K8" else n)
            m, var, rstd, dm, rel = _norm_fin(S, SS, dS, dSS, 1.0 / cnt, cnt if mutant == "unbiased_var" else None)
            ch = np.repeat(np.arange(G_), gs)
            gam, bet = sg["gamma"][:n_norm].astype(np.float64), sg["beta"][:n_norm].astype(np.float64)
            g[:, :n_norm] = gam * rstd[:, ch]
            sh[:, :n_norm] = bet - m[:, ch] * g[:, :n_norm]
            dg[:, :n_norm] = np.abs(g[:, :n_norm]) * rel[:, ch]
            dsh[:, :n_norm] = (np.abs(m[:, ch]) * dg[:, :n_norm] + np.abs(g[:, :n_norm]) * dm[:, ch] +
                               3 * U * (np.abs(bet) + np.abs(m[:, ch] * g[:, :n_norm])))
            if mutant == "norm_tail_channels":  # (the packed gamma / beta of the tail channels are zero)
                g[:, n_norm:] = 0
        G3, S3 = g[:, None, :], sh[:, None, :]
        ta, tb = a * G3 + S3, b * G3 + (S3 if mutant == "shift_in_both_tables" else 0)
        dta = np.abs(G3) * da + np.abs(a) * dg[:, None] + dsh[:, None] + 2 * U * (np.abs(a * G3) + np.abs(S3))
        dtb = np.abs(G3) * db + np.abs(b) * dg[:, None] + U * np.abs(b * G3)
        for nm, t, dt in (("ta", ta, dta), ("tb", tb, dtb)):
            st, bd = _store(c, t.reshape(B * 16, N), dt.reshape(B * 16, N))
            outs["%s%d" % (nm, i)] = (t.reshape(B * 16, N), st, bd)
        if K == 8:
            gv = np.ones_like(g) if mutant == "vv_unscaled" else g
            vv = np.stack([vd * gv, vw * gv], 1)
            dvv = np.stack([np.abs(vd) * dg + 2 * U * np.abs(vd * g), np.abs(vw) * dg + 2 * U * np.abs(vw * g)], 1)
            outs["vv%d" % i] = (vv, r32(vv), dvv + 2.0 ** -149)
        ctx.append(dict(ta=ta, tb=tb, dta=outs["ta%d" % i][2], dtb=outs["tb%d" % i][2], g=g, dg=dg, vd=vd, vw=vw, ss=ss, dss=dss, noab=noab))
    if c["lead"]:
        gc = G._c(c["name"], "fp16", 4, B, C, c["lead"], EPI_STATS, c["kernel"], pre_relu=True, stats_scale=float(K))
        fl = G.forward(gc, dict(X=d["feat"], W=d["lead_w"], bias=d["lead_bias"], gamma=None, beta=None))
        outs["lead"] = (fl["y"], fl["stored"], fl["b"])
        outs["lead_sum"] = (fl["stats"][0], r32(fl["stats"][0]), fl["stats_b"][0])
        outs["lead_sq"] = (fl["stats"][1], r32(fl["stats"][1]), fl["stats_b"][1])
    if c["fin"]:
        Cq, Ck = c["fin"], c["segs"][-1][0]
        Cf = Cq + Ck
        gsf = Cf // 32
        cs = np.concatenate([d["qsum"].astype(np.float64), csum_key[0]], 1)
        cq = np.concatenate([d["qsq"].astype(np.float64), csum_key[1]], 1)
        dcs = np.concatenate([np.zeros((B, Cq)), csum_key[2]], 1)
        dcq = np.concatenate([np.zeros((B, Cq)), csum_key[3]], 1)
        grp = lambda t: t.reshape(B, 32, gsf).sum(2)
        S, SS = grp(cs), grp(cq)
        dS, dSS = grp(dcs) + gsf * U * grp(np.abs(cs)), grp(dcq) + gsf * U * SS
        m, var, rstd, dm, rel = _norm_fin(S, SS, dS, dSS, 1.0 / (gsf * 16 * K))
        gid = np.arange(Cf) // gsf
        if mutant == "fin_group_of_neighbour":
            gid = np.minimum((np.arange(Cf) + 1) // gsf, 31)
        gam, bet = d["fin_gamma"].astype(np.float64), d["fin_beta"].astype(np.float64)
        scl = gam * rstd[:, gid]
        sft = bet - m[:, gid] * scl
        dscl = np.abs(scl) * rel[:, gid]
        dsft = np.abs(m[:, gid]) * dscl + np.abs(scl) * dm[:, gid] + 3 * U * (np.abs(bet) + np.abs(m[:, gid] * scl))
        outs["fin_scale"] = (scl, r32(scl), dscl + U * np.abs(scl))
        outs["fin_shift"] = (sft, r32(sft), dsft + U * np.abs(sft))
    outs["_ctx"] = ctx
    return outs


# =================================================================================================================== composition
def expanded_input(c, d):
    """the K-expanded grouped input of a block's first layer [B][16][K][C + 9 (+ 2)]: [feat[q] | rel | abs | centre (| d2 | w)]"""
    B, K = c["B"], c["K"]
    x = d["xyz"].astype(np.float64).reshape(B, 16, 3)
    ft = r16(d["feat"]).reshape(B, 16, -1)
    bi = np.arange(B)[:, None, None]
    nb = d["nbr"].reshape(B, 16, 16)[:, :, :8] if K == 8 else np.broadcast_to(np.arange(16), (B, 16, 16))
    xq, xp = x[bi, nb], np.broadcast_to(x[:, :, None, :], (B, 16, K, 3))
    cols = [ft[bi, nb], xq - xp, xq, xp]
    if K == 8:
        cols += [d[k].astype(np.float64).reshape(B, 16, 16)[:, :, :8, None] for k in ("d2", "w")]
    return np.concatenate(cols, -1)


def comp_first_layer(c, d, expanded):
    """relu(GroupNorm(first layer)) + add of a composition case, float64, [B * 16 * K][c1]: K-expanded evaluation or the pair form"""
    B, K, sg = c["B"], c["K"], d["segs"][0]
    c1 = c["segs"][0][0]
    G_, n_norm, gs = gn_params(c1)
    assert n_norm == c1
    if expanded:
        Wfull = np.concatenate([r16(sg["wf"]), sg["wc"].astype(np.float64)], 1)
        z = expanded_input(c, d) @ Wfull.T + sg["bias"]
        zz = z.reshape(B, 16 * K, G_, gs)
        m = zz.mean((1, 3), keepdims=True)
        var = ((zz - m) ** 2).mean((1, 3), keepdims=True)
        hn = ((zz - m) / np.sqrt(var + EPS)).reshape(B, 16, K, c1) * sg["gamma"].astype(np.float64) + sg["beta"].astype(np.float64)
    else:
        t = table_forward(c, d)["_ctx"][0]
        bi = np.arange(B)[:, None, None]
        if K == 16:
            hn = t["ta"][:, None, :, :] + t["tb"][:, :, None, :]
        else:
            nb = d["nbr"].reshape(B, 16, 16)[:, :, :8]
            d2, w = (d[k].astype(np.float64).reshape(B, 16, 16)[:, :, :8, None] for k in ("d2", "w"))
            hn = t["ta"][bi, nb] + t["tb"][:, :, None, :] + d2 * (t["vd"] * t["g"])[:, None, None, :] + w * (t["vw"] * t["g"])[:, None, None, :]
    return (np.maximum(hn, 0) + d["add"].astype(np.float64)[:, None, None, :]).reshape(B * 16 * K, c1)


def comp_forward(c, d, mutant=None):
    """composition case: reference = the K-expanded float64 evaluation; bound = the consumer's, with the producer's table bounds as
    input uncertainty carried through the consumer's fp16 generation steps"""
    B, K = c["B"], c["K"]
    c1 = c["segs"][0][0]
    X = comp_first_layer(c, d, True)
    t = table_forward(c, d)["_ctx"][0]
    bi = np.arange(B)[:, None, None]
    ta, tb, eta, etb = t["ta"], t["tb"], t["dta"].reshape(B, 16, c1), t["dtb"].reshape(B, 16, c1)
    if K == 16:
        y = ta[:, None, :, :] + tb[:, :, None, :]
        e = (eta[:, None] + etb[:, :, None]) * (1 + H) + H * np.abs(y) + 2.0 ** -25
    else:
        nb = d["nbr"].reshape(B, 16, 16)[:, :, :8]
        d2, w = (d[k].astype(np.float64).reshape(B, 16, 16)[:, :, :8, None] for k in ("d2", "w"))
        y = ta[bi, nb] + tb[:, :, None, :]
        e = (eta[bi, nb] + etb[:, :, None]) * (1 + H) + H * np.abs(y) + 2.0 ** -25
        for s_, v_, dv_ in ((d2, t["vd"] * t["g"], np.abs(t["vd"]) * t["dg"]), (w, t["vw"] * t["g"], np.abs(t["vw"]) * t["dg"])):
            v3, dv3 = v_[:, None, None, :], (dv_ + 2 * U * np.abs(v_))[:, None, None, :]
            # the scalar and the coefficient each rounded to fp16 when staged, then one fp16 FMA
            e = (e + np.abs(s_) * (dv3 + H * np.abs(v3)) + H * np.abs(s_ * v3) * (1 + H)) * (1 + H)
            y = y + s_ * v3
            e = e + H * np.abs(y) + 2.0 ** -25
    add = d["add"].astype(np.float64)[:, None, None, :]
    xr = np.maximum(y, 0) + add
    e = (e + H * np.abs(add)) * (1 + H) + H * np.abs(xr) + 2.0 ** -25
    gc = G._c(c["name"], "fp16", c["npxl"], B, c1, c["N2"], c["epi2"], c["kernel"], post_relu=c["epi2"] == EPI_NORM)
    gd = dict(X=X, W=d["W2"], bias=d["bias2"], gamma=d["gamma2"], beta=d["beta2"])
    return G.forward(gc, gd, xb=e.reshape(B * 16 * K, c1))
