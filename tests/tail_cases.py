"""The case matrix of the attention tails (SLIDE_OP_ATTN_TAIL and the three-launch form ending in SLIDE_OP_ATTN_COMBINE), their float64
reference, error bound, CPU kernel model and mutants -- shared by tests/test_hip_attn_tail.py (every case on the GPU against the
reference; on the CPU every bound against the mutants and against the kernel model).

A case is ONE launch emitted by DenoiserEngine._attn_tail on a bare plan builder (three-launch cases: scores GEMM, then
DenoiserEngine._attn_combine = values GEMM + combine), so the host packing -- w5 scattered through the intermediate layer's PADDED
GroupNorm layout, wv zero-padded, _tail_vectors, chunk-major weights, the bits of f[1], _ldp -- is under test as well.

  S = u W5^T + b5                                      u [rows][k1]: the intermediate layer's output, logical width `inter`
  V = relu(GN(mo Wv^T + bv))                           mo [rows][k2], logical width k2l; MyGroupNorm(min(32, cout), cout), eps = EPS
  out[p] = sum_k softmax_k(S)[p, k] V[p, k]            over the point's K = 16 (npxl 8) or 8 (npxl 7) consecutive rows
Operands as the kernel reads them: fp16 cases round u, mo, W5, Wv to fp16 first; split cases take the fp32 values; all else is fp32.

branch of the product build's launchers                 | cases
  attn_tail_rx_kernel<8, true>  (fragment-major u / mo) | fm8_b1_c8, fm8_b9_c72, fm8_b1_c1024, fm8_b3_c40_pad, fm8_b3_c256_cm, fm8_b3_c128_out2
  attn_tail_rx_kernel<7, true>                          | fm7_b1_c8_flat, fm7_b3_c72, fm7_b3_c40_var0, fm7_b3_c512_out2, fm7_b3_c128_pad
  attn_tail_rx_kernel<8, false> (chunk- / row-major)    | cm8_b1_c32, cm8_b9_c40_cm, cm8_b3_c72_out2, cm8_b1_c8, rm8_b3_c256
  attn_tail_rx_kernel<7, false>                         | cm7_b3_c8, cm7_b1_c72_flat, cm7_b3_c512_out2, cm7_b3_c40_var0, rm7_b3_c128
  attn_tail_kernel<8>  (ring: k2 / 32 no multiple of 4) | ring8_cm_k1, ring8_cm_k2_cm, ring8_rm_k3, ring8_cm_k5_out2
  attn_tail_kernel<7>                                   | ring7_cm_k1, ring7_rm_k2_flat, ring7_cm_k3_out2, ring7_rm_k5
  attn_tail_split_kernel<8>                             | sp8_b1_c8, sp8_b9_c72, sp8_b1_c1024, sp8_b3_c40_out2, sp8_b3_c128_pad
  attn_tail_split_kernel<7>                             | sp7_b3_c8_flat, sp7_b1_c72, sp7_b3_c40_out2, sp7_b3_c256
  attn_combine_kernel<16 / 8, _Float16>                 | three16_f16 / three8_f16        (SLIDE_ATTN_TAIL=0 at plan time)
  attn_combine_kernel<16 / 8, float>                    | three16_w315 (|w| = 31.5: _split1_ok refuses the split tail) / three8_f32
  host-side refusals, no launch                         | st_fm_rows (-3), st_fm_no_cm (-3), st_k1 (-3), st_ring_n6 (-4)
The scores loop of the register-X form leaves after chunk j = (k1 / 32 - 1) mod 4 of a round: k1 / 32 = 1 .. 5 all occur (inter 8 / 32 ->
1, 40 / 64 -> 2, 72 -> 3, 96 (groups of 3 padded to 4: physical 128) / 128 -> 4, 136 / 100 (padded: 132) -> 5).  Ring form: k2 / 32 = 1, 2
(fewer chunks than the NST - 1 = 2 primed stages / exactly two), 3 (one more), 5 (the ring wraps).  B = 1, 3 (384 rows at npxl 7: half a
tile clamped), 9 at npxl 8 (a ninth row tile: tr wraps into the second grid round).  cout 8 / 32 / 40 / 72 / 128 / 256 / 512 / 1024 = every
unpermuted layout: gs 1 .. 32 (1024: the ds_swizzle step), n_norm < n_cob * 32 (8, 40, 72), odd n_cob (72, 8, 32).
The padding columns of u (the physical columns no logical channel maps to) and of mo (past k2l) hold +-3e4: only zero weights meet them.

BOUND, elementwise, against the UNROUNDED float64 result (u = 2^-24, H = 2^-11):
  contractions   bs = C_ACC As, bp = C_ACC Av with gemm_cases' A = |X| . |W|^T + |bias| (the bias add is one more term of the sum).
  GroupNorm      gemm_cases' NORM step over n = 2^npxl gs values: dm, dv, dr, b' as written there (rsq ~1 ulp: gemm_cases); channels past
                 n_norm keep bp; ReLU is 1-Lipschitz.  dv_k is the result.
  base-2 scores  t = fma(acc, L, bL), L = fp32(log2 e), bL = fl(b5 L): the product's rounding u |b5| L, the fma's u |s| L, both in base-2
                 units; 2^t has relative error ln 2 times that: u (|b5| + |s|) in natural units -- this scales with |s|, not with |s - max|.
                 L itself is off by DL = 0.22 u relative (1.44269502162933 against 1.44269504088896), which acts on the DIFFERENCE:
                 DL |s - max|.  The subtraction rounds once: u |s - max| (rows_cases' d_k).  v_exp_f32: 1 ulp = 2 u relative (the ISA
                 reference's "1ULP accuracy" for V_EXP_F32; the figure rows_cases takes for expf: E_EXP).
                 ds_k = bs_k + u (|b5| + |s_k|),   d_k = |s_k - max| (u + DL)
  soft-max       rows_cases' ATTN bound with W = sum_k w_k |v_k|:
                   b = (2 K + 8 + 2 E_EXP) u W + sum_k w_k |v_k| d_k + W sum_j w_j d_j          (its own roundings)
                     + R (sum_k w_k |v_k| ds_k + W sum_j w_j ds_j)                               (score uncertainty, first order)
                     + sum_k w_k dv_k                                                            (value uncertainty)
                 R = exp(2 max ds) covers the remainder of the first-order expansion (ds is 1e-3 at most in the fused cases).
  reciprocal     v_rcp_f32 in place of the division: 1 ulp (csrc/attn_tail_split.hip: "v_rcp instead of an IEEE division (1 ulp)") = 2 u |out|,
                 taken as 2 u W.  rows_cases' count already holds 3 u for 1 / l; both are kept.
  underflow      the max slot contributes e = 1 exactly, so den >= 1: a weight that underflows (or is flushed) costs at most 2^-126 |v|
                 absolute, nothing relative -- not a term.
  store          fp16: b (1 + H) + H |ref| + 2^-25;  float: b + u |ref|.
  three launches S and V are STORED between the launches: ds_k = store(bs_k + u |s|), dv_k = store(dv_k + 4 u |v|) with the store step
                 above; attn_combine_kernel uses expf and a true division: rows_cases' ATTN bound as it is (no base-2 terms, no rcp).
                 three8_f16 runs the combine launch ALONE on S and V as the reference stores them (ds = dv = 0): the product build's
                 run_gemm has no fp16 kernel for 128-row samples on stored inputs without an input affine (SLIDE_ST_EXPERIMENT).

KERNEL MODEL (model): the fused epilogue's steps in numpy float32 in the kernel's order -- bias add, per lane the two register-pair
chains over its 32 rows (sum and fma sum of squares), lane halves, the WPS wave partials in order, the gs ladder as a pairwise tree,
mean, var = max(ss inv - m^2, 0), g = gamma rsq, bt = beta - m g, fma(x, g, bt), fma(acc, L, b L), exp2 of the difference, the pair
chains of numerator and denominator per lane half, their sums, tot * rcp.  rsq / exp2 / rcp: float64 rounded to fp32; the accumulators:
the float64 contraction rounded to fp32.  The test asserts the model inside the bound for every case.

MUTANTS (MUTANT_DOC) are applied to the reference and rounded to the stored type; each must leave the bound in at least one element, or
EXEMPT names a case of the same kernel where it does.  A mutant that is the same computation on a case's inputs does not apply there
(flat: W5 = 0, every score mutant; a neighbouring sample at B = 1).  NON_MUTANTS stay INSIDE: drop_score_bias -- a per-channel score bias
is the same for all K slots of a point and cancels in the soft-max, only its rounding remains, which the bias50 cases bound;
ieee_division -- a true division in place of v_rcp (applied to the kernel model: the reference divides anyway)."""
import zlib

import numpy as np

from gemm_cases import C_ACC, EPS, U, gn_params, r16, r32, ru  # noqa: F401
from rows_cases import E_EXP, PREFILL  # noqa: F401

H = 2.0 ** -11
LOG2E = 1.4426950408889634
L32 = float(np.float32(LOG2E))
DL = abs(L32 - LOG2E) / LOG2E  # relative error of log2 e in fp32
BIG = 3e4  # padding columns of u / mo

MUTANT_DOC = {
    "half_softmax": "soft-max over the K / 2 rows of one lane half", "point_shift": "soft-max over rows k + K / 2 .., straddling two points",
    "k16_at_k8": "16-row groups at npxl 7", "tile_pooled_stats": "both samples of a 256-row tile pooled at npxl 7",
    "count_256_at_K8": "the 256-row inv_count at K = 8", "unbiased_var": "variance over n - 1", "gs_double": "groups of 2 gs lanes",
    "tail_normalised": "channel n_norm normalised (its gamma and beta are 0)", "stats_after_relu": "statistics of the rectified values",
    "no_value_relu": "values not rectified", "relu_before_affine": "relu(x) g + bt",
    "natural_exp": "exp of the base-2 scaled difference (log2 e applied twice)", "no_log2e": "exp2 of natural scores",
    "k_tail_scores": "last logical column of u ignored", "k_tail_values": "last logical column of mo ignored",
    "scores_values_swapped": "u and mo exchanged (k1 == k2)", "sample_vec": "GroupNorm statistics of the neighbouring sample",
    "row_clamp_leak": "the clamped rows of a half-empty tile counted in the last sample's statistics",
    "out2_all_channels": "out2 written for every channel", "drop_whi_xlo": "split: w_hi x_lo dropped", "drop_wlo_xhi": "split: w_lo x_hi dropped",
}
NON_MUTANTS = ("drop_score_bias", "ieee_division")

_KERNEL = {"rx_fm": "attn_tail_rx_kernel<%d, true>", "rx": "attn_tail_rx_kernel<%d, false>", "ring": "attn_tail_kernel<%d>",
           "split": "attn_tail_split_kernel<%d>"}


def _t(name, form, npxl, B, inter, k2l, cout, dist="normal", xlay="cm", prec=None, **kw):
    prec = prec or ("split" if form == "split" else "fp16")
    if form == "three":
        kernel = "attn_combine_kernel<%d, %s>" % (1 << (npxl - 4), "_Float16" if prec == "fp16" else "float")
    else:
        kernel = _KERNEL[form] % npxl
    c = dict(name=name, form=form, prec=prec, npxl=npxl, B=B, inter=inter, k2l=k2l, k2=ru(k2l), cout=cout, dist=dist, xlay=xlay,
             out_cm=False, out2=None, wmax=None, env={}, status=0, patch=None, combine_only=False, kernel=kernel)
    c.update(kw)
    if c["out_cm"]:
        c["env"] = dict(c["env"], SLIDE_CM_TABLES="1")
    return c


CM = dict(out_cm=True)
# name, form, log2 rows per sample, samples, logical width of u, logical width of mo, cout, distribution, layout of u / mo
FUSED16 = [
    _t("fm8_b1_c8", "rx_fm", 8, 1, 8, 128, 8, xlay="fm"),
    _t("fm8_b9_c72", "rx_fm", 8, 9, 40, 256, 72, xlay="fm"),
    _t("fm8_b1_c1024", "rx_fm", 8, 1, 72, 100, 1024, xlay="fm"),
    _t("fm8_b3_c40_pad", "rx_fm", 8, 3, 96, 128, 40, "peaked", xlay="fm"),
    _t("fm8_b3_c256_cm", "rx_fm", 8, 3, 136, 128, 256, "bias50", xlay="fm", **CM),
    _t("fm8_b3_c128_out2", "rx_fm", 8, 3, 128, 128, 128, "common", xlay="fm", out2=(50, 96)),
    _t("fm7_b1_c8_flat", "rx_fm", 7, 1, 40, 128, 8, "flat", xlay="fm"),
    _t("fm7_b3_c72", "rx_fm", 7, 3, 72, 256, 72, xlay="fm"),
    _t("fm7_b3_c40_var0", "rx_fm", 7, 3, 8, 128, 40, "var0", xlay="fm"),
    _t("fm7_b3_c512_out2", "rx_fm", 7, 3, 136, 128, 512, "common", xlay="fm", out2=(70, 80)),
    _t("fm7_b3_c128_pad", "rx_fm", 7, 3, 100, 128, 128, "bias50", xlay="fm"),
    _t("cm8_b1_c32", "rx", 8, 1, 128, 128, 32),
    _t("cm8_b9_c40_cm", "rx", 8, 9, 72, 256, 40, "bias50", **CM),
    _t("cm8_b3_c72_out2", "rx", 8, 3, 40, 128, 72, "peaked", out2=(33, 72)),
    _t("cm8_b1_c8", "rx", 8, 1, 136, 128, 8, "common"),
    _t("rm8_b3_c256", "rx", 8, 3, 96, 120, 256, xlay="rm"),
    _t("cm7_b3_c8", "rx", 7, 3, 8, 128, 8),
    _t("cm7_b1_c72_flat", "rx", 7, 1, 72, 256, 72, "flat"),
    _t("cm7_b3_c512_out2", "rx", 7, 3, 128, 128, 512, out2=(100, 104)),
    _t("cm7_b3_c40_var0", "rx", 7, 3, 136, 128, 40, "var0"),
    _t("rm7_b3_c128", "rx", 7, 3, 40, 128, 128, "common", xlay="rm"),
    _t("ring8_cm_k1", "ring", 8, 1, 32, 32, 8),
    _t("ring8_cm_k2_cm", "ring", 8, 3, 96, 64, 72, "peaked", **CM),
    _t("ring8_rm_k3", "ring", 8, 9, 32, 96, 40, "bias50", xlay="rm"),
    _t("ring8_cm_k5_out2", "ring", 8, 1, 128, 160, 256, "common", out2=(50, 64)),
    _t("ring7_cm_k1", "ring", 7, 3, 32, 32, 40),
    _t("ring7_rm_k2_flat", "ring", 7, 1, 8, 64, 8, "flat", xlay="rm"),
    _t("ring7_cm_k3_out2", "ring", 7, 3, 96, 90, 72, "var0", out2=(70, 80)),
    _t("ring7_rm_k5", "ring", 7, 3, 128, 160, 512, xlay="rm"),
]
SPLIT = [
    _t("sp8_b1_c8", "split", 8, 1, 32, 32, 8, xlay="rm", wmax=30.9),
    _t("sp8_b9_c72", "split", 8, 9, 72, 96, 72, "bias50", xlay="rm"),
    _t("sp8_b1_c1024", "split", 8, 1, 32, 32, 1024, xlay="rm"),
    _t("sp8_b3_c40_out2", "split", 8, 3, 136, 160, 40, "peaked", xlay="rm", out2=(33, 48)),
    _t("sp8_b3_c128_pad", "split", 8, 3, 96, 96, 128, "common", xlay="rm"),
    _t("sp7_b3_c8_flat", "split", 7, 3, 72, 32, 8, "flat", xlay="rm"),
    _t("sp7_b1_c72", "split", 7, 1, 32, 96, 72, xlay="rm", wmax=30.9),
    _t("sp7_b3_c40_out2", "split", 7, 3, 136, 150, 40, "var0", xlay="rm", out2=(9, 40)),
    _t("sp7_b3_c256", "split", 7, 3, 32, 32, 256, "common", xlay="rm"),
]
THREE = [
    _t("three16_f16", "three", 8, 3, 40, 64, 72, prec="fp16", env={"SLIDE_ATTN_TAIL": "0"}),
    # (the product build has no fp16 ring GEMM for 128-row samples on stored inputs without an input affine -- run_gemm returns
    #  SLIDE_ST_EXPERIMENT, asserted --, so this instantiation runs alone, on S and V as the reference stores them)
    _t("three8_f16", "three", 7, 3, 96, 128, 40, prec="fp16", env={"SLIDE_ATTN_TAIL": "0"}, combine_only=True),
    # |w| = 31.5 >= 31: DenoiserEngine._split1_ok refuses the single-accumulator split tail, the plan takes the three launches
    _t("three16_w315", "three", 8, 3, 32, 96, 40, prec="split", xlay="rm", wmax=31.5),
    _t("three8_f32", "three", 7, 3, 72, 32, 8, prec="split", xlay="rm", env={"SLIDE_TAIL_SPLIT": "0"}),
]
# host-side refusals (run_attn_tail returns before any launch): the op of a valid case with one field patched
STATUS = [
    _t("st_fm_rows", "rx_fm", 7, 1, 8, 128, 8, xlay="fm", status=-3, patch=("i", 0, 112), kernel="(none: status -3)"),
    _t("st_fm_no_cm", "rx_fm", 8, 1, 8, 128, 8, xlay="fm", status=-3, patch=("f", 1, 16.0), kernel="(none: status -3)"),
    _t("st_k1", "rx", 8, 1, 40, 128, 8, status=-3, patch=("i", 2, 40), kernel="(none: status -3)"),
    _t("st_ring_n6", "ring", 7, 1, 32, 32, 8, status=-4, patch=("i", 6, 6), kernel="(none: status -4)"),
]
CASES = FUSED16 + SPLIT + THREE + STATUS
CASE_BY_NAME = {c["name"]: c for c in CASES}
RUN = [c for c in CASES if c["status"] == 0]
KERNELS = ([k % n for k in _KERNEL.values() for n in (8, 7)] +
           ["attn_combine_kernel<%d, %s>" % (k, t) for k in (16, 8) for t in ("_Float16", "float")])

# (case, mutant) -> the case of the same kernel where that mutant IS visible
EXEMPT = {
    # n = 2^npxl gs >= 1024 values per group: n / (n - 1) moves V by <= 5e-4 of |y - m| rstd, at or below half an fp16 ulp of the output; the
    # common-mode cases carry the statistics' cancellation (900 x the variance) in their bound as well
    ("fm8_b1_c1024", "unbiased_var"): "fm8_b1_c8", ("fm8_b3_c256_cm", "unbiased_var"): "fm8_b1_c8",
    ("fm8_b3_c128_out2", "unbiased_var"): "fm8_b1_c8", ("fm7_b3_c512_out2", "unbiased_var"): "fm7_b1_c8_flat",
    ("cm8_b1_c8", "unbiased_var"): "cm8_b1_c32", ("rm7_b3_c128", "unbiased_var"): "cm7_b3_c8",
    ("ring8_cm_k5_out2", "unbiased_var"): "ring8_cm_k1", ("sp8_b3_c128_pad", "unbiased_var"): "sp8_b1_c8",
    ("sp7_b3_c256", "unbiased_var"): "sp7_b3_c8_flat",
    # a common mode of 30 in V's pre-activation: the fp32 statistics' share of the bound (4 (d + 2) u mean(y^2) / var) is above the
    # 2^-22 a dropped cross product moves a product by
    ("sp8_b3_c128_pad", "drop_whi_xlo"): "sp8_b1_c8", ("sp8_b3_c128_pad", "drop_wlo_xhi"): "sp8_b1_c8",
    ("sp7_b3_c256", "drop_whi_xlo"): "sp7_b3_c8_flat", ("sp7_b3_c256", "drop_wlo_xhi"): "sp7_b3_c8_flat",
}


def layout(C):
    """(physical index of every logical channel, padded physical width) of the intermediate layer's GroupNorm layout: engine.gn_layout"""
    from slide_amd.engine import gn_layout
    lay = gn_layout(C)
    return lay.index, ru(lay.width)


def dispatch(i, f1, tail_rx=True):
    """the kernel run_attn_tail / slide_launch_attn_tail_split (csrc/attn_tail.hip, csrc/attn_tail_split.hip) picks for an op's i[] and f[1] in
    the product build, or its status"""
    f1 = int(f1)
    rows, x1_ld, k1, x2_ld, k2, n_cob, npxl = i[:7]
    if f1 & 8:
        if k1 % 32 or k2 % 32 or x1_ld % 4 or x2_ld % 4:
            return -3
        return "attn_tail_split_kernel<%d>" % npxl if npxl in (7, 8) else -4
    if k1 % 32 or k2 % 32 or rows <= 0 or n_cob <= 0:
        return -3
    if tail_rx and npxl in (7, 8) and (k2 // 32) % 4 == 0:
        if f1 & 16:
            if x1_ld != 32 or x2_ld != 32 or rows % 32 or not f1 & 1:
                return -3
            return "attn_tail_rx_kernel<%d, true>" % npxl
        return "attn_tail_rx_kernel<%d, false>" % npxl
    if f1 & 16:
        return -3
    return "attn_tail_kernel<%d>" % npxl if npxl in (7, 8) else -4


def mutants(c):
    if c["status"] != 0:
        return []
    npxl, B, cout, flat = c["npxl"], c["B"], c["cout"], c["dist"] == "flat"
    G, n_norm, gs = gn_params(cout)
    m = ["half_softmax", "point_shift", "unbiased_var", "no_value_relu", "k_tail_values"]
    if c["dist"] != "common":  # (pre-activations of 30 +- 1 are all positive: the ReLU is the identity on them)
        m += ["stats_after_relu", "relu_before_affine"]
    if not flat:  # (W5 = 0: every score is the bias)
        m += ["natural_exp", "no_log2e", "k_tail_scores"]
    if npxl == 7:
        m += ["k16_at_k8", "count_256_at_K8"]
        if B > 1:
            m.append("tile_pooled_stats")
        if B % 2:
            m.append("row_clamp_leak")
    if G >= 2:
        m.append("gs_double")
    if cout > n_norm:
        m.append("tail_normalised")
    if c["inter"] == c["k2l"] and np.array_equal(layout(c["inter"])[0], np.arange(c["inter"])):
        m.append("scores_values_swapped")
    if B > 1:
        m.append("sample_vec")
    if c["out2"] is not None:
        m.append("out2_all_channels")
    if c["prec"] == "split" and c["form"] == "split":
        m += ["drop_whi_xlo", "drop_wlo_xhi"]
    return m


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_data(c):
    """the case's fp32 inputs in logical layouts -- deterministic per case name"""
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    rows, inter, k2l, cout, dist = c["B"] << c["npxl"], c["inter"], c["k2l"], c["cout"], c["dist"]
    G, n_norm, gs = gn_params(cout)
    d = dict(u=f(rows, inter), mo=f(rows, k2l), W5=f(cout, inter) / np.float32(np.sqrt(inter)), Wv=f(cout, k2l) / np.float32(np.sqrt(k2l)),
             b5=0.5 * f(cout), bv=0.5 * f(cout), gamma=1 + 0.2 * f(n_norm), beta=0.2 * f(n_norm))
    if dist == "common":  # the cancellation case of gemm_cases: pre-activation of mean 30, std 1
        d["bv"] = d["bv"] + np.float32(30.0)
    elif dist == "peaked":  # scores of +-60: one slot carries the weight, the rest underflow
        d["W5"] = d["W5"] * np.float32(20.0)
    elif dist == "flat":  # equal scores: weights exactly 1 / K
        d["W5"] = np.zeros_like(d["W5"])
    elif dist == "bias50":  # cancels in the soft-max, not in the fp32 rounding
        d["b5"] = d["b5"] + np.float32(50.0) * np.where(np.arange(cout) % 2, -1, 1).astype(np.float32)
    elif dist == "var0":  # group 0 of V constant over the sample: var = 0, rsq(eps)
        d["Wv"][:gs] = 0
        d["bv"][:gs] = d["bv"][0]
    if c["wmax"] is not None:
        for k in ("W5", "Wv"):
            i, j = rs.randint(d[k].size, size=2)
            d[k].flat[i], d[k].flat[j] = c["wmax"], -c["wmax"]
    return {k: v.astype(np.float32) for k, v in d.items()}


def physical(c, d):
    """u [rows][k1] and mo [rows][k2] as the kernel's buffers hold them: logical columns in place, +-BIG in every padding column"""
    idx, k1 = layout(c["inter"])
    rows = d["u"].shape[0]

    def alt(n):
        a = np.full((rows, n), BIG, np.float32)
        a[:, 1::2] *= -1
        return a
    u, mo = alt(k1), alt(c["k2"])
    u[:, idx] = d["u"]
    mo[:, :c["k2l"]] = d["mo"]
    return u, mo


# ------------------------------------------------------------------------------------------------------------------ reference
def _split(a):
    hi = r16(a)
    return hi, r16((a - hi) * 2048.0)


def _mm(X, W, mutant):
    if mutant in ("drop_whi_xlo", "drop_wlo_xhi"):
        xh, xl = _split(X)
        wh, wl = _split(W)
        return xh @ wh.T + (xh @ wl.T if mutant == "drop_whi_xlo" else xl @ wh.T) / 2048.0
    return X @ W.T


def _store(c, y, b):
    """(stored value, bound after the store) of the case's output type"""
    if c["prec"] == "fp16":
        return r16(y), b * (1 + H) + H * np.abs(y) + 2.0 ** -25
    return r32(y), b + U * np.abs(y)


def _groupnorm(c, d, P, bp, mutant):
    """V = relu(GN(P)) and its bound: gemm_cases' NORM step over n = 2^npxl gs"""
    B, npxl, cout = c["B"], c["npxl"], c["cout"]
    npx, rows = 1 << npxl, c["B"] << c["npxl"]
    G, n_norm, gs = gn_params(cout)
    n = npx * gs
    dd = np.ceil(np.log2(n)) + 2
    part = P[:, :n_norm].reshape(B, npx, G, gs)
    bq = bp[:, :n_norm].reshape(B, npx, G, gs)
    ax = (1, 3)
    m = part.mean(ax, keepdims=True)
    var = ((part - m) ** 2).mean(ax, keepdims=True)
    if mutant in ("tile_pooled_stats", "count_256_at_K8", "gs_double", "sample_vec", "row_clamp_leak", "stats_after_relu"):
        src = np.maximum(part, 0) if mutant == "stats_after_relu" else part
        s, q, cnt = src.sum(ax), (src * src).sum(ax), float(n)  # [B][G]
        if mutant == "tile_pooled_stats":
            for t in range(B // 2):
                s[2 * t:2 * t + 2], q[2 * t:2 * t + 2] = s[2 * t:2 * t + 2].sum(0), q[2 * t:2 * t + 2].sum(0)
        elif mutant == "count_256_at_K8":
            cnt = 2.0 * n
        elif mutant == "gs_double":
            s = np.repeat(s.reshape(B, G // 2, 2).sum(2), 2, axis=1)
            q = np.repeat(q.reshape(B, G // 2, 2).sum(2), 2, axis=1)
            cnt = 2.0 * n
        elif mutant == "sample_vec":
            s, q = np.roll(s, -1, 0), np.roll(q, -1, 0)
        elif mutant == "row_clamp_leak":
            last = src[B - 1, npx - 1]  # [G][gs]
            s[B - 1] += 128 * last.sum(1)
            q[B - 1] += 128 * (last * last).sum(1)
        m = (s / cnt)[:, None, :, None]
        var = np.maximum((q / cnt)[:, None, :, None] - m * m, 0)
    if mutant == "unbiased_var":
        var = var * n / (n - 1)
    rstd = 1 / np.sqrt(var + EPS)
    gam = d["gamma"].astype(np.float64).reshape(1, 1, G, gs)
    bet = d["beta"].astype(np.float64).reshape(1, 1, G, gs)
    x = np.maximum(part, 0) if mutant == "relu_before_affine" else part
    o = (x - m) * rstd * gam + bet
    dm = bq.mean(ax, keepdims=True) + (dd + 2) * U * np.abs(part).mean(ax, keepdims=True)
    dv = (2 * (np.abs(part - m) * bq).mean(ax, keepdims=True) + bq.mean(ax, keepdims=True) ** 2 +
          4 * (dd + 2) * U * (part * part).mean(ax, keepdims=True))
    dr = rstd * (0.6 * dv / (var + EPS) + 4 * U)
    g = gam * rstd
    bo = np.abs(gam) * rstd * (bq + dm) + np.abs(gam) * np.abs(part - m) * dr + 3 * U * (np.abs(part * g) + np.abs(m * g) + np.abs(bet))
    V, bV = P.copy(), bp.copy()
    V[:, :n_norm], bV[:, :n_norm] = o.reshape(rows, n_norm), bo.reshape(rows, n_norm)
    if mutant == "tail_normalised":
        V[:, n_norm] = 0
    if mutant != "no_value_relu":
        V = np.maximum(V, 0)
    return V, bV


def _groups(c, mutant):
    """[points][rows of the soft-max group] row indices"""
    K, rows = 1 << (c["npxl"] - 4), c["B"] << c["npxl"]
    p = np.arange(rows // K)[:, None]
    if mutant == "half_softmax":
        return p * K + np.array([0, 1, 2, 3, 8, 9, 10, 11][:K // 2])[None]
    if mutant == "point_shift":
        return (p * K + K // 2 + np.arange(K)[None]) % rows
    if mutant == "k16_at_k8":
        return (p // 2) * 16 + np.arange(16)[None]
    return p * K + np.arange(K)[None]


def _scores_values(c, d, mutant=None):
    """float64 S and V [rows][cout] of the case (or of a mutant) with their elementwise uncertainties where the soft-max step reads them"""
    h = c["prec"] == "fp16"
    q = r16 if h else (lambda a: np.asarray(a, np.float64))
    u, mo, W5, Wv = q(d["u"]), q(d["mo"]), q(d["W5"]), q(d["Wv"])
    b5, bv = d["b5"].astype(np.float64), d["bv"].astype(np.float64)
    if mutant == "scores_values_swapped":
        u, mo = mo, u
    us, mv = u, mo
    if mutant == "k_tail_scores":
        us = u.copy()
        us[:, -1] = 0
    if mutant == "k_tail_values":
        mv = mo.copy()
        mv[:, -1] = 0
    S = _mm(us, W5, mutant) + (0 if mutant == "drop_score_bias" else b5)
    P = _mm(mv, Wv, mutant) + bv
    bs = C_ACC * (np.abs(u) @ np.abs(W5).T + np.abs(b5))
    bp = C_ACC * (np.abs(mo) @ np.abs(Wv).T + np.abs(bv))
    V, bV = _groupnorm(c, d, P, bp, mutant)
    if c["combine_only"]:  # the combine launch alone, on S and V as the reference stores them: exact inputs
        S, V = _store(c, S, 0)[0], _store(c, V, 0)[0]
        return S, V, np.zeros_like(S), np.zeros_like(V)
    if c["form"] == "three":  # S and V are stored between the launches
        return S, V, _store(c, S, bs + U * np.abs(S))[1], _store(c, V, bV + 4 * U * np.abs(V))[1]
    return S, V, bs + U * (np.abs(b5) + np.abs(S)), bV


def forward(c, d, mutant=None):
    """float64 reference of the case (or of one of its mutants): dict(y = unrounded output [points][cout], stored = y rounded to the
    stored type, b = elementwise bound against y)"""
    K = 1 << (c["npxl"] - 4)
    S, V, ds, bV = _scores_values(c, d, mutant)
    cd, rcp = (U, 0.0) if c["form"] == "three" else (U + DL, 2.0)
    idx = _groups(c, mutant)
    Sg, Vg, dsg, dvg = S[idx], V[idx], ds[idx], bV[idx]  # [points][K][cout]
    mx = Sg.max(1, keepdims=True)
    diff = Sg - mx
    e = np.exp(diff * LOG2E) if mutant == "natural_exp" else np.exp2(diff) if mutant == "no_log2e" else np.exp(diff)
    w = e / e.sum(1, keepdims=True)
    y = (w * Vg).sum(1)
    av = w * np.abs(Vg)
    W = av.sum(1)
    dk = np.abs(diff) * cd
    R = np.exp(2 * ds.max())
    b = ((2 * K + 8 + 2 * E_EXP + rcp) * U * W + (av * dk).sum(1) + W * (w * dk).sum(1) +
         R * ((av * dsg).sum(1) + W * (w * dsg).sum(1)) + (w * dvg).sum(1))
    stored, b = _store(c, y, b)
    return dict(y=y, stored=stored, b=b)


def second_stores(c, stored, mutant=None):
    """what the optional stores must hold, from the values `stored` [points][n_cob * 32] that went to out: out_cm [n_cob][points][32]
    (None without one), out2 [points][out2_ld] with the prefill everywhere but in the first out2_n columns (None without one)"""
    pts, Cp = stored.shape
    ocm = np.ascontiguousarray(stored.reshape(pts, Cp // 32, 32).transpose(1, 0, 2)) if c["out_cm"] else None
    o2 = None
    if c["out2"] is not None:
        n2, ld2 = c["out2"]
        o2 = np.full((pts, ld2), PREFILL)
        n = min(Cp, ld2) if mutant == "out2_all_channels" else n2
        o2[:, :n] = stored[:, :n]
    return ocm, o2


# ------------------------------------------------------------------------------------------------------------------ kernel model
def _f(a):
    return np.asarray(a, np.float32)


def _fma(a, b, c_):
    return _f(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c_, np.float64))


def _chain(x, sq=False):
    """sequential fp32 sum over axis 1 (sq: fma sum of squares) in two interleaved chains (even / odd registers), then their sum"""
    acc = [np.zeros(x.shape[:1] + x.shape[2:], np.float32), np.zeros(x.shape[:1] + x.shape[2:], np.float32)]
    for j in range(x.shape[1]):
        acc[j & 1] = _fma(x[:, j], x[:, j], acc[j & 1]) if sq else acc[j & 1] + x[:, j]
    return acc[0] + acc[1]


def _wave_rows(half):
    """the 32 rows of a 64-row wave a lane of `half` holds, in register order (reg r of block rb: row 32 rb + (r & 3) + 8 (r >> 2) + 4 half)"""
    r = np.arange(16)
    return np.concatenate([32 * rb + (r & 3) + 8 * (r >> 2) + 4 * half for rb in (0, 1)])


def _point_rows(K, half):
    """the K / 2 rows of a point a lane of `half` holds, in register order"""
    qq = np.arange(K // 2)
    return (qq & 3) + 8 * (qq >> 2) + 4 * half


def model(c, d, variant=None):
    """the kernel's arithmetic in float32 steps (module docstring); returns the value as stored, [points][cout] float64"""
    h = c["prec"] == "fp16"
    B, npxl, cout = c["B"], c["npxl"], c["cout"]
    K, npx, rows = 1 << (npxl - 4), 1 << npxl, B << npxl
    G, n_norm, gs = gn_params(cout)
    q = r16 if h else (lambda a: np.asarray(a, np.float64))
    sacc = _f(q(d["u"]) @ q(d["W5"]).T)
    vacc = _f(q(d["mo"]) @ q(d["Wv"]).T)
    gam, bet = np.ones(cout, np.float32), np.zeros(cout, np.float32)
    gam[:n_norm], bet[:n_norm] = d["gamma"], d["beta"]
    st = (lambda a: r16(a)) if h else (lambda a: r32(a))
    if c["combine_only"]:
        S, V = (_f(a) for a in _scores_values(c, d)[:2])
    elif c["form"] == "three":
        S = _f(st(sacc + d["b5"]))
        x = vacc + d["bv"]
        part = x[:, :n_norm].astype(np.float64).reshape(B, npx, G, gs)
        m = part.mean((1, 3), keepdims=True)
        var = ((part - m) ** 2).mean((1, 3), keepdims=True)
        o = x.astype(np.float64)
        o[:, :n_norm] = ((part - m) / np.sqrt(var + EPS) * gam[:n_norm].reshape(1, 1, G, gs) + bet[:n_norm].reshape(1, 1, G, gs)).reshape(rows, n_norm)
        V = _f(st(_f(np.maximum(o, 0))))
    if c["form"] == "three":
        Sg, Vg = S.reshape(-1, K, cout), V.reshape(-1, K, cout)
        e = _f(np.exp((Sg - Sg.max(1, keepdims=True)).astype(np.float64)))
        den = np.zeros_like(e[:, 0])
        for k in range(K):
            den = den + e[:, k]
        inv = np.float32(1) / den
        o = np.zeros_like(den)
        for k in range(K):
            o = o + Vg[:, k] * (e[:, k] * inv)
        return st(o)
    L = np.float32(LOG2E)
    x = vacc + d["bv"]
    xw = x.reshape(-1, 64, cout)
    s = _chain(xw[:, _wave_rows(0)]) + _chain(xw[:, _wave_rows(1)])
    ss = _chain(xw[:, _wave_rows(0)], True) + _chain(xw[:, _wave_rows(1)], True)
    WPS = npx // 64
    s, ss = s.reshape(B, WPS, cout), ss.reshape(B, WPS, cout)
    ts, tss = np.zeros((B, cout), np.float32), np.zeros((B, cout), np.float32)
    for w_ in range(WPS):
        ts, tss = ts + s[:, w_], tss + ss[:, w_]
    gsum, gsq = ts[:, :n_norm].reshape(B, G, gs), tss[:, :n_norm].reshape(B, G, gs)
    while gsum.shape[2] > 1:  # the DPP / swizzle ladder: partners 1, 2, 4, .. lanes apart
        gsum, gsq = gsum[:, :, 0::2] + gsum[:, :, 1::2], gsq[:, :, 0::2] + gsq[:, :, 1::2]
    inv = np.float32(1.0 / (gs * npx))
    mean = gsum[:, :, 0] * inv
    var = np.maximum(gsq[:, :, 0] * inv - mean * mean, np.float32(0))
    rsq = _f(1 / np.sqrt((var + np.float32(EPS)).astype(np.float64)))
    g, bt = np.ones((B, cout), np.float32), np.zeros((B, cout), np.float32)
    g[:, :n_norm] = gam[None, :n_norm] * np.repeat(rsq, gs, axis=1)
    bt[:, :n_norm] = _fma(-np.repeat(mean, gs, axis=1), g[:, :n_norm], bet[None, :n_norm])
    smp = np.arange(rows) >> npxl
    vv = np.maximum(_fma(x, g[smp], bt[smp]), np.float32(0))
    bsl = np.zeros(cout, np.float32) if variant == "drop_score_bias" else d["b5"] * L
    sc = _fma(sacc, L, bsl)
    scg, vg = sc.reshape(-1, K, cout), vv.reshape(-1, K, cout)
    dd = scg - scg.max(1, keepdims=True)
    e = _f(np.exp2(dd.astype(np.float64)))
    num = den = None
    for half in (0, 1):
        rws = _point_rows(K, half)
        acc_d = [np.zeros_like(e[:, 0]), np.zeros_like(e[:, 0])]
        acc_n = [np.zeros_like(e[:, 0]), np.zeros_like(e[:, 0])]
        for j, r_ in enumerate(rws):
            acc_d[j & 1] = acc_d[j & 1] + e[:, r_]
            acc_n[j & 1] = _fma(e[:, r_], vg[:, r_], acc_n[j & 1])
        dh, nh = acc_d[0] + acc_d[1], acc_n[0] + acc_n[1]
        num, den = (nh, dh) if num is None else (num + nh, den + dh)
    if variant == "ieee_division":
        o = _f(num.astype(np.float64) / den.astype(np.float64))
    else:
        o = num * _f(1 / den.astype(np.float64))
    return st(o)
