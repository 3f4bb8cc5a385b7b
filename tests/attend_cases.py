"""The SLIDE_OP_GEMM_ATTEND case matrix, its float64 reference, its error bound and its mutants -- shared by
tests/test_attend_host.py (the table, the bound against the mutants: CPU) and tests/test_hip_attend.py (every case on the GPU).
The companion of tests/gemm_cases.py (SLIDE_OP_GEMM) and tests/rows_cases.py (SLIDE_OP_ROWS_ATTN) for their FUSION:
`gemm_attend_kernel<AFF>` (csrc/gemm_ring.hip) with `attend_epilogue` (csrc/gemm_common.h), launcher `run_gemm_attend` -- the score
convolution of an AttentionModule, the soft-max over the K neighbour rows of a point and the weighted sum of the value rows in one
launch, hand-built SlideOps through slide_run_ops, no module involved.

Reference, float64, on the operands as the kernel reads them: X, W, V rounded to fp16; bias and the vss table fp32; counts int32.
  input affine (AFF = true)   sample of a row = (row >> 8) / tps.  gemm_cases.py's fp16 model: scale, shift, add rounded to fp16,
                              X' = fp16(X scale + shift) is ONE rounding (v_pk_fma_f16); with the deferred step
                              X' = fp16(max(X', 0)? + fp16(add)), add on the columns < add_n only
  scores                      s = X' W^T + bias, NOT rounded: the point of the fusion
  slots                       n = clamp(count, 1, K) (rows_cases._slots), w = softmax(s[:n])
  values                      v' = relu?(v vs + vh) with the vss row of sample pt / pps
  out                         sum_k w_k v'_k, stored fp16; 0 for the channels [C, n_cob * 32)

Bound, elementwise (u = 2^-24).  A bound of 0 marks an element that must be EXACT.
  score     |s^ - s| <= sig = C_ACC A,  A = |X'| |W|^T + |bias|: gemm_cases.py's RAW bound (fp16 products are exact in fp32, the fp32
            accumulation and the bias addition are what it counts).
  weights   the kernel forms e_k = __expf(s^_k - m^), m^ = max_k s^_k, l = sum e_k, out = (sum e_k v'_k) / l.  A common shift of the
            exponents cancels in the quotient, so against e_k = exp(s_k - m) every e^_k carries the RELATIVE error
              eps_k = expm1(sig_k)              the score uncertainty (not linearised: sig reaches 1e-2 at scores of +-100)
                    + d_k u                     the subtraction, d_k = |s_k - m|      (rows_cases.py's d_k u)
                    + (2 + 2 d_k) u             __expf, DERIVED from its definition in the toolchain's __clang_hip_math.h,
                                                __expf(x) = exp2(0x1.715476p+0f * x) on v_exp_f32: the constant is log2(e) to
                                                0.23 u and the product rounds once, so the argument t = x log2(e) is off by
                                                <= 1.23 u |t| and 2^t by ln 2 * 1.23 u |t| = 1.23 u |x| -- taken as 2 u |x|; the
                                                instruction itself is 1 ulp = 2 u (ISA manual).  It grows with |s_k - max|, which
                                                the 1-ulp expf that rows_cases.py cites does not.  (v_exp_f32 flushes results below
                                                2^-126: an ABSOLUTE error of 2^-126 next to l >= 1, far inside the store's 2^-25.)
            in the numerator and, weighted, in l -- the places of rows_cases.py's d_k u term:
              b_w = (sum_k w_k |v'_k| eps_k + W sum_j w_j eps_j) / (1 - sum_j w_j eps_j),       W = sum_k w_k |v'_k|
  sums      rows_cases.py's accumulation terms: (2 K + 8) u W (l's additions, the fmas into the numerator, the division), and
            2 u sum_k w_k (|v vs| + |vh|) for the deferred values.
  store     rows_cases.store: b (1 + 2^-11) + 2^-11 |ref| + 2^-25; pad channels [C, n_cob * 32): 0, exact.
  probes    "w0": W = 0, every score IS the bias (0 + bias, exact), e_k = exp2(0) = 1 exactly, l = n exactly: the output is the
            fp32 mean of the n counted values -- n - 1 additions and one division, b = K u mean|v|, i.e. the correctly rounded
            fp16 mean to within K 2^-13 of an fp16 ulp (a tie may fall either way): half an ulp of the store decides.
            "onehot": one slot at +100, the others at -100 (products of fp16 powers of two and 100: exact), bias 0: e = 1 for the
            top slot and exp2(-288.5) = 0 for the others, l = 1, the numerator is v_top + 0: b = 0, the output IS fp16 v_top.

Mutants (tests/test_attend_host.py::test_bounds_see_the_mutants), applied to the float64 reference and rounded to fp16:
  scores_fp16 (the two-launch form's arithmetic) | k_tail | affine_sample (tps 1: the next sample's scale / shift; tps 2: the
  sample of row0 >> 8 without / tps) | add_all_columns | aff_relu_dropped | slot_past_count | zero_count_empty |
  count_unclamped_high (K + 5 read as K + 5 slots, into the next point) | no_max_shift (in fp32) |
  vss_sample_of_tile | v_relu_dropped | pad_channels_not_zeroed
`mutants(c)` lists those a case can express; one below a case's resolution is in EXEMPT with the case that shows it.
INEXPRESSIBLE: "bias_block0" (every channel block takes the first block's bias).  The bias of this convolution is one number per
CHANNEL, added to all K scores of a (point, channel): it cancels in softmax(s + bias 1) = softmax(s), so NO data can show a wrong
bias -- it only changes which way s^ = fl(acc + bias) rounds, u |s| inside sig.  forward() still takes the mutant and
test_attend_host.py::test_a_wrong_bias_cancels_in_the_soft_max pins that it stays inside every case's bound (with distinct
per-channel biases, as asked); what a wrong block index does break -- V, vss, the pad mask and the output column -- is per-channel
data here and is seen by every n_cob >= 2 case."""
import zlib

import numpy as np

from gemm_cases import C_ACC, r16
from rows_cases import _slots, ratio, store  # noqa: F401  (ratio is re-exported to the test modules)
from slide_amd.abi import ru  # noqa: F401

U = 2.0 ** -24
TM = 256
MASKED_V = 6e4  # value rows of the slots past a point's count: finite, so that any weight but exactly 0 leaves a trace


def _c(name, K, rows, kl, k_pad, n_cob, C, **kw):
    c = dict(name=name, K=K, rows=rows, kl=kl, k_pad=k_pad, n_cob=n_cob, C=C, x_ld=k_pad, ldv=n_cob * 32, ldo=n_cob * 32, counts=False,
             vss=None, pps=rows // K, aff=False, tps=1, add_n=0, aff_relu=False, dist="normal", packed=True)
    c.update(kw)
    assert rows % K == 0 and kl <= k_pad <= c["x_ld"] and C <= n_cob * 32 <= min(c["ldv"], c["ldo"]) and c["add_n"] <= kl
    assert c["x_ld"] != 32 or k_pad == 32  # (x_ld == 32 means CHUNK-major X to the ring kernels)
    return c


# name, K, rows, logical input columns, k_pad, n_cob, logical channels
CASES = [
    # K, one tile each; n_cob 1 / 2 / 3 (C < n_cob * 32: pad channels); k_pad 32 (the ring is only primed) / 64 / 96 (odd chunk count)
    _c("k4_counts", 4, 256, 40, 64, 2, 51, counts=True, x_ld=96, ldv=96, ldo=128),
    _c("k8_ncob1", 8, 256, 64, 64, 1, 20, ldv=64, ldo=32, packed=False),
    _c("k16_ncob3_vss_relu", 16, 512, 90, 96, 3, 70, counts=True, vss="relu", pps=4, x_ld=128, ldv=128, ldo=128),
    _c("k32_kp32_vss", 32, 256, 30, 32, 2, 64, vss="plain", pps=2),
    # row tiles: 2 (above), 9 (the XCD map wraps, 7 workgroups per column tile exit idle), ragged; a value-sample over two tiles
    _c("t9_vss_pps512", 8, 2304, 50, 64, 3, 70, counts=True, vss="plain", pps=64, ldv=128, packed=False),
    _c("ragged_k32", 32, 256 + 32, 64, 64, 2, 51, counts=True, vss="relu", pps=3),
    # the widest input the module sends, with and without the affine
    _c("kp1536_t9", 16, 2304, 1530, 1536, 3, 70, x_ld=1568),
    _c("kp1536_aff", 16, 768, 1530, 1536, 2, 51, aff=True, counts=True),
    # the input affine: tiles per sample 1 / 2 over 3 samples; add + ReLU, add alone, ReLU alone, plain on a common mode
    _c("aff_tps1_add_relu", 8, 768, 60, 64, 2, 51, aff=True, add_n=40, aff_relu=True, vss="relu", pps=8),
    _c("aff_tps2_add", 4, 1536, 90, 96, 3, 70, aff=True, tps=2, add_n=64, counts=True, packed=False),
    _c("aff_relu_noadd", 32, 768, 64, 64, 1, 32, aff=True, aff_relu=True, counts=True, vss="plain", pps=8),
    _c("aff_common", 16, 768, 96, 96, 2, 64, aff=True, dist="common"),
    # score spread
    _c("pm100", 16, 256, 64, 64, 2, 51, dist="pm100"),
    _c("ties8", 8, 256, 64, 64, 2, 51, dist="ties8", counts=True),
    # exact probes
    _c("w0_mean", 16, 256, 64, 64, 2, 51, dist="w0", counts=True),
    _c("onehot", 32, 256, 32, 32, 2, 64, dist="onehot"),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# (case, mutant) -> the case where that mutant IS visible
EXEMPT = {}
# mutants no case can express, with the reason (module docstring)
INEXPRESSIBLE = {"bias_block0": "a per-channel constant added to all K scores cancels in the soft-max"}


def n_vss(c):
    """rows of the vss table: the samples pt / pps reaches"""
    return (c["rows"] // c["K"] + c["pps"] - 1) // c["pps"]


def n_smp(c):
    return c["rows"] // (TM * c["tps"])


def mutants(c):
    if c["dist"] == "onehot":  # (scores of exactly +-100, no bias, no pad channel: nothing below applies but the shift)
        return ["no_max_shift"]
    m = [] if c["dist"] == "w0" else ["scores_fp16", "k_tail"]
    if c["aff"]:
        m.append("affine_sample")
        if c["add_n"]:
            m.append("add_all_columns")
        if c["aff_relu"]:
            m.append("aff_relu_dropped")
    if c["counts"]:
        m += ["slot_past_count", "zero_count_empty", "count_unclamped_high"]
    if c["dist"] == "pm100":
        m.append("no_max_shift")
    if c["vss"]:
        if c["pps"] * c["K"] != TM:  # (a value-sample of exactly one tile: the tile index IS the sample)
            m.append("vss_sample_of_tile")
        if c["vss"] == "relu":
            m.append("v_relu_dropped")
    if c["C"] < c["n_cob"] * 32:
        m.append("pad_channels_not_zeroed")
    return m


def reach(c):
    """the launcher's and the kernel's branch values of a case (run_gemm_attend, gemm_attend_kernel, attend_epilogue)"""
    ntr = (c["rows"] + TM - 1) // TM
    ntc = (c["n_cob"] + 1) // 2
    aff_form = None
    if c["aff"]:
        aff_form = ("add_relu" if c["add_n"] and c["aff_relu"] else "add" if c["add_n"] else "relu" if c["aff_relu"] else
                    "common" if c["dist"] == "common" else "plain")
    return dict(AFF=c["aff"], K=c["K"], n_cob=c["n_cob"], k_pad=c["k_pad"], tiles=ntr, ragged=c["rows"] % TM != 0, counts=c["counts"],
                vss=c["vss"], vss_span=c["pps"] * c["K"] if c["vss"] else 0, tps=c["tps"] if c["aff"] else 0,
                samples=n_smp(c) if c["aff"] else 0, aff_form=aff_form, add_short=bool(c["add_n"]) and c["add_n"] < c["k_pad"],
                dist=c["dist"], grid=(ntr + 7) // 8 * 8 * ntc, idle=((ntr + 7) // 8 * 8 - ntr) * ntc, half_tile=c["n_cob"] % 2 == 1,
                pad_channels=c["C"] < c["n_cob"] * 32, x_gap=c["x_ld"] > c["k_pad"], v_gap=c["ldv"] > c["n_cob"] * 32,
                o_gap=c["ldo"] > c["n_cob"] * 32, packed=c["packed"])


# ------------------------------------------------------------------------------------------------------------------ data
def make_counts(rs, pts, K):
    """int32 counts with 0, 1, K, K + 5 and -3 among them"""
    cnt = rs.randint(0, K + 3, pts).astype(np.int32)
    cnt[:5] = (0, 1, K, K + 5, -3)
    return cnt


def make_data(c):
    """the case's fp32 / int inputs in LOGICAL layouts (physical ones: `physical`) -- deterministic per case name"""
    rs = np.random.RandomState(zlib.crc32(("attend_" + c["name"]).encode()) & 0x7fffffff)
    K, rows, kl, C, n_cob, dist = c["K"], c["rows"], c["kl"], c["C"], c["n_cob"], c["dist"]
    pts, nch = rows // K, n_cob * 32
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    X = f(rows, kl)
    W = f(C, kl) / np.float32(np.sqrt(kl))
    bias = 0.5 * f(nch)  # (distinct per channel, also past C)
    if dist == "common":
        X = X + np.float32(30.0)
    elif dist == "pm100":  # scores of standard deviation ~35: the top slots of most (point, channel)s pass +-88.7
        W = W * np.float32(35.0)
    elif dist == "ties8":  # every slot within a few 1e-2 of 8: fp16 spaces scores there by 2^-7 = 0.0078
        W = W * np.float32(0.02)
        bias = (8.0 + 0.25 * f(nch)).astype(np.float32)
    elif dist == "w0":
        W = np.zeros_like(W)
    elif dist == "onehot":  # X row (p, k) = unit vector (k + p) % K, W[c][j] = +100 for ONE j per channel, else -100
        assert kl == K
        X = np.zeros((rows, kl), np.float32)
        r = np.arange(rows)
        X[r, (r % K + r // K) % K] = 1.0
        W = np.full((C, kl), -100.0, np.float32)
        W[np.arange(C), rs.randint(0, K, C)] = 100.0
        bias = np.zeros(nch, np.float32)
    V = f(rows, nch)  # (finite also in the pad channels [C, nch): a kernel that stores them is seen)
    d = dict(X=X.astype(np.float32), W=W.astype(np.float32), bias=bias.astype(np.float32))
    if c["counts"]:
        d["counts"] = make_counts(rs, pts, K)
        masked = (np.arange(K)[None] >= np.clip(d["counts"], 1, K)[:, None]).reshape(-1)
        V[masked] = MASKED_V
    d["V"] = V
    if c["vss"]:
        nv = n_vss(c)
        d["vss"] = np.stack([rs.uniform(0.5, 1.5, (nv, nch)), 0.5 * rs.standard_normal((nv, nch))], 1).astype(np.float32)
    if c["aff"]:
        B = n_smp(c)
        d["scale"] = rs.uniform(0.5, 1.5, (B, kl)).astype(np.float32)
        d["shift"] = (0.5 * f(B, kl)).astype(np.float32)
        if dist == "common":
            d["shift"] = (d["shift"] - np.float32(30.0) * d["scale"]).astype(np.float32)
        if c["add_n"]:
            d["add"] = f(B, kl)  # (all kl columns hold values: the kernel may use the first add_n only)
    return d


def physical(c, d):
    """the arrays of the launch as they lie in memory.  X pad columns [kl, k_pad) and W's pad rows / columns are zero; what the kernel must
    NOT read is NaN: X beyond k_pad, V and vss beyond n_cob * 32.  X, W, V fp16; the rest fp32 / int32."""
    K, rows, kl, kp, C, n_cob = c["K"], c["rows"], c["kl"], c["k_pad"], c["C"], c["n_cob"]
    nch = n_cob * 32
    p = {}
    X = np.full((rows, c["x_ld"]), np.nan, np.float32)
    X[:, :kp] = 0
    X[:, :kl] = d["X"]
    W = np.zeros((nch, kp), np.float32)
    W[:C, :kl] = d["W"]
    V = np.full((rows, c["ldv"]), np.nan, np.float32)
    V[:, :nch] = d["V"]
    p["X"], p["W"], p["V"] = X.astype(np.float16), W.astype(np.float16), V.astype(np.float16)
    p["bias"] = d["bias"].astype(np.float32)
    if c["counts"]:
        p["counts"] = d["counts"].astype(np.int32)
    if c["vss"]:
        vss = np.full((n_vss(c), 2, c["ldv"]), np.nan, np.float32)
        vss[:, :, :nch] = d["vss"]
        p["vss"] = vss
    if c["aff"]:
        B = n_smp(c)
        ss = np.zeros((B, 2, kp), np.float32)  # [sample][scale | shift][k_pad], as slide_amd.rows publishes it: in_bs = 2 k_pad
        ss[:, 0] = 1
        ss[:, 0, :kl], ss[:, 1, :kl] = d["scale"], d["shift"]
        p["ss"] = ss
        if c["add_n"]:
            add = np.zeros((B, kp), np.float32)
            add[:, :kl] = d["add"]
            p["add"] = add  # add_bs = k_pad
    return p


# -------------------------------------------------------------------------------------------------------------- reference
def forward(c, d, mutant=None):
    """float64 reference of the case (or of one of its mutants): dict(y [pts][ldo-logical = n_cob * 32], b, stored) -- b holds the fp16
    store term and is 0 where the element must be exact"""
    K, rows, kl, C, n_cob, dist = c["K"], c["rows"], c["kl"], c["C"], c["n_cob"], c["dist"]
    pts, nch = rows // K, n_cob * 32
    X, W = r16(d["X"]), r16(d["W"])
    if c["aff"]:
        B, tps = n_smp(c), c["tps"]
        tile = np.arange(rows) >> 8
        smp = tile // tps
        if mutant == "affine_sample":
            smp = (smp + 1) % B if tps == 1 else np.minimum(tile, B - 1)
        X = r16(X * r16(d["scale"])[smp] + r16(d["shift"])[smp])
        if c["aff_relu"] and mutant != "aff_relu_dropped":
            X = np.maximum(X, 0)
        if c["add_n"]:
            n = kl if mutant == "add_all_columns" else c["add_n"]
            X = X.copy()
            X[:, :n] = r16(X[:, :n] + r16(d["add"])[smp][:, :n])
    if mutant == "k_tail":
        X = X.copy()
        X[:, kl - 1] = 0
    bias = d["bias"].astype(np.float64)
    if mutant == "bias_block0":
        bias = np.tile(bias[:32], n_cob)
    Wf = np.zeros((nch, kl))
    Wf[:C] = W
    s = X @ Wf.T + bias
    sig = C_ACC * (np.abs(X) @ np.abs(Wf).T + np.abs(bias))
    if mutant == "scores_fp16":
        s = r16(s)
    # slots [pts][KM]: row of slot k of point p is p K + k; KM > K only for the mutant that walks into the next point
    mask, n, zero = _slots(dict(pts=pts, K=K, counts=c["counts"]), d, mutant)
    KM = K
    if mutant == "count_unclamped_high":
        KM = K + 5
        n = np.where(d["counts"] > K, d["counts"], n)
        mask = np.arange(KM)[None] < n[:, None]
    ridx = np.minimum(np.arange(pts)[:, None] * K + np.arange(KM)[None], rows - 1)
    mask = mask[:, :, None]
    v = r16(d["V"])[ridx]                                       # [pts][KM][nch]
    extra = 0.0
    if c["vss"]:
        pt = np.arange(pts)
        vs_smp = pt // c["pps"]
        if mutant == "vss_sample_of_tile":
            vs_smp = np.minimum((pt * K) >> 8, n_vss(c) - 1)
        sc, sh = d["vss"].astype(np.float64)[vs_smp, 0, None, :], d["vss"].astype(np.float64)[vs_smp, 1, None, :]
        extra = 2 * (np.abs(v * sc) + np.abs(sh))
        v = v * sc + sh
        if c["vss"] == "relu" and mutant != "v_relu_dropped":
            v = np.maximum(v, 0)
    v = np.where(mask, v, 0.0)
    sm = np.where(mask, s[ridx], -np.inf)
    sg = np.where(mask, sig[ridx], 0.0)
    mx = sm.max(1, keepdims=True)
    if mutant == "no_max_shift":  # in fp32, as the kernel would: exp overflows from 88.7 on, and all-underflow gives 0 / 0
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            e = np.exp(sm.astype(np.float32))
            w = (e / e.sum(1, keepdims=True)).astype(np.float64)
    else:
        e = np.exp(sm - mx)
        w = e / e.sum(1, keepdims=True)
    dk = np.where(mask, np.abs(sm - mx), 0.0)
    with np.errstate(invalid="ignore"):
        y = (w * v).sum(1)
    av = np.abs(v)
    Wt = (w * av).sum(1)
    if dist == "onehot":
        b = np.zeros_like(y)
    elif dist == "w0":
        b = K * U * Wt
    else:
        eps = np.expm1(sg) + (3 * dk + 2) * U
        se = (w * eps).sum(1)
        assert mutant is not None or (se < 0.25).all()
        b = ((w * av * eps).sum(1) + Wt * se) / (1 - np.minimum(se, 0.5)) + (2 * K + 8) * U * Wt + U * (w * extra * mask).sum(1)
    y[zero] = 0
    if mutant != "pad_channels_not_zeroed":
        y[:, C:] = 0
    b[:, C:] = 0
    return store(dict(y=y, b=np.nan_to_num(b)), True)
