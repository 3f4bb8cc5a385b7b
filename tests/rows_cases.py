"""The SLIDE_OP_ROWS_* case matrix, its float64 references, its error bounds and its mutants -- shared by
tests/test_hip_rows_arith.py (every case on the GPU against the reference, and, on the CPU, every bound against the mutants).
The companion of tests/gemm_cases.py for the other half of the module-level path: the byte movers and reductions of
csrc/rows_ops.hip (`launch_rows<float>` and `launch_rows<_Float16>`), launched one op at a time through slide_amd.rows._rop.

A reference takes the operands as the kernel reads them: activation rows ("rows" below) are fp32, or rounded to fp16 first (r16)
when the case runs the fp16 instantiation; coordinates, gamma, beta, addvec, scale / shift tables, tile sums, the pair table
and counts / indices are fp32 / int as passed.  All arithmetic is float64, written from the semantics in the kernel comments and
oracle/denoiser_np.py (softmax over the first max(1, count) slots, MyGroupNorm's pass-through tail, QueryAndGroup's empty ball).

Bounds, elementwise (u = 2^-24, the fp32 unit roundoff; every kernel computes in fp32 whatever the row type).  A bound of 0
marks an element that must be EXACT (bit-equal to the reference rounded to the stored type).
  store   rows fp16: b (1 + 2^-11) + 2^-11 |ref| + 2^-25      fp32 rows / fp32 tables: b + u |ref|     (gemm_cases.py's store)
  NCX, CONCAT_QK, POOL max, GROUP feature / abs / centre / d2 columns, every pad column: exact.
  GROUP   rel = nbr - centre is one fp32 subtraction: b = u |rel|.  The FP weight w_k = t_k / sum_j t_j, t = 1 / (d2 + 1e-8f):
          t carries one addition and one division (<= 2.5 ulp unless correctly rounded: 1 + 3 = 4 u), the sum K - 1 additions,
          the quotient 3 u more: b = (K + 12) u w.
  GN      the NORM derivation of gemm_cases.py with an exact input (b = 0 there), over the n = S * gs values of a (sample, group)
          with mean m and variance v (from E[y^2] - m^2 in fp32), d = ceil(log2 n) + 2:
            dm = (d + 2) u mean|y|        dv = 4 (d + 2) u mean(y^2)        dr = rstd (0.6 dv / (v + eps) + 4 u)
            b' = |gamma| rstd dm + |gamma| |y - m| dr + 3 u (|y g| + |m g| + |beta|),   g = gamma rstd
          channels past n_norm are exact; then ReLU (1-Lipschitz) -> + addvec -> + residual: b += 4 u (|value| + |addvec| +
          |residual|).  (The kernel's sums are chains, not trees: rows of a thread, rt threads, <= 64 chunks, gs channels, at most
          ~150 links in the matrix below; their error grows like sqrt(links) u, which d + 2 >= 11 covers.  The worst-case linear
          growth is not claimed.)  With tile sums in place of the statistics pass the sums are fp32 INPUTS (rounded once: inside
          dm / dv) of a tensor of the case's choosing -- a different one than x, so that a kernel that ignored them is seen.
          The published tables: dsc = |gamma| dr + 2 u |sc|,  dsh = |m| dsc + |sc| dm + 3 u (|beta| + |m sc|);  mean / rstd
          output: dm + u |m|, dr.  GN_APPLY_ONLY with the published table must reproduce the one-call output bit for bit.
  JOINT   the same table bounds from the producers' tile sums (q's counted K times), n = S_k * gs.
  ATTN    weights w_k = e_k / l, e_k = expf(s_k - max), l = sum e_j.  The subtraction rounds once: e_k carries d_k u with
          d_k = |s_k - max|, plus the device expf's error E_EXP = 2 u (1 ulp: ROCm documentation, "HIP math API", table of
          single-precision functions, expf: maximum error 1 ULP), in the numerator and again (weighted) in l; l adds K - 1
          times, 1 / l is 3 u, e * l, v * w and the K accumulations one each: (2 K + 4) u, taken as (2 K + 8) u:
            b = [ (2 K + 8 + 2 E) W + sum_k w_k |v_k| d_k + W sum_j w_j d_j ] u,      W = sum_k w_k |v_k|
          with deferred values v' = relu?(v scale + shift): + 2 u sum_k w_k (|v scale| + |shift|).  Slots past the count have
          weight exactly 0: the reference leaves them out and the bound does not know them.  (A thread reads ldo columns of
          every score and value row: the cases keep ldo <= lds, ldv, as slide_amd.rows.attend and pool do.)
          exp(60) = 1.1e26 is inside fp32's range, so a softmax WITHOUT the max shift is still correct at scores of +-60 (the case
          the issue names for it); it overflows from 88.7 on, and the +-100 case is the one that shows that mutant (EXEMPT).
  POOL    mean over n slots: n - 1 additions and a division: b = (K + 1) u sum|x| / n.
  PAIR    t = A[src] + (bias + Cc . centre) (+ wd d2 + ww w): three fmas, an addition, two fmas:
          b = 6 u (|A| + |bias| + sum|Cc c| + |wd d2| + |ww w|) + (K + 12) u |ww w|; tile sums of the UNROUNDED fp32 t with the
          STATS bound of gemm_cases.py: |ds| <= sum b + d u sum|t|, |dsq| <= sum (2 |t| b + b^2) + d u sum t^2, d = log2 256 + 2.

Mutants (test_bounds_see_the_mutants): the nearest plausible wrong arithmetic, applied to the float64 reference and rounded to
the stored type; `mutants(c)` lists those a case can express (a neighbouring sample needs B > 1, a count mutant needs counts).
  GN     unbiased_var | count_rpc_nchunk (S taken as rpc * nchunk) | drop_last_row (of the last chunk, from the sums) |
         neighbour_sample (scale / shift of sample b + 1) | tail_normalised (channel n_norm) | stats_no_relu
  ATTN / POOL   slot_past_count | zero_count_empty | max_first_n | no_max_shift (evaluated in fp32, where it overflows)
  GROUP  rel_sign | w_k_minus_1 | idx32_as_64         CONCAT_QK  seam_other_source | q_row_mod
  PAIR   cc_without_wrel | sums_of_rounded            NCX  pad_not_cleared       JOINT  q_once
A mutant below a case's resolution is listed in EXEMPT with the case of the same op and row type that shows it.

Measured on an MI355X, worst err / tol per op and row type (183 GPU tests of tests/test_hip_rows_arith.py in 3.8 s, next to
3.0 s for the 36 of tests/test_hip_gemm_arith.py on the same machine):
  op            fp32 rows   fp16 rows        op            fp32 rows   fp16 rows
  GROUP         0.500       0.991            ATTN          0.142       0.975
  GN            0.353       0.998            POOL          0.262       0.989
  GN tables     0.059 (table), 0.205 (mean / rstd, common mode)      PAIR_EXPAND   --          0.999 (tile sums 0.129)
  GN_JOINT      0.131 (tables and end to end; fp32 tables whatever the row type)
  NCX, CONCAT_QK, POOL max, GROUP without coordinates: exact (0) in both.
fp16 rows sit at half an ulp of the store, as the GEMM suite found.  GROUP's 0.5 in fp32 rows is the one subtraction (half an ulp =
u |rel|) under a bound that counts it and the store: 2 u |rel|.  Bounded cases at exactly 0: K = 1 attention and K = 1 mean (a
weight of exactly 1, a division by 1), and the +-60 / +-100 attention (the other weights underflow to 0: the output IS the top
slot's value), and GN with G = 0 and a ReLU only (a mover)."""
import zlib

import numpy as np

from slide_amd.abi import ru  # noqa: F401  (used here and re-exported to the test modules)

U = 2.0 ** -24
EPS = 1e-5
E_EXP = 2.0  # expf: 1 ulp = 2 u
PREFILL = 7.0  # what every output buffer holds before the launch
GROUP_FP, GROUP_ABS, GROUP_CENTER, GROUP_NO_XYZ, GROUP_IDX32 = 1, 2, 4, 8, 16
POOL_MAX, POOL_AVG, POOL_MAX_AVG = 0, 1, 2
GN_PRE_RELU, GN_POST_RELU, GN_STATS_ONLY, GN_APPLY_ONLY = 1, 2, 4, 8
OPS = ("from_ncx", "to_ncx", "group", "gn", "gn_joint", "concat_qk", "attn", "pool", "pair_expand")


def r16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def T(c, a):
    """rows as the kernel reads them"""
    return r16(a) if c["half"] else np.asarray(a, np.float64)


def ncoord(flags):
    return 11 if flags & GROUP_FP else 0 if flags & GROUP_NO_XYZ else 3 + (3 if flags & GROUP_ABS else 0) + (3 if flags & GROUP_CENTER else 0)


def gn_map(half, ld, S):
    """the launcher's thread map (rows_ops.hip, SLIDE_OP_ROWS_GN): cn threads per row, rt rows in flight, nchunk chunks of rpc rows"""
    vec = 8 if half else 4
    cn = ld // vec
    rt = 256 // cn
    nchunk = min(64, max(1, (S + rt * 8 - 1) // (rt * 8)))
    rpc = (S + nchunk - 1) // nchunk
    nchunk = (S + rpc - 1) // rpc
    return dict(cn=cn, rt=rt, idle=256 - rt * cn, nchunk=nchunk, rpc=rpc, clamped=(S + rt * 8 - 1) // (rt * 8) > 64,
                last_short=rpc * nchunk != S)


# --------------------------------------------------------------------------------------------------------------- the matrix
CASES = []


def _add(op, name, half, **kw):
    c = dict(op=op, name="%s_%s_%s" % (op, name, "f16" if half else "f32"), half=half, status=0, wrap=False)
    c.update(kw)
    CASES.append(c)


for _h in (False, True):
    # 1. module boundary: every C and every P of the issue, B > 1
    for _C, _P in ((1, 1), (3, 31), (31, 32), (32, 33), (33, 1000), (515, 33), (3, 1000)):
        _add("from_ncx", "c%d_p%d" % (_C, _P), _h, B=3, C=_C, P=_P, wrap=(_C, _P) == (33, 1000))
        _add("to_ncx", "c%d_p%d" % (_C, _P), _h, B=3, C=_C, P=_P, wrap=(_C, _P) == (33, 1000))
    # 2. grouping: flags x index width; C so that the coordinates start inside a piece (5, 13), on a boundary (0, 8, 64) and span
    #    two pieces (5 + 6, 13 + 9, 5 + 11); ldf != ldg; counts with zeros also in the FP layout
    for _n, _fl, _i32, _C, _K, _cnt, _xf, _xg in (
            ("plain", 0, False, 0, 1, False, 0, 0), ("plain_i32", 0, True, 5, 5, True, 32, 0),
            ("abs", GROUP_ABS, False, 8, 48, False, 0, 32), ("abs_i32", GROUP_ABS, True, 13, 5, True, 32, 0),
            ("ctr", GROUP_CENTER, False, 64, 5, True, 32, 0), ("ctr_i32", GROUP_CENTER, True, 5, 1, False, 0, 32),
            ("absctr", GROUP_ABS | GROUP_CENTER, False, 13, 48, True, 0, 0), ("absctr_i32", GROUP_ABS | GROUP_CENTER, True, 8, 5, False, 64, 0),
            ("fp", GROUP_FP, False, 5, 5, True, 32, 0), ("fp_i32", GROUP_FP, True, 64, 48, False, 0, 0),
            ("fp_nofeat", GROUP_FP, False, 0, 48, False, 0, 0),
            ("noxyz", GROUP_NO_XYZ, False, 13, 1, False, 32, 0), ("noxyz_i32", GROUP_NO_XYZ, True, 64, 5, True, 0, 32)):
        _ldg = ru(_C + ncoord(_fl)) + _xg
        _add("group", _n, _h, B=2, N=37, np=11, K=_K, C=_C, flags=_fl | (GROUP_IDX32 if _i32 else 0), ldf=ru(max(_C, 1)) + _xf,
             ldg=_ldg, counts=_cnt, wrap=_n in ("abs_i32", "fp"))
    _add("group", "bad_ldg_mod8", _h, B=2, N=37, np=11, K=5, C=8, flags=0, ldf=32, ldg=36, counts=False, status=-3)
    _add("group", "bad_ldg_narrow", _h, B=2, N=37, np=11, K=5, C=30, flags=GROUP_ABS | GROUP_CENTER, ldf=32, ldg=32, counts=False,
         status=-3)
    # 3. GroupNorm on rows
    _gn = dict(B=3, G=32, flags=0, addvec_ld=0, res_ld=0, inplace=True, dist="normal", tiles=False, mr=False, split=False)
    for _n, _kw in (
            ("ld32_s1", dict(ld=32, C=24, S=1, G=1, n_norm=24)),
            ("ld32_s16_b33", dict(ld=32, C=32, S=16, B=33, n_norm=32, flags=GN_POST_RELU, addvec_ld=20, inplace=False)),
            ("ld96_s40_tail", dict(ld=96, C=70, S=40, n_norm=64, flags=GN_PRE_RELU, res_ld=128)),
            ("ld96_s40_common", dict(ld=96, C=64, S=40, n_norm=64, dist="common", mr=True)),
            ("ld96_s255", dict(ld=96, C=96, S=255, G=1, n_norm=96, flags=GN_PRE_RELU | GN_POST_RELU, addvec_ld=96, inplace=False)),
            ("ld128_s256_tiles", dict(ld=128, C=128, S=256, G=64, n_norm=128, flags=GN_PRE_RELU | GN_POST_RELU, tiles=True)),
            ("ld128_s257_zero", dict(ld=128, C=100, S=257, n_norm=96, dist="zero_sample", inplace=False, res_ld=160)),
            ("ld128_s512_split", dict(ld=128, C=128, S=512, G=64, n_norm=128, flags=GN_POST_RELU, addvec_ld=100, split=True, mr=True)),
            ("ld128_s512_split_tiles", dict(ld=128, C=120, S=512, G=1, n_norm=120, flags=GN_PRE_RELU, split=True, tiles=True)),
            ("ld128_s8500_clamp", dict(ld=128, C=128, S=8500, B=2, G=64, n_norm=128, flags=GN_PRE_RELU)),
            ("ld544_s255", dict(ld=544, C=515, S=255, B=2, n_norm=512, flags=GN_POST_RELU)),
            ("ld544_s4096", dict(ld=544, C=515, S=4096, B=2, n_norm=512, addvec_ld=515)),
            ("ld1024_s16", dict(ld=1024, C=1024, S=16, G=64, n_norm=1024, flags=GN_PRE_RELU | GN_POST_RELU)),
            ("ld1024_s1100_clamp", dict(ld=1024, C=1000, S=1100, B=2, G=1, n_norm=1000, inplace=False)),
            ("g0_relu", dict(ld=96, C=70, S=40, G=0, n_norm=0, flags=GN_PRE_RELU)),
            ("g0_add", dict(ld=96, C=70, S=257, G=0, n_norm=0, flags=GN_POST_RELU, addvec_ld=64, res_ld=128, inplace=False))):
        _c = dict(_gn)
        _c.update(_kw)
        _add("gn", _n, _h, wrap=_n in ("ld96_s40_tail", "ld128_s256_tiles"), **_c)
    # 5. relu([q | k]): the seam inside a 16-byte piece and on one (C1 = 4: aligned in fp32 rows only); three different strides
    for _C1, _C2, _K in ((3, 12, 1), (4, 60, 8), (8, 139, 16), (51, 12, 8), (256, 60, 1), (8, 60, 16)):
        _add("concat_qk", "c%d_c%d_k%d" % (_C1, _C2, _K), _h, pts=37, K=_K, C1=_C1, C2=_C2, ldq=ru(_C1) + 64, ldk=ru(_C2) + 32,
             ldo=ru(_C1 + _C2), wrap=False)
    _add("concat_qk", "wrap", _h, pts=37, K=8, C1=51, C2=60, ldq=64, ldk=64, ldo=128, wrap=True)
    # 6. softmax over the neighbours + weighted sum
    for _n, _kw in (
            ("k1", dict(K=1, C=20, lds=96, ldv=64, ldo=32)),
            ("k4_counts", dict(K=4, C=51, lds=128, ldv=96, ldo=64, counts=True)),
            ("k16_vss", dict(K=16, C=51, lds=96, ldv=128, ldo=64, vss=True, v_relu=0, pps=8)),
            ("k16_vss_relu_counts", dict(K=16, C=60, lds=128, ldv=96, ldo=64, counts=True, vss=True, v_relu=1, pps=8)),
            ("k48_counts", dict(K=48, C=33, lds=160, ldv=96, ldo=64, counts=True)),
            ("k48", dict(K=48, C=64, lds=96, ldv=128, ldo=64)),
            ("k16_pm60", dict(K=16, C=51, lds=96, ldv=128, ldo=64, dist="pm60")),
            ("k16_pm100", dict(K=16, C=51, lds=96, ldv=128, ldo=64, dist="pm100")),
            ("wrap", dict(K=16, C=51, lds=64, ldv=64, ldo=64, counts=True, vss=True, v_relu=1, pps=8, wrap=True))):
        _c = dict(pts=24, counts=False, vss=False, v_relu=0, pps=24, dist="normal")
        _c.update(_kw)
        _add("attn", _n, _h, **_c)
    # 7. pooling: odd C (the C / 2 split inside a piece)
    for _n, _mode, _K, _cnt in (("max", POOL_MAX, 16, True), ("avg", POOL_AVG, 16, False), ("avg_counts", POOL_AVG, 48, True),
                                ("maxavg", POOL_MAX_AVG, 5, False), ("maxavg_counts", POOL_MAX_AVG, 16, True), ("avg_k1", POOL_AVG, 1, True)):
        _add("pool", _n, _h, pts=24, K=_K, C=51, ldx=96, ldo=64, mode=_mode, counts=_cnt)
    _add("pool", "wrap", _h, pts=24, K=16, C=51, ldx=64, ldo=64, mode=POOL_MAX_AVG, counts=True, wrap=True)

# 4. joint GroupNorm of the virtual [q x K | k] (untyped kernel; dispatched from both instantiations)
for _n, _h, _kw in (("straddle", True, dict(np_=256, K=4, C1=50, C2=46, n_norm=96)),       # tq = 1 from S_q % 256 == 0
                    ("two_tiles", False, dict(np_=512, K=2, C1=50, C2=53, n_norm=96)),      # tq = 2, n_norm < C1 + C2
                    ("one_row", True, dict(np_=64, K=4, C1=35, C2=61, n_norm=96))):        # S_q = 64: ONE row of sums per sample
    _add("gn_joint", _n, _h, B=3, G=32, wrap=True, **_kw)
for _n, _kw in (("bad_g0", dict(G=0)), ("bad_n_norm", dict(n_norm=95)), ("bad_c1", dict(C1=70, ldq=64)), ("bad_null", dict(null=True))):
    _c = dict(np_=256, K=4, C1=50, C2=46, n_norm=96, B=3, G=32, status=-3)
    _c.update(_kw)
    _add("gn_joint", _n, True, **_c)

# 8. pair expansion (fp16 rows only): CH 4 / 8, the XCD tile map with B around 8, the linear map with a ragged last tile
for _n, _kw in (("ld64_b1", dict(ld=64, B=1, np_=16, K=16, fp=False, relu=True, stats=True)),
                ("ld64_b7_fp", dict(ld=64, B=7, np_=32, K=8, fp=True, relu=False, stats=True, idx32=True)),
                ("ld256_b8", dict(ld=256, B=8, np_=16, K=16, fp=False, relu=False, stats=False)),
                ("ld256_b9_fp", dict(ld=256, B=9, np_=64, K=8, fp=True, relu=True, stats=True)),
                ("ld64_ragged_fp", dict(ld=64, B=3, np_=50, K=7, fp=True, relu=True, stats=True)),
                ("ld256_ragged", dict(ld=256, B=2, np_=37, K=5, fp=False, relu=True, stats=False, idx32=True))):
    _c = dict(N=40, idx32=False, ldA_extra=8)
    _c.update(_kw)
    _add("pair_expand", _n, True, **_c)
_add("pair_expand", "fp32_rows", False, ld=64, B=1, np_=16, K=16, fp=False, relu=True, stats=False, N=40, idx32=False, ldA_extra=0,
     status=-3)

CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# (case, mutant) -> the case of the same op and row type where that mutant IS visible
EXEMPT = {}


def _exempt(op, names, mutant, other, halves=(False, True)):
    for h in halves:
        sfx = "_f16" if h else "_f32"
        for n in names:
            EXEMPT[("%s_%s%s" % (op, n, sfx), mutant)] = "%s_%s%s" % (op, other, sfx)


# ld = ru(C): no pad column exists
_exempt("from_ncx", ["c32_p33"], "pad_not_cleared", "c33_p1000")
# exp(60) is inside fp32's range (docstring, ATTN)
_exempt("attn", ["k16_pm60"], "no_max_shift", "k16_pm100")
# one group of 1000 channels x 1100 rows (n = 1.1e6): n - 1 for n moves the output by 4.5e-7 |y - m| rstd, inside the fp32
# statistics' share of the bound (dv: 4 (d + 2) u = 6e-6 of the variance)
_exempt("gn", ["ld1024_s1100_clamp"], "unbiased_var", "ld96_s40_tail")


def mutants(c):
    op = c["op"]
    if c["status"] != 0:
        return []
    if op == "from_ncx":
        return ["pad_not_cleared"]
    if op == "group":
        m = [] if c["flags"] & GROUP_NO_XYZ else ["rel_sign"]
        if c["flags"] & GROUP_FP:
            m.append("w_k_minus_1")
        if c["flags"] & GROUP_IDX32:
            m.append("idx32_as_64")
        return m
    if op == "gn":
        if c["G"] == 0:
            return []
        mp = gn_map(c["half"], c["ld"], c["S"])
        m = ["unbiased_var"] if c["S"] * (c["n_norm"] // c["G"]) > 1 else []
        if not c["tiles"]:
            m.append("drop_last_row")
            if mp["last_short"]:
                m.append("count_rpc_nchunk")
            if c["flags"] & GN_PRE_RELU:
                m.append("stats_no_relu")
        if c["B"] > 1:
            m.append("neighbour_sample")
        if c["n_norm"] < c["C"]:
            m.append("tail_normalised")
        return m
    if op == "gn_joint":
        return ["q_once", "unbiased_var"]
    if op == "concat_qk":
        return ["seam_other_source", "q_row_mod"]
    if op == "attn":
        return (["slot_past_count", "zero_count_empty"] if c["counts"] else []) + (["no_max_shift"] if c["dist"] != "normal" else [])
    if op == "pool":
        m = ["slot_past_count", "zero_count_empty"] if (c["counts"] and c["mode"] != POOL_MAX and c["K"] > 1) else []
        return m + (["max_first_n"] if (c["counts"] and c["mode"] != POOL_AVG) else [])
    if op == "pair_expand":
        return ["cc_without_wrel"] + (["sums_of_rounded"] if c["stats"] else [])
    return []


def reach(c):
    """the launcher's branch values of a case, by the launcher's own formulas (rows_ops.hip)"""
    op, h = c["op"], c["half"]
    vec = 8 if h else 4
    r = dict(op=op, half=h)
    if op in ("from_ncx", "to_ncx"):
        r.update(C=c["C"], P=c["P"], pad=ru(c["C"]) - c["C"])
    elif op == "group":
        C, nc = c["C"], ncoord(c["flags"])
        r.update(flags=c["flags"] & 15, idx32=bool(c["flags"] & GROUP_IDX32), C=C, K=c["K"], counts=c["counts"],
                 coord_start="none" if nc == 0 else ("boundary" if C % 8 == 0 else "inside"),
                 coord_span=nc > 0 and C // 8 != (C + nc - 1) // 8, ld_differ=c["ldf"] != c["ldg"], status=c["status"])
    elif op == "gn":
        r.update(gn_map(h, c["ld"], c["S"]))
        r.update(ld=c["ld"], S=c["S"], G=c["G"], relu=c["flags"] & 3, tail=c["G"] > 0 and c["n_norm"] < c["C"], B=c["B"],
                 addvec=c["addvec_ld"] > 0 and c["addvec_ld"] < c["ld"], res=c["res_ld"] > c["ld"], inplace=c["inplace"],
                 dist=c["dist"], tps=c["S"] // 256 if c["tiles"] else 0, mr=c["mr"], split=c["split"])
    elif op == "gn_joint":
        gs = c["n_norm"] // c["G"] if c["G"] else 0
        Sq = c["np_"]
        r.update(tq=Sq // 256 if Sq % 256 == 0 else 1, one_row=Sq % 256 != 0, tk=Sq * c["K"] // 256,
                 straddle=bool(gs) and c["C1"] % gs != 0, tail=c["n_norm"] < c["C1"] + c["C2"], status=c["status"])
    elif op == "concat_qk":
        r.update(C1=c["C1"], C2=c["C2"], K=c["K"], seam_aligned=c["C1"] % vec == 0,
                 strides_differ=len({c["ldq"], c["ldk"], c["ldo"]}) == 3)
    elif op == "attn":
        r.update(K=c["K"], counts=c["counts"], vss=c["vss"], v_relu=c["v_relu"], dist=c["dist"], pad=c["C"] < c["ldo"],
                 strides_differ=len({c["lds"], c["ldv"], c["ldo"]}) == 3, pps=c["pps"])
    elif op == "pool":
        r.update(mode=c["mode"], counts=c["counts"], split_inside=(c["C"] // 2) % vec != 0, strides_differ=c["ldx"] != c["ldo"])
    elif op == "pair_expand":
        S = c["np_"] * c["K"]
        r.update(CH=8 if c["ld"] >= 256 else 4, tps=S // 256 if S % 256 == 0 else 0, B=c["B"], fp=c["fp"], relu=c["relu"],
                 stats=c["stats"], idx32=c["idx32"], ragged=(c["B"] * S) % 256 != 0, status=c["status"])
    return r


# ------------------------------------------------------------------------------------------------------------------ data
def _rs(c):
    return np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)


def _mat(rs, rows, C, ld, pad="garbage", scale=1.0):
    """[rows][ld] fp32: N(0, scale) in the C logical columns; pad columns zero, or finite garbage the kernel must ignore"""
    a = np.zeros((rows, ld), np.float32)
    a[:, :C] = rs.standard_normal((rows, C)) * scale
    if pad == "garbage" and ld > C:
        a[:, C:] = rs.uniform(100.0, 200.0, (rows, ld - C)) * rs.choice([-1.0, 1.0], (rows, ld - C))
    return a


def _counts(rs, pts, K):
    """0, 1, K and above K all occur"""
    cnt = rs.randint(0, K + 3, pts).astype(np.int32)
    cnt[:4] = (0, 1, K, K + 2)
    return cnt


def make_data(c):
    """the case's inputs in the PHYSICAL layouts the op reads (fp32 / int arrays; "rows" are converted to the row type by the
    launcher of the test) -- deterministic per case name"""
    rs = _rs(c)
    op = c["op"]
    d = {}
    if op == "from_ncx":
        d["x"] = (rs.standard_normal((c["B"], c["C"], c["P"])) * 30).astype(np.float32)
    elif op == "to_ncx":
        d["rows"] = _mat(rs, c["B"] * c["P"], c["C"], ru(c["C"]), scale=30.0)
    elif op == "group":
        B, N, npt, K, C = c["B"], c["N"], c["np"], c["K"], c["C"]
        d["xyz"] = rs.uniform(0, 1, (B, N, 3)).astype(np.float32)
        d["new_xyz"] = rs.uniform(0, 1, (B, npt, 3)).astype(np.float32)
        d["feat"] = _mat(rs, B * N, C, c["ldf"])
        idx = rs.randint(0, N, (B, npt, K))
        idx[:, 0, 0], idx[:, 1, -1] = 0, N - 1
        if K > 1:
            idx[:, 2, 1] = idx[:, 2, 0]
        d["idx"] = idx.astype(np.int32 if c["flags"] & GROUP_IDX32 else np.int64)
        d["d2"] = rs.uniform(0.01, 4.0, (B, npt, K)).astype(np.float32)
        if c["counts"]:
            cnt = rs.randint(0, K + 1, (B, npt)).astype(np.int32)
            cnt[:, 3], cnt[0, 0] = 0, 0
            d["counts"] = cnt
    elif op == "gn":
        B, S, ld, C = c["B"], c["S"], c["ld"], c["C"]
        x = _mat(rs, B * S, C, ld, pad="zero")
        if c["dist"] == "common":
            x[:, :C] += np.float32(30.0)
        elif c["dist"] == "zero_sample":
            x[S:2 * S] = 0
        d["x"] = x
        n_norm = c["n_norm"]
        d["gamma"] = (1 + 0.2 * rs.standard_normal(max(n_norm, 1))).astype(np.float32)
        d["beta"] = (0.2 * rs.standard_normal(max(n_norm, 1))).astype(np.float32)
        if c["addvec_ld"]:
            d["addvec"] = rs.standard_normal((B, c["addvec_ld"])).astype(np.float32)
        if c["res_ld"]:
            d["res"] = _mat(rs, B * S, C, c["res_ld"], pad="zero")
            d["res"][:, ld:] = 50.0  # (columns past ld belong to somebody else)
        if c["tiles"]:  # per-256-row-tile channel sums of ANOTHER tensor (of its ReLU with PRE_RELU), as a GEMM would publish them
            x2 = _mat(rs, B * S, C, ld, pad="zero", scale=1.5) + np.float32(0.5) * (np.arange(ld) < C)
            d["x2"] = x2.astype(np.float32)
            s = T(c, d["x2"])
            if c["flags"] & GN_PRE_RELU:
                s = np.maximum(s, 0)
            s = s.reshape(B * S // 256, 256, ld)
            d["tsum"], d["tsq"] = s.sum(1).astype(np.float32), (s * s).sum(1).astype(np.float32)
    elif op == "gn_joint":
        B, npt, K, C1, C2 = c["B"], c["np_"], c["K"], c["C1"], c["C2"]
        ldq, ldk = c.get("ldq", ru(C1) + 32), c.get("ldk", ru(C2))
        q = np.maximum(_mat(rs, B * npt, min(C1, ldq), ldq, pad="zero") + np.float32(0.3), 0)
        k = np.maximum(_mat(rs, B * npt * K, C2, ldk, pad="zero", scale=2.0), 0)
        d["q"], d["k"] = q.astype(np.float32), k.astype(np.float32)
        tq = npt // 256 if npt % 256 == 0 else 1
        tk = npt * K // 256
        qv, kv = T(c, d["q"]).reshape(B * tq, -1, ldq), T(c, d["k"]).reshape(B * tk, 256, ldk)
        d["qsum"], d["qsq"] = qv.sum(1).astype(np.float32), (qv * qv).sum(1).astype(np.float32)
        d["ksum"], d["ksq"] = kv.sum(1).astype(np.float32), (kv * kv).sum(1).astype(np.float32)
        n = max(c["n_norm"], 1)
        d["gamma"] = (1 + 0.2 * rs.standard_normal(n)).astype(np.float32)
        d["beta"] = (0.2 * rs.standard_normal(n)).astype(np.float32)
    elif op == "concat_qk":
        d["q"] = _mat(rs, c["pts"], c["C1"], c["ldq"])
        d["k"] = _mat(rs, c["pts"] * c["K"], c["C2"], c["ldk"])
    elif op == "attn":
        pts, K, C = c["pts"], c["K"], c["C"]
        s = _mat(rs, pts * K, c["lds"], c["lds"], scale=2.0)
        if c["dist"] in ("pm60", "pm100"):
            a = 60.0 if c["dist"] == "pm60" else 100.0
            s[:] = -a
            top = rs.randint(0, K, (pts, c["lds"]))
            s.reshape(pts, K, -1)[np.arange(pts)[:, None], top, np.arange(c["lds"])[None]] = a
        v = _mat(rs, pts * K, c["ldv"], c["ldv"])
        if c["counts"]:
            d["counts"] = _counts(rs, pts, K)
            masked = (np.arange(K)[None] >= np.clip(d["counts"], 1, K)[:, None]).reshape(-1)
            s[masked] = 30.0                                  # the largest score of the point: a maximum over all K slots is seen
            v[masked] = 6e4 if c["half"] else 1e30            # finite but huge: any weight but exactly 0 leaves a trace
        d["S"], d["V"] = s, v
        if c["vss"]:
            nsmp = pts // c["pps"]
            d["vss"] = np.stack([rs.uniform(0.5, 1.5, (nsmp, c["ldv"])), 0.5 * rs.standard_normal((nsmp, c["ldv"]))], 1).astype(np.float32)
    elif op == "pool":
        pts, K = c["pts"], c["K"]
        d["x"] = _mat(rs, pts * K, c["C"], c["ldx"])
        if c["counts"]:
            d["counts"] = _counts(rs, pts, K)
            masked = (np.arange(K)[None] >= np.clip(d["counts"], 1, K)[:, None]).reshape(-1)
            d["x"][masked] += np.float32(10.0)  # (the maximum of the point lies in a masked slot; the mean must not see it)
    elif op == "pair_expand":
        B, N, npt, K, ld = c["B"], c["N"], c["np_"], c["K"], c["ld"]
        ldA = ld + c["ldA_extra"]
        f = lambda *s: rs.standard_normal(s).astype(np.float32)
        d["xyz"] = rs.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        d["new_xyz"] = rs.uniform(-1, 1, (B, npt, 3)).astype(np.float32)
        d["w_rel"], d["w_abs"], d["w_ctr"] = f(ld, 3), f(ld, 3), f(ld, 3)
        d["bias"] = 0.5 * f(ld)
        coef = np.zeros((ld, 8), np.float32)
        coef[:, 0:3] = d["w_rel"] + d["w_abs"]
        coef[:, 3:6] = d["w_ctr"] - d["w_rel"]
        if c["fp"]:
            coef[:, 6], coef[:, 7] = 0.3 * f(ld), f(ld)
        d["coef"] = coef
        A = np.full((B * N, ldA), 1e30, np.float32)
        A[:, :ld] = (f(B * N, ld).astype(np.float64) + d["xyz"].reshape(-1, 3).astype(np.float64) @ coef[:, 0:3].T.astype(np.float64))
        d["A"] = A
        idx = rs.randint(0, N, (B, npt, K))
        idx[:, 0, 0], idx[:, 1, -1] = 0, N - 1
        d["idx"] = idx.astype(np.int32 if c["idx32"] else np.int64)
        d["d2"] = rs.uniform(0.01, 4.0, (B, npt, K)).astype(np.float32)
    return d


# ------------------------------------------------------------------------------------------------------------- references
def _fp_weight(d2, K, mutant=None):
    t = 1.0 / (d2.astype(np.float64) + np.float64(np.float32(1e-8)))
    s = t[..., :K - 1].sum(-1, keepdims=True) if mutant == "w_k_minus_1" else t.sum(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return t / s


def _group(c, d, mutant):
    B, N, npt, K, C, flags, ldg = c["B"], c["N"], c["np"], c["K"], c["C"], c["flags"], c["ldg"]
    idx = d["idx"].astype(np.int64)
    if mutant == "idx32_as_64":  # the low word of each 8-byte read: every second int32 (reads past the end wrapped)
        flat = idx.reshape(-1)
        idx = flat[(2 * np.arange(flat.size)) % flat.size].reshape(idx.shape)
    empty = (d["counts"] == 0) if c["counts"] else np.zeros((B, npt), bool)
    bi = np.arange(B)[:, None, None]
    ctr = np.broadcast_to(d["new_xyz"].astype(np.float64)[:, :, None, :], (B, npt, K, 3))
    q = np.where(empty[:, :, None, None], ctr, d["xyz"].astype(np.float64)[bi, idx])
    y = np.zeros((B, npt, K, ldg))
    b = np.zeros_like(y)
    if C:
        f = T(c, d["feat"]).reshape(B, N, -1)[bi, idx][..., :C]
        y[..., :C] = np.where(empty[:, :, None, None], 0.0, f)
    rel = (ctr - q) if mutant == "rel_sign" else (q - ctr)
    if flags & GROUP_FP:
        w = _fp_weight(d["d2"], K, mutant)
        y[..., C] = d["d2"]
        y[..., C + 1] = w
        b[..., C + 1] = (K + 12) * U * np.abs(w)
        y[..., C + 2:C + 5], y[..., C + 5:C + 8], y[..., C + 8:C + 11] = q, rel, ctr
        b[..., C + 5:C + 8] = U * np.abs(rel)
    elif not flags & GROUP_NO_XYZ:
        y[..., C:C + 3] = rel
        b[..., C:C + 3] = U * np.abs(rel)
        o = C + 3
        if flags & GROUP_ABS:
            y[..., o:o + 3] = q
            o += 3
        if flags & GROUP_CENTER:
            y[..., o:o + 3] = ctr
    return dict(out=dict(y=y.reshape(-1, ldg), b=b.reshape(-1, ldg)))


def gn_stats(c, d, mutant=None):
    """float64 group statistics of a GN case and their bounds: dict(m, rstd, var, dm, dr, n) each [B][G]"""
    B, S, ld, G, n_norm = c["B"], c["S"], c["ld"], c["G"], c["n_norm"]
    gs = n_norm // G
    n = S * gs
    src = T(c, d["x2"] if c["tiles"] else d["x"]).reshape(B, S, ld)
    if c["flags"] & GN_PRE_RELU and not (mutant == "stats_no_relu"):
        src = np.maximum(src, 0)
    if c["tiles"]:
        tps = S // 256
        s = d["tsum"].astype(np.float64).reshape(B, tps, ld).sum(1)
        q = d["tsq"].astype(np.float64).reshape(B, tps, ld).sum(1)
    else:
        s, q = src.sum(1), (src * src).sum(1)
        if mutant == "drop_last_row":
            s, q = s - src[:, -1], q - src[:, -1] ** 2
    g3 = lambda a: a[:, :n_norm].reshape(B, G, gs).sum(2)
    cnt = n
    if mutant == "count_rpc_nchunk":
        mp = gn_map(c["half"], ld, S)
        cnt = gs * mp["rpc"] * mp["nchunk"]
    m = g3(s) / cnt
    ex2 = g3(q) / cnt
    var = np.maximum(ex2 - m * m, 0)
    if mutant == "unbiased_var":
        var = var * n / (n - 1)
    rstd = 1 / np.sqrt(var + EPS)
    dd = np.ceil(np.log2(n)) + 2
    dm = (dd + 2) * U * g3(np.abs(src).sum(1)) / n
    dv = 4 * (dd + 2) * U * g3((src * src).sum(1)) / n
    dr = rstd * (0.6 * dv / (var + EPS) + 4 * U)
    if mutant == "neighbour_sample":
        m, rstd = np.roll(m, -1, 0), np.roll(rstd, -1, 0)
    return dict(m=m, rstd=rstd, var=var, dm=dm, dr=dr, n=n, gs=gs)


def _gn(c, d, mutant):
    B, S, ld, C, G, n_norm, flags = c["B"], c["S"], c["ld"], c["C"], c["G"], c["n_norm"], c["flags"]
    x = T(c, d["x"]).reshape(B, S, ld)
    xa = np.maximum(x, 0) if flags & GN_PRE_RELU else x
    y = xa.copy()
    b = np.zeros_like(y)
    outs = {}
    if G > 0:
        st = gn_stats(c, d, mutant)
        gs = st["gs"]
        ch = np.arange(n_norm) // gs
        e = lambda a: a[:, ch][:, None, :]  # [B][G] -> [B][1][n_norm]
        gam, bet = d["gamma"][:n_norm].astype(np.float64), d["beta"][:n_norm].astype(np.float64)
        m, rstd, dm, dr = e(st["m"]), e(st["rstd"]), e(st["dm"]), e(st["dr"])
        g = gam * rstd
        part = xa[:, :, :n_norm]
        y[:, :, :n_norm] = (part - m) * g + bet
        b[:, :, :n_norm] = (np.abs(gam) * rstd * dm + np.abs(gam) * np.abs(part - m) * dr +
                            3 * U * (np.abs(part * g) + np.abs(m * g) + np.abs(bet)))
        if mutant == "tail_normalised":
            y[:, :, n_norm] = (xa[:, :, n_norm] - st["m"][:, -1:]) * st["rstd"][:, -1:]
        # the published table [B][2][ld] and the statistics [B][64][2]
        sc, sh = np.ones((B, ld)), np.zeros((B, ld))
        dsc, dsh = np.zeros((B, ld)), np.zeros((B, ld))
        sc[:, :n_norm] = g[:, 0]
        sh[:, :n_norm] = bet - m[:, 0] * g[:, 0]
        dsc[:, :n_norm] = np.abs(gam) * dr[:, 0] + 2 * U * np.abs(g[:, 0])
        dsh[:, :n_norm] = (np.abs(m[:, 0]) * dsc[:, :n_norm] + np.abs(g[:, 0]) * dm[:, 0] +
                           3 * U * (np.abs(bet) + np.abs(m[:, 0] * g[:, 0])))
        outs["table"] = dict(y=np.stack([sc, sh], 1), b=np.stack([dsc, dsh], 1), typ="f32")
        mr = np.full((B, 64, 2), PREFILL)
        mb = np.zeros((B, 64, 2))
        mr[:, :G, 0], mr[:, :G, 1] = st["m"], st["rstd"]
        mb[:, :G, 0], mb[:, :G, 1] = st["dm"] + U * np.abs(st["m"]), st["dr"]
        outs["mr"] = dict(y=mr, b=mb, typ="f32")
    if flags & GN_POST_RELU:
        y = np.maximum(y, 0)
    extra = np.abs(y)
    if c["addvec_ld"]:
        av = np.zeros((B, 1, ld))
        av[:, 0, :c["addvec_ld"]] = d["addvec"]
        y = y + av
        extra = extra + np.abs(av)
    if c["res_ld"]:
        r = T(c, d["res"]).reshape(B, S, -1)[:, :, :ld]
        y = y + r
        extra = extra + np.abs(r)
    b = b + 4 * U * extra
    b[:, :, n_norm:] = np.where((c["addvec_ld"] > 0) | (c["res_ld"] > 0), b[:, :, n_norm:], 0.0)  # plain copies / ReLUs: exact
    outs["out"] = dict(y=y.reshape(B * S, ld), b=b.reshape(B * S, ld))
    return outs


def _gn_joint(c, d, mutant):
    B, npt, K, C1, C2, G, n_norm = c["B"], c["np_"], c["K"], c["C1"], c["C2"], c["G"], c["n_norm"]
    ldq, ldk = d["q"].shape[1], d["k"].shape[1]
    gs = n_norm // G
    Sk = npt * K
    n = Sk * gs
    mult = 1.0 if mutant == "q_once" else float(K)
    f = lambda a, w: a.astype(np.float64).reshape(B, -1, a.shape[1]).sum(1)[:, :w]
    s = np.concatenate([mult * f(d["qsum"], C1), f(d["ksum"], C2)], 1)
    q = np.concatenate([mult * f(d["qsq"], C1), f(d["ksq"], C2)], 1)
    g3 = lambda a: a[:, :n_norm].reshape(B, G, gs).sum(2)
    m = g3(s) / n
    var = np.maximum(g3(q) / n - m * m, 0)
    if mutant == "unbiased_var":
        var = var * n / (n - 1)
    rstd = 1 / np.sqrt(var + EPS)
    dd = np.ceil(np.log2(n)) + 2
    dm = (dd + 2) * U * g3(np.abs(s)) / n
    dv = 4 * (dd + 2) * U * g3(q) / n
    dr = rstd * (0.6 * dv / (var + EPS) + 4 * U)
    ch = np.arange(n_norm) // gs
    gam, bet = d["gamma"][:n_norm].astype(np.float64), d["beta"][:n_norm].astype(np.float64)
    C = C1 + C2
    sc, sh, dsc, dsh = np.ones((B, C)), np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, C))
    g = gam * rstd[:, ch]
    sc[:, :n_norm], sh[:, :n_norm] = g, bet - m[:, ch] * g
    dsc[:, :n_norm] = np.abs(gam) * dr[:, ch] + 2 * U * np.abs(g)
    dsh[:, :n_norm] = np.abs(m[:, ch]) * dsc[:, :n_norm] + np.abs(g) * dm[:, ch] + 3 * U * (np.abs(bet) + np.abs(m[:, ch] * g))

    def tab(lo, hi, ld):
        y, b = np.zeros((B, 2, ld)), np.zeros((B, 2, ld))
        y[:, 0] = 1.0
        y[:, 0, :hi - lo], y[:, 1, :hi - lo] = sc[:, lo:hi], sh[:, lo:hi]
        b[:, 0, :hi - lo], b[:, 1, :hi - lo] = dsc[:, lo:hi], dsh[:, lo:hi]
        return dict(y=y, b=b, typ="f32")
    return dict(ssq=tab(0, C1, ldq), ssk=tab(C1, C, ldk))


def joint_end_to_end(c, d):
    """float64 GroupNorm of the materialised relu([q x K | k]) and its NORM bound (no store): (yq [B*np][C1], yk [B*np*K][C2],
    bq, bk) -- what the two tables applied to the stored q and k must reproduce"""
    B, npt, K, C1, C2, G, n_norm = c["B"], c["np_"], c["K"], c["C1"], c["C2"], c["G"], c["n_norm"]
    q, k = T(c, d["q"])[:, :C1].reshape(B, npt, 1, C1), T(c, d["k"])[:, :C2].reshape(B, npt, K, C2)
    cat = np.concatenate([np.broadcast_to(q, (B, npt, K, C1)), k], 3).reshape(B, npt * K, C1 + C2)
    gs = n_norm // G
    n = npt * K * gs
    part = cat[:, :, :n_norm].reshape(B, npt * K, G, gs)
    m = part.mean((1, 3), keepdims=True)
    var = ((part - m) ** 2).mean((1, 3), keepdims=True)
    rstd = 1 / np.sqrt(var + EPS)
    dd = np.ceil(np.log2(n)) + 2
    dm = (dd + 2) * U * np.abs(part).mean((1, 3), keepdims=True)
    dv = 4 * (dd + 2) * U * (part * part).mean((1, 3), keepdims=True)
    dr = rstd * (0.6 * dv / (var + EPS) + 4 * U)
    gam, bet = d["gamma"][:n_norm].astype(np.float64).reshape(1, 1, G, gs), d["beta"][:n_norm].astype(np.float64).reshape(1, 1, G, gs)
    g = gam * rstd
    y, b = cat.copy(), np.zeros_like(cat)
    y[:, :, :n_norm] = ((part - m) * g + bet).reshape(B, npt * K, n_norm)
    b[:, :, :n_norm] = (np.abs(gam) * rstd * dm + np.abs(gam) * np.abs(part - m) * dr +
                        3 * U * (np.abs(part * g) + np.abs(m * g) + np.abs(bet))).reshape(B, npt * K, n_norm)
    y4, b4 = y.reshape(B, npt, K, -1), b.reshape(B, npt, K, -1)
    return y4[:, :, 0, :C1].reshape(-1, C1), y4[..., C1:].reshape(-1, C2), b4[:, :, 0, :C1].reshape(-1, C1), b4[..., C1:].reshape(-1, C2)


def _concat_qk(c, d, mutant):
    pts, K, C1, C2, ldo = c["pts"], c["K"], c["C1"], c["C2"], c["ldo"]
    q, k = T(c, d["q"]), T(c, d["k"])
    rows = np.arange(pts * K)
    qrow = rows % K if mutant == "q_row_mod" else rows // K
    y = np.zeros((pts * K, ldo))
    y[:, :C1] = q[qrow % pts][:, :C1]
    y[:, C1:C1 + C2] = k[:, :C2]
    if mutant == "seam_other_source":
        y[:, C1] = q[qrow][:, C1]
    return dict(out=dict(y=np.maximum(y, 0), b=np.zeros_like(y)))


def _slots(c, d, mutant):
    """[pts][K] bool: the slots that take part, by the kernel's rule n = max(1, min(K, count))"""
    pts, K = c["pts"], c["K"]
    n = np.full(pts, K)
    zero = np.zeros(pts, bool)
    if c["counts"]:
        n = np.clip(d["counts"], 1, K)
        if mutant == "slot_past_count":
            n = np.minimum(n + 1, K)
        if mutant == "zero_count_empty":
            zero = d["counts"] == 0
    return np.arange(K)[None] < n[:, None], n, zero


def _attn(c, d, mutant):
    pts, K, C, ldo = c["pts"], c["K"], c["C"], c["ldo"]
    mask, n, zero = _slots(c, d, mutant)
    mask = mask[:, :, None]
    s = T(c, d["S"]).reshape(pts, K, -1)[:, :, :ldo]
    v = T(c, d["V"]).reshape(pts, K, -1)[:, :, :ldo]
    extra = 0.0
    if c["vss"]:
        smp = np.arange(pts) // c["pps"]
        sc, sh = d["vss"].astype(np.float64)[smp, 0, None, :ldo], d["vss"].astype(np.float64)[smp, 1, None, :ldo]
        extra = 2 * (np.abs(v * sc) + np.abs(sh))
        v = v * sc + sh
        if c["v_relu"]:
            v = np.maximum(v, 0)
    v = np.where(mask, v, 0.0)
    sm = np.where(mask, s, -np.inf)
    mx = sm.max(1, keepdims=True)
    if mutant == "no_max_shift":  # in fp32, as the kernel would: exp overflows from 88.7 on
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(sm.astype(np.float32)).astype(np.float64)
            w = (e.astype(np.float32) / e.astype(np.float32).sum(1, keepdims=True)).astype(np.float64)
    else:
        e = np.exp(sm - mx)
        w = e / e.sum(1, keepdims=True)
    dk = np.where(mask, np.abs(s - mx), 0.0)
    with np.errstate(invalid="ignore"):
        y = (w * v).sum(1)
    W = (w * np.abs(v)).sum(1)
    b = ((2 * K + 8 + 2 * E_EXP) * W + (w * np.abs(v) * dk).sum(1) + W * (w * dk).sum(1) + (w * extra * mask).sum(1)) * U
    y[zero] = 0
    y[:, C:] = 0
    b[:, C:] = 0
    return dict(out=dict(y=y, b=np.nan_to_num(b)))


def _pool(c, d, mutant):
    pts, K, C, ldo, mode = c["pts"], c["K"], c["C"], c["ldo"], c["mode"]
    mask, n, zero = _slots(c, d, mutant)
    x = T(c, d["x"]).reshape(pts, K, -1)[:, :, :ldo]
    mx = np.where(mask[:, :, None], x, -np.inf).max(1) if mutant == "max_first_n" else x.max(1)
    avg = np.where(mask[:, :, None], x, 0).sum(1) / n[:, None]
    avg[zero] = 0
    ab = (K + 1) * U * np.where(mask[:, :, None], np.abs(x), 0).sum(1) / n[:, None]
    cols = np.arange(ldo)
    use_max = np.full(ldo, mode == POOL_MAX) | ((mode == POOL_MAX_AVG) & (cols < C // 2))
    y = np.where(use_max[None], mx, avg)
    b = np.where(use_max[None], 0.0, ab)
    y[:, C:] = 0
    b[:, C:] = 0
    return dict(out=dict(y=y, b=b))


def _pair_expand(c, d, mutant):
    B, N, npt, K, ld = c["B"], c["N"], c["np_"], c["K"], c["ld"]
    idx = d["idx"].astype(np.int64)
    src = (np.arange(B)[:, None, None] * N + idx).reshape(-1)
    A = d["A"].astype(np.float64)[src, :ld]
    ctr = np.repeat(d["new_xyz"].astype(np.float64).reshape(-1, 3), K, 0)
    coef = d["coef"].astype(np.float64)
    cc = coef[:, 3:6] + (d["w_rel"].astype(np.float64) if mutant == "cc_without_wrel" else 0.0)
    bias = d["bias"].astype(np.float64)
    t = A + bias + ctr @ cc.T
    mag = np.abs(A) + np.abs(bias) + np.abs(ctr) @ np.abs(cc).T
    b = np.zeros_like(t)
    if c["fp"]:
        d2 = d["d2"].astype(np.float64).reshape(-1, 1)
        w = _fp_weight(d["d2"], K).reshape(-1, 1)
        t = t + d2 * coef[:, 6] + w * coef[:, 7]
        mag = mag + np.abs(d2 * coef[:, 6]) + np.abs(w * coef[:, 7])
        b = b + (K + 12) * U * np.abs(w * coef[:, 7])
    b = b + 6 * U * mag
    if c["relu"]:
        t = np.maximum(t, 0)
    outs = dict(out=dict(y=t, b=b))
    if c["stats"]:
        rows = t.shape[0]
        nt = (rows + 255) // 256
        tp, bp = np.zeros((nt * 256, ld)), np.zeros((nt * 256, ld))
        tp[:rows], bp[:rows] = (r16(t) if mutant == "sums_of_rounded" else t), b
        tp, bp = tp.reshape(nt, 256, ld), bp.reshape(nt, 256, ld)
        tr = np.zeros((nt * 256, ld))
        tr[:rows] = t
        tr = tr.reshape(nt, 256, ld)
        dd = 8 + 2
        outs["sum"] = dict(y=tp.sum(1), b=bp.sum(1) + dd * U * np.abs(tr).sum(1) + 1e-300, typ="f32")
        outs["sq"] = dict(y=(tp * tp).sum(1), b=(2 * np.abs(tr) * bp + bp * bp).sum(1) + dd * U * (tr * tr).sum(1) + 1e-300, typ="f32")
    return outs


def _from_ncx(c, d, mutant):
    B, C, P = c["B"], c["C"], c["P"]
    ld = ru(C)
    y = np.full((B, P, ld), PREFILL if mutant == "pad_not_cleared" else 0.0)
    y[:, :, :C] = d["x"].astype(np.float64).transpose(0, 2, 1)
    return dict(out=dict(y=y.reshape(B * P, ld), b=np.zeros((B * P, ld))))


def _to_ncx(c, d, mutant):
    B, C, P = c["B"], c["C"], c["P"]
    y = T(c, d["rows"]).reshape(B, P, -1)[:, :, :C].transpose(0, 2, 1)
    return dict(out=dict(y=np.ascontiguousarray(y), b=np.zeros((B, C, P)), typ="f32"))


_FORWARD = dict(from_ncx=_from_ncx, to_ncx=_to_ncx, group=_group, gn=_gn, gn_joint=_gn_joint, concat_qk=_concat_qk, attn=_attn,
                pool=_pool, pair_expand=_pair_expand)


def store(o, half):
    """the store term of an output dict(y, b): adds `stored` (y rounded to the stored type) and widens b where it is not 0 (exact)"""
    y = o["y"]
    b = np.broadcast_to(np.asarray(o["b"], np.float64), y.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        if half:
            o["stored"] = r16(y)
            o["b"] = np.where(b > 0, b * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(y) + 2.0 ** -25, 0.0)
        else:
            o["stored"] = r32(y)
            o["b"] = np.where(b > 0, b + U * np.abs(y), 0.0)
    return o


def forward(c, d, mutant=None):
    """float64 reference of the case (or of one of its mutants): {output name: dict(y, b, stored)}; b already holds the store
    term of the output's type, and is 0 where the element must be exact"""
    outs = _FORWARD[c["op"]](c, d, mutant)
    for o in outs.values():
        store(o, o.get("typ", "rows") == "rows" and c["half"])
    return outs


def ratio(o, got):
    """elementwise err / tol of `got` against a reference output: exact elements give 0 or inf"""
    got = np.asarray(got, np.float64)
    assert got.shape == o["y"].shape, (got.shape, o["y"].shape)
    exact = o["b"] == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(exact, np.where(got == o["stored"], 0.0, np.inf), np.abs(got - o["y"]) / np.where(exact, 1.0, o["b"]))
    return np.where(np.isfinite(got), r, np.inf)
