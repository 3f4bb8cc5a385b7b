"""The case matrix of the training backward kernels (csrc/train_ops.hip, include/slide_train.h, slide_amd/train/functions.py), its
float64 references, its error bounds and its mutants -- shared by tests/test_hip_train_arith.py (every case on the GPU against
the reference, and, on the CPU, every bound against the mutants).  The companion of tests/rows_cases.py (the forward kernels of the
same layers) and tests/gemm_cases.py; U, EPS, E_EXP, PREFILL, r32, ru, ratio, the store term (rows_cases.store) and GroupNorm's
forward bound (rows_cases.gn_stats / _gn) are theirs.

A reference takes the operands as the kernel reads them -- fp32 inputs widened to float64, int tables as passed -- and is numpy
float64 written from the semantics in the comments of train_ops.hip and slide_train.h; nothing of the code under test is called.
Every output buffer holds PREFILL before the launch, so an element the contract leaves alone must still hold it.

Bounds, elementwise (u = 2^-24; a bound of 0 marks an element that must be EXACT; rows_cases.store adds u |ref| to the others).
  GN bwd   z = relu?(x), n = (z - mean) rstd: one subtraction, one product: dn = 2 u |n| (+ the statistics term below).
           dg = dy [g > 0] is a move.  s1 = sum_rows dg, s2 = sum_rows dg n are chains of S links (rows of a thread, rt threads,
           <= 64 chunks); with the chain convention of rows_cases.py, d = ceil(log2 S) + 2:
             B1 = (d + 2) u sum|dg|            B2 = (d + 5) u sum|dg n| + sum|dg| dn_s       (3 u: n and the product)
           dbeta = s1 and dgamma = s2 per sample, exactly 0 past n_norm.  The group means m1 = sum_c gamma_c s1_c / n and m2
           (from s2), n = gs S: one product per channel, gs - 1 additions (dgs = ceil(log2 gs) + 2), 1 / n and a product:
             Bm = [ sum_c |gamma_c| B_c + (dgs + 3) u sum_c |gamma_c s_c| ] / n
           dx = rstd (dg gamma - m1 - n m2): t1 = dg gamma (u), t2 = t1 - m1 (u), t3 = n m2 (3 u), t4 = t2 - t3 (u), the last
           product is the store:
             b = rstd [ Bm1 + |n| Bm2 + 4 u (|dg gamma| + |m1| + |n m2|) ] + |m2| rstd dn_s + |t4| dr_s
           and dx is exactly 0 where the pre-ReLU masks it; pass-through channels and pad columns are moves (dy or 0): exact.
           mean_rstd is an INPUT: the C-ABI cases feed the float64 statistics rounded to fp32 and the reference reads those fp32
           values, so dn_s = dr_s = 0 and the bound concerns the backward alone.  The `wrap` cases run GroupNormRows, whose backward
           reads the forward's own statistics: the reference uses the float64 statistics and carries the forward's published
           mean / rstd bound of rows_cases.py (dm + u |m|, dr): dn_s = rstd dm' + |z - m| dr, dr_s = dr.  Through the Function
           dgamma / dbeta are summed over the batch by slide_col_sums: the per-sample bounds add, plus the column-sum bound over B.
           ReLU masks: the kernel recomputes g = n gamma + beta > 0 in fp32; make_data redraws every element whose float64 g lies
           within the forward bound b' (+ 5 u |g|, what rows_cases._gn adds for the epilogue and the store) of 0, until none is left
           (`ambiguous` counts them: the cap is 0).  x > 0 is a comparison of an input: always decidable.  Planted exact zeros:
           x == 0, and gamma == beta == 0 (g == 0 in both arithmetics: gradient 0 by the > 0 convention).
  col_sums a chain over the rows (rows of a thread, rt threads; then 32 rows of partials per thread, 32 threads):
           b = (d + 2) u sum|x|, d = ceil(log2 rows) + 2; rows = 0: exactly 0.
  group    atomics: the order is not fixed, so the order-free bound: an element with T terms (its initial value and the T - 1
           gradient rows that land on it) has b = (T - 1) u sum|terms|; T = 1 (never indexed, a channel >= C, an empty ball's
           rows only): exactly as initialised.
  concat   dk is a masked move: exact, columns >= C2 untouched.  dq = the K masked terms added in ascending k from 0 (the first
           addition is exact): b = (K - 1) u sum|terms|; deterministic: two launches are bit-equal.  Columns >= C1 untouched.
  attn     over the first cnt = max(1, min(K, count)) slots: e_k = expf(s_k - max) carries (d_k + E_EXP) u, d_k = |s_k - max| (the
           subtraction rounds once); den = sum e_j: sum_j w_j (d_j + E) u and cnt - 1 additions; the division 3 u:
             rho_k = d_k + E + sum_j w_j (d_j + E) + cnt + 2,         dw_k = rho_k u w_k + ETA
           ETA = 2^-126: a weight below fp32's normal range may be flushed or rounded as a denormal (exp(-120), exp(-200)).
           o = num / den, num = sum e_k v_k (one product, cnt - 1 additions), W = sum w_k |v_k|:
             Bo = u [ sum_k w_k |v_k| (d_k + E + cnt) + W (sum_j w_j (d_j + E) + cnt + 2) ]
           dv_k = w_k dout: b = dw_k |dout| + ETA;   ds_k = w_k (v_k - o) dout, t = v_k - o (u), two products (one is the store):
             b = |dout| [ dw_k |t| + w_k (Bo + 2 u |t|) ] + ETA
           Slots past the count are exactly 0 in ds and dv; columns >= C untouched; K = 1: ds exactly 0, dv = dout exactly
           (expf(0) = 1, 1 / 1 = 1, v / 1 = v).
           exp(60) = 1.1e26 is inside fp32's range: the softmax without the max shift is still right at +-60 and overflows at
           +-100, which is the case that shows that mutant (EXEMPT).
  ConvRows y = x W^T + bias and dx = dy W: the split-arithmetic RAW bound of gemm_cases.py, b = C_ACC (|x| |W|^T + |bias|); pad
           columns exactly 0.  dW = dy^T x is a library GEMM over the rows: the plain dot-product bound (rows + 2) u sum|dy||x|
           (row slabs added in any order stay inside it).  db: the col_sums bound.  (rows + 2) u is 0.4 % at 65536 rows: that case
           draws positive dy and x, so that one slab of 64 is 1.6 % of every element and `dw_drop_last_slab` is seen there as well.

Mutants (test_bounds_see_the_mutants): the nearest wrong arithmetic, applied to the float64 reference and rounded to fp32.
  GN bwd    count_rpc_nchunk | drop_last_row | neighbour_sample | no_m2_term | post_mask_from_x | no_pre_mask | tail_normalised |
            tail_no_mask | dgamma_dbeta_swapped | dn_without_gamma
  col_sums  drop_last_row | drop_last_chunk (the last that holds rows) | second_stage_first_32 | rpc_floor (rows per chunk rounded down)
  group     zero_count_receives | batch_stride_np | tail_channels_dropped | strides_swapped
  concat    mask_from_dout | q_sum_K_minus_1 | seam_off_by_one | q_row_mod
  attn      slot_past_count | zero_count_empty | no_out_term | no_max_shift (in fp32)
  ConvRows  dw_drop_last_slab | db_drop_last_row

Measured on an MI355X (one run, every value <= 1; the worst err / bound over the elements of every case of the op):
  gn_bwd 0.33 (C-ABI; 0.19 ... 0.33 over the normalised cases, the G = 0 cases are exact)   | through GroupNormRows 0.091
  col_sums 0.22   | group_bwd 0.57   | concat_bwd 0.32   | attn_bwd 0.46   | ConvRows 0.15 (y, dx, dW, db together)
No op sits below 0.01: no bound could shrink by more than 2 ... 7 x without refusing the kernels (the nearest mutant of a single
case is 4.2 bounds away: dw_drop_last_slab at 65536 rows; col_sums drop_last_row at 140001 rows 5.6), and none was changed after the run.  Single CASES sit lower, for reasons of
the case and not of the bound: col_sums at 65536 / 70001 rows 0.002 (the chain convention is linear in d = ceil(log2 rows) + 2 on
sum|x|, the rounding errors of 65536 zero-mean terms add like a random walk; the same bound is at 0.13 on the common-offset 140001
rows, where they do not cancel), group_bwd one-point 0.006 (592 terms on one element: the order-free bound is linear in the terms,
any order's error is not), attn_bwd at +-60 / +-100 < 1e-14 (every weight is 0 or 1 to fp32: those cases are there for the shift).
The suite is 88 GPU tests (75 C-ABI cases, 12 Function cases, the zero-row test) and 3 CPU tests: the GPU half ran in 4.4 s, next to
4.4 s for the 183 GPU tests of tests/test_hip_rows_arith.py in the same run; no test above 1 s.  Each GPU test prints
"WORST <op> <case> <err / bound>"."""
import zlib

import numpy as np

import rows_cases as RC
from gemm_cases import C_ACC
from rows_cases import E_EXP, EPS, PREFILL, U, r32, ratio, ru  # noqa: F401  (re-exported to the test module)

ETA = 2.0 ** -126
OPS = ("gn_bwd", "col_sums", "group_bwd", "concat_bwd", "attn_bwd", "conv")


def gn_bwd_map(ld, S):
    """slide_gn_rows_bwd's thread map (train_ops.hip): cn threads per row, rt rows in flight, nchunk chunks of rpc rows"""
    cn = ld // 4
    rt = 256 // cn
    raw = (S + rt * 4 - 1) // (rt * 4)
    nchunk = min(64, max(1, raw))
    rpc = (S + nchunk - 1) // nchunk
    nchunk = (S + rpc - 1) // rpc
    return dict(cn=cn, rt=rt, idle=256 - rt * cn, nchunk=nchunk, rpc=rpc, clamped=raw > 64, last_short=rpc * nchunk != S)


def col_sums_map(rows, ld):
    """slide_col_sums' stage map: one launch of 32-column stripes below 128 rows, else row chunks + stripes over the partials"""
    raw = rows // 64
    nchunk = min(1024, max(1, raw))
    rpc = (rows + nchunk - 1) // nchunk
    two = nchunk > 1
    return dict(stages=2 if two else 1, nchunk=nchunk, rpc=max(rpc, 1), clamped=raw > 1024, ragged=rpc * nchunk != rows,
                rt=256 // (ld // 4) if two else 32, partial_rows_per_thread=(nchunk + 31) // 32 if two else 0)


def conv_map(rows, I, O):
    """functions.py: the row slabs of the weight gradient and the GEMM tile form of the forward / data-gradient launches"""
    slabs = 1
    while slabs < 64 and rows % (slabs * 2) == 0 and rows // (slabs * 2) >= 256:
        slabs *= 2
    npx = lambda n_cob: 4 if ((rows + 255) // 256) * ((n_cob + 1) // 2) < 256 else 8
    return dict(slabs=slabs, npx_fwd=npx(ru(O) // 32), npx_bwd=npx(ru(I) // 32))


# --------------------------------------------------------------------------------------------------------------- the matrix
CASES = []


def _add(op, name, **kw):
    c = dict(op=op, name="%s_%s" % (op, name), status=0, wrap=False, half=False)
    c.update(kw)
    CASES.append(c)


# 1. GroupNorm backward.  `tiles`, `half` and the forward-only keys make a case readable by rows_cases.gn_stats / _gn.
_gn = dict(B=3, G=32, flags=0, dist="normal", stats="input", gzero=False, tiles=False, addvec_ld=0, res_ld=0)
for _n, _kw in (
        ("ld32_s1", dict(ld=32, C=24, S=1, G=1, n_norm=24)),
        ("ld32_s16_b33", dict(ld=32, C=32, S=16, B=33, n_norm=32, flags=2)),
        ("ld32_s40_straddle", dict(ld=32, C=22, S=40, G=6, n_norm=18, flags=1)),
        ("ld32_s4096_straddle", dict(ld=32, C=31, S=4096, B=2, G=10, n_norm=30, flags=3)),
        ("ld96_s40_tail", dict(ld=96, C=70, S=40, n_norm=64, flags=1, gzero=True)),
        ("ld96_s40_common", dict(ld=96, C=64, S=40, G=64, n_norm=64, flags=2, dist="common")),
        ("ld96_s255_g1", dict(ld=96, C=96, S=255, G=1, n_norm=96, flags=3)),
        ("ld128_s256", dict(ld=128, C=128, S=256, G=64, n_norm=128, flags=3, gzero=True)),
        ("ld128_s257_zero", dict(ld=128, C=100, S=257, n_norm=96, flags=2, dist="zero_sample", gzero=True)),
        ("ld128_s4100_clamp", dict(ld=128, C=128, S=4100, B=2, G=8, n_norm=128, flags=1)),
        ("ld544_s255", dict(ld=544, C=515, S=255, B=2, n_norm=512, flags=2)),
        ("ld1024_s16", dict(ld=1024, C=1024, S=16, B=2, G=64, n_norm=1024)),
        ("ld1024_s301_clamp", dict(ld=1024, C=1000, S=301, B=2, G=1, n_norm=1000, flags=0)),
        ("g0_f0", dict(ld=96, C=70, S=40, G=0, n_norm=0, flags=0)), ("g0_f1", dict(ld=96, C=70, S=40, G=0, n_norm=0, flags=1)),
        ("g0_f2", dict(ld=96, C=70, S=257, G=0, n_norm=0, flags=2)), ("g0_f3", dict(ld=96, C=70, S=40, G=0, n_norm=0, flags=3)),
        ("wrap_f0", dict(ld=96, C=70, S=40, n_norm=64, flags=0, stats="forward", wrap=True)),
        ("wrap_f1", dict(ld=96, C=70, S=40, n_norm=64, flags=1, stats="forward", wrap=True)),
        ("wrap_f2", dict(ld=96, C=70, S=40, n_norm=64, flags=2, stats="forward", wrap=True)),
        ("wrap_f3", dict(ld=128, C=128, S=257, G=64, n_norm=128, flags=3, stats="forward", wrap=True))):
    _c = dict(_gn)
    _c.update(_kw)
    _add("gn_bwd", _n, **_c)
# every clause of the argument check, and a NULL among the pointers G > 0 requires
for _n, _kw in (("bad_ld_mod32", dict(ld=48)), ("bad_ld_1056", dict(ld=1056)), ("bad_ld_0", dict(ld=0, G=0, n_norm=0)), ("bad_g_neg", dict(G=-1)), ("bad_g_65", dict(G=65, n_norm=65)),
                ("bad_nnorm_neg", dict(n_norm=-32)), ("bad_nnorm_gt_ld", dict(n_norm=128)), ("bad_nnorm_mod_g", dict(n_norm=65)),
                ("bad_g0_nnorm", dict(G=0)), ("bad_null_mr", dict(null="mr")), ("bad_null_scratch", dict(null="scratch")),
                ("bad_null_gamma", dict(null="gamma")), ("bad_null_beta", dict(null="beta")), ("bad_null_dgamma", dict(null="dgamma")),
                ("bad_null_dbeta", dict(null="dbeta"))):
    _c = dict(_gn, ld=96, C=70, S=40, n_norm=64, flags=3, status=-3, null=None)
    _c.update(_kw)
    _add("gn_bwd", _n, **_c)

# 2. column sums
for _rows, _ld, _kw in ((0, 32, {}), (1, 128, {}), (5, 544, {}), (63, 1024, {}), (64, 32, {}), (127, 128, dict(scratch=False)),
                        (128, 544, {}), (129, 1024, {}), (4096, 128, dict(dist="common")), (65536, 32, {}), (70001, 32, {}),
                        (140001, 32, dict(dist="common")), (5, 32, dict(dist="common", scratch=False))):
    _c = dict(rows=_rows, ld=_ld, dist="normal", scratch=True)
    _c.update(_kw)
    _add("col_sums", "r%d_ld%d" % (_rows, _ld), **_c)
_add("col_sums", "bad_null_scratch_r128", rows=128, ld=32, dist="normal", scratch=False, status=-3)
_add("col_sums", "bad_ld_mod32", rows=64, ld=48, dist="normal", scratch=True, status=-3)
_add("col_sums", "bad_ld_1056", rows=64, ld=1056, dist="normal", scratch=True, status=-3)
_add("col_sums", "bad_ld_0", rows=64, ld=0, dist="normal", scratch=True, status=-3)
_add("col_sums", "bad_rows_neg", rows=-1, ld=32, dist="normal", scratch=True, status=-3)

# 3. grouping backward
for _n, _kw in (("c1_k1", dict(C=1, K=1, ldf=32, ldg=64)),
                ("c5_k5_counts", dict(C=5, K=5, ldf=64, ldg=32, counts=True)),
                ("c8_k16", dict(C=8, K=16, ldf=32, ldg=32, init=0.0)),
                ("c13_k5_counts", dict(C=13, K=5, ldf=32, ldg=96, counts=True)),
                ("c64_k16", dict(C=64, K=16, ldf=96, ldg=64)),
                ("c13_k16_onepoint", dict(C=13, K=16, ldf=64, ldg=32, onepoint=True)),
                ("c5_k5_n_lt_np", dict(C=5, K=5, N=7, np=20, ldf=32, ldg=64, B=3)),
                ("wrap", dict(C=13, K=5, ldf=32, ldg=32, init=0.0, wrap=True))):
    _c = dict(B=2, N=37, np=11, counts=False, onepoint=False, init=PREFILL)
    _c.update(_kw)
    _add("group_bwd", _n, **_c)

# 4. relu([q | k]) backward
for _C1, _C2, _K in ((3, 12, 1), (4, 60, 8), (8, 139, 16), (51, 12, 8), (256, 60, 1), (8, 60, 16)):
    _add("concat_bwd", "c%d_c%d_k%d" % (_C1, _C2, _K), pts=37, K=_K, C1=_C1, C2=_C2, ldq=ru(_C1) + 64, ldk=ru(_C2) + 32, ldo=ru(_C1 + _C2))
_add("concat_bwd", "wrap", pts=37, K=8, C1=51, C2=60, ldq=64, ldk=64, ldo=128, wrap=True)

# 5. softmax + weighted sum backward
for _n, _kw in (("k1", dict(K=1, C=20, lds=96, ldv=64, ldo=32)),
                ("k1_counts", dict(K=1, C=20, lds=96, ldv=64, ldo=32, counts=True)),
                ("k4_counts", dict(K=4, C=51, lds=128, ldv=96, ldo=64, counts=True)),
                ("k16", dict(K=16, C=51, lds=96, ldv=128, ldo=64)),
                ("k16_counts", dict(K=16, C=60, lds=128, ldv=96, ldo=64, counts=True)),
                ("k48_counts", dict(K=48, C=33, lds=160, ldv=96, ldo=64, counts=True)),
                ("k48", dict(K=48, C=64, lds=96, ldv=128, ldo=64)),
                ("k16_pm60", dict(K=16, C=51, lds=96, ldv=128, ldo=64, dist="pm60")),
                ("k16_pm100", dict(K=16, C=51, lds=96, ldv=128, ldo=64, dist="pm100")),
                ("wrap", dict(K=16, C=51, lds=64, ldv=64, ldo=64, wrap=True))):
    _c = dict(pts=24, counts=False, dist="normal")
    _c.update(_kw)
    _add("attn_bwd", _n, **_c)

# 6. ConvRows (Function level only)
for _rows, _I, _O, _bias, _dist in ((16, 3, 51, True, "normal"), (510, 45, 70, False, "normal"), (512, 131, 128, True, "normal"),
                                    (1283, 515, 256, False, "normal"), (65536, 45, 70, True, "positive")):
    _add("conv", "r%d_i%d_o%d" % (_rows, _I, _O), rows=_rows, I=_I, O=_O, bias=_bias, dist=_dist, wrap=True)

CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# (case, mutant) -> the case of the same op where that mutant IS visible
EXEMPT = {
    # exp(60) is inside fp32's range (docstring, attn)
    ("attn_bwd_k16_pm60", "no_max_shift"): "attn_bwd_k16_pm100",
}


def mutants(c):
    op = c["op"]
    if c["status"] != 0:
        return []
    if op == "gn_bwd":
        m = []
        if c["G"] > 0:
            m += ["drop_last_row", "no_m2_term", "dgamma_dbeta_swapped", "dn_without_gamma"]
            if gn_bwd_map(c["ld"], c["S"])["last_short"]:
                m.append("count_rpc_nchunk")
            if c["B"] > 1:
                m.append("neighbour_sample")
            if c["flags"] & 2:
                m.append("post_mask_from_x")
            if c["n_norm"] < c["C"]:
                m.append("tail_normalised")
        if c["flags"] & 1 and c["G"] > 0:
            m.append("no_pre_mask")
        if c["flags"] & 3 and c["n_norm"] < c["C"]:
            m.append("tail_no_mask")
        return m
    if op == "col_sums":
        mp = col_sums_map(c["rows"], c["ld"])
        m = ["drop_last_row"] if c["rows"] > 0 else []
        if mp["stages"] == 2:
            m.append("drop_last_chunk")
            if mp["nchunk"] > 32:
                m.append("second_stage_first_32")
            if mp["ragged"]:
                m.append("rpc_floor")
        return m
    if op == "group_bwd":
        m = ["zero_count_receives"] if c["counts"] else []
        if c["B"] > 1 and c["N"] != c["np"]:
            m.append("batch_stride_np")
        if c["C"] % 4:
            m.append("tail_channels_dropped")
        if c["ldf"] != c["ldg"]:
            m.append("strides_swapped")
        return m
    if op == "concat_bwd":
        return ["mask_from_dout", "seam_off_by_one"] + (["q_sum_K_minus_1", "q_row_mod"] if c["K"] > 1 else [])
    if op == "attn_bwd":
        return ((["slot_past_count", "zero_count_empty"] if c["counts"] and c["K"] > 1 else []) +
                (["zero_count_empty"] if c["counts"] and c["K"] == 1 else []) +
                (["no_out_term"] if c["K"] > 1 else []) + (["no_max_shift"] if c["dist"] != "normal" else []))
    if op == "conv":
        return (["dw_drop_last_slab"] if conv_map(c["rows"], c["I"], c["O"])["slabs"] > 1 else []) + (["db_drop_last_row"] if c["bias"] else [])
    return []


def reach(c):
    """the launcher's branch values of a case, by the launcher's own formulas (train_ops.hip, functions.py)"""
    op = c["op"]
    r = dict(op=op, status=c["status"], wrap=c["wrap"])
    if op == "gn_bwd":
        if c["ld"] % 32 == 0 and 0 < c["ld"] <= 1024:
            r.update(gn_bwd_map(c["ld"], c["S"]))
        G, n_norm = c["G"], c["n_norm"]
        r.update(ld=c["ld"], S=c["S"], B=c["B"], G=G, flags=c["flags"], gs=n_norm // G if G > 0 and n_norm > 0 else 0,
                 tail=G > 0 and n_norm < c["C"], straddle=G > 0 and n_norm % 4 != 0, full=G > 0 and n_norm == c["C"], dist=c["dist"],
                 gzero=c["gzero"], stats=c["stats"], null=c.get("null"))
    elif op == "col_sums":
        if c["ld"] % 32 == 0 and 0 < c["ld"] <= 1024 and c["rows"] >= 0:
            r.update(col_sums_map(c["rows"], c["ld"]))
        r.update(rows=c["rows"], ld=c["ld"], scratch=c["scratch"], dist=c["dist"])
    elif op == "group_bwd":
        r.update(C=c["C"], K=c["K"], B=c["B"], n_ne_np=c["N"] != c["np"], ld_differ=c["ldf"] != c["ldg"], counts=c["counts"],
                 onepoint=c["onepoint"], tail_channels=c["C"] % 4, init=c["init"])
    elif op == "concat_bwd":
        r.update(C1=c["C1"], C2=c["C2"], K=c["K"], strides_differ=len({c["ldq"], c["ldk"], c["ldo"]}) == 3)
    elif op == "attn_bwd":
        r.update(K=c["K"], counts=c["counts"], dist=c["dist"], strides_differ=len({c["lds"], c["ldv"], c["ldo"]}) == 3,
                 pad=c["C"] < min(c["lds"], c["ldv"], c["ldo"]))
    elif op == "conv":
        r.update(conv_map(c["rows"], c["I"], c["O"]))
        r.update(rows=c["rows"], I=c["I"], O=c["O"], bias=c["bias"])
    return r


# ------------------------------------------------------------------------------------------------------------------ data
def _rs(c):
    return np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)


def _gn_fwd_case(c):
    """the case as rows_cases reads it: the forward up to g = n gamma + beta (pre-ReLU kept, post-ReLU and epilogue off)"""
    return dict(c, op="gn", flags=c["flags"] & 1)


def _gn_planted(c, d):
    """[n_norm] bool: channels with gamma == beta == 0 (g == 0 exactly in fp32 and in float64)"""
    n = c["n_norm"]
    return (d["gamma"][:n] == 0) & (d["beta"][:n] == 0)


def _gn_ambiguous(c, d):
    """[B*S][n_norm] bool: elements whose post-ReLU mask g > 0 the fp32 kernel may decide differently from float64"""
    if not (c["G"] > 0 and c["flags"] & 2):
        return np.zeros((c["B"] * c["S"], max(c["n_norm"], 0)), bool)
    o = RC._gn(_gn_fwd_case(c), d, None)["out"]
    n = c["n_norm"]
    return (np.abs(o["y"][:, :n]) <= o["b"][:, :n] + U * np.abs(o["y"][:, :n])) & ~_gn_planted(c, d)[None]


def ambiguous(c, d):
    """the number of elements of a GN case that the comparison would have to exclude (must be 0)"""
    n = int(_gn_ambiguous(c, d).sum())
    if c["flags"] & 1:  # x > 0 compares an input: only a denormal could be read differently (flushed)
        n += int(((d["x"] != 0) & (np.abs(d["x"]) < 2.0 ** -126)).sum())
    return n


def _gn_mr(c, d):
    """mean_rstd [B][64][2] as the forward publishes it: the float64 statistics rounded to fp32; unused groups hold PREFILL"""
    mr = np.full((c["B"], 64, 2), PREFILL, np.float32)
    if c["G"] > 0:
        st = RC.gn_stats(_gn_fwd_case(c), d)
        mr[:, :c["G"], 0], mr[:, :c["G"], 1] = st["m"], st["rstd"]
    return mr


def make_data(c):
    """the case's inputs in the PHYSICAL layouts the entry point reads -- deterministic per case name"""
    rs = _rs(c)
    op = c["op"]
    d = {}
    if op == "gn_bwd":
        B, S, ld, C, n_norm = c["B"], c["S"], c["ld"], c["C"], max(c["n_norm"], 0)
        ld = ld if ld % 32 == 0 and ld > 0 else max(ru(ld), 32)
        C = min(C, ld)
        x = RC._mat(rs, B * S, C, ld, pad="zero")
        off = np.float32(30.0 if c["dist"] == "common" else 0.0)
        x[:, :C] += off
        if c["dist"] == "zero_sample":
            x[S:2 * S] = 0
        x[::7, 1] = 0   # planted exact zeros: a normalised channel, and a pass-through one where there is one
        x[3::5, C - 1] = 0
        planted = np.zeros(x.shape, bool)   # the redraw below leaves these alone
        planted[::7, 1] = planted[3::5, C - 1] = True
        if c["dist"] == "zero_sample":
            planted[S:2 * S] = True
        d["x"] = x
        gam = (1 + 0.2 * rs.standard_normal(max(n_norm, 1))).astype(np.float32)
        bet = (0.2 * rs.standard_normal(max(n_norm, 1))).astype(np.float32)
        if c["gzero"]:
            gam[[2, 9]], bet[2] = 0, 0   # channel 2: gamma == beta == 0; channel 9: gamma == 0 alone (g = beta)
        d["gamma"], d["beta"] = gam, bet
        d["dy"] = rs.standard_normal((B * S, ld)).astype(np.float32)  # (pad columns too: dx is written in full)
        if c["status"] == 0:
            for _ in range(20):
                amb = _gn_ambiguous(c, d) & ~planted[:, :n_norm]
                if not amb.any():
                    break
                x[:, :n_norm][amb] = (rs.standard_normal(int(amb.sum())) + off).astype(np.float32)
            else:
                raise AssertionError("%s: undecidable ReLU masks remain" % c["name"])
        d["mr"] = _gn_mr(c, d) if c["status"] == 0 else np.full((B, 64, 2), 1.0, np.float32)
    elif op == "col_sums":
        rows, ld = max(c["rows"], 0), c["ld"] if c["ld"] > 0 else 32   # (a refused ld never launches)
        x = rs.standard_normal((rows, ld)).astype(np.float32)
        if c["dist"] == "common":
            x += np.float32(30.0)
        d["x"] = x
    elif op == "group_bwd":
        B, N, npt, K = c["B"], c["N"], c["np"], c["K"]
        idx = rs.randint(0, N, (B, npt, K))
        idx[:, 0, 0], idx[:, 1, -1] = 0, N - 1
        idx[idx == 5] = 6   # row 5 of every sample is never indexed
        if K > 1:
            idx[:, 2, 1] = idx[:, 2, 0]
        if c["onepoint"]:
            idx[:] = 3
        d["idx"] = idx.astype(np.int64)
        if c["counts"]:
            cnt = rs.randint(0, K + 1, (B, npt)).astype(np.int32)
            cnt[:, 3], cnt[0, 0], cnt[:, 4] = 0, 0, K
            d["counts"] = cnt
        d["dout"] = rs.standard_normal((B * npt * K, c["ldg"])).astype(np.float32)
        if c["wrap"]:
            d["xyz"] = rs.uniform(0, 1, (B, N, 3)).astype(np.float32)
            d["new_xyz"] = rs.uniform(0, 1, (B, npt, 3)).astype(np.float32)
            d["feat"] = RC._mat(rs, B * N, c["C"], c["ldf"], pad="zero")
    elif op == "concat_bwd":
        pts, K, C1, C2, ldo = c["pts"], c["K"], c["C1"], c["C2"], c["ldo"]
        d["q"] = RC._mat(rs, pts, C1, c["ldq"], pad="zero")
        d["k"] = RC._mat(rs, pts * K, C2, c["ldk"], pad="zero")
        out = np.zeros((pts * K, ldo), np.float32) if c["wrap"] else rs.uniform(1.0, 2.0, (pts * K, ldo)).astype(np.float32)
        out[:, :C1] = np.maximum(np.repeat(d["q"][:, :C1], K, 0), 0)   # the forward's output: a move, about half of it exact zeros
        out[:, C1:C1 + C2] = np.maximum(d["k"][:, :C2], 0)
        d["out"] = out
        d["dout"] = rs.standard_normal((pts * K, ldo)).astype(np.float32)
    elif op == "attn_bwd":
        pts, K = c["pts"], c["K"]
        s = RC._mat(rs, pts * K, c["lds"], c["lds"], scale=2.0)
        if c["dist"] in ("pm60", "pm100"):
            a = 60.0 if c["dist"] == "pm60" else 100.0
            s[:] = -a
            top = rs.randint(0, K, (pts, c["lds"]))
            s.reshape(pts, K, -1)[np.arange(pts)[:, None], top, np.arange(c["lds"])[None]] = a
        v = RC._mat(rs, pts * K, c["ldv"], c["ldv"])
        if c["counts"]:
            d["counts"] = RC._counts(rs, pts, K)
            masked = (np.arange(K)[None] >= np.clip(d["counts"], 1, K)[:, None]).reshape(-1)
            s[masked] = 30.0    # the largest score of the point: a maximum over all K slots is seen
            v[masked] = 1e30    # finite but huge: any weight but exactly 0 leaves a trace
        d["S"], d["V"] = s, v
        d["dout"] = rs.standard_normal((pts, c["ldo"])).astype(np.float32)
    elif op == "conv":
        rows, I, O = c["rows"], c["I"], c["O"]
        pos = c["dist"] == "positive"
        f = (lambda *s: rs.uniform(0.5, 1.5, s).astype(np.float32)) if pos else (lambda *s: rs.standard_normal(s).astype(np.float32))
        x, dy = np.zeros((rows, ru(I)), np.float32), np.zeros((rows, ru(O)), np.float32)
        x[:, :I], dy[:, :O] = f(rows, I), f(rows, O)
        d["x"], d["dy"] = x, dy
        d["W"] = (rs.standard_normal((O, I)) / np.sqrt(I)).astype(np.float32)
        d["bias"] = rs.standard_normal(O).astype(np.float32) if c["bias"] else None
    return d


# ------------------------------------------------------------------------------------------------------------- references
def _gn_bwd(c, d, mutant):
    B, S, ld, C, G, n_norm, flags = c["B"], c["S"], c["ld"], c["C"], c["G"], c["n_norm"], c["flags"]
    pre, post = bool(flags & 1), bool(flags & 2)
    x = d["x"].astype(np.float64).reshape(B, S, ld)
    dy = d["dy"].astype(np.float64).reshape(B, S, ld)
    # pass-through channels and pad columns: y = relu?(relu?(x)), a move
    dx = np.where(x > 0, dy, 0.0) if (flags & 3 and mutant != "tail_no_mask") else dy.copy()
    bdx = np.zeros_like(dx)
    outs = {}
    if G > 0:
        gs = n_norm // G
        n = S * gs
        ch = np.arange(n_norm) // gs
        gam, bet = d["gamma"][:n_norm].astype(np.float64), d["beta"][:n_norm].astype(np.float64)
        xn, dyn = x[:, :, :n_norm], dy[:, :, :n_norm]
        z = np.maximum(xn, 0) if pre else xn
        if c["stats"] == "forward":   # the Function: the forward kernel's own statistics, inside their published bound
            st = RC.gn_stats(_gn_fwd_case(c), d)
            e = lambda a: a[:, ch][:, None, :]
            mean, rstd = e(st["m"]), e(st["rstd"])
            dr_s = e(st["dr"])
            dn_s = rstd * e(st["dm"] + U * np.abs(st["m"])) + np.abs(z - mean) * dr_s
        else:
            mr = d["mr"].astype(np.float64)
            mean, rstd = mr[:, ch, 0][:, None, :], mr[:, ch, 1][:, None, :]
            dn_s = dr_s = 0.0
        nv = (z - mean) * rstd
        pm = (xn > 0) if mutant == "post_mask_from_x" else (nv * gam + bet > 0)
        dg = np.where(pm, dyn, 0.0) if post else dyn
        s1, s2 = dg.sum(1), (dg * nv).sum(1)
        if mutant == "drop_last_row":
            s1, s2 = s1 - dg[:, -1], s2 - (dg * nv)[:, -1]
        a1, a2 = np.abs(dg).sum(1), np.abs(dg * nv).sum(1)
        dd = np.ceil(np.log2(S)) + 2
        B1 = (dd + 2) * U * a1
        B2 = (dd + 5) * U * a2 + (np.abs(dg) * dn_s).sum(1)
        gm = np.ones_like(gam) if mutant == "dn_without_gamma" else gam
        cnt = n
        if mutant == "count_rpc_nchunk":
            mp = gn_bwd_map(ld, S)
            cnt = gs * mp["rpc"] * mp["nchunk"]
        g3 = lambda a: a.reshape(B, G, gs).sum(2)
        m1g, m2g = g3(gm * s1) / cnt, g3(gm * s2) / cnt
        dgs = np.ceil(np.log2(gs)) + 2
        Bm1 = (g3(np.abs(gam) * B1) + (dgs + 3) * U * g3(np.abs(gam * s1))) / n
        Bm2 = (g3(np.abs(gam) * B2) + (dgs + 3) * U * g3(np.abs(gam * s2))) / n
        if mutant == "neighbour_sample":
            m1g, m2g = np.roll(m1g, -1, 0), np.roll(m2g, -1, 0)
        if mutant == "no_m2_term":
            m2g = np.zeros_like(m2g)
        m1, m2 = m1g[:, ch][:, None, :], m2g[:, ch][:, None, :]
        t4 = dg * gm - m1 - nv * m2
        o = rstd * t4
        bo = (rstd * (Bm1[:, ch][:, None, :] + np.abs(nv) * Bm2[:, ch][:, None, :] +
                      4 * U * (np.abs(dg * gam) + np.abs(m1) + np.abs(nv * m2))) + np.abs(m2) * rstd * dn_s + np.abs(t4) * dr_s)
        keep = (xn > 0) if (pre and mutant != "no_pre_mask") else np.ones(xn.shape, bool)
        dx[:, :, :n_norm] = np.where(keep, o, 0.0)
        bdx[:, :, :n_norm] = np.where(keep, bo, 0.0)
        if mutant == "tail_normalised":   # channel n_norm taken into the last group (gamma 1, beta 0)
            zt = np.maximum(x[:, :, n_norm], 0) if pre else x[:, :, n_norm]
            mt, rt_ = mean[:, :, -1], rstd[:, :, -1]
            ot = rt_ * (dy[:, :, n_norm] - m1[:, :, -1] - (zt - mt) * rt_ * m2[:, :, -1])
            dx[:, :, n_norm] = np.where(x[:, :, n_norm] > 0, ot, 0.0) if pre else ot
        dgam, dbet = np.zeros((B, ld)), np.zeros((B, ld))
        bg, bb = np.zeros((B, ld)), np.zeros((B, ld))
        dgam[:, :n_norm], dbet[:, :n_norm], bg[:, :n_norm], bb[:, :n_norm] = s2, s1, B2, B1
        if mutant == "dgamma_dbeta_swapped":
            dgam, dbet = dbet, dgam
        if c["wrap"]:   # through the Function: summed over the batch by slide_col_sums, the first n_norm channels returned
            db_ = (np.ceil(np.log2(B)) + 4) * U
            outs["dgamma"] = dict(y=dgam.sum(0)[:n_norm], b=(bg.sum(0) + db_ * np.abs(r32(dgam)).sum(0))[:n_norm] + 1e-300)
            outs["dbeta"] = dict(y=dbet.sum(0)[:n_norm], b=(bb.sum(0) + db_ * np.abs(r32(dbet)).sum(0))[:n_norm] + 1e-300)
        else:
            outs["dgamma"], outs["dbeta"] = dict(y=dgam, b=bg), dict(y=dbet, b=bb)
    outs["dx"] = dict(y=dx.reshape(B * S, ld), b=bdx.reshape(B * S, ld))
    return outs


def _col_sums(c, d, mutant):
    rows, ld = c["rows"], c["ld"]
    x = d["x"].astype(np.float64)
    mp = col_sums_map(rows, ld)
    use = np.ones(rows, bool)
    if mutant == "drop_last_row":
        use[-1] = False
    elif mutant == "drop_last_chunk":   # the last chunk that holds rows (with the 1024 clamp the trailing chunks are empty)
        use[(rows - 1) // mp["rpc"] * mp["rpc"]:] = False
    elif mutant == "rpc_floor":         # rows / nchunk rounded down: the chunks stop short of the last rows
        use[rows // mp["nchunk"] * mp["nchunk"]:] = False
    elif mutant == "second_stage_first_32":
        use[32 * mp["rpc"]:] = False
    return dict(out=dict(y=x[use].sum(0), b=col_bound(x)))


def col_bound(x):
    rows = x.shape[0]
    return (np.ceil(np.log2(max(rows, 1))) + 4) * U * np.abs(x).sum(0)


def _group_bwd(c, d, mutant):
    B, N, npt, K, C, ldf, ldg = c["B"], c["N"], c["np"], c["K"], c["C"], c["ldf"], c["ldg"]
    rows = B * npt * K
    dout = d["dout"].astype(np.float64)
    idx = d["idx"].reshape(-1)
    pt = np.arange(rows) // K
    live = np.ones(rows, bool)
    if c["counts"] and mutant != "zero_count_receives":
        live = d["counts"].reshape(-1)[pt] != 0
    b = pt // npt
    tgt = (b * (npt if mutant == "batch_stride_np" else N) + idx) % (B * N)
    Cw = C - C % 4 if mutant == "tail_channels_dropped" else C
    y = np.full((B * N, ldf), float(c["init"]))
    mag = np.abs(y)
    terms = np.ones((B * N, ldf))
    if mutant == "strides_swapped":   # dout read at the features' stride, dfeat written at the groups' (flat, wrapped into the buffers)
        src = (np.arange(rows)[:, None] * ldf + np.arange(Cw)[None]) % dout.size
        dst = (tgt[:, None] * ldg + np.arange(Cw)[None]) % y.size
        val = dout.reshape(-1)[src][live]
        np.add.at(y.reshape(-1), dst[live], val)
        np.add.at(mag.reshape(-1), dst[live], np.abs(val))
        np.add.at(terms.reshape(-1), dst[live], 1.0)
    else:
        np.add.at(y[:, :Cw], tgt[live], dout[live, :Cw])
        np.add.at(mag[:, :Cw], tgt[live], np.abs(dout[live, :Cw]))
        np.add.at(terms[:, :Cw], tgt[live], 1.0)
    return dict(dfeat=dict(y=y, b=(terms - 1) * U * mag))


def _concat_bwd(c, d, mutant):
    pts, K, C1, C2, ldq, ldk = c["pts"], c["K"], c["C1"], c["C2"], c["ldq"], c["ldk"]
    out, dout = d["out"].astype(np.float64), d["dout"].astype(np.float64)
    m = np.where((dout if mutant == "mask_from_dout" else out) > 0, dout, 0.0)
    dk = np.full((pts * K, ldk), c.get("fill", PREFILL))
    dk[:, :C2] = m[:, C1:C1 + C2]
    dq = np.full((pts, ldq), c.get("fill", PREFILL))
    bq = np.zeros((pts, ldq))
    mq = m.reshape(K, pts, -1).transpose(1, 0, 2) if mutant == "q_row_mod" else m.reshape(pts, K, -1)
    Ks = K - 1 if mutant == "q_sum_K_minus_1" else K
    w = C1 + 1 if mutant == "seam_off_by_one" else C1
    dq[:, :w] = mq[:, :Ks, :w].sum(1)
    bq[:, :C1] = (K - 1) * U * np.abs(m.reshape(pts, K, -1)[:, :, :C1]).sum(1)
    if mutant == "seam_off_by_one":
        dk[:, 0] = c.get("fill", PREFILL)
    return dict(dq=dict(y=dq, b=bq), dk=dict(y=dk, b=np.zeros_like(dk)))


def _attn_bwd(c, d, mutant):
    pts, K, C, lds, ldv = c["pts"], c["K"], c["C"], c["lds"], c["ldv"]
    n = np.full(pts, K)
    zero = np.zeros(pts, bool)
    if c["counts"]:
        n = np.clip(d["counts"], 1, K)
        if mutant == "slot_past_count":
            n = np.minimum(n + 1, K)
        if mutant == "zero_count_empty":
            zero = d["counts"] == 0
    mask = (np.arange(K)[None] < n[:, None])[:, :, None]
    cnt = n[:, None, None].astype(np.float64)
    s = d["S"].astype(np.float64).reshape(pts, K, lds)[:, :, :C]
    v = np.where(mask, d["V"].astype(np.float64).reshape(pts, K, ldv)[:, :, :C], 0.0)
    do = d["dout"].astype(np.float64)[:, None, :C]
    sm = np.where(mask, s, -np.inf)
    mx = sm.max(1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        if mutant == "no_max_shift":   # in fp32, as the kernel would: exp overflows from 88.7 on
            e = np.exp(sm.astype(np.float32))
            w = (e / e.sum(1, keepdims=True)).astype(np.float64)
        else:
            e = np.exp(sm - mx)
            w = e / e.sum(1, keepdims=True)
        o = (w * v).sum(1, keepdims=True)
        t = np.where(mask, v - (0.0 if mutant == "no_out_term" else o), 0.0)
        dvv, dss = w * do, w * t * do
    dk = np.where(mask, np.abs(s - mx), 0.0)
    wd = (w * (dk + E_EXP)).sum(1, keepdims=True)
    rho = dk + E_EXP + wd + cnt + 2
    dw = rho * U * w + ETA
    W = (w * np.abs(v)).sum(1, keepdims=True)
    Bo = U * ((w * np.abs(v) * (dk + E_EXP + cnt)).sum(1, keepdims=True) + W * (wd + cnt + 2))
    with np.errstate(invalid="ignore"):
        bv = np.where(mask, dw * np.abs(do) + ETA, 0.0)
        bs = np.where(mask, np.abs(do) * (dw * np.abs(t) + w * (Bo + 2 * U * np.abs(t))) + ETA, 0.0)
    if K == 1:
        bv, bs = np.zeros_like(bv), np.zeros_like(bs)
    dvv[zero], dss[zero] = 0, 0
    ds, dv = np.full((pts, K, lds), c.get("fill", PREFILL)), np.full((pts, K, ldv), c.get("fill", PREFILL))
    bds, bdv = np.zeros((pts, K, lds)), np.zeros((pts, K, ldv))
    ds[:, :, :C], dv[:, :, :C], bds[:, :, :C], bdv[:, :, :C] = dss, dvv, np.nan_to_num(bs), np.nan_to_num(bv)
    return dict(ds=dict(y=ds.reshape(-1, lds), b=bds.reshape(-1, lds)), dv=dict(y=dv.reshape(-1, ldv), b=bdv.reshape(-1, ldv)))


def _conv(c, d, mutant):
    rows, I, O = c["rows"], c["I"], c["O"]
    x, dy, W = d["x"].astype(np.float64), d["dy"].astype(np.float64), d["W"].astype(np.float64)
    bias = d["bias"].astype(np.float64) if c["bias"] else np.zeros(O)
    y, by = np.zeros((rows, ru(O))), np.zeros((rows, ru(O)))
    y[:, :O] = x[:, :I] @ W.T + bias
    by[:, :O] = C_ACC * (np.abs(x[:, :I]) @ np.abs(W).T + np.abs(bias)) + 1e-300
    dx, bx = np.zeros((rows, ru(I))), np.zeros((rows, ru(I)))
    dx[:, :I] = dy[:, :O] @ W
    bx[:, :I] = C_ACC * (np.abs(dy[:, :O]) @ np.abs(W)) + 1e-300
    use = rows
    if mutant == "dw_drop_last_slab":
        use = rows - rows // conv_map(rows, I, O)["slabs"]
    outs = dict(y=dict(y=y, b=by), dx=dict(y=dx, b=bx),
                dw=dict(y=dy[:use, :O].T @ x[:use, :I], b=(rows + 2) * U * (np.abs(dy[:, :O]).T @ np.abs(x[:, :I])) + 1e-300))
    if c["bias"]:
        outs["db"] = dict(y=dy[:rows - (mutant == "db_drop_last_row"), :O].sum(0), b=col_bound(dy)[:O] + 1e-300)
    return outs


_BACKWARD = dict(gn_bwd=_gn_bwd, col_sums=_col_sums, group_bwd=_group_bwd, concat_bwd=_concat_bwd, attn_bwd=_attn_bwd, conv=_conv)


def backward(c, d, mutant=None):
    """float64 reference of the case (or of one of its mutants): {output name: dict(y, b, stored)}; b holds the store term and is
    0 where the element must be exact"""
    outs = _BACKWARD[c["op"]](c, d, mutant)
    for o in outs.values():
        RC.store(o, False)
    return outs
