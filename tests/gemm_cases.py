"""The SLIDE_OP_GEMM case matrix, its float64 reference, its error bounds and its mutants -- shared by
tests/test_hip_gemm_arith.py (every case on the GPU against the reference, and, on the CPU, every bound against the mutants).

A case is one GEMM launch of `run_gemm` (csrc/gemm_ring.hip): y = X' . W^T + bias (+ pre_add) -> epilogue (include/slide_engine.h,
SlideEpi).  X' is X, or with an input affine X * scale + shift of the row's sample.  The reference takes the operands as the
kernel reads them:
  fp32, split: the fp32 values of X, W, scale, shift, residual, pre_add, tables (split rebuilds fp32-grade products from them);
  fp16:        X, W, residual, pre_add, pair tables rounded to fp16; scale / shift rounded to fp16 and X' = fp16(X * scale + shift)
               with ONE rounding (v_pk_fma_f16); with the module path's deferred ReLU X' = fp16(max(X', 0) + fp16(add)).
Everything else (bias, gamma, beta, addvec, statistics) is fp32.

Error bound, elementwise (u = 2^-24, the fp32 unit roundoff):
  A     = |X'| . |W|^T + |bias| + |pre_add|     (fp32 / split affine: |X| |scale| + |shift| in place of |X'|)
  RAW   b = C_ACC * A,  C_ACC = 2^-18 = 64 u.  That admits a few dozen fp32 roundings of the accumulation (an error that grows
        like sqrt(K) u A: 40 u at K = 1568), and the split's operand error 3 * 2^-22 |x||w| per product (low terms rounded to
        fp16, lo*lo dropped), and stays 32x below ONE fp16 operand rounding (2^-11 |x||w|): fp16 operands, or a split that
        drops one cross product, move y by ~2^-12 A.
  NORM  over the n = rows_per_sample * gs values of a (sample, group), mean m, variance v (from E[y^2] - m^2 in fp32):
        dm  = mean(b) + (d + 2) u mean|y|,                   d = ceil(log2 n) + 2 (tree sums)
        dv  = 2 mean(|y - m| b) + mean(b)^2 + 4 (d + 2) u mean(y^2)
        dr  = rstd (0.6 dv / (v + eps) + 4 u)                 (rsq is ~1 ulp)
        b'  = |gamma| rstd (b + dm) + |gamma| |y - m| dr + 3 u (|y g| + |m g| + |beta|),   g = gamma rstd
        channels past n_norm keep b.  The mean(y^2) term is what a large common mode (mean 30, std 1) costs: 900 x the
        variance, cancelled in fp32.
  then  ReLU (1-Lipschitz) -> + addvec -> + residual: b += 4 u (|value| + |addvec| + |residual|)
  store fp16: b (1 + 2^-11) + 2^-11 |ref| + 2^-25        fp32: b + u |ref|       (ref: the float64 result, unrounded)
  STATS sums over the sample's rows: |ds| <= sum b + d u sum|y|,   |dsq| <= sum (2 |y| b + b^2) + d u sum y^2   (x stats_scale)

Mutants (tests/test_hip_gemm_arith.py::test_bounds_see_the_mutants, CPU): the nearest plausible wrong arithmetic of each case --
  every case  "k_tail":        the last logical input column ignored (ragged K masked one column short)
  fp32        "fp16_operands": X' and W rounded to fp16 (the kernel silently on the fp16 matrix pipe)
  split       "drop_whi_xlo" / "drop_wlo_xhi": one cross product of the two-term split dropped
  NORM        "unbiased_var":  variance over n - 1
  affine      "affine_sample": the scale / shift of the neighbouring sample
A mutant counts as seen when its STORED output (rounded to the output type) leaves the bound around the reference somewhere.
A mutant that falls below the arithmetic's resolution in a case is listed in EXEMPT with the case that shows it instead."""
import zlib

import numpy as np

from slide_amd.abi import ru  # noqa: F401  (used here and re-exported to the test modules)

U = 2.0 ** -24
C_ACC = 2.0 ** -18
EPS = 1e-5
EPI_RAW, EPI_NORM, EPI_STATS = 0, 1, 2


def r16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _c(name, prec, npxl, B, K, N, mode, kernel, dist="normal", **kw):
    c = dict(name=name, prec=prec, npxl=npxl, B=B, K=K, N=N, mode=mode, kernel=kernel, dist=dist, pre_relu=False,
             post_relu=False, out_f32=False, addvec=None, resid=False, pre_add=None, aff=False, gn_fin=False, pair=None,
             stats_scale=1.0, status=0)
    c.update(kw)
    return c


# name, arithmetic, log2 rows per sample, samples, K, N, epilogue, the kernel run_gemm picks (product build)
CASES = [
    _c("f32_n4_raw", "fp32", 4, 37, 35, 51, EPI_RAW, "gemm_kernel<0, 4, 2, false>", addvec="plain", resid=True),
    _c("f32_n4_norm_aff", "fp32", 4, 17, 96, 111, EPI_NORM, "gemm_kernel<0, 4, 2, false>", "common", aff=True, post_relu=True),
    _c("f32_n7_norm", "fp32", 7, 3, 544, 51, EPI_NORM, "gemm_kernel<0, 7, 2, false>", pre_add=3, post_relu=True),
    _c("f32_n7_raw_gather", "fp32", 7, 17, 3, 3, EPI_RAW, "gemm_kernel<0, 7, 2, false>", pre_add="gather", post_relu=True),
    _c("f32_n8_stats", "fp32", 8, 3, 1568, 32, EPI_STATS, "gemm_kernel<0, 8, 2, false>", "small", pre_relu=True),
    _c("f32_n8_norm_aff", "fp32", 8, 3, 96, 512, EPI_NORM, "gemm_kernel<0, 8, 2, false>", "common", aff=True, addvec="idx",
       resid=True),
    _c("f32_n8_norm", "fp32", 8, 1, 35, 32, EPI_NORM, "gemm_kernel<0, 8, 2, false>", post_relu=True),
    _c("split_n4_raw", "split", 4, 37, 3, 32, EPI_RAW, "gemm_split_small_kernel<4>", addvec="plain", resid=True),
    _c("split_n4_norm_aff", "split", 4, 17, 544, 111, EPI_NORM, "gemm_split_small_kernel<4>", "common", aff=True,
       post_relu=True),
    # k_pad 1568 >= 736: the affine's LDS no longer fits the small kernel's 64 KB -- the 256-row split kernel takes it
    _c("split_n4_raw_aff_wide", "split", 4, 3, 1568, 51, EPI_RAW, "gemm_kernel<2, 4, 2, false>", aff=True),
    _c("split_n4_stats_wide", "split", 4, 1, 1568, 32, EPI_STATS, "gemm_split_small_kernel<4>", "small"),
    _c("split_n7_norm", "split", 7, 3, 96, 51, EPI_NORM, "gemm_kernel<2, 7, 2, false>", "bigw", pre_add="gather",
       addvec="plain"),
    _c("split_n7_stats", "split", 7, 17, 35, 32, EPI_STATS, "gemm_kernel<2, 7, 2, false>", "common", stats_scale=0.25),
    _c("split_n8_raw", "split", 8, 1, 544, 512, EPI_RAW, "gemm_kernel<2, 8, 2, false>", "bigw", pre_add=8, resid=True),
    _c("split_n8_norm_aff", "split", 8, 3, 35, 111, EPI_NORM, "gemm_kernel<2, 8, 2, false>", "small", aff=True),
    _c("split_n8_pair", "split", 8, 3, 96, 64, EPI_RAW, "gemm_kernel<2, 8, 2, true>", pair="pair"),
    _c("split_n7_pair_nbr", "split", 7, 3, 96, 32, EPI_RAW, "gemm_kernel<2, 7, 2, true>", pair="nbr", post_relu=True),
    _c("f16_n4_raw", "fp16", 4, 37, 35, 51, EPI_RAW, "gemm_small_kernel<2, false>", out_f32=True, addvec="plain"),
    _c("f16_n4_norm", "fp16", 4, 17, 1568, 512, EPI_NORM, "gemm_small_kernel<2, false>", "common", post_relu=True, resid=True),
    _c("f16_n4_norm_aff", "fp16", 4, 37, 96, 111, EPI_NORM, "gemm_small_kernel<2, true>", aff=True),
    _c("f16_n4_gnfin", "fp16", 4, 17, 35, 32, EPI_RAW, "gemm_small_kernel<2, true>", "common", aff=True, gn_fin=True),
    # (rows / 64) * ceil(n_cob / 2) tiles: 1024 is the most the statistics finalisation runs in one launch
    _c("f16_n4_gnfin_1024", "fp16", 4, 4096, 35, 64, EPI_RAW, "gemm_small_kernel<2, true>", aff=True, gn_fin=True),
    _c("f16_n4_gnfin_1025", "fp16", 4, 4097, 35, 64, EPI_RAW, "(none: status -10)", aff=True, gn_fin=True, status=-10),
    _c("f16_n8_norm", "fp16", 8, 3, 96, 111, EPI_NORM, "gemm_glds_occ3_kernel<8, false, false, false>", "small", addvec="idx"),
    _c("f16_n8_stats", "fp16", 8, 1, 3, 3, EPI_STATS, "gemm_glds_occ3_kernel<8, false, false, false>", pre_add=4),
    _c("f16_n8_norm_aff", "fp16", 8, 17, 544, 512, EPI_NORM, "gemm_glds_occ3_kernel<8, true, false, false>", aff=True,
       resid=True),
    # k_pad 2048: the affine vectors push the three-workgroup tile past its 53 KB -- the two-workgroup form takes it
    _c("f16_n8_raw_aff_wide", "fp16", 8, 3, 2021, 32, EPI_RAW, "gemm_glds_kernel<8, 2, 3, 32, true, false, false>", aff=True,
       pre_relu=True),
    _c("f16_n7_norm_aff", "fp16", 7, 3, 35, 51, EPI_NORM, "gemm_glds_kernel<7, 2, 3, 32, true, false, false>", "common", aff=True,
       pre_add="gather"),
    _c("f16_n8_pair", "fp16", 8, 3, 96, 64, EPI_NORM, "gemm_glds_kernel<8, 2, 3, 32, false, false, true>", pair="pair",
       post_relu=True),
    _c("f16_n7_pair_nbr", "fp16", 7, 3, 96, 32, EPI_RAW, "gemm_glds_kernel<7, 2, 3, 32, false, false, true>", pair="nbr"),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}

# (case, mutant) -> the case of the same kernel where that mutant IS visible
EXEMPT = {
    # groups of 16 channels x 256 rows (n = 4096) at a common mode of 30: the (n - 1) variance moves the output by 1.2e-4 of
    # |y - m| rstd, below the fp32 statistics' share of the bound there (900 x the variance, cancelled)
    ("f32_n8_norm_aff", "unbiased_var"): "f32_n8_norm",
}


def mutants(c):
    m = ["k_tail"]
    m += {"fp32": ["fp16_operands"], "split": ["drop_whi_xlo", "drop_wlo_xhi"], "fp16": []}[c["prec"]]
    if c["mode"] == EPI_NORM:
        m.append("unbiased_var")
    if c["aff"]:
        m.append("affine_sample")
    return m


def gn_params(N):
    """MyGroupNorm(min(32, N), N) over logical channels: groups, normalised channels, group size"""
    G = min(32, N)
    n_norm = N - N % G
    return G, n_norm, n_norm // G


def make_data(c):
    """the case's fp32 inputs (logical layouts; padding is the caller's business) -- deterministic per case name"""
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)
    B, K, N, npx = c["B"], c["K"], c["N"], 1 << c["npxl"]
    rows = B * npx
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    d = {}
    dist = c["dist"]
    X = f(rows, K)
    W = f(N, K) / np.float32(np.sqrt(K))
    bias = 0.5 * f(N)
    if dist == "common":
        X = X + np.float32(30.0)
    elif dist == "small":
        X, bias = X * np.float32(1e-3), bias * np.float32(1e-3)
    elif dist == "bigw":  # two-accumulator split kernels: no |w| < 32 limit
        W = rs.uniform(-64.0, 64.0, (N, K)).astype(np.float32)
        W.flat[rs.randint(W.size)] = 64.0
    d.update(X=X.astype(np.float32), W=W.astype(np.float32), bias=bias.astype(np.float32),
             gamma=(1 + 0.2 * f(N)).astype(np.float32), beta=(0.2 * f(N)).astype(np.float32))
    if c["aff"]:
        if c["gn_fin"]:
            # statistics of X as its producer published them: per-(sample, channel) sums over the sample's rows, groups of gs
            # channels (MyGroupNorm(min(32, K), K)); the launch turns them into scale / shift itself
            Xk = r16(X).reshape(B, npx, K)
            d["sum"] = Xk.sum(1).astype(np.float32)
            d["sq"] = (Xk * Xk).sum(1).astype(np.float32)
            d["fin_gamma"] = (1 + 0.2 * f(K)).astype(np.float32)
            d["fin_beta"] = (0.2 * f(K)).astype(np.float32)
        else:
            d["scale"] = rs.uniform(0.5, 1.5, (B, K)).astype(np.float32)
            d["shift"] = (-(30.0 if dist == "common" else 0.0) + 0.5 * f(B, K)).astype(np.float32)
            if dist == "small":
                d["shift"] *= np.float32(1e-3)
    if c["addvec"] == "plain":
        d["addvec"] = f(B, N)
    elif c["addvec"] == "idx":  # row t of a per-timestep table [T][B][N], t read on the device
        d["addvec_tab"], d["addvec_t"] = f(4, B, N), 2
        d["addvec"] = d["addvec_tab"][2]
    if c["resid"]:
        d["resid"] = f(rows, N)
    if c["pre_add"] is not None or c["pair"] == "nbr":
        # neighbour table of 16-point samples: 16 neighbours per point, the first 2^(npxl - 4) used
        d["nbr"] = np.stack([rs.permutation(16) for _ in range(B * 16)]).astype(np.int32).reshape(-1)
    if c["pre_add"] == "gather":
        d["pre"] = f(B * 16, N)
    elif c["pre_add"] is not None:
        d["pre"] = f(rows >> c["pre_add"], N)
    if c["pair"] is not None:
        d["ta"], d["tb"] = f(B * 16, N), f(B * 16, N)
        if c["pair"] == "nbr":
            d["d2"] = rs.uniform(0, 4, (B * 16, 16)).astype(np.float32)
            d["w"] = rs.uniform(0, 1, (B * 16, 16)).astype(np.float32)
            d["vd"], d["vw"] = 0.3 * f(N), 0.3 * f(N)
    return d


def _pre_rows(c):
    """the per-point row of every output row that pre_add reads"""
    B, npxl = c["B"], c["npxl"]
    rows = np.arange(B << npxl)
    if c["pre_add"] == "gather":
        return None
    return rows >> c["pre_add"]


def _gather_rows(c, d, kl):
    rows = np.arange(c["B"] << c["npxl"])
    smp, pxl = rows >> c["npxl"], rows & ((1 << c["npxl"]) - 1)
    slot = (smp * 16 + (pxl >> kl)) * 16 + (pxl & ((1 << kl) - 1))
    return smp * 16 + d["nbr"][slot], slot


def fin_scale_shift(c, d):
    """float64 scale / shift of the statistics finalisation, [B][K], from the fp32 sums (channels past n_norm: 1 / 0)"""
    B, K, npx = c["B"], c["K"], 1 << c["npxl"]
    G, n_norm, gs = gn_params(K)
    s = d["sum"].astype(np.float64)[:, :n_norm].reshape(B, G, gs).sum(2)
    q = d["sq"].astype(np.float64)[:, :n_norm].reshape(B, G, gs).sum(2)
    mean = s / (gs * npx)
    var = np.maximum(q / (gs * npx) - mean * mean, 0)
    rstd = 1 / np.sqrt(var + EPS)
    sc, sh = np.ones((B, K)), np.zeros((B, K))
    g = np.repeat(np.arange(G), gs)
    sc[:, :n_norm] = d["fin_gamma"][:n_norm] * rstd[:, g]
    sh[:, :n_norm] = d["fin_beta"][:n_norm] - mean[:, g] * sc[:, :n_norm]
    # bound of the kernel's fp32 arithmetic on them (sums of gs values, E[x^2] - m^2, 1 / sqrt, two products)
    ex2 = q / (gs * npx)
    rel = (gs + 8) * U * (1 + 2 * ex2 / (var + EPS))
    dsc = np.ones((B, K)) * 0.0
    dsc[:, :n_norm] = np.abs(sc[:, :n_norm]) * rel[:, g]
    dsh = np.zeros((B, K))
    dsh[:, :n_norm] = (np.abs(mean[:, g]) * dsc[:, :n_norm] + np.abs(sc[:, :n_norm]) * (gs + 4) * U * np.abs(mean[:, g]) +
                       4 * U * (np.abs(d["fin_beta"][:n_norm]) + np.abs(mean[:, g] * sc[:, :n_norm])))
    return sc, sh, dsc, dsh


def _split(a):
    hi = r16(a)
    return hi, r16((a - hi) * 2048.0)


def forward(c, d, mutant=None, fin=None, xb=None):
    """float64 reference of the case (or of one of its mutants).  fin: the scale / shift the launch published (statistics
    finalisation cases: the GEMM's operands are their fp16 copies).  xb: elementwise uncertainty [rows][K] of an X that its
    producer hands over in registers (tests/pair_cases.py): X is then taken as given -- its rounding is part of xb -- and
    the contraction's bound gains xb . |W|^T.  Returns dict(y = output [rows][N], A, b = bound,
    stats = (sum, sq) [B][N] or None, stats_b)."""
    prec, B, K, N, npxl = c["prec"], c["B"], c["K"], c["N"], c["npxl"]
    npx = 1 << npxl
    rows = B * npx
    smp = np.arange(rows) >> npxl
    h = prec == "fp16"
    X = d["X"].astype(np.float64)
    W = d["W"].astype(np.float64)
    if h:
        X, W = (r16(X) if xb is None else X), r16(W)
    Xabs = np.abs(X)
    if c["aff"]:
        if c["gn_fin"]:
            sc, sh = (fin if fin is not None else fin_scale_shift(c, d)[:2])
        else:
            sc, sh = d["scale"].astype(np.float64), d["shift"].astype(np.float64)
        if mutant == "affine_sample":
            sc, sh = np.roll(sc, -1, 0), np.roll(sh, -1, 0)
        if h:
            X = r16(X * r16(sc)[smp] + r16(sh)[smp])
            Xabs = np.abs(X)
        else:
            Xabs = np.abs(X * sc[smp]) + np.abs(sh[smp])
            X = X * sc[smp] + sh[smp]
    if mutant == "k_tail":
        X = X.copy()
        X[:, K - 1] = 0
    if mutant == "fp16_operands":
        acc = r16(X) @ r16(W).T
    elif mutant in ("drop_whi_xlo", "drop_wlo_xhi"):
        xh, xl = _split(X)
        wh, wl = _split(W)
        acc = xh @ wh.T + (xh @ wl.T if mutant == "drop_whi_xlo" else xl @ wh.T) / 2048.0
    else:
        acc = X @ W.T
    A = Xabs @ np.abs(W).T + np.abs(d["bias"])
    y = acc + d["bias"]
    if c["pre_add"] is not None:
        pre = d["pre"].astype(np.float64)
        if h:
            pre = r16(pre)
        prow = _gather_rows(c, d, npxl - 4)[0] if c["pre_add"] == "gather" else _pre_rows(c)
        y = y + pre[prow]
        A = A + np.abs(pre[prow])
    b = C_ACC * A
    if xb is not None:
        b = b + xb @ np.abs(W).T
    if c["pre_relu"]:
        y = np.maximum(y, 0)
    stats = stats_b = None
    if c["mode"] == EPI_STATS:
        n = npx
        dd = np.ceil(np.log2(n)) + 2
        yb, bb = y.reshape(B, npx, N), b.reshape(B, npx, N)
        stats = (yb.sum(1) * c["stats_scale"], (yb * yb).sum(1) * c["stats_scale"])
        stats_b = ((bb.sum(1) + dd * U * np.abs(yb).sum(1)) * c["stats_scale"],
                   ((2 * np.abs(yb) * bb + bb * bb).sum(1) + dd * U * (yb * yb).sum(1)) * c["stats_scale"])
    elif c["mode"] == EPI_NORM:
        G, n_norm, gs = gn_params(N)
        n = npx * gs
        dd = np.ceil(np.log2(n)) + 2
        part = y[:, :n_norm].reshape(B, npx, G, gs)
        bp = b[:, :n_norm].reshape(B, npx, G, gs)
        ax = (1, 3)
        m = part.mean(ax, keepdims=True)
        var = ((part - m) ** 2).mean(ax, keepdims=True)
        if mutant == "unbiased_var":
            var = var * n / (n - 1)
        rstd = 1 / np.sqrt(var + EPS)
        gam = d["gamma"][:n_norm].reshape(1, 1, G, gs).astype(np.float64)
        bet = d["beta"][:n_norm].reshape(1, 1, G, gs).astype(np.float64)
        o = (part - m) * rstd * gam + bet
        dm = bp.mean(ax, keepdims=True) + (dd + 2) * U * np.abs(part).mean(ax, keepdims=True)
        dv = (2 * (np.abs(part - m) * bp).mean(ax, keepdims=True) + bp.mean(ax, keepdims=True) ** 2 +
              4 * (dd + 2) * U * (part * part).mean(ax, keepdims=True))
        dr = rstd * (0.6 * dv / (var + EPS) + 4 * U)
        g = gam * rstd
        bo = (np.abs(gam) * rstd * (bp + dm) + np.abs(gam) * np.abs(part - m) * dr +
              3 * U * (np.abs(part * g) + np.abs(m * g) + np.abs(bet)))
        y = y.copy(); b = b.copy()
        y[:, :n_norm] = o.reshape(rows, n_norm)
        b[:, :n_norm] = bo.reshape(rows, n_norm)
    if c["post_relu"]:
        y = np.maximum(y, 0)
    extra = np.abs(y)
    if "addvec" in d:
        av = d["addvec"].astype(np.float64)[smp]
        y = y + av
        extra = extra + np.abs(av)
    if c["resid"]:
        r = d["resid"].astype(np.float64)
        if h:
            r = r16(r)
        y = y + r
        extra = extra + np.abs(r)
    if c["pair"] is not None:
        r = pair_residual(c, d)
        y = y + r
        ra, rb, _ = pair_rows(c, d)
        # (fp32 tables: the residual's own two or four roundings, relative to its terms)
        extra = extra + np.abs(r) + (0 if h else np.abs(d["ta"][ra]) + np.abs(d["tb"][rb]) + 4 * np.abs(d["vd"] if "vd" in d else 0))
    b = b + 4 * U * extra
    # (the bound is against the UNROUNDED result: a kernel within b of it may round to either neighbour)
    if h and not c["out_f32"]:
        stored = r16(y)
        b = b * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(y) + 2.0 ** -25
    else:
        stored = r32(y)
        b = b + U * np.abs(y)
    return dict(y=y, stored=stored, A=A, b=b, stats=stats, stats_b=stats_b)


def pair_rows(c, d):
    """the two table rows of every output row's PAIR residual, and the neighbour slot (RES_PAIR_NBR)"""
    npxl = c["npxl"]
    rows = np.arange(c["B"] << npxl)
    smp, pxl = rows >> npxl, rows & ((1 << npxl) - 1)
    if c["pair"] == "pair":  # 16 x 16-row samples in natural neighbour order
        return smp * 16 + (pxl & 15), rows >> 4, None
    a, slot = _gather_rows(c, d, 3)
    return a, rows >> 3, slot


def pair_residual(c, d):
    """ta[q] + tb[p] (+ d2 vd + w vw), evaluated as the kernel does: fp32 (split), or in fp16 steps (fp16 plans)"""
    ra, rb, slot = pair_rows(c, d)
    ta, tb = d["ta"].astype(np.float64)[ra], d["tb"].astype(np.float64)[rb]
    if c["prec"] == "fp16":
        r = r16(r16(ta) + r16(tb))
        if slot is not None:
            d2 = r16(np.minimum(d["d2"].reshape(-1)[slot], 65504.0))[:, None]
            w = r16(d["w"].reshape(-1)[slot])[:, None]
            r = r16(d2 * r16(d["vd"]) + r)
            r = r16(w * r16(d["vw"]) + r)
        return r
    r = ta + tb
    if slot is not None:
        r = r + d["d2"].reshape(-1)[slot][:, None] * d["vd"] + d["w"].reshape(-1)[slot][:, None] * d["vw"]
    return r
