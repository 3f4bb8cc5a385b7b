"""SLIDE_OP_POINT_CHAIN (slide_amd/csrc/point_chain.hip) as ONE launch on synthetic data: the case table, the float64 reference, the
error bounds and the mutants -- shared by tests/test_point_chain_host.py (every bound against the mutants, on the CPU) and
tests/test_hip_point_chain.py (every case on the GPU against the reference).

THE LAUNCH.  Four dependent 16-rows-per-sample layers, 128 channels each, GroupNorm(32, 128) = groups of FOUR consecutive channels over the
sample's 16 rows (n = 64 values):
  1  h  = relu(GN(Wz[:128] z + b1)) + tvec[sample]           r = Wz[128:] z + b_res  (raw, stays in fp32 registers)
  2  o  = relu(GN(W2 h + b2)) + cvec[sample] + r             X[:, :128] = fp16(o)    (observable, an fp16 store)
  3  hh = relu(GN(W0 [o | X[:, 128:k0]] + b0))
  4  eps = W1 hh + b_out                                     (observable, fp32; columns below eps_ld in whole groups of four)
A workgroup owns 32 rows (two samples); rows past `rows` are clamped duplicates of the last row and are never stored.

OPERANDS as the kernel sees them: Z and X[:, 128:] are fp16 as stored; a weight is fp16(w) (form "fp16") or hi + 2^-11 lo' with
hi = fp16(w), lo' = fp16((w - hi) 2^11) (form "wide", all four *_lo pointers set); every vector is fp32.  The reference evaluates the
four layers in float64 on exactly these operands and keeps h, o, hh UNROUNDED; what the kernel does to them where they cross the waves
through LDS is input uncertainty of the next layer (below).  So the float64 evaluation with unrounded crossings IS the reference, and the
evaluation that rounds at the crossings as the kernel does ("crossings_rounded") is a NON-mutant: it must stay inside the bound.

BOUNDS, elementwise, u = 2^-24, H = 2^-11; x the layer's float64 input, xb the bound of the kernel's input against it:
  contraction   v = W x + bias:  bv = C_ACC A + xb . |W|^T,  A = |x| . |W|^T + |bias|,  C_ACC = 64 u (gemm_cases: a few dozen fp32
                roundings of the MFMA accumulation, the fold hi += 2^-11 lo, the bias add)
                wide, layers 2..4 (the input crossed as two planes):  + 2 * 2^-22 |x| . |W|^T -- the dropped lo'.lo' product
                (|2^-11 lo'_w| <= H |w| (1 + H), |2^-11 lo'_x| <= H |x| (1 + H): 2^-22 (1 + H)^2, taken as 2 * 2^-22); the planes' own residual is in xb
  GroupNorm     the kernel's own arithmetic: sums over the group's 64 values, four sequential fp32 adds / FMAs in the lane and four DPP
                levels -- NSUM = 8 roundings: dS = NSUM u sum |v|, dSS = (NSUM + 1) u sum v^2 (the square's own rounding); mean,
                var = max(SS / 64 - mean^2, 0) and the relative bound `rel` of rstd come from pair_cases._norm_fin, which ASSERTS its
                first-order regime dvar / (var + eps) <= 0.3; __builtin_amdgcn_rsqf is a one-ulp function (inside _norm_fin's 4 u).
                Its 3 u (SS / 64 + mean^2) is what a group whose mean is far above its spread costs (case "gnmean").
                The INPUTS' uncertainty bv enters S and SS with the same sign, so it does not pay that cancellation: the variance of
                v + e differs from that of v by 2 cov(v, e) + var(e) <= prop = 2 mean(|v - m| bv) + mean(bv^2) (gemm_cases' NORM term);
                64 prop is handed to _norm_fin inside dSS, so its regime assertion covers the total, and dm gains mean(bv).
                g = gamma rstd: dg = |g| (rel + u).  The kernel forms y = fma(v, g, beta - mean g):
                y_k - y = ((v_k - v) - (m_k - m)) g_k + (v - m) (g_k - g) + three roundings, so
                dy = 1.01 (|g| (bv + dm) + |v - m| dg) + 3 u (|v g| + |m g| + |beta|)          (1 %: products of two errors)
  then          ReLU: 1-Lipschitz, and where y + dy <= 0 the kernel's value is exactly 0 too: min(dy, max(y + dy, 0));
                + tvec (one fp32 add: u |h|); layer 2: + cvec + r, two adds, r = acc + b_res with br = C_ACC A_r + u |r|:
                bo = dy + br + 2 u (|y| + |cvec| + |r| + |o|)
  crossing      fp16 form: one rounding to fp16 of a value within b of x: xb' = b + half an fp16 ulp at |x| + b (half_ulp16; 2^-25 in the
                subnormals)
                wide: x_k = hi + 2^-11 lo' + e, |x_k - hi| <= H |x_k|, lo' rounds that once more: |e| <= H^2 |x_k| (1 + H) + 2^-36
                (2^-36 = 2^-11 2^-25: lo' in fp16's subnormals):  xb' = b + 2^-22 (|x| + b) (1 + H) + 2^-36
  stores        X: b + half an fp16 ulp in BOTH forms (put16);  eps: b + u |eps| (the add of b_out; the fp32 store is exact)
The wide bound is ~2^-18 A where the fp16 form's is ~2^-11 |x| . |W|: judged against the WIDE bound the whole fp16-form evaluation
must fail on every case ("fp16_form"); if it passed, the wide rows could not tell hi-only arithmetic from the split.

PROBES.  The bound is a worst case carried through up to three further contractions and GroupNorms, each of which multiplies it by
~sqrt(K) against what random errors do; at eps of the dense cases it is two to three orders of magnitude above the kernel's error and a
2^-12-relative operand error of layers 2..4 (a missing lo'.x, a dropped low plane) stays below it.  probe_l2 / l3 / l4 isolate ONE layer:
the weights in front of it are zero, so its input is relu(GN(bias)) + vectors, exact to a few u; the weights behind it are selectors
(W0 = I on the first 128 columns, W1 = I on the first 32 n1c), exact in fp16 with lo' = 0, so its output reaches eps through at most one
GroupNorm.  There the WIDE mutants of that layer miss the bound; "wide_drop_lo_l1", "wide_lo_2_10" and "fp16_form" miss it on the dense
cases as well (mutants() applies each where the bound can see it; profiles/point_chain_arith.md has all ratios).

INPUTS.  gemm_cases' distributions: "normal" (N(0, 1)) and "common" (Z + 30); weights N(0, 1) / sqrt(K), so the activations of the four
layers stay O(1) after their GroupNorm; biases 0.5 N, gamma 1 + 0.2 N, beta 0.2 N, t / class rows N(0, 1).  "gnmean": GNMEAN is added
to b1 of group 5 and b2 of group 9 -- a group whose mean is GNMEAN / spread ~ 40 x its spread, the cancellation of ss / 64 - mean^2.
No case may leave _norm_fin's regime: forward() runs the assertion for every layer of every case, the host test runs forward() on all.

Mutants (MUTANT_DOC) are evaluated like the kernel (crossings rounded) and count as seen when a STORED output (X as fp16, eps as fp32)
leaves the bound around the reference somewhere; profiles/point_chain_arith.md records by how many bounds."""
import zlib

import numpy as np

import pair_cases as P
from gemm_cases import C_ACC, U, r16, r32

H = 2.0 ** -11
NSUM = 8
GNMEAN = 40.0
T_ROW = 5  # t_idx[0] of the shared-row form
T_ROWS = 8  # rows of the shared table

MUTANT_DOC = {
    "t_other_sample": "the t row of the other sample of the workgroup", "t_minus_1": "row t - 1 of the shared table",
    "c_before_relu": "the class row added before the ReLU", "drop_residual": "the residual dropped", "drop_b_res": "b_res dropped",
    "gn_32_rows": "GroupNorm statistics over the workgroup's 32 rows", "gn_groups_of_8": "groups of 8 channels",
    "head_blind_xyz": "the head blind to X[:, 128:]", "w1_block0": "n1c 2: wave 1 using wave 0's W1 block",
    "wide_drop_lo_l1": "wide: lo'.x missing in layer 1", "wide_drop_lo_l2": "wide: lo'.x missing in layer 2",
    "wide_drop_lo_l3": "wide: lo'.x missing in the head's first layer", "wide_drop_lo_l4": "wide: lo'.x missing in the head's second layer",
    "wide_lo_2_10": "wide: lo' scaled by 2^-10", "wide_drop_xlo": "wide: an activation's low plane dropped (h)",
    "fp16_form": "the whole fp16-form evaluation judged against the WIDE bound",
}
NON_MUTANTS = ("crossings_rounded",)
FORMS = ("fp16", "wide")


def _c(name, rows, kz, zpad, x_ld, n1c, eps_ld, tvec, cvec, dist="normal", probe=0):
    return dict(name=name, rows=rows, kz=kz, z_ld=kz + zpad, k0=160, x_ld=x_ld, n1c=n1c, eps_ld=eps_ld, tvec=tvec, cvec=cvec, dist=dist,
                probe=probe)


# tvec: None | "shared" (row t_idx[0] of a table, t_bs 0) | "sample" (t_idx NULL, one row per sample);  cvec: False | True
CASES = [
    _c("r16_kz32", 16, 32, 0, 160, 1, 20, None, False),
    _c("r32_kz96_pad", 32, 96, 8, 168, 2, 52, "shared", True),
    _c("r48_kz192_common", 48, 192, 0, 160, 2, 64, "sample", True, "common"),
    _c("r112_kz192_pad", 112, 192, 8, 168, 1, 32, "shared", False),
    _c("r48_kz32_pad_common", 48, 32, 8, 160, 1, 32, "sample", False, "common"),
    _c("r16_kz96_gnmean", 16, 96, 0, 168, 2, 64, "shared", True, "gnmean"),
    _c("r112_kz96", 112, 96, 0, 160, 2, 52, "sample", True),
    _c("r32_kz192_n1", 32, 192, 8, 160, 1, 20, None, True),
    # probes of ONE layer (module docstring, PROBES): zero weights before it, selector weights behind it
    _c("probe_l2", 32, 32, 0, 160, 2, 64, "sample", True, probe=2),
    _c("probe_l3", 32, 32, 0, 160, 2, 64, "shared", True, probe=3),
    _c("probe_l4", 32, 32, 0, 160, 2, 64, "sample", True, probe=4),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
T_STRIDE, T_COFF, T_BS, T_BS_COFF, C_BS, C_COFF = 200, 24, 160, 8, 144, 16  # leading dimensions > 128 and the pointer offsets into them
EXTRA_ROWS = 5  # rows past `rows` in the over-allocated Z / X / eps buffers


def mutants(c, form):
    if c["probe"]:
        return ["wide_drop_lo_l%d" % c["probe"], "wide_drop_xlo", "wide_lo_2_10", "fp16_form"] if form == "wide" else []
    m = ["drop_residual", "drop_b_res", "gn_groups_of_8", "head_blind_xyz"]
    if c["rows"] >= 32:  # (at rows 16 the workgroup's second sample is a duplicate of the first)
        m.append("gn_32_rows")
        if c["tvec"] == "sample":
            m.append("t_other_sample")
    if c["tvec"] == "shared":
        m.append("t_minus_1")
    if c["cvec"]:
        m.append("c_before_relu")
    if c["n1c"] == 2 and c["eps_ld"] > 32:
        m.append("w1_block0")
    if form == "wide":
        m += ["wide_drop_lo_l1", "wide_lo_2_10", "fp16_form"]
    return m


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_data(c):
    """the case's inputs in logical layouts, fp32 (Z and the head's extra columns already fp16 values) -- deterministic per case name"""
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    rows, kz, k0, n1c = c["rows"], c["kz"], c["k0"], c["n1c"]
    nsm = rows // 16
    Z = f(rows, kz) + np.float32(30.0 if c["dist"] == "common" else 0.0)
    d = dict(Z=Z.astype(np.float16).astype(np.float32), Xin=f(rows, k0 - 128).astype(np.float16).astype(np.float32),
             Wz=f(256, kz) / np.float32(np.sqrt(kz)), W2=f(128, 128) / np.float32(np.sqrt(128.0)), W0=f(128, k0) / np.float32(np.sqrt(k0)),
             W1=f(32 * n1c, 128) / np.float32(np.sqrt(128.0)), b_out=0.5 * f(32 * n1c))
    for k in ("vz", "v2", "v0"):
        d[k] = np.stack([0.5 * f(128), 1 + 0.2 * f(128), 0.2 * f(128)] + ([0.5 * f(128)] if k == "vz" else [])).astype(np.float32)
    if c["dist"] == "gnmean":
        d["vz"][0, 20:24] += np.float32(GNMEAN)
        d["v2"][0, 36:40] += np.float32(GNMEAN)
    L = c["probe"]
    if L:
        sel = lambda n, k: np.eye(n, k, dtype=np.float32)
        d["Wz"] *= 0
        if L >= 3:
            d["W2"] *= 0
        if L == 4:
            d["W0"] *= 0
        if L == 2:
            d["W0"] = sel(128, k0)
        if L <= 3:
            d["W1"] = sel(32 * n1c, 128)
    if c["tvec"] == "shared":
        d["ttab"] = f(T_ROWS, T_STRIDE)
    elif c["tvec"] == "sample":
        d["ttab"] = f(nsm, T_BS)
    if c["cvec"]:
        d["ctab"] = f(nsm, C_BS)
    return {k: np.ascontiguousarray(v, np.float32) for k, v in d.items()}


def split(w):
    """(hi, lo') fp32 arrays holding fp16 values: w = hi + 2^-11 lo' + O(2^-22 |w|), formed as the engine does (in fp32)"""
    w = np.asarray(w, np.float32)
    hi = w.astype(np.float16).astype(np.float32)
    return hi, ((w - hi) * np.float32(2048.0)).astype(np.float16).astype(np.float32)


def t_rows(c, d, sm, t=T_ROW):
    """the t-embedding row of samples `sm` ([len(sm)][128], float64); zero without a tvec"""
    if c["tvec"] is None:
        return np.zeros((len(sm), 128))
    if c["tvec"] == "shared":
        return np.broadcast_to(d["ttab"][t, T_COFF:T_COFF + 128].astype(np.float64), (len(sm), 128))
    return d["ttab"][sm, T_BS_COFF:T_BS_COFF + 128].astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ reference
def _weights(d, form, mutant):
    out = {}
    for li, k in enumerate(("Wz", "W2", "W0", "W1"), 1):
        hi, lo = split(d[k])
        hi, lo = hi.astype(np.float64), lo.astype(np.float64)
        if form == "fp16" or mutant == "wide_drop_lo_l%d" % li:
            out[k] = hi
        else:
            out[k] = hi + lo / (1024.0 if mutant == "wide_lo_2_10" else 2048.0)
    return out


def _gn_relu(v, bv, vec, rows_per=16, gs=4, bounded=True):
    """relu(GroupNorm(v)) of v [R][128] with the bound dy; vec = [bias | gamma | beta] (the bias is already in v).  bounded False (a
    mutant's evaluation, whose clamped duplicate rows and wrong groups are outside any regime): the values alone"""
    R = v.shape[0]
    shp = (R // rows_per, rows_per, 128 // gs, gs)
    vv, bb = v.reshape(shp), bv.reshape(shp)
    S, SS = vv.sum((1, 3)), (vv * vv).sum((1, 3))
    if not bounded:
        m = vv.mean((1, 3), keepdims=True)
        y = ((vv - m) / np.sqrt(((vv - m) ** 2).mean((1, 3), keepdims=True) + P.EPS)).reshape(R, 128) * vec[1] + vec[2]
        return np.maximum(y, 0), 0.0 * y, y
    n = rows_per * gs
    mu = S[:, None, :, None] / n
    prop = 2 * (np.abs(vv - mu) * bb).mean((1, 3)) + (bb * bb).mean((1, 3))  # of the variance, from the inputs' uncertainty
    m, var, rstd, dm, rel = P._norm_fin(S, SS, NSUM * U * np.abs(vv).sum((1, 3)), (NSUM + 1) * U * SS + n * prop, 1.0 / n)
    dm = dm + bb.mean((1, 3))
    ex = lambda a: np.broadcast_to(a[:, None, :, None], shp).reshape(R, 128)
    m, rstd, dm, rel = ex(m), ex(rstd), ex(dm), ex(rel)
    gam, bet = vec[1].astype(np.float64), vec[2].astype(np.float64)
    g = gam * rstd
    dg = np.abs(g) * (rel + U)
    y = (v - m) * g + bet
    dy = 1.01 * (np.abs(g) * (bv + dm) + np.abs(v - m) * dg) + 3 * U * (np.abs(v * g) + np.abs(m * g) + np.abs(bet))
    return np.maximum(y, 0), np.minimum(dy, np.maximum(y + dy, 0)), y


def half_ulp16(x, b):
    """half an fp16 ulp at a value within b of x (2^-25 in the subnormals)"""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x) + b, 2.0 ** -14))) - 11)


def _cross(x, b, form, emu, drop_lo=False):
    """a value crossing the waves through LDS: (the next layer's input, its bound).  emu: round as the kernel does"""
    if form == "fp16":
        return (r16(x) if emu else x), b + half_ulp16(x, b)
    if emu:
        hi = r16(x)
        x = hi if drop_lo else hi + r16((x - hi) * 2048.0) / 2048.0
    return x, b + 2.0 ** -22 * (np.abs(x) + b) * (1 + H) + 2.0 ** -36


def forward(c, d, form, mutant=None, t=T_ROW):
    """float64 reference of a case in one form, or (mutant set: evaluated with the kernel's roundings at the crossings) of a mutant /
    non-mutant.  Returns dict(X=(ref [rows][128], stored, bound), eps=(ref [rows][eps_ld], stored, bound))."""
    if mutant == "fp16_form":
        return forward(c, d, "fp16", "crossings_rounded", t)
    emu = mutant is not None
    rows, kz, k0, n1c, eps_ld = c["rows"], c["kz"], c["k0"], c["n1c"], c["eps_ld"]
    nsm = rows // 16
    # a mutant sees the workgroups' rows: past `rows` clamped duplicates of the last one; the reference needs the real rows only
    rp = np.arange((rows + 31) // 32 * 32 if emu else rows)
    grow = np.minimum(rp, rows - 1)
    sm = np.minimum(rp >> 4, nsm - 1)
    W = _weights(d, form, mutant)
    wide = form == "wide"
    lolo = lambda x, w: 2 * 2.0 ** -22 * (np.abs(x) @ np.abs(w).T) if wide else 0.0
    other = lambda a: a.reshape(-1, 2, 16, a.shape[-1])[:, ::-1].reshape(a.shape)  # per row: the other sample of the workgroup
    gn = lambda v, bv, vec: _gn_relu(v, bv, vec, 32 if mutant == "gn_32_rows" else 16, 8 if mutant == "gn_groups_of_8" else 4, not emu)
    vz, v2, v0 = (d[k].astype(np.float64) for k in ("vz", "v2", "v0"))
    # ---- layer 1
    z = d["Z"].astype(np.float64)[grow]
    acc = z @ W["Wz"].T
    A = np.abs(z) @ np.abs(W["Wz"]).T
    v, bv = acc[:, :128] + vz[0], C_ACC * (A[:, :128] + np.abs(vz[0]))
    y, dy, _ = gn(v, bv, vz)
    tv = t_rows(c, d, sm, t - 1 if mutant == "t_minus_1" else t)
    if mutant == "t_other_sample":
        tv = other(np.ascontiguousarray(tv))
    h = y + tv
    bh = dy + U * np.abs(h)
    bres = 0.0 if mutant == "drop_b_res" else vz[3]
    r = acc[:, 128:] + bres
    br = C_ACC * (A[:, 128:] + np.abs(vz[3])) + U * np.abs(r)
    if mutant == "drop_residual":
        r = 0.0 * r
    xlo = lambda L: mutant == "wide_drop_xlo" and (c["probe"] or 2) == L
    x, xb = _cross(h, bh, form, emu, drop_lo=xlo(2))
    # ---- layer 2
    cv = d["ctab"][sm, C_COFF:C_COFF + 128].astype(np.float64) if c["cvec"] else np.zeros((len(rp), 128))
    v = x @ W["W2"].T + v2[0]
    bv = C_ACC * (np.abs(x) @ np.abs(W["W2"]).T + np.abs(v2[0])) + xb @ np.abs(W["W2"]).T + lolo(x, W["W2"])
    y, dy, ypre = gn(v, bv, v2)
    if mutant == "c_before_relu":
        y = np.maximum(ypre + cv, 0) - cv
    o = y + cv + r
    bo = dy + br + 2 * U * (np.abs(y) + np.abs(cv) + np.abs(r) + np.abs(o))
    Xref, Xb = o[:rows], (bo + half_ulp16(o, bo))[:rows]
    x, xb = _cross(o, bo, form, emu, drop_lo=xlo(3))
    # ---- head
    xin = d["Xin"].astype(np.float64)[grow]
    x = np.concatenate([x, 0.0 * xin if mutant == "head_blind_xyz" else xin], 1)
    xb = np.concatenate([xb, np.zeros_like(xin)], 1)
    v = x @ W["W0"].T + v0[0]
    bv = C_ACC * (np.abs(x) @ np.abs(W["W0"]).T + np.abs(v0[0])) + xb @ np.abs(W["W0"]).T + lolo(x, W["W0"])
    y, dy, _ = gn(v, bv, v0)
    x, xb = _cross(y, dy, form, emu, drop_lo=xlo(4))
    w1 = W["W1"]
    if mutant == "w1_block0":
        w1 = np.concatenate([w1[:32], w1[:32]])
    bo_ = d["b_out"].astype(np.float64)
    e = x @ w1.T + bo_
    be = C_ACC * (np.abs(x) @ np.abs(w1).T + np.abs(bo_)) + xb @ np.abs(w1).T + lolo(x, w1)
    be = be + U * np.abs(e)
    e, be = e[:rows, :eps_ld], be[:rows, :eps_ld]
    return dict(X=(Xref, r16(Xref), Xb), eps=(e, r32(e), be))


def ratios(got, ref):
    """max |stored - reference| / bound per observable (got: {name: stored array} of the kernel, or a forward() result of a mutant)"""
    st = lambda v: v[1] if isinstance(v, tuple) else v
    return {k: float((np.abs(st(got[k]) - ref[k][0]) / ref[k][2]).max()) for k in ("X", "eps")}


def ratio(got, ref):
    return max(ratios(got, ref).values())
