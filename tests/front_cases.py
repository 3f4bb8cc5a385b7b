"""The launches that OPEN a denoiser step (slide_amd/csrc/engine.hip: SLIDE_OP_PREP_POINTS, TEMB, COND, FINALIZE_GN, COPY_COLS, ASSEMBLE_SA,
ASSEMBLE_FP), one launch at a time on synthetic data: case tables, numpy references, bounds and mutants -- shared by
tests/test_front_ops_host.py (CPU: shares, regimes, mutants) and tests/test_hip_front_ops.py (every case on the GPU).

u = 2^-24 (fp32 unit roundoff), H = 2^-11.  A library function "at one ulp" is within 2 u relative of the true function of its argument.

PREP_POINTS (prep_points_kernel).  Per sample of 16 points x [16][cx]: xyz = x[:, :3]; feat0 = [x[:, 3:] | xyz] (cast to the table's
type, leading dimension ldf); feat0_cm the same values chunk-major [c / 32][B * 16][32]; every SlidePrepCopy: kind 0 the first n
columns of feat0, kind 1 the first n columns of x; the 16 x 16 neighbour table kidx / kd2 sorted by (squared distance, index); kw the
interpolation weights of the 8 nearest BY SLOT, (1 / (d_s + 1e-8)) / sum_{s' < 8} 1 / (d_s' + 1e-8), zero in slots 8..15.
  lattice clouds (coordinates k / 8, duplicated points, equidistant neighbours): every distance is exact in fp32, so kidx / kd2 are
  BIT-EQUAL to a numpy stable sort by (float32 d2, index) and to the oracle's ora_knn_points; every copy is exact (fp16: one RNE).
  Gaussian clouds: d = fma(dz, dz, fma(dy, dy, dx dx)) with dx = fl(a - b): each difference carries u, its square 2 u, and the product and
  the two FMAs round once each on partial sums <= d:  |kd2 - d| <= D2_ULPS u d (1 + 8 u), D2_ULPS = 5.  kidx must be a permutation that
  sorts the kernel's own kd2 (ties by index), with kd2[s] within the bound of d(i, kidx[s]); it must EQUAL the reference's order in every
  slot whose reference distance is more than two bounds away from both neighbours in the sorted row; the other slots are excluded.
  kw, against float64 on the float64 distances (sorting preserves a relative bound): r = 1 / (d + c): d carries 5 u, the addition and the
  division one u each -> 7 u; the sum of eight such terms, seven additions -> 14 u; the quotient one more division:
  |kw - ref| <= KW_ULPS u ref (1 + 64 u), KW_ULPS = 7 + 14 + 1 = 22 -- relative, so it holds at duplicate points (d = 0, r = 1e8) too.

TEMB (temb_kernel).  arg = fl32(t freq[k]) as the kernel forms it; from there float64: emb = [sin arg | cos arg], h1 = swish(b1 + emb W1),
h2 = swish(b2 + h1 W2), out = bfc + h2 Wfc (weights input-major [in][out]).  sinf / cosf / expf at one ulp: d emb = 2 u |emb|.  A GEMV is
four interleaved accumulators of n_in / 4 terms, summed pairwise, plus the bias: at most n_in / 4 + 3 roundings (with or without FMA
contraction): dv = (n_in / 4 + 3) u (|in| . |W| + |b|) + d_in . |W|.  swish(v) = v / (1 + exp(-v)): expf 2 u on a term that is at most
the denominator, the addition, the division and the product one u each -> 5 u |swish(v)|; the input's uncertainty goes through swish's
slope, at most SWISH_SLOPE = 1.1 (sup |swish'| = 1.0998): d swish = SWISH_SLOPE dv + 5 u |swish(v)|.  The output layer has no swish.

COND (cond_kernel).  out = bfc + class_emb[label] Wfc, one sequential fp32 accumulation started at the bias: dim roundings:
d = (dim + 1) u (|bfc| + |ce| . |Wfc|).

FINALIZE_GN (finalize_gn_kernel).  Per (sample, channel c) with g = gid[c] >= 0: S, SS = sequential sums of sum / sq over
[gstart[g], gend[g]) (n_g terms: dS = n_g u sum |.|), mean = S inv_count, var = max(SS inv_count - mean^2, 0), rstd = 1 / sqrtf(var + eps),
scale = gamma rstd, shift = beta - mean scale; mean / var / rstd bounds: pair_cases._norm_fin (which asserts its first-order regime);
d scale = |scale| (rel + u), d shift = |mean| d scale + |scale| dm + 3 u (|beta| + |mean scale|) (pair_cases' SlideGnFin).  gid < 0:
scale 1, shift 0, exactly.  A constant group has var = 0 in the reference: rstd = 1 / sqrt(eps).

COPY_COLS (copy_cols_kernel).  dst[:, :n] = (TD)(float)src[:, :n]: exact; fp32 -> fp16 is one round-to-nearest-even (ties, subnormals,
overflow to inf included); columns past n untouched.

ASSEMBLE_SA / ASSEMBLE_FP (assemble_kernel).  Row (p, k) of a sample, nb = kidx[p][k]:
  SA  [feat[nb][:C] | xyz[nb] - xyz[p] | xyz[nb] | xyz[p] | 0 ...]            FP  [feat[nb][:C] | d2 | w | xyz[nb] | xyz[nb] - xyz[p] | xyz[p] | 0 ...]
feature and absolute columns exact copies; rel = ONE fp32 subtraction (then the cast to the table's type); d2 = kd2[p][k];
w = (1 / (d2_k + 1e-8)) / sum_{k' < K} 1 / (d2_k' + 1e-8) from the GIVEN fp32 kd2: a term 2 u (addition, division), K - 1 additions,
one division: |w - ref| <= (K + 4) u ref (1 + 64 u), then the cast (fp16: d (1 + H) + H |ref| + 2^-25).  With c_begin > 0 only the
columns >= c_begin are produced, into rows of ld_out elements; the caller's contract is c_begin <= 8 (C / 8) with 16-byte aligned
feature rows (the launcher returns -3 otherwise: the coordinate pieces would land in front of the row)."""
import zlib

import numpy as np

import pair_cases as P
from gemm_cases import EPS, U

H = 2.0 ** -11
F32, F16 = np.float32, np.float16
D2_ULPS, KW_ULPS, SWISH_SLOPE = 5, 22, 1.1
C8 = F32(1e-8)  # the kernels' 1e-8f


# A point is its own nearest neighbour: d_0 = 0 puts 1e8 into the weights' norm, and the eight far slots move it by
# sum_{s >= 8} 1 / (1e8 d_s) relative -- below KW_ULPS u unless d_8 < ~0.05.  On the k / 8 lattice and on Gaussian clouds the
# "kw_over_16" mutant is therefore the same computation at fp32 resolution; on the k / 64 lattice (d <= 3 / 256) it is not.
LATTICES = ("lattice", "lattice64")


def rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


# =================================================================================================================== PREP_POINTS
def _pp(B, cx, f16, cm, copies, kw, cloud):
    nm = "B%d_cx%d_%s_%s_%s_%s_%s" % (B, cx, "f16" if f16 else "f32", "cm" if cm else "nocm", copies, "kw" if kw else "nokw", cloud)
    return dict(name=nm, B=B, cx=cx, f16=f16, cm=cm, copies=copies, kw=kw, cloud=cloud, ldf=cx + (5 if cx % 2 else 2))


PREP_CASES = [
    _pp(1, 3, False, False, "none", True, "lattice"),
    _pp(3, 6, True, True, "one", False, "lattice"),
    _pp(17, 51, True, True, "three", True, "lattice"),
    _pp(3, 51, False, False, "one", True, "gauss"),
    _pp(17, 6, False, True, "three", True, "gauss"),
    _pp(1, 51, True, False, "three", False, "gauss"),
    _pp(3, 3, True, True, "none", True, "gauss"),
    # the k / 64 lattice: the only cloud on which the weights' normalisation over 16 slots shows (LATTICE64 below)
    _pp(3, 6, False, False, "none", True, "lattice64"),
]
PREP_BY_NAME = {c["name"]: c for c in PREP_CASES}


def prep_copies(c):
    """(n, ld, kind) per SlidePrepCopy: kind 0 copies the first n columns of feat0 (n < cx), kind 1 the coordinates (n = 3)"""
    cx = c["cx"]
    n0 = max(cx - 2, 1)
    return {"none": (), "one": ((n0, cx + 6, 0),), "three": ((n0, cx + 6, 0), (3, 5, 1), (min(cx, 4) - 1 or 1, 9, 0))}[c["copies"]]


def prep_inputs(c):
    rs = rng("prep_" + c["name"])
    B, cx = c["B"], c["cx"]
    x = rs.standard_normal((B, 16, cx)).astype(F32)
    if c["cloud"] in LATTICES:  # 125 lattice sites for 16 points: duplicates and ties
        x[:, :, :3] = rs.randint(-2, 3, (B, 16, 3)).astype(F32) / F32(8 if c["cloud"] == "lattice" else 64)
        x[:, 5, :3] = x[:, 2, :3]
        x[:, 11, :3] = x[:, 2, :3]
    return x


def d2_f32(xyz):
    """the kernel's float32 squared distances [B][16][16] (exact on the lattice)"""
    a, b = xyz[:, :, None, :], xyz[:, None, :, :]
    dx, dy, dz = (a[..., k] - b[..., k] for k in range(3))
    # fma(dz, dz, fma(dy, dy, dx dx)) evaluated in float64 and rounded per step (a float32 product is exact in float64; on the lattice
    # every step is exact anyway)
    t = (dx.astype(np.float64) ** 2).astype(F32)
    t = (dy.astype(np.float64) ** 2 + t).astype(F32)
    return (dz.astype(np.float64) ** 2 + t).astype(F32)


def d2_f64(xyz):
    x = xyz.astype(np.float64)
    return ((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1)


def kw_of(dsort, n=8):
    """float64 weights by SLOT from sorted distances [..., 16]"""
    r = 1.0 / (dsort.astype(np.float64) + np.float64(C8))
    w = r / r[..., :n].sum(-1, keepdims=True)
    w[..., 8:] = 0
    return w


def prep_reference(c, x, mutant=None):
    """dict of the launch's outputs; kd2 / kidx from float32 distances (the lattice's exact answer), kd2_64 / kw in float64"""
    B, cx = c["B"], c["cx"]
    xyz = x[:, :, :3]
    dt = F16 if c["f16"] else F32
    feat = np.concatenate([xyz, x[:, :, 3:]] if mutant == "feat_halves_swapped" else [x[:, :, 3:], xyz], 2).reshape(B * 16, cx)
    out = dict(xyz=xyz.reshape(B * 16, 3).copy(), feat0=feat.astype(dt))
    nch = (cx + 31) // 32
    cm = np.zeros((nch, B * 16, 32), dt)
    for ch in range(nch):
        w = min(32, cx - 32 * ch)
        cm[ch, :, :w] = out["feat0"][:, 32 * ch:32 * ch + w]
    out["feat0_cm"], out["cm_valid"] = cm, np.arange(nch * 32).reshape(nch, 1, 32) < cx
    out["copies"] = [(x.reshape(B * 16, cx)[:, :n] if kind else feat[:, :n]).astype(dt) for n, _, kind in prep_copies(c)]
    d32, d64 = d2_f32(xyz), d2_f64(xyz)
    key = -np.arange(16) if mutant == "tie_larger_index" else np.arange(16)
    order = np.lexsort((np.broadcast_to(key, d32.shape), d32), axis=-1).astype(np.int32)
    out["kidx"], out["kd2"] = order, np.take_along_axis(d32, order, -1)
    out["kidx_64"] = np.argsort(d64, -1, kind="stable").astype(np.int32)
    out["kd2_64"], out["d64"] = np.take_along_axis(d64, out["kidx_64"].astype(np.int64), -1), d64
    kw = kw_of(out["kd2_64"], 16 if mutant == "kw_over_16" else 8)
    if mutant == "kw_by_neighbour":
        byn = np.zeros_like(kw)
        np.put_along_axis(byn, order.astype(np.int64), kw, -1)
        kw = byn
    out["kw"] = kw
    return out


def tied_share(kd2):
    """the share of adjacent slots of the sorted rows that hold the same distance"""
    return float((kd2[..., 1:] == kd2[..., :-1]).mean())


def d2_bound(d):
    return D2_ULPS * U * d * (1 + 8 * U)


def decided_slots(kd2_64):
    """slots whose reference distance is more than two bounds from both neighbours of the sorted row: the order is decided there"""
    b = d2_bound(kd2_64)
    gap = np.diff(kd2_64, axis=-1)
    need = 2 * np.maximum(b[..., 1:], b[..., :-1])
    ok = np.ones(kd2_64.shape, bool)
    ok[..., 1:] &= gap > need
    ok[..., :-1] &= gap > need
    return ok


PREP_MUTANTS = ("tie_larger_index", "kw_over_16", "kw_by_neighbour", "feat_halves_swapped")


# =================================================================================================================== TEMB
def _te(nsamp, t_dim, n_out, ts):
    return dict(name="n%d_td%d_o%d_%s" % (nsamp, t_dim, n_out, "tdev" if ts is None else "ts"), nsamp=nsamp, t_dim=t_dim, n_out=n_out, ts=ts)


T_DEV0 = 7
TEMB_CASES = [_te(1, 32, 40, None), _te(5, 128, 600, (0.0, 1.0, 999.0, 500.0, 37.0)), _te(5, 32, 600, (999.0, 0.0, 1.0, 2.0, 250.0)),
              _te(1, 128, 40, (999.0,))]
TEMB_MUTANTS = ("sincos_swapped", "sigmoid", "weights_out_in", "t_minus_1")


def temb_inputs(c):
    rs = rng("temb_" + c["name"])
    td, no = c["t_dim"], c["n_out"]
    Hd = 4 * td
    f = lambda *s: rs.standard_normal(s).astype(F32)
    hd = td // 2
    return dict(freq=np.exp(-np.log(10000.0) * np.arange(hd) / (hd - 1)).astype(F32), w1=f(td, Hd) / F32(np.sqrt(td)), b1=0.5 * f(Hd),
                w2=f(Hd, Hd) / F32(np.sqrt(Hd)), b2=0.5 * f(Hd), wfc=f(Hd, no) / F32(np.sqrt(Hd)), bfc=0.5 * f(no))


def _swish(v, dv, sigmoid=False):
    s = 1.0 / (1.0 + np.exp(-v))
    y = s if sigmoid else v * s
    return y, SWISH_SLOPE * dv + 5 * U * np.abs(y)


def temb_forward(c, d, mutant=None):
    """(out [nsamp][n_out] float64, bound)"""
    t = np.array(c["ts"] if c["ts"] is not None else [float(T_DEV0)], F32)
    if mutant == "t_minus_1":
        t = t - F32(1)
    arg = (t[:, None] * d["freq"][None, :]).astype(F32).astype(np.float64)  # the kernel's own float32 product
    halves = [np.cos(arg), np.sin(arg)] if mutant == "sincos_swapped" else [np.sin(arg), np.cos(arg)]
    x = np.concatenate(halves, 1)
    dx = 2 * U * np.abs(x)
    for wk, bk, act in (("w1", "b1", True), ("w2", "b2", True), ("wfc", "bfc", False)):
        w, b = d[wk].astype(np.float64), d[bk].astype(np.float64)
        if mutant == "weights_out_in":
            w = d[wk].reshape(w.shape[1], w.shape[0]).T.astype(np.float64)  # the same memory read as [out][in]
        n_in = w.shape[0]
        v = x @ w + b
        dv = (n_in / 4 + 3) * U * (np.abs(x) @ np.abs(w) + np.abs(b)) + dx @ np.abs(w)
        x, dx = _swish(v, dv, mutant == "sigmoid") if act else (v, dv)
    return x, dx


# =================================================================================================================== COND
NCLS = 6
COND_CASES = [dict(name="B%d_d%d_o%d" % (B, dim, no), B=B, dim=dim, n_out=no) for B, dim, no in ((1, 8, 40), (5, 128, 600), (5, 8, 600),
                                                                                                  (1, 128, 40))]
COND_MUTANTS = ("label_of_neighbour", "weights_out_in")


def cond_inputs(c):
    rs = rng("cond_" + c["name"])
    f = lambda *s: rs.standard_normal(s).astype(F32)
    label = np.array([NCLS - 1, 0, 3, NCLS - 1, 1][:c["B"]] if c["B"] > 1 else [0 if c["dim"] == 8 else NCLS - 1], np.int64)
    return dict(label=label, emb=f(NCLS, c["dim"]), wfc=f(c["dim"], c["n_out"]) / F32(np.sqrt(c["dim"])), bfc=0.5 * f(c["n_out"]))


def cond_forward(c, d, mutant=None):
    lab = d["label"]
    if mutant == "label_of_neighbour":
        lab = np.roll(lab, -1) if c["B"] > 1 else (lab + 1) % NCLS
    w = d["wfc"].astype(np.float64)
    if mutant == "weights_out_in":
        w = d["wfc"].reshape(w.shape[1], w.shape[0]).T.astype(np.float64)
    ce, b = d["emb"].astype(np.float64)[lab], d["bfc"].astype(np.float64)
    return ce @ w + b, (c["dim"] + 1) * U * (np.abs(ce) @ np.abs(w) + np.abs(b))


# =================================================================================================================== FINALIZE_GN
# runs [gstart, gend) of unequal lengths that straddle the producers' boundaries (a producer = a block of PRODUCER channels)
PRODUCER = 8
FIN_RUNS = ((0, 3), (3, 11), (11, 12), (12, 21), (21, 29))  # lengths 3, 8, 1, 9, 8; (12, 21) is the CONSTANT group
FIN_CONST = 3
FIN_C, FIN_BS, FIN_NPX = 32, 40, 128  # channels 29..31 belong to no group (gid -1); bs > C
FIN_CASES = [dict(name="B%d" % B, B=B) for B in (1, 5)]
FIN_MUTANTS = ("gend_inclusive", "mean_by_len")


def fin_inputs(c):
    rs = rng("fin_" + c["name"])
    B = c["B"]
    v = rs.standard_normal((B, FIN_NPX, FIN_BS)) + rs.uniform(-2, 2, (B, 1, FIN_BS))
    lo, hi = FIN_RUNS[FIN_CONST]
    v[:, :, lo:hi] = 0.5  # sums FIN_NPX / 2 and FIN_NPX / 4: exact in fp32
    gid = np.full(FIN_C, -1, np.int32)
    for g, (a, b) in enumerate(FIN_RUNS):
        gid[a:b] = g
    gid[1], gid[2] = 1, 4  # a channel need not lie inside the run of its group
    f = lambda *s: rs.standard_normal(s).astype(F32)
    return dict(sum=v.sum(1).astype(F32), sq=(v * v).sum(1).astype(F32), gid=gid, gstart=np.array([r[0] for r in FIN_RUNS], np.int32),
                gend=np.array([r[1] for r in FIN_RUNS], np.int32), gamma=1 + 0.2 * f(FIN_C), beta=0.2 * f(FIN_C),
                inv_count=F32(1.0 / (PRODUCER * FIN_NPX)))


def fin_forward(c, d, mutant=None):
    """(scale, shift, dscale, dshift) [B][C] float64; (1, 0, 0, 0) where gid < 0"""
    B = c["B"]
    G = len(FIN_RUNS)
    S, SS, dS, dSS = (np.zeros((B, G)) for _ in range(4))
    inv = np.full(G, float(d["inv_count"]))
    for g, (a, b) in enumerate(FIN_RUNS):
        b = b + 1 if mutant == "gend_inclusive" else b
        s, q = d["sum"].astype(np.float64)[:, a:b], d["sq"].astype(np.float64)[:, a:b]
        S[:, g], SS[:, g] = s.sum(1), q.sum(1)
        dS[:, g], dSS[:, g] = (b - a) * U * np.abs(s).sum(1), (b - a) * U * q.sum(1)
        if mutant == "mean_by_len":
            inv[g] = 1.0 / ((b - a) * FIN_NPX)
    m, var, rstd, dm, rel = P._norm_fin(S, SS, dS, dSS, inv[None, :])
    gid = d["gid"]
    on = gid >= 0
    gi = np.where(on, gid, 0)
    gam, bet = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
    scl = np.where(on, gam * rstd[:, gi], 1.0)
    sft = np.where(on, bet - m[:, gi] * scl, 0.0)
    dscl = np.where(on, np.abs(scl) * (rel[:, gi] + U), 0.0)
    dsft = np.where(on, np.abs(m[:, gi]) * dscl + np.abs(scl) * dm[:, gi] + 3 * U * (np.abs(bet) + np.abs(m[:, gi] * scl)), 0.0)
    return scl, sft, dscl, dsft, var


# =================================================================================================================== COPY_COLS
COPY_CASES = [dict(name="%s_to_%s" % ("f16" if s else "f32", "f16" if t else "f32"), src_f16=s, dst_f16=t, rows=37, n=21, src_ld=24, dst_ld=29)
              for s in (0, 1) for t in (0, 1)]
# fp32 values whose conversion to fp16 is a tie, a subnormal, an underflow or an overflow
COPY_EDGES = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, -(1 + 2.0 ** -11), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                       2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -14 - 2.0 ** -25, 65504.0, 65519.996, 65520.0, -65520.0, 0.0, -0.0, 1e-10, 1e10,
                       np.inf, -np.inf, 0.1, 1 / 3], F32)


def copy_inputs(c):
    rs = rng("copy_" + c["name"])
    src = rs.standard_normal((c["rows"], c["src_ld"])).astype(F32)
    src[:3, :7] = COPY_EDGES.reshape(3, 7)
    src[5:8, 14:21] = -COPY_EDGES.reshape(3, 7)
    with np.errstate(over="ignore"):  # (1e10 and 65520 become inf in an fp16 source: inf is a value to copy like any other)
        return src.astype(F16) if c["src_f16"] else src


# =================================================================================================================== ASSEMBLE
def _as(fp, K, f16, C, ldf_pad, c_begin, ld_extra=0):
    ncoord = 11 if fp else 9
    ldg = (C + ncoord + 7) // 8 * 8 + 8  # a whole piece of zero pad behind the coordinates
    nm = "%s_K%d_%s_C%d_ldf%d_cb%d" % ("fp" if fp else "sa", K, "f16" if f16 else "f32", C, C + ldf_pad, c_begin)
    return dict(name=nm, fp=fp, K=K, f16=f16, C=C, ldf=C + ldf_pad, ldg=ldg, c_begin=c_begin, ld_out=(ldg - c_begin + ld_extra) if c_begin else ldg,
                B=3, status=0)


ASM_CASES = [
    _as(False, 16, True, 48, 8, 0), _as(False, 8, False, 51, 5, 0), _as(False, 16, False, 51, 1, 0),  # (ldf 52 floats: aligned; 53 would not be)
    _as(False, 8, True, 51, 5, 32, 8), _as(False, 16, True, 51, 2, 0),  # ldf 53 halves: nbulk = 0
    _as(True, 8, True, 48, 0, 32, 8), _as(True, 16, False, 51, 2, 0), _as(True, 8, False, 48, 8, 32, 8), _as(True, 16, True, 51, 4, 0),
    _as(True, 8, False, 51, 2, 0),
]
for _c in (_as(False, 8, True, 51, 2, 32, 8), _as(True, 16, False, 16, 0, 32, 8)):  # c_begin beyond the whole-vector pieces: refused
    _c["status"] = -3
    _c["name"] += "_refused"
    ASM_CASES.append(_c)
ASM_BY_NAME = {c["name"]: c for c in ASM_CASES}
ASM_MUTANTS = ("rel_swapped", "w_over_16", "fp_abs_rel_exchanged")


def asm_nbulk(c):
    return c["C"] // 8 if ((2 if c["f16"] else 4) * c["ldf"]) % 16 == 0 else 0


def asm_mutants(c):
    if c["status"]:
        return []
    return ["rel_swapped"] + ((["w_over_16"] if c["K"] == 8 else []) + ["fp_abs_rel_exchanged"] if c["fp"] else [])


def asm_inputs(c):
    rs = rng("asm_" + c["name"])
    B, C = c["B"], c["C"]
    dt = F16 if c["f16"] else F32
    feat = np.full((B * 16, c["ldf"]), np.nan, dt)
    feat[:, :C] = rs.standard_normal((B * 16, C)).astype(dt)
    kidx = rs.randint(0, 16, (B * 16, 16)).astype(np.int32)  # any table: repeated neighbours, the point itself anywhere
    kidx[::3, 1] = kidx[::3, 0]
    return dict(xyz=rs.standard_normal((B * 16, 3)).astype(F32), feat=feat, kidx=kidx, kd2=rs.uniform(0, 4, (B * 16, 16)).astype(F32) *
                (rs.uniform(size=(B * 16, 16)) > 0.1).astype(F32))  # (a tenth of the distances zero: duplicate points)


def asm_forward(c, d, mutant=None):
    """(g [B * 16 * K][ldg] float64 of the FULL source layout, bound, exact mask): exact columns must match bit for bit after the cast"""
    B, C, K, ldg = c["B"], c["C"], c["K"], c["ldg"]
    rows = B * 16 * K
    p = np.repeat(np.arange(B * 16), K)
    k = np.tile(np.arange(K), B * 16)
    nb = (p // 16) * 16 + d["kidx"][p, k]
    g, bnd = np.zeros((rows, ldg)), np.zeros((rows, ldg))
    g[:, :C] = d["feat"][nb, :C].astype(np.float64)
    xq, xp = d["xyz"][nb], d["xyz"][p]
    rel = (xp - xq if mutant == "rel_swapped" else xq - xp).astype(np.float64)  # (float32 subtraction, then widened)
    if not c["fp"]:
        g[:, C:C + 9] = np.concatenate([rel, xq, xp], 1)
    else:
        kd = d["kd2"].astype(np.float64)
        r = 1.0 / (kd + np.float64(C8))
        w = r / r[:, :16 if mutant == "w_over_16" else K].sum(1, keepdims=True)
        g[:, C], g[:, C + 1] = kd[p, k], w[p, k]
        bnd[:, C + 1] = (K + 4) * U * w[p, k] * (1 + 64 * U)
        g[:, C + 2:C + 11] = np.concatenate([rel, xq, xp] if mutant == "fp_abs_rel_exchanged" else [xq, rel, xp], 1)
    if c["fp"] and c["f16"]:
        bnd[:, C + 1] = bnd[:, C + 1] * (1 + H) + H * np.abs(g[:, C + 1]) + 2.0 ** -25
    exact = np.ones(ldg, bool)
    if c["fp"]:
        exact[C + 1] = False
    return g, bnd, exact
