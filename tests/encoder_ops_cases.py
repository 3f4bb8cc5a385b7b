"""Cases, float64 references and derived error bounds of the encode-side training kernels (csrc/encoder_ops.hip,
include/slide_train.h): slide_col_max_seg(_bwd) and slide_gauss_posterior_fwd / _bwd.  numpy only: the host tests use it to show
that the bounds refuse the nearest wrong arithmetic, the GPU tests to judge the kernels.

COLUMN MAX.  Integer-valued data: maxima, first indices and the scattered gradient are exact, so the comparison is equality.  The
kernel spreads a sample's rows over rt = 256 / (ld / 4) thread rows (thread row p scans rows p, p + rt, ...); the cases sit at
S = 1, 16 and rt - 1, rt, rt + 1 for each ld.

POSTERIOR.  u = 2^-24 is the unit roundoff of fp32, EXP_REL = 2^-23 the relative error of one expf (1 ulp, the intrinsic the kernel
calls).  The reference evaluates the SAME fp32 inputs in float64; the clamp and the factor 0.5 are exact.
  z = mean + std * eps, std = exp(0.5 lv):   |dz| <= std |eps| (EXP_REL + 2u) + u |z|
      (the expf, the product's rounding, the sum's rounding; a fused multiply-add only drops one of them)
  t = mean^2 + exp(lv) - 1 - lv per element: |dt| <= u mean^2 + EXP_REL exp(lv) + 3u (mean^2 + exp(lv) + 1 + |lv|)
      (the square, the expf, three additions whose partial results are bounded by the sum of the magnitudes)
  kl = 0.5 * sum t:  a term passes through at most L = ceil(S * ldz / 256) + 6 + 3 additions (the thread's own chain over its
      elements, six butterfly levels, the four wave sums), so |dkl| <= 0.5 (sum |dt| + L u sum |t|)
  dmean = dz + dkl mean:                     |d| <= u |dkl mean| + u |dmean|
  dlogvar = m (t1 + t2), t1 = dz eps 0.5 exp(0.5 lv), t2 = dkl 0.5 (exp(lv) - 1):
      |d| <= (2u + EXP_REL) |t1| + |dkl| 0.5 (EXP_REL exp(lv) + u |exp(lv) - 1|) + u |t2| + u |t1 + t2|
Every bound is multiplied by 1.01 for the second-order terms, plus one denormal (1e-45)."""
import numpy as np

U = 2.0 ** -24
EXP_REL = 2.0 ** -23
SLACK = 1.01
LV_MIN, LV_MAX = -30.0, 20.0


def ru(x, m=32):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------- column max
def row_partition(ld):
    return 256 // (ld // 4)


def _s_values(ld):
    rt = row_partition(ld)
    return sorted({1, 16, rt - 1, rt, rt + 1})


COL_MAX_CASES = [dict(name="C%d_ld%d_S%d_%s" % (C, ld, S, kind), C=C, ld=ld, S=S, kind=kind, B=3)
                 for C, ld in ((32, 32), (7, 32), (40, 64)) for S in _s_values(ld) for kind in ("mixed", "negative")]


def col_max_data(case, seed=0):
    """x [B * S, ld] float32, integer-valued with many repeated maxima; 'negative': every entry below zero (a zero-initialised
    maximum would win).  Pad columns zero, as every row-major activation."""
    rs = np.random.RandomState(seed + case["S"] * 131 + case["ld"] + case["C"])
    lo, hi = (-9, 0) if case["kind"] == "negative" else (-4, 4)
    x = rs.randint(lo, hi, size=(case["B"] * case["S"], case["ld"])).astype(np.float32)
    x[:, case["C"]:] = 0
    return x


def col_max_ref(x, B, S, C):
    ld = x.shape[1]
    v = x.reshape(B, S, ld)
    out, arg = v.max(axis=1), v.argmax(axis=1).astype(np.int32)  # numpy's argmax: the first maximum
    out[:, C:] = 0
    arg[:, C:] = -1
    return out, arg


def col_max_bwd_ref(arg, dy, S):
    B, ld = arg.shape
    dx = np.zeros((B, S, ld), np.float32)
    for b in range(B):
        for c in range(ld):
            if arg[b, c] >= 0:
                dx[b, arg[b, c], c] = dy[b, c]
    return dx.reshape(B * S, ld)


COL_MAX_STATUS = [  # (name, kwargs, NULL pointers, status)
    ("ld_zero", dict(B=2, S=4, C=0, ld=0), (), -3), ("ld_odd", dict(B=2, S=4, C=8, ld=48), (), -3),
    ("ld_big", dict(B=2, S=4, C=8, ld=1056), (), -3), ("B_negative", dict(B=-1, S=4, C=8, ld=32), (), -3),
    ("S_zero", dict(B=2, S=0, C=8, ld=32), (), -3), ("C_wide", dict(B=2, S=4, C=33, ld=32), (), -3),
    ("x_null", dict(B=2, S=4, C=8, ld=32), ("x",), -3), ("arg_null", dict(B=2, S=4, C=8, ld=32), ("arg",), -3),
    ("B_zero", dict(B=0, S=4, C=8, ld=32), ("x", "out", "arg"), 0), ("B_zero_S_zero", dict(B=0, S=0, C=8, ld=32), (), 0),
]


# ---------------------------------------------------------------------------------------------------- posterior
POSTERIOR_CASES = [dict(name="S%d_C%d_%s" % (S, C, kind), S=S, C=C, kind=kind, B=3)
                   for S, C in ((16, 16), (16, 32), (5, 7)) for kind in ("inside", "edges")]


def posterior_data(case, seed=0):
    """-> params [B * S, ldp], eps, dz [B * S, ldz], dkl [B] (float32).  'inside': log-variances in (-6, 3); 'edges': a share of them
    at +-40 (outside the clamps) and exactly at -30 and 20 (where torch's clamp passes the gradient)."""
    B, S, C = case["B"], case["S"], case["C"]
    rs = np.random.RandomState(seed + 17 * S + C + (1000 if case["kind"] == "edges" else 0))
    ldp, ldz = ru(2 * C), ru(C)
    params = np.zeros((B * S, ldp), np.float32)
    params[:, :C] = rs.standard_normal((B * S, C))
    lv = rs.uniform(-6, 3, (B * S, C))
    if case["kind"] == "edges":
        pick = rs.randint(0, 8, (B * S, C))
        for k, v in ((0, 40.0), (1, -40.0), (2, -30.0), (3, 20.0)):
            lv[pick == k] = v
    params[:, C:2 * C] = lv
    eps = np.zeros((B * S, ldz), np.float32)
    eps[:, :C] = rs.standard_normal((B * S, C))
    dz = np.zeros((B * S, ldz), np.float32)
    dz[:, :C] = rs.standard_normal((B * S, C))
    dkl = rs.uniform(0.5, 2.0, B).astype(np.float32) * np.array([1, -1, 1], np.float32)[:B]
    return params, eps, dz, dkl


def chain_length(S, ldz):
    return -(-S * ldz // 256) + 6 + 3


def posterior_fwd_ref(params, eps, B, S, C, variant=None):
    """float64 -> (z [B*S, C], kl [B], bound_z, bound_kl).  variant: one of the WRONG arithmetics of the host test (the bounds
    returned are always those of the right one)."""
    mean = params[:, :C].astype(np.float64)
    raw = params[:, C:2 * C].astype(np.float64)
    lv = raw if variant == "no_clamp" else np.clip(raw, LV_MIN, LV_MAX)
    std = np.exp(lv) if variant == "var_for_std" else np.exp(0.5 * lv)
    e = 0.0 if eps is None else eps[:, :C].astype(np.float64)
    z = mean + std * e
    var = np.exp(lv)
    t = mean ** 2 + var - 1.0 - lv
    if variant == "dropped_row":
        t = t.copy().reshape(B, S, C)
        t[:, S - 1] = 0
    kl = (1.0 if variant == "dropped_half" else 0.5) * t.reshape(B, -1).sum(axis=1)
    bz = SLACK * (std * np.abs(e) * (EXP_REL + 2 * U) + U * np.abs(z)) + 1e-45
    dt = U * mean ** 2 + EXP_REL * var + 3 * U * (mean ** 2 + var + 1.0 + np.abs(lv))
    L = chain_length(S, ru(C))
    bkl = SLACK * 0.5 * (dt.reshape(B, -1).sum(axis=1) + L * U * np.abs(t).reshape(B, -1).sum(axis=1)) + 1e-45
    return z, kl, bz, bkl


def posterior_bwd_ref(params, eps, dz, dkl, B, S, C, variant=None):
    """float64 -> (dparams [B*S, 2C], bound); dz / dkl / eps None: that term is 0"""
    mean = params[:, :C].astype(np.float64)
    raw = params[:, C:2 * C].astype(np.float64)
    lv = np.clip(raw, LV_MIN, LV_MAX)
    e = np.zeros_like(mean) if eps is None else eps[:, :C].astype(np.float64)
    g = np.zeros_like(mean) if dz is None else dz[:, :C].astype(np.float64)
    k = np.zeros(B) if dkl is None else dkl.astype(np.float64)
    if variant == "neighbour_dkl":
        k = np.roll(k, 1)
    k = np.repeat(k, S)[:, None]
    m = ((raw > LV_MIN) & (raw < LV_MAX)) if variant == "masked_at_bounds" else ((raw >= LV_MIN) & (raw <= LV_MAX))
    half = 1.0 if variant == "dropped_half" else 0.5
    dmean = g + k * mean
    var = np.exp(lv)
    t1 = g * e * half * np.exp(0.5 * lv)
    t2 = k * half * (var - 1.0)
    dlv = m * (t1 + t2)
    b_mean = U * np.abs(k * mean) + U * np.abs(dmean)
    b_lv = (2 * U + EXP_REL) * np.abs(t1) + np.abs(k) * 0.5 * (EXP_REL * var + U * np.abs(var - 1.0)) + U * np.abs(t2) + U * np.abs(t1 + t2)
    return np.concatenate([dmean, dlv], axis=1), SLACK * np.concatenate([b_mean, b_lv], axis=1) + 1e-45


def ratio(got, ref, bound):
    """worst |got - ref| / bound"""
    return float((np.abs(np.asarray(got, np.float64) - ref) / bound).max())


POSTERIOR_STATUS = [  # (name, kwargs, NULL pointers, status) for slide_gauss_posterior_fwd; params / z are required
    ("ldp_odd", dict(B=2, S=4, C=8, ldp=48, ldz=32), (), -3), ("ldz_zero", dict(B=2, S=4, C=8, ldp=32, ldz=0), (), -3),
    ("ldp_big", dict(B=2, S=4, C=8, ldp=2048, ldz=32), (), -3), ("two_C_wide", dict(B=2, S=4, C=17, ldp=32, ldz=32), (), -3),
    ("C_over_ldz", dict(B=2, S=4, C=40, ldp=96, ldz=32), (), -3), ("C_zero", dict(B=2, S=4, C=0, ldp=32, ldz=32), (), -3),
    ("S_zero", dict(B=2, S=0, C=8, ldp=32, ldz=32), (), -3), ("B_negative", dict(B=-2, S=4, C=8, ldp=32, ldz=32), (), -3),
    ("params_null", dict(B=2, S=4, C=8, ldp=32, ldz=32), ("params",), -3), ("z_null", dict(B=2, S=4, C=8, ldp=32, ldz=32), ("z",), -3),
    ("B_zero", dict(B=0, S=4, C=8, ldp=32, ldz=32), ("params", "z"), 0),
]
