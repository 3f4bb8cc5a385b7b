"""The definition of the refine-and-upsample front (include/slide_hip.h Part 9) restated in numpy float32, the cases the tests run it
on, and the error bound of the network case.

Every numpy operation below acts on float32 arrays and float32 scalars, so every product, sum and quotient is rounded once, in the
order the header writes them -- the order of the reference's torch expressions (data_utils/mirror_partial.py,
models/point_upsample_module.py, the tail of dpsr_evaluation.network_output_to_dpsr_grid).  tests/test_refine_host.py pins this
restatement to the reference's own outputs (tests/golden/golden_refine.npz, tools/gen_golden_refine.py) bit for bit.

`wrong` selects one of the nearest wrong arithmetics instead; the host test shows that each of them differs from the golden somewhere,
so bit equality on the GPU tells them apart:
  fma          child = fma(t, s, x): the product t * s is not rounded
  gs           d * (g * s) for (d * g) * s
  rsqrtf       g = 1 / sqrtf(factor) in float32 for (float)(1 / sqrt((double)factor))
  centroid     the centroid of the children for the centre of their box
  rcp12        * (1 / 1.2f) for / 1.2f
  parent_box   the box of the parents X for the box of the children
  no_roundtrip (mirror) only the mirrored axis is recomputed; the other two are copied and not taken through (x - c) + c
"""
import numpy as np

F = np.float32
TILE = 256  # output rows per workgroup (slide_refine_span(0))


# ------------------------------------------------------------------------------------------------------------ restatement
def mirror_center(x):
    """(B, 3) float32: the float64 mean rounded once"""
    return x[:, :, 0:3].astype(np.float64).mean(axis=1).astype(F)


def mirror_concat(x, center, axis=2, attach_label=True, perm=None, wrong=None):
    """x (B, N, C) f32, center (B, 3) f32 -> (B, 2N, C + attach_label)"""
    x = np.asarray(x, F)
    B, N, C = x.shape
    c = np.asarray(center, F)[:, None, :]
    m = x.copy()
    xyz = m[:, :, 0:3] - c
    xyz[:, :, axis] = -xyz[:, :, axis]
    back = xyz + c
    if wrong == "no_roundtrip":
        keep = x[:, :, 0:3].copy()
        keep[:, :, axis] = back[:, :, axis]
        back = keep
    else:
        assert wrong is None
    m[:, :, 0:3] = back
    if C >= 6:
        m[:, :, axis + 3] = -m[:, :, axis + 3]
    a, b = x, m
    if attach_label:
        a = np.concatenate([x, np.ones((B, N, 1), F)], axis=2)
        b = np.concatenate([m, -np.ones((B, N, 1), F)], axis=2)
    out = np.concatenate([a, b], axis=1)
    if perm is not None:
        out = out[:, np.asarray(perm, np.int64), :]
    return np.ascontiguousarray(out)


def _fma(t, s, x):
    """x + t * s with the product unrounded (float32 x float32 is exact in float64)"""
    return (x.astype(np.float64) + t.astype(np.float64) * np.float64(s)).astype(F)


def point_upsample(X, disp, factor, first=False, center=False, out_scale=0.001, wrong=None):
    """X (B, n, 6), disp (B, n, 6 k) -> the children (B, R, 6)"""
    X, disp = np.asarray(X, F), np.asarray(disp, F)
    B, n, _ = X.shape
    g = F(1.0 / np.sqrt(np.float64(factor)))
    if wrong == "rsqrtf":
        g = F(1) / np.sqrt(F(factor))
    s = F(out_scale)
    assert first or not center
    kp = factor - 1 if center else factor
    if first:
        assert disp.shape[2] == 6 * (kp + 1)
        mid = _fma(disp[:, :, 0:6], s, X) if wrong == "fma" else X + disp[:, :, 0:6] * s
        d = disp[:, :, 6:]
    else:
        assert disp.shape[2] == 6 * kp
        mid, d = X, disp
    d = d.reshape(B, n, kp, 6)
    if wrong == "gs":
        child = mid[:, :, None, :] + d * (g * s)
    elif wrong == "fma":
        child = _fma(d * g, s, np.broadcast_to(mid[:, :, None, :], d.shape))
    else:
        child = mid[:, :, None, :] + (d * g) * s
    child = child.reshape(B, n * kp, 6)
    if center:
        child = np.concatenate([child, mid], axis=1)
    return np.ascontiguousarray(child.astype(F))


def refine_to_dpsr(X, disp, factor, first=False, center=False, out_scale=0.001, mode="normalize", scale=1, ldx=6, only_orig=False,
                   wrong=None):
    """-> points (B, R, 3), normals (B, R, 3), bbox (B, 2, 3), all float32"""
    X, disp = np.asarray(X, F), np.asarray(disp, F)
    assert X.shape[2] == ldx
    rows = X.shape[1] // 2 if only_orig else X.shape[1]
    X6, d = X[:, :rows, 0:6], disp[:, :rows]
    child = point_upsample(X6, d, factor, first, center, out_scale, wrong if wrong in ("fma", "gs", "rsqrtf") else None)
    p, normals = child[:, :, 0:3], child[:, :, 3:6]
    box_of = X6[:, :, 0:3] if wrong == "parent_box" else p
    mn, mx = box_of.min(axis=1, keepdims=True), box_of.max(axis=1, keepdims=True)
    bbox = np.concatenate([mn, mx], axis=1)
    if mode == "normalize":
        ctr = (mx + mn) / F(2)
        if wrong == "centroid":
            ctr = p.astype(np.float64).mean(axis=1, keepdims=True).astype(F)
        L = (mx - mn).max(axis=2, keepdims=True)
        q = (p - ctr) / L * F(0.99)
    else:
        assert mode == "scale"
        q = p / F(scale) / F(2)
    q = q * (F(1) / F(1.2)) + F(0.5) if wrong == "rcp12" else q / F(1.2) + F(0.5)
    q = np.minimum(np.maximum(q, F(0)), F(0.99))
    assert q.dtype == F and normals.dtype == F
    return np.ascontiguousarray(q), np.ascontiguousarray(normals), np.ascontiguousarray(bbox)


# ------------------------------------------------------------------------------------------------------------ cases
# name: B, M (points per sample as the kernel sees them), factor, form, ldx, only_orig, mode, scale, out_scale, sigma of the points
REFINE_CASES = {
    # 185 children: one ragged tile
    "n37_plain_norm": dict(B=3, M=37, factor=5, form="plain", ldx=6, only_orig=False, mode="normalize", scale=1, out_scale=0.001, sigma=0.4),
    "n37_first_norm": dict(B=2, M=37, factor=5, form="first", ldx=6, only_orig=False, mode="normalize", scale=1, out_scale=0.05, sigma=0.4),
    "n37_center_norm": dict(B=2, M=37, factor=5, form="center", ldx=6, only_orig=False, mode="normalize", scale=1, out_scale=0.05, sigma=0.4),
    # scale mode with elements clamped at both ends
    "n37_plain_scale": dict(B=3, M=37, factor=5, form="plain", ldx=6, only_orig=False, mode="scale", scale=0.7, out_scale=0.05, sigma=0.4),
    "n37_first_scale_ldx7": dict(B=2, M=37, factor=5, form="first", ldx=7, only_orig=False, mode="scale", scale=0.7, out_scale=0.001, sigma=0.4),
    # the indicator behind the six channels, only the first half split
    "n74_split_norm_ldx7": dict(B=2, M=74, factor=5, form="plain", ldx=7, only_orig=True, mode="normalize", scale=1, out_scale=0.001, sigma=0.4),
    # 7000 children over 28 tiles, the last ragged (88 rows): every axis has one extreme in the first tile and one in the last
    "n700_plain_norm": dict(B=2, M=700, factor=10, form="plain", ldx=6, only_orig=False, mode="normalize", scale=1, out_scale=0.001, sigma=0.4),
    # factor 6: the smallest factor above 1 at which the float32 1 / sqrtf differs from the rounded double 1 / sqrt (5 and 10 agree)
    "n37_plain_norm_f6": dict(B=1, M=37, factor=6, form="plain", ldx=6, only_orig=False, mode="normalize", scale=1, out_scale=0.05, sigma=0.4),
}
BIG = "n700_plain_norm"
BIG_ROWS = 384  # rows of the big case the fixture records: the first and the last 128 (they hold the extremes) and 128 spread between


def big_rows(R):
    e = BIG_ROWS // 3
    mid = np.linspace(e, R - e - 1, e).astype(np.int64)
    return np.unique(np.concatenate([np.arange(e), mid, np.arange(R - e, R)]))


def form_flags(form):
    return {"plain": (False, False), "first": (True, False), "center": (True, True)}[form]


def disp_width(factor, form):
    return 6 * {"plain": factor, "first": factor + 1, "center": factor}[form]


def out_rows(c):
    rows = c["M"] // 2 if c["only_orig"] else c["M"]
    return rows * (c["factor"] - 1) + rows if c["form"] == "center" else rows * c["factor"]


def refine_inputs(name):
    """X (B, M, ldx), disp (B, M, dw) float32 of a case (seeded by its position in the table)"""
    c = REFINE_CASES[name]
    rs = np.random.RandomState(1000 + list(REFINE_CASES).index(name))
    B, M = c["B"], c["M"]
    X = np.zeros((B, M, c["ldx"]), F)
    X[:, :, 0:3] = (c["sigma"] * rs.standard_normal((B, M, 3))).astype(F)
    nrm = rs.standard_normal((B, M, 3))
    X[:, :, 3:6] = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(F)
    if c["ldx"] == 7:
        X[:, :, 6] = np.where(np.arange(M) < M // 2, 1, -1).astype(F)
    disp = rs.standard_normal((B, M, disp_width(c["factor"], c["form"]))).astype(F)
    if name == BIG:
        # x: maximum in the first tile, minimum in the last; y: minimum first, maximum last; z: maximum first, minimum last
        last = M - 1
        for b in range(B):
            X[b, 0, 0], X[b, last, 0] = 3.0 + b, -2.5
            X[b, 1, 1], X[b, last - 1, 1] = -2.75, 2.25 + b
            X[b, 2, 2], X[b, last - 2, 2] = 2.0, -3.5
    return X, disp


def refine_kwargs(name):
    c = REFINE_CASES[name]
    first, center = form_flags(c["form"])
    return dict(factor=c["factor"], first=first, center=center, out_scale=c["out_scale"], mode=c["mode"], scale=c["scale"], ldx=c["ldx"],
                only_orig=c["only_orig"])


# mirror: every axis with 3, 6 and 7 channels (label and permutation on), and the label / permutation switches on one of them
MIRROR_CASES = {"a%d_c%d_lp" % (a, C): dict(B=2, N=19, C=C, axis=a, label=True, perm=True) for a in (0, 1, 2) for C in (3, 6, 7)}
MIRROR_CASES.update({
    "a2_c6_l": dict(B=2, N=19, C=6, axis=2, label=True, perm=False),
    "a1_c6_p": dict(B=2, N=19, C=6, axis=1, label=False, perm=True),
    "a0_c3": dict(B=1, N=300, C=3, axis=0, label=False, perm=False),  # more rows than one workgroup's threads in the centre's sum
})
MIRROR_PERM_SEED = 5


def mirror_inputs(name):
    c = MIRROR_CASES[name]
    rs = np.random.RandomState(2000 + list(MIRROR_CASES).index(name))
    x = rs.standard_normal((c["B"], c["N"], c["C"])).astype(F)
    x[:, :, 0:3] = (x[:, :, 0:3] * F(0.4) + rs.uniform(-0.3, 0.3, (c["B"], 1, 3)).astype(F)).astype(F)
    return x


# ------------------------------------------------------------------------------------------------------------ the network case's bound
NET_DISP_TOL = 2e-4  # the module path's displacement against the reference's, max-norm relative to the largest entry
EPS = 2.0 ** -24     # half an ulp of a float32 in [1, 2): the relative error of one rounding


def network_point_bound(disp_ref, refined_child_absmax, L, factor, out_scale):
    """The largest |points - reference points| (and |normals - reference normals|) that a displacement within NET_DISP_TOL of the
    reference's allows, per sample of box length L (array):

      e_d  = NET_DISP_TOL max |d|                                     the displacement's error
      e_c  = g s e_d + 3 EPS max |child|                              child = x + (d g) s: linear in d, and three roundings
      mn, mx move by at most e_c, so ctr by e_c and L by 2 e_c;  with |child - ctr| <= L / 2 (the child is inside the box)
      |d p| <= 0.99 / (1.2 (L - 2 e_c)) (e_c + e_c + (L / 2) 2 e_c / L) = 0.99 / (1.2 (L - 2 e_c)) 3 e_c,
      plus five roundings of values below 1 ((. - ctr), / L, * 0.99, / 1.2, + 0.5); the clamp is 1-Lipschitz.
    -> (bound on the points (B,), bound on the normals (scalar))"""
    g, s = 1.0 / np.sqrt(float(factor)), float(out_scale)
    e_d = NET_DISP_TOL * float(np.abs(disp_ref).max())
    e_c = g * s * e_d + 3 * EPS * float(refined_child_absmax)
    L = np.asarray(L, np.float64)
    return 0.99 / (1.2 * (L - 2 * e_c)) * 3 * e_c + 5 * EPS, e_c
