"""Shared by the tests of the grouping layer's coordinate gradient (no test in here, no GPU): a float64 torch restatement of the
reference's two grouping operators on GIVEN neighbour indices, a second, direct statement of their gradient (the closed formulas
of include/slide_train.h slide_group_rows_coord_bwd as explicit loops, with deliberately wrong variants), the case matrix and the
elementwise error bound.

THE OPERATORS (pointnet2_ops_lib/pointnet2_ops/pointnet2_utils.py).  `oracle_rows` restates QueryAndGroup.forward lines 383-408
(abs = xyz gathered at idx, the empty-ball substitution have_neigh * abs + no_neigh * centre, rel = abs - centre, the concatenation
[rel | abs | centre]) and group_knn lines 506-520 (dist, dist_recip = 1 / (dist + 1e-8), norm, weight, [dist | weight | abs | rel |
x_repeat]) with torch.gather, in float64, and torch's autograd differentiates them.  pytorch3d's knn_points returns dist as a
differentiable |x - nn|^2; its VALUE here is the fp32 array the forward kernel was given.

THE BOUND.  An element of a gradient is a sum of n terms, one per grouped row that touches it: n = K for a centre, the in-degree for
a source point.  |err| <= gamma(n + c) S, gamma(m) = m u / (1 - m u), u = 2^-24, S = the sum of the magnitudes of the element's
terms (every product and difference taken at the magnitudes of its parts: no cancellation credit).  Rounding steps of the kernel
(csrc/group_coord_bwd.hip, compiled without contraction: one rounding per operation), relative to the exact value from the same
fp32 inputs:
  SA form.  A term is g_rel + g_abs (source) or -g_rel + g_ctr (centre; empty ball: g_abs + g_ctr): 1.  The n terms are added to
    a zero: n - 1.  Together n: c = 0.
  FP form, K neighbours.
    r = 1 / (d2 + 1e-8)            the fp32 constant, the addition, the division              3
    S = sum_k r_k                  positive terms, so relative: 3 + (K - 1)                   K + 2
    w = r / S                      3 + (K + 2) + 1                                            K + 6
    T = sum_j g_w_j w_j            product 1, K - 1 additions, relative to sum |g_w_j| w_j    2 K + 6
    g_w - T                        1 more, relative to M_w = |g_w| + sum |g_w_j| w_j          2 K + 7
    r r / S                        (3 + 3 + 1) + (K + 2) + 1                                  K + 10
    (r r / S) (g_w - T)            (K + 10) + (2 K + 7) + 1                                   3 K + 18
    G = g_d2 - ...                 1 more, relative to M_G = |g_d2| + (r r / S) M_w           3 K + 19
    v = (2 G) (q - c)              the difference 1, the product 1 (2 x is exact)             3 K + 21
    (v + g_abs) + g_rel  or  (-v - g_rel) + g_ctr                                     2       3 K + 23
    the n terms are added to a zero: n - 1.  Together n + 3 K + 22: c = 3 K + 22.
  With a coincident neighbour r = 1e8 and r r / S is up to 1e8: the magnitude sum carries that factor, and carries (q - c) = 0 with
  it, so v is bounded by -- and is -- exactly 0 there.
A gradient that arrives through further fp32 operations (the chain test: a linear map's row sums, a scale) adds their roundings to c
(`extra`).  Nothing here is fitted to a result."""
import functools

import numpy as np
import torch

from slide_amd import abi

U = 2.0 ** -24
FP, ABS, CENTER, NO_XYZ, IDX32 = 1, 2, 4, 8, 16
MUTANTS = ("no_w_coupling", "no_factor_2", "centre_rel_sign", "no_g_d2", "counts_ignored")


def ru(c):
    return max(32, abi.ru(c))  # (a row has at least one 32-column block)


def ncoord(flags):
    return 11 if flags & FP else 0 if flags & NO_XYZ else 3 + (3 if flags & ABS else 0) + (3 if flags & CENTER else 0)


def extra_roundings(flags, K):
    return 3 * K + 22 if flags & FP else 0


def tolerance(S, n, flags, K, extra=0):
    """S (..., 3) magnitude sums, n (...) term counts -> the elementwise bound"""
    m = (np.asarray(n, np.float64)[..., None] + extra_roundings(flags, K) + extra) * U
    return m / (1 - m) * S


def worst(got, want, tol):
    """largest err / tol (an element whose bound is zero must be exact: inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    if not np.all(err[tol == 0] == 0) or not np.isfinite(err).all():
        return float("inf")
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------------------- the case matrix
def _knn(centres, src, K):
    """float64 brute force -> (idx (B, np, K) int64 ascending distance, d2 fp32 of the float64 squared distances)"""
    D = ((centres.astype(np.float64)[:, :, None] - src.astype(np.float64)[:, None]) ** 2).sum(-1)
    idx = np.argsort(D, axis=2, kind="stable")[:, :, :K]
    return idx.astype(np.int64), np.take_along_axis(D, idx, axis=2).astype(np.float32)


def _ball(centres, src, radius, nsample):
    """ball_query's rule: the first nsample source points (index order) inside the radius, the first one repeated to fill up; an
    empty ball keeps index 0 -> (idx int32, counts int32)"""
    D = ((centres.astype(np.float64)[:, :, None] - src.astype(np.float64)[:, None]) ** 2).sum(-1)
    B, P, _ = D.shape
    idx, counts = np.zeros((B, P, nsample), np.int32), np.zeros((B, P), np.int32)
    for b in range(B):
        for p in range(P):
            hit = np.nonzero(D[b, p] < radius * radius)[0][:nsample]
            counts[b, p] = len(hit)
            if len(hit):
                idx[b, p] = hit[0]
                idx[b, p, :len(hit)] = hit
    return idx, counts


SHAPES = {  # name: (N, np, nsample)
    "base8": (40, 24, 8), "base16": (40, 24, 16), "clamp": (5, 7, 8), "fan300": (3, 300, 3), "one": (40, 1, 8)}
FORMS = {"sa": 0, "sa_abs": ABS, "sa_ctr": CENTER, "sa_abs_ctr": ABS | CENTER, "fp": FP}


def _cases():
    out = []
    for form in FORMS:
        for C in (0, 5, 29, 32):
            out.append(dict(name="%s-base8-C%d" % (form, C), form=form, shape="base8", C=C))
        for shape in ("base16", "clamp", "fan300", "one"):
            out.append(dict(name="%s-%s-C5" % (form, shape), form=form, shape=shape, C=5))
    for form in ("sa", "sa_abs_ctr"):
        out.append(dict(name="%s-ball-C5" % form, form=form, shape="ball", C=5))
    out.append(dict(name="fp-coincident-C5", form="fp", shape="coincident", C=5))
    return out


CASES = _cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}
B = 2


@functools.lru_cache(maxsize=None)
def make_data(name):
    """fp32 inputs of a case: xyz (B, N, 3), new_xyz (B, np, 3), idx, d2 (FP form), counts (ball case), dout [B*np*K, ldg] (random in
    EVERY column: the kernel must read the coordinate columns only), feat [B*N, ldf] or None.  Never modified."""
    c = CASE_BY_NAME[name]
    flags, C = FORMS[c["form"]], c["C"]
    rs = np.random.RandomState(hash_name(name))
    d2 = counts = None
    if c["shape"] == "ball":
        N, P, K = 24, 12, 6
        xyz = rs.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        new_xyz = rs.uniform(-1, 1, (B, P, 3)).astype(np.float32)
        new_xyz[:, 0] = 9.0                       # far from every source point: an empty ball
        new_xyz[:, 1] = xyz[:, 3] + 0.01          # at least one neighbour
        idx, counts = _ball(new_xyz, xyz, 0.6, K)
        part = (counts > 0) & (counts < K)
        assert (counts == 0).any() and part.any() and (idx[part][:, -1] == idx[part][:, 0]).all()  # empty, and partly filled with repeats
        flags |= IDX32
    elif c["shape"] == "coincident":
        N = P = 20
        K = 8
        xyz = rs.standard_normal((B, N, 3)).astype(np.float32)
        new_xyz = xyz.copy()                      # every centre IS a source point: d2 = 0 for its first neighbour
        idx, d2 = _knn(new_xyz, xyz, K)
        assert (d2[:, :, 0] == 0).all()
    else:
        N, P, ns = SHAPES[c["shape"]]
        K = min(ns, N)
        xyz = rs.standard_normal((B, N, 3)).astype(np.float32)
        new_xyz = rs.standard_normal((B, P, 3)).astype(np.float32)
        idx, d2 = _knn(new_xyz, xyz, K)
    if not flags & FP:
        d2 = None
    ldg = ru(C + ncoord(flags))
    dout = rs.standard_normal((B * P * K, ldg)).astype(np.float32)
    feat = None
    if C:
        feat = np.zeros((B * N, ru(C)), np.float32)
        feat[:, :C] = rs.standard_normal((B * N, C))
    d = dict(name=name, flags=flags, C=C, N=N, np=P, K=K, ldg=ldg, xyz=xyz, new_xyz=new_xyz, idx=idx, d2=d2, counts=counts, dout=dout,
             feat=feat)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def coord_grad(d, dout=None):
    """the coordinate-gradient columns of dout as (B, np, K, ncoord)"""
    dout = d["dout"] if dout is None else dout
    return dout.reshape(B, d["np"], d["K"], -1)[..., d["C"]:d["C"] + ncoord(d["flags"])]


# ------------------------------------------------------------------------------------------- the reference operators, float64
def oracle_rows(xyz, new_xyz, idx, flags, d2=None, counts=None, feat=None):
    """float64 torch tensors (idx int64) -> rows (B, np, K, C + ncoord) = [feat | coordinate columns], differentiable by autograd.
    feat (B, N, C) or None."""
    Bn, P, K = idx.shape
    gi = idx.reshape(Bn, P * K, 1)
    nn_abs = torch.gather(xyz, 1, gi.expand(-1, -1, 3)).reshape(Bn, P, K, 3)
    centre = new_xyz.unsqueeze(2)
    parts = []
    have = None
    if counts is not None:
        assert not flags & FP
        have = (counts > 0).to(xyz.dtype).reshape(Bn, P, 1, 1)
        nn_abs = have * nn_abs + (1 - have) * centre                        # :391-394
    if feat is not None:
        f = torch.gather(feat, 1, gi.expand(-1, -1, feat.shape[2])).reshape(Bn, P, K, -1)
        parts.append(f if have is None else have * f)                          # :412-419
    rel = nn_abs - centre                                                      # :395 / :398, :509
    rep = centre.expand(-1, -1, K, -1)
    if flags & FP:
        e = (rel * rel).sum(-1, keepdim=True)
        dist = d2.unsqueeze(3) + (e - e.detach())                              # value: the given array; gradient: |nn - x|^2
        recip = 1.0 / (dist + 1e-8)                                            # :511
        weight = recip / recip.sum(dim=2, keepdim=True)                        # :512-513
        parts += [dist, weight, nn_abs, rel, rep]                              # :520
    elif not flags & NO_XYZ:
        parts.append(rel)
        if flags & ABS:
            parts.append(nn_abs)                                               # :401
        if flags & CENTER:
            parts.append(rep)                                                  # :407-408
    return torch.cat(parts, dim=3)


def _t64(a):
    return None if a is None else torch.from_numpy(np.array(a, np.float64))


def oracle_grads(d, dout=None, xyz=None, new_xyz=None, same=False):
    """float64 (dxyz, dnew_xyz) of sum(rows * dout) by torch's autograd on the CPU; same=True: xyz and new_xyz are ONE leaf, and
    its summed gradient comes back twice"""
    x = _t64(d["xyz"] if xyz is None else xyz).requires_grad_(True)
    c = x if same else _t64(d["new_xyz"] if new_xyz is None else new_xyz).requires_grad_(True)
    rows = oracle_rows(x, c, torch.from_numpy(d["idx"].astype(np.int64)), d["flags"], _t64(d["d2"]),
                       None if d["counts"] is None else torch.from_numpy(d["counts"].astype(np.int64)))
    (rows * _t64(coord_grad(d, dout))).sum().backward()
    return x.grad.numpy(), c.grad.numpy()


# ------------------------------------------------------------------------------------------- the closed formulas, explicit loops
def closed_form(d, dout=None, dtype=np.float64, mutant=None, gmag=None):
    """slide_group_rows_coord_bwd's formulas in the kernel's order of operations, in `dtype` arithmetic -> (dxyz, dnew_xyz, Sx, Sc,
    indeg): the gradients, the float64 magnitude sums of their elements' terms and the source points' in-degrees.  mutant: one of
    MUTANTS (a wrong formula).  gmag: magnitudes to use in place of |dout| in the magnitude sums (same shape as coord_grad)."""
    f = dtype
    flags, N, P, K = d["flags"], d["N"], d["np"], d["K"]
    fp = bool(flags & FP)
    g = coord_grad(d, dout).astype(f)
    gm = np.abs(g).astype(np.float64) if gmag is None else np.asarray(gmag, np.float64)
    xyz, new = d["xyz"].astype(f), d["new_xyz"].astype(f)
    has_abs, has_ctr = fp or bool(flags & ABS), fp or bool(flags & CENTER)
    o_rel, o_abs, o_ctr = (5, 2, 8) if fp else (0, 3, 6 if flags & ABS else 3)
    dx, dc = np.zeros((B, N, 3), f), np.zeros((B, P, 3), f)
    Sx, Sc, indeg = np.zeros((B, N, 3)), np.zeros((B, P, 3)), np.zeros((B, N), np.int64)
    eps = f(np.float32(1e-8)) if f is np.float32 else f(1e-8)
    zero3 = np.zeros(3, f)
    for b in range(B):
        for p in range(P):
            c = new[b, p]
            empty = d["counts"] is not None and d["counts"][b, p] == 0 and mutant != "counts_ignored"
            if fp:
                dd = d["d2"][b, p].astype(f)
                r = [f(1) / (dd[k] + eps) for k in range(K)]
                S = f(0)
                for k in range(K):
                    S = S + r[k]
                T, Tm = f(0), 0.0
                for k in range(K):
                    T = T + g[b, p, k, 1] * (r[k] / S)
                    Tm += gm[b, p, k, 1] * float(r[k]) / float(S)
                if mutant == "no_w_coupling":
                    T = f(0)
            for k in range(K):
                nb = int(d["idx"][b, p, k])
                gk, mk = g[b, p, k], gm[b, p, k]
                g_rel, m_rel = gk[o_rel:o_rel + 3], mk[o_rel:o_rel + 3]
                g_abs, m_abs = (gk[o_abs:o_abs + 3], mk[o_abs:o_abs + 3]) if has_abs else (zero3, np.zeros(3))
                g_ctr, m_ctr = (gk[o_ctr:o_ctr + 3], mk[o_ctr:o_ctr + 3]) if has_ctr else (zero3, np.zeros(3))
                if empty:
                    dc[b, p] = dc[b, p] + (g_abs + g_ctr)
                    Sc[b, p] += m_abs + m_ctr
                    continue
                q = xyz[b, nb]
                v, vm = zero3, np.zeros(3)
                if fp:
                    gd = f(0) if mutant == "no_g_d2" else gk[0]
                    G = gd - ((r[k] * r[k]) / S) * (gk[1] - T)
                    two = f(1) if mutant == "no_factor_2" else f(2)
                    v = (two * G) * (q - c)
                    rr = float(r[k]) ** 2 / float(S)
                    vm = 2 * (mk[0] + rr * (mk[1] + Tm)) * np.abs(q.astype(np.float64) - c.astype(np.float64))
                dx[b, nb] = dx[b, nb] + ((v + g_abs) + g_rel)
                Sx[b, nb] += vm + m_abs + m_rel
                indeg[b, nb] += 1
                dc[b, p] = dc[b, p] + (((-v + g_rel) if mutant == "centre_rel_sign" else (-v - g_rel)) + g_ctr)
                Sc[b, p] += vm + m_rel + m_ctr
    return dx, dc, Sx, Sc, indeg


def applies(mutant, d):
    """whether the wrong formula differs from the right one on this case"""
    if mutant in ("no_w_coupling", "no_factor_2", "no_g_d2"):
        return bool(d["flags"] & FP)
    if mutant == "counts_ignored":
        return d["counts"] is not None
    return True


def forward_tolerance(rows64, flags, C, K):
    """bound of the forward kernel's coordinate columns against oracle_rows: rel = fl(q - c) rounds once, w carries K + 6 roundings
    (above); d2, abs and centre are copies"""
    tol = np.zeros_like(rows64)
    if flags & FP:
        m = (K + 6) * U
        tol[..., C + 1] = m / (1 - m) * np.abs(rows64[..., C + 1])
        tol[..., C + 5:C + 8] = U * np.abs(rows64[..., C + 5:C + 8])
    elif not flags & NO_XYZ:
        tol[..., C:C + 3] = U * np.abs(rows64[..., C:C + 3])
    return tol
