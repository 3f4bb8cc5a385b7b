"""DPSR backward test cases: a numpy float64 restatement of the backward of DPSR.forward on top of tests/dpsr_cases.py, the wrong
arithmetics the tests must tell from it, the upstream gradient of every case, and the bounds.

The restatement.  g = dL/dphi; phi, pre (the grid before shift and scale), off and fv0 from dpsr_cases.restate; a = |fv0|, s = pre - off.
  1. finish    scale: ds = -0.5 g / a, da = 0.5 sum(g s) / a^2, ds[0,0,0] += sign(fv0) da; else ds = g
  2. shift     dfv = -sum(ds) / n (every point's); dpre = ds + dfv W, W = rasterize(V, 1); dV_n += dfv sum_c (dw_c/dV_n) pre[idx_c]
  3. solve     dras_d = irfftn(conj(m_d) rfftn(dpre)), bin (0,0,0) zeroed, m_d = dpsr_cases.multipliers
  4. points    dN_{n,d} = sum_c w_c dras_d[idx_c];  dV_n += sum_d N_{n,d} sum_c (dw_c/dV_n) dras_d[idx_c]
  5. weights   a factor |p - x| / cs has the derivative sign(p - x) r, sign(0) = 0; floor, ceil and fmod carry none

Wrong arithmetics (WRONG): `noconj` -- m_d instead of its conjugate; `nyquist` -- the adjoint of a full c2c with fftfreq on all three
axes; `abs1` -- sign(0) = 1 on lattice planes (dV only); `noshiftV` -- the shift's dV term dropped (shift cases, dV only);
`noshiftgrid` -- the dfv W term dropped (shift cases); `nofv0` -- the cell-0 term dropped (scale cases).

Upstream gradient (upstream): the gradient of a mean-squared error of phi against 0.9 tanh(phi) + 0.05 noise,
g = 2 (phi - target) / phi.size, phi the float64 restatement, noise = RandomState(G_SEED + case index).standard_normal, as float32.

Bounds, per sample, of max |dN - dN64| and max |dV - dV64| over the sample's points.  u = 2^-24; the forward's quantities are those of
dpsr_cases (B_s: the bound of the unscaled, shifted grid s = pre - off per element, of which a = |fv0| is one cell; ETA, LAMBDA,
t = 3 log2 r, the probabilistic accumulation through a transform).  The kernels read the forward's OWN float phi and a, so the bound
charges the forward's error of what they read as well as their own roundings.  Two kinds of error are kept apart.

Scalar errors (with scale only).  The backward is linear in g, and with O the output (dV or dN) it splits into
    O = O_g + O_0,   O_0 = the response to the cell-0 term c0 = sign(fv0) da = -sign(fv0) sum(g phi) / a alone
                           (dpre = c0 (delta_0 - W / n), dfv = -c0 / n),   O_g = the response to ds = -0.5 g / a without it.
Both carry a factor 1 / a, and c0 reads sum(g phi) = -0.5 sum(g s) / a of the forward's float phi.  So the backward reads two SCALARS
of the forward, a and sum(g s), and they are charged with the forward's own model, evaluated for what they are.  The forward models the
error of pre as independent per cell, of standard deviation s_pre (dpsr_cases: the probabilistic accumulation through both transforms),
and takes LAMBDA = 7 deviations because its bound must hold for the largest of 2^21 cells.  A scalar is one deviate, not the largest
of 2^21: of the at most 8 scalar deviates of a test case (2 per sample, 2 samples, both outputs) the largest exceeds 3.9 deviations
with probability 1e-3 -- the forward's level -- and LAMBDA_1 = 4.5 keeps the forward's margin over it.  The roundings that are not
accumulated through a transform stay worst-case, with the forward's constants, on the values they act on (not on max |pre|):
    a         a = |pre_0 - off|, off = sum_c W_c pre_c / n (W = rasterize(V, 1): the gathers' weights).  The cells' errors enter as
              e_0 - sum_c (W_c / n) e_c: LAMBDA_1 s_pre sqrt(1 + (||W||_2 / n)^2); cell 0's last rounding u |pre_0|; the gathers
              15.1 u mean_n interp(|pre|, V_n) (dpsr_cases.interp_bound); the mean's rounding u |off|; the subtraction u a
              (without shift: LAMBDA_1 s_pre + u |pre_0|).  rel_a = B_a / a', a' = a - B_a: a common relative error of EVERY entry
    sum(g s)  sum_c g_c (e_c - e_off): LAMBDA_1 s_pre ||g||_2 + u sum |g pre| (the cells' last roundings) + |sum g| B_off
              + u sum |g s| (the subtractions), B_off = LAMBDA_1 s_pre ||W||_2 / n + the gathers + u |off|: e_gs
    c0        rel_0 = rel_a + ((0.5 / a') e_gs + 2 u sum |g phi|) / |sum g phi| + u: phi's division by a once more, phi's two
              roundings, c0 rounded once
A scalar error propagates exactly along the response of the term it multiplies:
    per entry   rel_a |O| + rel_0 |O_0|          (O, O_0 from the float64 restatement; the shift's dV term is charged with them)

Rounding errors, independent per element:
  finish    ds = (-0.5 g) / a: 2 u |ds|; cell 0 once more u |ds_0|
  shift     dfv rounded once from double; W: the rasterizer's bound for values 1 (dpsr_cases.rasterize_bound): e_W;
            dpre = ds + dfv W, a product and a sum: e_dpre = 2 u |ds| + u |dfv| W + |dfv| e_W + 2 u (|ds| + |dfv| W)     (per cell)
  r2c       every bin of Y carries an error of scale sigma_Y = ETA sqrt(t) ||dpre||_2 + ||e_dpre||_2
  adjoint   dRas_dk = conj(m_dk) Y_k, charged 12 roundings as the forward's solve is
  c2r       per element s_d = sigma_Y sqrt(sum_k |m_dk|^2) / N + (ETA sqrt(t) + 12 u) rms(dras_d)                     (k over the FULL spectrum)
            B_d = LAMBDA s_d + u max |dras_d|
  points    dN_d = sum_c w_c dras_d[idx_c], sum_c w_c = 1, charged as grid_interp is: B_d + 15.1 u max |dras_d|, the largest over d
            dV_e = sum_c (dw_c/dV_e) q_c, q_c = sum_d N_d dras_d[idx_c] + dfv pre[idx_c], sum_c |dw_c/dV_e| <= 2 r.  The kernel rebuilds
            pre from the forward's phi and off, (-2 a) phi + off with scale (phi + off without): within B_s + 4 u M of exact,
            M = max(max |s|, max |pre|); dfv is rounded once.  Per point
            |q| <= Q = sum_d |N_d| max |dras_d| + |dfv| M
            e_q = sum_d |N_d| B_d + |dfv| (B_s + 5 u M) + 8 u Q
            2 r (e_q + 15.1 u Q)
B_dN, B_dV = the largest sum of the two kinds over the sample's entries.
"""
import numpy as np

import dpsr_cases as C

U = C.U
G_SEED = 4100
LAMBDA_1 = 4.5  # standard deviations for ONE scalar (module docstring)
WRONG = ("noconj", "nyquist", "abs1", "noshiftV", "noshiftgrid", "nofv0")
CASES = C.CASES


def applies(wrong, what, sig, shift, scale):
    """whether condition (b) holds the wrong arithmetic to account on `what` ('dV' / 'dN') of a case"""
    if wrong in ("abs1", "noshiftV") and what != "dV":
        return False
    if wrong in ("noshiftV", "noshiftgrid") and not shift:
        return False
    if wrong == "nofv0" and not scale:
        return False
    if wrong == "nyquist" and sig >= 10:  # (the filter erases the k3 = r/2 plane, as in the forward)
        return False
    return True


def upstream(index, phi):
    """the upstream gradient of case number `index` (position in CASES) for its float64 phi (B, r, r, r) -> float32"""
    phi = np.asarray(phi, np.float64)
    noise = np.random.RandomState(G_SEED + index).standard_normal(phi.shape)
    target = 0.9 * np.tanh(phi) + 0.05 * noise
    return (2.0 * (phi - target) / phi.size).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ restatement
def corner_grads(V, r, wrong=None):
    """V (B, n, 3) -> flat indices (B, n, 8), weights (B, n, 8) and their derivatives in the point (B, n, 8, 3)"""
    V = np.asarray(V, np.float64)
    cs = 1.0 / r
    q = V / cs
    f0, c1 = np.floor(q), np.ceil(q)
    i1 = np.fmod(c1, r)
    ea, eb = V - (f0 + 1) * cs, V - f0 * cs
    wa, wb = np.abs(ea) / cs, np.abs(eb) / cs
    da, db = np.sign(ea) / cs, np.sign(eb) / cs
    if wrong == "abs1":
        db = np.where(eb == 0, 1.0 / cs, db)
    idx, w, dw = [], [], []
    for c in range(8):
        b = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        ii = [(i1 if b[d] else f0)[..., d].astype(np.int64) for d in range(3)]
        ww = [(wb if b[d] else wa)[..., d] for d in range(3)]
        dd = [(db if b[d] else da)[..., d] for d in range(3)]
        idx.append((ii[0] * r + ii[1]) * r + ii[2])
        w.append(ww[0] * ww[1] * ww[2])
        dw.append(np.stack([dd[0] * ww[1] * ww[2], ww[0] * dd[1] * ww[2], ww[0] * ww[1] * dd[2]], -1))
    return np.stack(idx, -1), np.stack(w, -1), np.stack(dw, -2)


def solve_adjoint(dpre, r, sig, wrong=None):
    """dpre (B, r, r, r) -> dras (B, 3, r, r, r)"""
    if wrong == "nyquist":
        Y = np.fft.fftn(dpre, axes=(1, 2, 3))
        m = C.multipliers(r, sig, full=True)
        Z = np.stack([np.conj(md) * Y for md in m], 1)
        Z[:, :, 0, 0, 0] = 0
        return np.fft.ifftn(Z, axes=(2, 3, 4)).real
    Y = np.fft.rfftn(dpre, axes=(1, 2, 3))
    m = C.multipliers(r, sig)
    Z = np.stack([(md if wrong == "noconj" else np.conj(md)) * Y for md in m], 1)
    Z[:, :, 0, 0, 0] = 0
    return np.fft.irfftn(Z, s=(r, r, r), axes=(2, 3, 4))


def point_grads(V, N, dras, r, extra=None, wrong=None):
    """the gather of step 4: dras (B, 3, r, r, r), extra (B, r, r, r) or None (the grid dfv s of the shift's dV term) -> dV, dN"""
    N = np.asarray(N, np.float64)
    idx, w, dw = corner_grads(V, r, wrong)
    B = len(idx)
    flat = np.asarray(dras, np.float64).reshape(B, 3, r ** 3)
    dV, dN = np.zeros(N.shape), np.zeros(N.shape)
    for b in range(B):
        gat = flat[b][:, idx[b]]                       # (3, n, 8)
        dN[b] = (gat * w[b][None]).sum(2).T
        q = (N[b].T[:, :, None] * gat).sum(0)          # (n, 8)
        if extra is not None:
            q = q + np.asarray(extra, np.float64).reshape(B, -1)[b][idx[b]]
        dV[b] = (dw[b] * q[:, :, None]).sum(1)
    return dV, dN


def backward(V, N, r, sig, shift, scale, g, wrong=None, detail=False):
    """-> dV, dN (B, n, 3) float64; with detail also a dict of the intermediates the bounds need"""
    g = np.asarray(g, np.float64)
    phi, d = C.restate(V, N, r, sig, shift, scale, detail=True)
    B, n = np.asarray(V).shape[:2]
    pre, off, fv0 = d["pre"], d["offset"], d["fv0"]
    a = np.abs(fv0)
    s = pre - off[:, None, None, None]
    da = np.zeros(B)
    if scale:
        ds = -0.5 * g / a[:, None, None, None]
        da = 0.5 * (g * s).reshape(B, -1).sum(1) / a ** 2
        if wrong != "nofv0":
            ds[:, 0, 0, 0] += np.sign(fv0) * da
    else:
        ds = g.copy()
    dfv = -ds.reshape(B, -1).sum(1) / n if shift else np.zeros(B)
    dpre = ds.copy()
    W = None
    if shift:
        W = C.rasterize(V, np.ones((B, n, 1)), r)[:, 0]
        if wrong != "noshiftgrid":
            dpre = dpre + dfv[:, None, None, None] * W
    dras = solve_adjoint(dpre, r, sig, wrong)
    extra = dfv[:, None, None, None] * pre if shift and wrong != "noshiftV" else None
    dV, dN = point_grads(V, N, dras, r, extra, wrong)
    if detail:
        d = dict(d, phi=phi, s=s, a=a, da=da, ds=ds, dfv=dfv, W=W, dpre=dpre, dras=dras, g=g)
        return dV, dN, d
    return dV, dN


# ------------------------------------------------------------------------------------------------------------ bounds
def forward_bounds(r, sig, shift, d):
    """(s_pre, B_s) per sample (B,): dpsr_cases.phi_bound's per-element error scale of the unscaled grid and its bound after the shift"""
    N, t = r ** 3, 3 * np.log2(r)
    m = C.multipliers(r, sig)
    wt = np.full(r // 2 + 1, 2.0)
    wt[0] = wt[-1] = 1.0
    m2 = [float((np.abs(md) ** 2 * wt).sum()) for md in m]
    Sp, Bs = [], []
    for b in range(len(d["pre"])):
        pre = d["pre"][b]
        sig_d = [(C.ETA * np.sqrt(t) + U) * np.linalg.norm(d["ras"][b, k]) + np.linalg.norm(d["e_ras"][b, k]) for k in range(3)]
        rms = np.linalg.norm(pre) / np.sqrt(N)
        M = float(np.abs(pre).max())
        s_pre = np.sqrt(sum(s * s * q for s, q in zip(sig_d, m2))) / N + (C.ETA * np.sqrt(t) + 12 * U) * rms
        B = C.LAMBDA * s_pre + U * M
        Sp.append(s_pre)
        Bs.append(2 * B + 19 * U * M if shift else B)
    return np.array(Sp), np.array(Bs)


def scalar_bounds(V, shift, d, s_pre):
    """(B_a, e_gs) per sample (B,): of a = |pre[0,0,0] - off| and of sum(g s), the two scalars the backward reads from the forward"""
    nb, n = np.asarray(V).shape[:2]
    g, pre, s = d["g"].reshape(nb, -1), d["pre"].reshape(nb, -1), d["s"].reshape(nb, -1)
    B_a = LAMBDA_1 * s_pre + U * np.abs(pre[:, 0])
    B_off = np.zeros(nb)
    e_gs = LAMBDA_1 * s_pre * np.linalg.norm(g, axis=1) + U * (np.abs(g) * np.abs(pre)).sum(1)
    if shift:
        W = d["W"].reshape(nb, -1)
        gather = 15.1 * U * (W * np.abs(pre)).sum(1) / n   # = 15.1 u mean_n interp(|pre|, V_n)
        B_off = LAMBDA_1 * s_pre * np.linalg.norm(W, axis=1) / n + gather + U * np.abs(d["offset"])
        B_a = LAMBDA_1 * s_pre * np.sqrt(1 + (np.linalg.norm(W, axis=1) / n) ** 2) + U * np.abs(pre[:, 0]) + gather + \
            U * np.abs(d["offset"]) + U * d["a"]
        e_gs = e_gs + np.abs(g.sum(1)) * B_off + U * (np.abs(g) * np.abs(s)).sum(1)
    return B_a, e_gs


def dras_bound(r, sig, dpre, e_dpre, dras):
    """per sample and component (B, 3), of |dras - exact| per element, for dpre (B, r, r, r) known within e_dpre per cell"""
    N, t = r ** 3, 3 * np.log2(r)
    m = C.multipliers(r, sig)
    wt = np.full(r // 2 + 1, 2.0)
    wt[0] = wt[-1] = 1.0
    m2 = [float((np.abs(md) ** 2 * wt).sum()) for md in m]
    out = np.zeros((len(dpre), 3))
    for b in range(len(dpre)):
        sigma_y = C.ETA * np.sqrt(t) * np.linalg.norm(dpre[b]) + np.linalg.norm(e_dpre[b])
        for k in range(3):
            rms = np.linalg.norm(dras[b, k]) / np.sqrt(N)
            s_d = sigma_y * np.sqrt(m2[k]) / N + (C.ETA * np.sqrt(t) + 12 * U) * rms
            out[b, k] = C.LAMBDA * s_d + U * np.abs(dras[b, k]).max()
    return out


def points_bound(r, N, dras, B_d, dfv=None, smax=None, B_s=None):
    """the rounding part of the gather on grids known within B_d (B, 3) per element: (dV (B, n), dN (B,)) per point / per sample"""
    N = np.abs(np.asarray(N, np.float64))
    nb = len(dras)
    Md = np.abs(dras).reshape(nb, 3, -1).max(2)
    e_dN = (B_d + 15.1 * U * Md).max(1)
    e_dV = np.zeros(N.shape[:2])
    for b in range(nb):
        Q = N[b] @ Md[b]
        e_q = N[b] @ B_d[b]
        if dfv is not None:
            Q = Q + abs(dfv[b]) * smax[b]
            e_q = e_q + abs(dfv[b]) * (B_s[b] + 5 * U * smax[b])
        e_dV[b] = 2 * r * (e_q + 8 * U * Q + 15.1 * U * Q)
    return e_dV, e_dN


def cell0_response(V, N, r, sig, shift, d):
    """O_0 of the module docstring: (dV, dN) of the cell-0 term c0 alone"""
    nb, n = np.asarray(V).shape[:2]
    c0 = (np.sign(d["fv0"]) * d["da"])[:, None, None, None]
    dpre = np.zeros(d["dpre"].shape)
    dpre[:, 0, 0, 0] = 1.0
    extra = None
    if shift:
        dpre = dpre - d["W"] / n
        extra = (-c0 / n) * d["pre"]
    return point_grads(V, N, solve_adjoint(c0 * dpre, r, sig), r, extra)


def grad_bounds(V, N, r, sig, shift, scale, d, dV, dN):
    """(B_dV, B_dN) per sample (B,); dV, dN, d = backward(..., detail=True)"""
    nb, n = np.asarray(V).shape[:2]
    g = d["g"]
    s_pre, B_s = forward_bounds(r, sig, shift, d)
    a = d["a"]
    ds = d["ds"]
    co_V, co_N = np.zeros(dV.shape), np.zeros(dN.shape)
    if scale:
        B_a, e_gs = scalar_bounds(V, shift, d, s_pre)
        ap = a - B_a
        if (ap <= 0).any():
            return np.full(nb, np.inf), np.full(nb, np.inf)
        rel_a = B_a / ap
        gp = (g * d["phi"]).reshape(nb, -1)
        rel_0 = rel_a + ((0.5 / ap) * e_gs + 2 * U * np.abs(gp).sum(1)) / np.abs(gp.sum(1)) + U
        V0, N0 = cell0_response(V, N, r, sig, shift, d)
        co_V = rel_a[:, None, None] * np.abs(dV) + rel_0[:, None, None] * np.abs(V0)
        co_N = rel_a[:, None, None] * np.abs(dN) + rel_0[:, None, None] * np.abs(N0)
    e_dpre = (2 * U * np.abs(ds)) if scale else np.zeros(ds.shape)
    e_dpre[:, 0, 0, 0] += U * np.abs(ds[:, 0, 0, 0]) if scale else 0.0
    if shift:
        W, e_ras = C.rasterize(V, np.ones((nb, n, 1)), r, with_bound=True)
        W, e_W = W[:, 0], C.rasterize_bound(W, e_ras)[:, 0]
        dfv = np.abs(d["dfv"])[:, None, None, None]
        e_dpre = e_dpre + U * dfv * W + dfv * e_W + 2 * U * (np.abs(ds) + dfv * W)
    B_d = dras_bound(r, sig, d["dpre"], e_dpre, d["dras"])
    if shift:
        M = np.maximum(np.abs(d["s"]).reshape(nb, -1).max(1), np.abs(d["pre"]).reshape(nb, -1).max(1))
        e_dV, e_dN = points_bound(r, N, d["dras"], B_d, d["dfv"], M, B_s)
    else:
        e_dV, e_dN = points_bound(r, N, d["dras"], B_d)
    return (co_V + e_dV[:, :, None]).reshape(nb, -1).max(1), (co_N + e_dN[:, None, None]).reshape(nb, -1).max(1)
