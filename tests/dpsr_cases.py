"""DPSR test cases: a numpy float64 restatement of DPSR.forward, the wrong arithmetics the tests must tell from it, and the bounds.

The restatement (steps of pointnet2/dpsr_utils/dpsr.py; inputs are float32 values evaluated in double, as the fixture's phi64 is):
  1. ras = rasterize(V, N): every point adds w_c N to the 8 corners of its cell.  cs = 1 / r, ind0 = floor(p / cs),
     ind1 = fmod(ceil(p / cs), r), corner positions ind0 cs and (ind0 + 1) cs, weight = prod_axes |p - opposite corner| / cs
  2. S = rfftn(ras) over the grid axes
  3. Phi = sum_d(-i omega_d G S_d) / (-|omega|^2 + 1e-6), omega = 2 pi (fftfreq, fftfreq, rfftfreq), Phi[0,0,0] = 0
  4. phi = irfftn(Phi, s = (r, r, r))
  5. fv = interp(phi, V); shift: phi -= mean_n fv
  6. fv0 = phi[0,0,0] after the shift; scale: phi = -phi / |fv0| * 0.5

Wrong arithmetics (WRONG): `nyquist` -- a full c2c with fftfreq on all three axes, real part taken (differs on the k3 = r/2
plane); `nowrap` -- ind1 clamped to r - 1 instead of wrapped to 0; `corner` -- ind1 * cs as the upper corner position.

Bounds.  u = 2^-24 (float unit roundoff).

Rasterize, per cell.  A contribution is fl(w v) with w the product of three per-axis weights |p - x| / cs.  The division by cs = 2^-k
is exact; the subtraction is exact unless the cell index is 0 (Sterbenz), where it rounds once.  So at most 3 (subtractions) + 2
(products) + 1 (times v) roundings: |fl(w v) - w v| <= 6.01 u |w v|.  The conversion to fixed point adds at most half a quantum,
2^-33.  With A = sum of |w v| over a cell's contributions and c their number: |cell - exact| <= 6.01 u A + c 2^-33 =: e_ras; as a
float, once more u (|cell| + e_ras).  grid_interp: the same weights, one product and at most 8 sums per corner: 15.1 u sum_c |grid_c| w_c.

FFT (tests of fft3_r2c / fft3_c2r alone).  Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: a radix-2 FFT of t
stages with twiddles of absolute error mu has ||y^ - y||_2 <= t eta / (1 - t eta) ||y||_2, eta = mu + gamma_4 (sqrt 2 + mu).  Here
mu <= u (twiddles rounded once from double), gamma_4 = 4 u / (1 - 4 u): eta = (1 + 4 sqrt 2) u (1 + small) =: ETA = 6.66 u.  The
three axes apply 3 log2 r stages, so with eps = 2 u the relative L2 error is at most c eps log2 r, c = 3 * 6.66 / 2 = 10 (FFT_C;
the c2r's input extension and final scaling by a power of two are exact).  The tests assert the L2 norm of the error against
FFT_C eps log2(r) ||exact||_2 -- which also bounds every single element's error.

phi.  The worst-case chain (t eta ||.||_1 per element) exceeds a tenth of the distance to the wrong arithmetics at r 32, so the
phi bound uses the probabilistic model of rounding (Higham & Mary 2019: independent zero-mean errors accumulate as the square
root of their number) with worst-case constants per operation and LAMBDA = 7 standard deviations (the maximum of 2^21 normal
deviates exceeds 6.6 sigma with probability 1e-3):
  forward    every bin of S_d carries an error of scale sigma_d = (ETA sqrt(t) + u) ||ras_d||_2 + ||e_ras,d||_2, t = 3 log2 r
             (the + u: the fixed-point grid is rounded to float on load)
  solve      Phi_k = sum_d m_dk S_dk, |m_dk| = |omega_d| G / |den|, 12 roundings: relative error 12 u on top of the forward's
  inverse    ||dphi||_2 = ||dPhi||_2 / sqrt(N) (Parseval, N = r^3): per element
             s_pre = sqrt(sum_d sigma_d^2 sum_k m_dk^2) / N + (ETA sqrt(t) + 12 u) rms(phi)        (k over the FULL spectrum)
             B_pre = LAMBDA s_pre + u max |phi|
  interp     8 corners, 6 roundings per weight, 8 products and sums: fv within B_pre + 14 u M of exact, M = max |phi|; its mean
             is taken in double and rounded once: offset within B_pre + 15 u M
  shift      B_s = 2 B_pre + 19 u M (with shift; B_pre without)
  scale      a = |fv0| is itself within B_s: |d(phi / a)| <= B_s / a' + M_s B_s / (a a'), a' = a - B_s, M_s = max |phi - offset|;
             B = 0.5 (that) + 2 u max |result|
"""
import numpy as np

U = 2.0 ** -24
EPS = 2.0 ** -23
ETA = (1 + 4 * np.sqrt(2)) * U * 1.001
FFT_C = 10.0
LAMBDA = 7.0
FFT_SIZES = (16, 32, 64, 128, 256)
WRONG = ("nyquist", "nowrap", "corner")


# ------------------------------------------------------------------------------------------------------------ restatement
def corners(V, r, wrong=None):
    """V (B, n, 3) -> flat cell indices (B, n, 8) and weights (B, n, 8) of every point's corners, corner c = 4 b0 + 2 b1 + b2"""
    V = np.asarray(V, np.float64)
    cs = 1.0 / r
    q = V / cs
    f0, c1 = np.floor(q), np.ceil(q)
    i1 = np.minimum(c1, r - 1) if wrong == "nowrap" else np.fmod(c1, r)
    x0 = f0 * cs
    x1 = (i1 if wrong == "corner" else f0 + 1) * cs
    wa, wb = np.abs(V - x1) / cs, np.abs(V - x0) / cs
    idx, w = [], []
    for c in range(8):
        b = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        ii = [(i1 if b[d] else f0)[..., d].astype(np.int64) for d in range(3)]
        ww = [(wb if b[d] else wa)[..., d] for d in range(3)]
        idx.append((ii[0] * r + ii[1]) * r + ii[2])
        w.append(ww[0] * ww[1] * ww[2])
    return np.stack(idx, -1), np.stack(w, -1)


def rasterize(V, vals, r, wrong=None, with_bound=False):
    """-> (B, nf, r, r, r) float64; with_bound also e_ras of the module docstring, same shape"""
    vals = np.asarray(vals, np.float64)
    B, n, nf = vals.shape
    idx, w = corners(V, r, wrong)
    out = np.zeros((B, nf, r ** 3))
    A = np.zeros((B, nf, r ** 3))
    cnt = np.zeros((B, nf, r ** 3))
    for b in range(B):
        for f in range(nf):
            c = (w[b] * vals[b, :, f, None]).reshape(-1)
            np.add.at(out[b, f], idx[b].reshape(-1), c)
            if with_bound:
                np.add.at(A[b, f], idx[b].reshape(-1), np.abs(c))
                np.add.at(cnt[b, f], idx[b].reshape(-1), (c != 0).astype(np.float64))
    out = out.reshape(B, nf, r, r, r)
    if with_bound:
        return out, (6.01 * U * A + cnt * 2.0 ** -33).reshape(out.shape)
    return out


def interp(grid, V, wrong=None):
    """grid (B, r, r, r, C), V (B, n, 3) -> (B, n, C) float64"""
    grid = np.asarray(grid, np.float64)
    B, r, C = grid.shape[0], grid.shape[1], grid.shape[4]
    idx, w = corners(V, r, wrong)
    flat = grid.reshape(B, r ** 3, C)
    return np.stack([(flat[b][idx[b]] * w[b][..., None]).sum(1) for b in range(B)])


def frequencies(r, full=False):
    """(k1, k2, k3) integer-valued float64 frequency arrays, broadcastable over (r, r, h) (h = r with `full`)"""
    k = np.fft.fftfreq(r, d=1 / r)
    k3 = k if full else np.fft.rfftfreq(r, d=1 / r)
    return k[:, None, None], k[None, :, None], k3[None, None, :]


def gaussian(r, sig, full=False):
    k1, k2, k3 = frequencies(r, full)
    dis = np.sqrt(k1 ** 2 + k2 ** 2 + k3 ** 2)
    return np.exp(-0.5 * ((sig * 2 * dis / r) ** 2))


def multipliers(r, sig, full=False):
    """m_d = -i omega_d G / (-|omega|^2 + 1e-6), d = 0, 1, 2, each (r, r, h)"""
    om = [2 * np.pi * k for k in frequencies(r, full)]
    den = -(om[0] ** 2 + om[1] ** 2 + om[2] ** 2) + 1e-6
    G = gaussian(r, sig, full)
    return [(-1j) * (o * G) / den for o in om]


def restate(V, N, r, sig, shift=True, scale=True, wrong=None, detail=False):
    """phi (B, r, r, r) float64; with detail a dict of the intermediates the bound needs"""
    cell_wrong = wrong if wrong in ("nowrap", "corner") else None
    ras, e_ras = rasterize(V, N, r, cell_wrong, with_bound=True)
    if wrong == "nyquist":
        S = np.fft.fftn(ras, axes=(2, 3, 4))
        m = multipliers(r, sig, full=True)
        Phi = m[0] * S[:, 0] + m[1] * S[:, 1] + m[2] * S[:, 2]
        Phi[:, 0, 0, 0] = 0
        pre = np.fft.ifftn(Phi, axes=(1, 2, 3)).real
    else:
        S = np.fft.rfftn(ras, axes=(2, 3, 4))
        m = multipliers(r, sig)
        Phi = m[0] * S[:, 0] + m[1] * S[:, 1] + m[2] * S[:, 2]
        Phi[:, 0, 0, 0] = 0
        pre = np.fft.irfftn(Phi, s=(r, r, r), axes=(1, 2, 3))
    phi = pre.copy()
    offset = np.zeros(len(phi))
    if shift:
        offset = interp(phi[..., None], V, cell_wrong)[..., 0].mean(1)
        phi = phi - offset[:, None, None, None]
    fv0 = phi[:, 0, 0, 0].copy()
    if scale:
        phi = -phi / np.abs(fv0)[:, None, None, None] * 0.5
    if detail:
        return phi, {"ras": ras, "e_ras": e_ras, "pre": pre, "offset": offset, "fv0": fv0}
    return phi


# ------------------------------------------------------------------------------------------------------------ bounds
def rasterize_bound(ras, e_ras):
    """per cell, of point_rasterize's float output against the float64 rasterizer"""
    return e_ras + U * (np.abs(ras) + e_ras)


def interp_bound(grid, V):
    """per element, of grid_interp against the float64 gather: 6 roundings per weight, 1 product, 8 sums over sum_c |grid_c| w_c"""
    return 15.1 * U * interp(np.abs(np.asarray(grid, np.float64)), V)


def fft_bound(exact, r):
    """of the L2 norm of the error of fft3_r2c / fft3_c2r against the float64 transform `exact`"""
    return FFT_C * EPS * np.log2(r) * float(np.linalg.norm(np.asarray(exact).ravel()))


def phi_bound(r, sig, shift, scale, d):
    """per sample (B,), of |phi - phi64| per element; d = restate(..., detail=True)[1]"""
    N, t = r ** 3, 3 * np.log2(r)
    m = multipliers(r, sig)
    wt = np.full(r // 2 + 1, 2.0)
    wt[0] = wt[-1] = 1.0
    m2 = [float((np.abs(md) ** 2 * wt).sum()) for md in m]
    out = []
    for b in range(len(d["pre"])):
        pre = d["pre"][b]
        sig_d = [(ETA * np.sqrt(t) + U) * np.linalg.norm(d["ras"][b, k]) + np.linalg.norm(d["e_ras"][b, k]) for k in range(3)]
        rms = np.linalg.norm(pre) / np.sqrt(N)
        M = float(np.abs(pre).max())
        s_pre = np.sqrt(sum(s * s * q for s, q in zip(sig_d, m2))) / N + (ETA * np.sqrt(t) + 12 * U) * rms
        B = LAMBDA * s_pre + U * M
        if shift:
            B = 2 * B + 19 * U * M
        if scale:
            a = abs(d["fv0"][b])
            Ms = float(np.abs(pre - d["offset"][b]).max())
            if a <= B:
                out.append(np.inf)
                continue
            B = 0.5 * (B / (a - B) + Ms * B / (a * (a - B))) + 2 * U * 0.5 * Ms / a
        out.append(B)
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------ fixture
CASES = [("r16_s2_sh%d_sc%d" % (sh, sc), 16, 2, bool(sh), bool(sc)) for sh in (0, 1) for sc in (0, 1)] + \
        [("r32_s2", 32, 2, True, True), ("r32_s10", 32, 10, True, True)]
SIZE_CAP = 781323


def golden_cells(g, name, r, phi):
    """the cells of a (B, r, r, r) grid the fixture records for the case: all of them at r 16, g['cells_r32'] at r 32 -- shaped
    like g['phi64_' + name]"""
    return phi if r == 16 else phi.reshape(len(phi), -1)[:, g["cells_r32"]]


def sphere_cloud(seed, B, n):
    """the inputs of the cases beyond the fixture: spheres with outward normals of magnitude in [0.5, 2], plus the point at 0, a
    lattice-plane point and a last-cell point per sample"""
    rs = np.random.RandomState(seed)
    V = np.zeros((B, n, 3), np.float32)
    Nn = np.zeros((B, n, 3), np.float32)
    for b in range(B):
        u = rs.standard_normal((n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        V[b] = rs.uniform(0.4, 0.6, 3) + rs.uniform(0.18, 0.3) * u
        Nn[b] = u * rs.uniform(0.5, 2.0, (n, 1))
        V[b, 0] = (0.0, 0.0, 0.0)
        V[b, 1] = (0.25, 0.41, 0.5)
        V[b, 2] = (0.9995, 0.3, 0.9999)
    return V, Nn
