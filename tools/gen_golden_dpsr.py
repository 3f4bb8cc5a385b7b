"""tools/gen_golden_dpsr.py -- AUTHORING ONLY, CPU (never imported by tests, bench or smoke): records tests/golden/golden_dpsr.npz
from the reference's pointnet2/dpsr_utils/dpsr.py (DPSR) and utils.py (point_rasterize, grid_interp, fftfreqs,
spec_gaussian_filter).  The reference modules are imported where they lie; the packages their file imports and DPSR never touches
(trimesh, plyfile, skimage, pytorch3d.structures / renderer, igl) are empty stub modules.  Nothing of the reference is copied.

Inputs: per sample a sphere of random centre and radius inside the unit cube, outward normals with magnitudes in [0.5, 2], and
appended by hand: a point at 0, points on lattice planes (one, two and three coordinates on k / r), points in the last cell of each
axis (p > (r - 1) / r: the periodic wrap) and 40 copies of one point.

Cases: r 16 (B 2, n 257, sig 2) with all four shift / scale combinations; r 32 (B 1, n 1000) with sig 2 and sig 10.
Recorded (arrays only):
  V_r<r>, N_r<r>                 the inputs, f32 (the cases of one r share them)
  phi32_<case>, phi64_<case>     the reference's float32 phi and its float64 evaluation (inputs cast to double, G, omega and the
                                 rasteriser in double), f32 / f64
  eref_<case>                    max |phi32 - phi64| over the WHOLE grid
  fv0_ratio_<case>               |phi[0,0,0] - offset| / max |phi| before the scaling, float64 evaluation
  ras64_r16_idx, ras64_r16_val   point_rasterize(V, N) in float64, r 16: flat indices into (B, 3, r, r, r) and values of its non-zero cells
  interp_seed, interp64_r<r>     grid_interp of the grid RandomState(interp_seed + r).standard_normal((B, r, r, r, 4)) (as f32) in float64
  G_r<r>_s<sig>, freqs_r<r>      the module's buffer G (r, r, r/2 + 1) f32 and fftfreqs((r, r, r)) f32
  cells_r32                      see below
The r 16 grids are recorded whole.  Six dense float64 grids alone (786 KB) exceed the fixture cap, so the r 32 cases record phi32 /
phi64 at the 8192 cells `cells_r32` (flat indices: cell 0 and a seeded random draw, sorted); eref is still taken over all cells.
tests/test_dpsr_host.py pins the numpy restatement to these values within 1e-12, and the GPU tests compare the r 32 grids with the
recorded cells AND with that restatement on every cell.

A seed where |fv0| falls below 0.05 max |phi| before the scaling in any case is rejected (the division must not amplify): the next
seed is tried.  The file must stay within SIZE_CAP, the largest fixture before it.

usage:  python tools/gen_golden_dpsr.py [--reference DIR] [--seed 0] [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_CAP = 781323
N_CELLS_R32 = 8192
FV0_MIN = 0.05
CASES = [("r16_s2_sh%d_sc%d" % (sh, sc), 16, 2, bool(sh), bool(sc)) for sh in (0, 1) for sc in (0, 1)] + \
        [("r32_s2", 32, 2, True, True), ("r32_s10", 32, 10, True, True)]
SHAPES = {16: (2, 257), 32: (1, 1000)}


def load_reference(ref_root):
    """the reference's dpsr_utils.dpsr / dpsr_utils.utils modules, with stub modules for what their imports name and DPSR never uses"""
    sys.dont_write_bytecode = True
    for name in ("trimesh", "plyfile", "skimage", "skimage.measure", "pytorch3d", "pytorch3d.structures", "pytorch3d.renderer", "igl"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = None
    sys.modules["skimage"].measure = sys.modules["skimage.measure"]
    sys.modules["pytorch3d.structures"].Meshes = None
    sys.modules["pytorch3d.renderer"].PerspectiveCameras = None
    sys.modules["pytorch3d.renderer"].rasterize_meshes = None
    sys.modules["igl"].adjacency_matrix = None
    sys.modules["igl"].connected_components = None
    sys.path.insert(0, os.path.join(ref_root, "pointnet2"))
    for k in [k for k in sys.modules if k == "dpsr_utils" or k.startswith("dpsr_utils.")]:
        del sys.modules[k]
    import dpsr_utils.dpsr as D
    import dpsr_utils.utils as U
    assert os.path.abspath(D.__file__).startswith(os.path.abspath(ref_root))
    return D, U


def make_inputs(rs, r, B, n):
    hand = []
    k = [3, r // 2, r - 2]
    hand.append([0.0, 0.0, 0.0])                                                # the point at 0
    hand += [[k[0] / r, 0.41, 0.52], [0.37, k[1] / r, 0.61], [0.45, 0.58, k[2] / r]]  # one coordinate on a lattice plane
    hand += [[k[0] / r, k[1] / r, 0.33], [k[1] / r, k[2] / r, k[0] / r]]        # two and three
    hand += [[(r - 0.5) / r, 0.4, 0.6], [0.55, (r - 0.25) / r, 0.45], [0.5, 0.35, (r - 0.75) / r]]  # the last cell of each axis
    hand += [[(r - 0.3) / r, (r - 0.6) / r, (r - 0.1) / r], [0.99, 0.99, 0.3]]  # ... of several at once
    hand = np.array(hand, np.float64)
    n_copy = 40
    n_sphere = n - len(hand) - n_copy
    V = np.zeros((B, n, 3), np.float32)
    N = np.zeros((B, n, 3), np.float32)
    for b in range(B):
        centre = rs.uniform(0.4, 0.6, 3)
        radius = rs.uniform(0.18, 0.3)
        u = rs.standard_normal((n_sphere, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        V[b, :n_sphere] = centre + radius * u
        N[b, :n_sphere] = u * rs.uniform(0.5, 2.0, (n_sphere, 1))
        V[b, n_sphere:n_sphere + len(hand)] = hand
        d = rs.standard_normal((len(hand), 3))
        N[b, n_sphere:n_sphere + len(hand)] = d / np.linalg.norm(d, axis=1, keepdims=True) * rs.uniform(0.5, 2.0, (len(hand), 1))
        V[b, n - n_copy:] = V[b, 7]
        N[b, n - n_copy:] = N[b, 7]
    assert V.min() >= 0.0 and V.max() < 1.0
    assert (V[:, :, 0] > (r - 1) / r).any() and (V[:, :, 1] > (r - 1) / r).any() and (V[:, :, 2] > (r - 1) / r).any()
    return V, N


def run_case(D, U, torch, V, N, r, sig, shift, scale):
    res = (r, r, r)
    m32 = D.DPSR(res, sig=sig, scale=scale, shift=shift)
    phi32 = m32(torch.from_numpy(V), torch.from_numpy(N)).numpy()
    assert phi32.dtype == np.float32
    m64 = D.DPSR(res, sig=sig, scale=scale, shift=shift)
    m64.G = U.spec_gaussian_filter(res=res, sig=sig)
    m64.omega = U.fftfreqs(res, dtype=torch.float64).unsqueeze(-1) * (2 * np.pi)
    Vd, Nd = torch.from_numpy(V).double(), torch.from_numpy(N).double()
    phi64 = m64(Vd, Nd).numpy()
    assert phi64.dtype == np.float64 and m64.G.dtype == torch.float64
    # the ratio the division sees, from an unscaled float64 run
    mu = D.DPSR(res, sig=sig, scale=False, shift=shift)
    mu.G, mu.omega = m64.G, m64.omega
    pre = mu(Vd, Nd).numpy()
    ratio = float((np.abs(pre[:, 0, 0, 0]) / np.abs(pre).reshape(len(pre), -1).max(1)).min())
    return phi32, phi64, ratio, m32.G.numpy().reshape(r, r, r // 2 + 1)


def build(D, U, seed):
    import torch
    rs = np.random.RandomState(seed)
    out = {"seed": np.int64(seed), "interp_seed": np.int64(seed + 1000)}
    inputs = {}
    for r, (B, n) in SHAPES.items():
        V, N = make_inputs(rs, r, B, n)
        inputs[r] = (V, N)
        out["V_r%d" % r], out["N_r%d" % r] = V, N
        out["freqs_r%d" % r] = U.fftfreqs((r, r, r), dtype=torch.float32).numpy()
        grid = np.random.RandomState(seed + 1000 + r).standard_normal((B, r, r, r, 4)).astype(np.float32)
        out["interp64_r%d" % r] = U.grid_interp(torch.from_numpy(grid).double(), torch.from_numpy(V).double(), batched=True).numpy()
    cells = np.unique(np.concatenate([[0], rs.choice(32 ** 3, N_CELLS_R32 - 1, replace=False)])).astype(np.int32)
    while len(cells) < N_CELLS_R32:  # (the draw held cell 0)
        cells = np.unique(np.concatenate([cells, rs.choice(32 ** 3, N_CELLS_R32 - len(cells))])).astype(np.int32)
    out["cells_r32"] = cells
    for name, r, sig, shift, scale in CASES:
        V, N = inputs[r]
        phi32, phi64, ratio, G = run_case(D, U, torch, V, N, r, sig, shift, scale)
        if ratio < FV0_MIN:
            return None, "%s: |fv0| / max |phi| = %.3f" % (name, ratio)
        out["eref_" + name] = np.float64(np.abs(phi32.astype(np.float64) - phi64).max())
        out["fv0_ratio_" + name] = np.float64(ratio)
        out["G_r%d_s%d" % (r, sig)] = G
        if r == 32:
            phi32, phi64 = phi32.reshape(len(phi32), -1)[:, cells], phi64.reshape(len(phi64), -1)[:, cells]
        out["phi32_" + name], out["phi64_" + name] = phi32, phi64
    V, N = inputs[16]
    ras = U.point_rasterize(torch.from_numpy(V).double(), torch.from_numpy(N).double(), (16, 16, 16)).numpy().reshape(-1)
    assert ras.dtype == np.float64
    nz = np.flatnonzero(ras)
    out["ras64_r16_idx"], out["ras64_r16_val"] = nz.astype(np.int32), ras[nz]
    return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference tree (default: tools/ref_shims.REF)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    if a.reference is None:
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import ref_shims
        a.reference = ref_shims.REF
    D, U = load_reference(a.reference)
    seed = a.seed
    while True:
        out, why = build(D, U, seed)
        if out is not None:
            break
        print("seed %d rejected: %s" % (seed, why))
        seed += 1
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "golden_dpsr.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes, cap %d), seed %d" % (path, size, SIZE_CAP, seed))
    for name, *_ in CASES:
        print("  %-18s e_ref %.3e  max |phi64| %.3f  |fv0| / max |phi| %.3f" % (name, float(out["eref_" + name]),
                                                                               float(np.abs(out["phi64_" + name]).max()), float(out["fv0_ratio_" + name])))
    assert size <= SIZE_CAP, "the fixture exceeds the cap"


if __name__ == "__main__":
    main()
