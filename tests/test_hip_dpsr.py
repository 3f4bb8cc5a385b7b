"""GPU: the DPSR kernels of slide_amd/csrc/dpsr.hip, one launch group at a time and composed, against float64 -- the reference's own
float64 evaluation recorded in tests/golden/golden_dpsr.npz and the numpy restatement of tests/dpsr_cases.py (pinned to that
fixture within 1e-12 by tests/test_dpsr_host.py).  Every bound is derived in tests/dpsr_cases.py; every figure is printed before
it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import dpsr_cases as C

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_dpsr.npz")


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _dpsr(r, sig, shift, scale, dev):
    from dpsr_utils.dpsr import DPSR
    return DPSR((r, r, r), sig=sig, shift=shift, scale=scale).to(dev)


# ------------------------------------------------------------------------------------------------------------ rasterize
def test_rasterize_against_float64(golden, gpu_device):
    from dpsr_utils.utils import point_rasterize
    V, N, r = golden["V_r16"], golden["N_r16"], 16
    got = point_rasterize(_dev(V, gpu_device), _dev(N, gpu_device), (r, r, r))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, r, r, r)
    want64 = np.zeros(2 * 3 * r ** 3)
    want64[golden["ras64_r16_idx"]] = golden["ras64_r16_val"]
    ras, e_ras = C.rasterize(V, N, r, with_bound=True)
    assert np.abs(ras.reshape(-1) - want64).max() <= 1e-14
    err = np.abs(got.cpu().numpy().astype(np.float64) - ras)
    bound = C.rasterize_bound(ras, e_ras)
    print("rasterize r16: max err %.3e, max err / bound %.3f" % (err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    # one value column
    got1 = point_rasterize(_dev(V, gpu_device), _dev(N[:, :, 1:2], gpu_device), (r, r, r))
    assert torch.equal(got1[:, 0], got[:, 1])


def test_rasterize_is_reproducible_and_independent_of_the_batch(golden, gpu_device):
    from slide_amd import _ext
    V, N = _dev(golden["V_r16"], gpu_device), _dev(golden["N_r16"], gpu_device)
    a = _ext.point_rasterize_fixed(V, N, 16)
    b = _ext.point_rasterize_fixed(V, N, 16)
    assert a.dtype == torch.int64 and torch.equal(a, b)
    pick = torch.tensor([1, 0, 1], device=gpu_device)
    three = _ext.point_rasterize_fixed(V[pick].contiguous(), N[pick].contiguous(), 16)
    alone = _ext.point_rasterize_fixed(V[:1].contiguous(), N[:1].contiguous(), 16)
    assert torch.equal(alone[0], three[1]) and torch.equal(three[0], three[2]) and torch.equal(three[0], a[1])
    # a permutation of the points: integer sums do not depend on the order
    perm = torch.randperm(V.size(1), device=gpu_device)
    assert torch.equal(_ext.point_rasterize_fixed(V[:, perm].contiguous(), N[:, perm].contiguous(), 16), a)


# ------------------------------------------------------------------------------------------------------------ FFT
@pytest.mark.parametrize("r", C.FFT_SIZES)
def test_fft3_against_numpy(r, gpu_device):
    from slide_amd import _ext
    rs = np.random.RandomState(r)
    nb = 2 if r <= 64 else 1
    x = rs.standard_normal((nb, r, r, r)).astype(np.float32)
    S = np.fft.rfftn(x.astype(np.float64), axes=(1, 2, 3))
    xd = _dev(x, gpu_device)
    got = _ext.fft3_r2c(xd)
    assert got.dtype == torch.complex64 and tuple(got.shape) == (nb, r, r, r // 2 + 1)
    err = float(np.linalg.norm((got.cpu().numpy().astype(np.complex128) - S).ravel()))
    bound = C.fft_bound(S, r)
    print("fft3_r2c r%d: L2 err %.3e, bound %.3e (%.3f), max element err %.3e" % (
        r, err, bound, err / bound, np.abs(got.cpu().numpy() - S).max()))
    assert err <= bound
    # round trip: the forward's error carried through the inverse, plus the inverse's own
    back = _ext.fft3_c2r(got)
    assert back.dtype == torch.float32 and tuple(back.shape) == (nb, r, r, r)
    err = float(np.linalg.norm((back.cpu().numpy().astype(np.float64) - x).ravel()))
    bound = 2.001 * C.fft_bound(x, r)
    print("round trip r%d: L2 err %.3e, bound %.3e (%.3f)" % (r, err, bound, err / bound))
    assert err <= bound
    assert torch.equal(_ext.fft3_c2r(got), back) and torch.equal(_ext.fft3_r2c(xd), got)
    del S, back
    # c2r of a half spectrum that is NOT the transform of a real grid: the imaginary parts of the self-conjugate bins are dropped
    Z = (rs.standard_normal((1, r, r, r // 2 + 1)) + 1j * rs.standard_normal((1, r, r, r // 2 + 1))).astype(np.complex64)
    want = np.fft.irfftn(Z.astype(np.complex128), s=(r, r, r), axes=(1, 2, 3))
    out = _ext.fft3_c2r(_dev(Z, gpu_device), overwrite=True).cpu().numpy().astype(np.float64)
    err = float(np.linalg.norm((out - want).ravel()))
    bound = C.fft_bound(want, r)
    print("fft3_c2r r%d: L2 err %.3e, bound %.3e (%.3f), max element err %.3e" % (r, err, bound, err / bound, np.abs(out - want).max()))
    assert err <= bound


def test_fft3_reads_the_fixed_point_grid(golden, gpu_device):
    from slide_amd import _ext
    V, N = _dev(golden["V_r16"], gpu_device), _dev(golden["N_r16"], gpu_device)
    fixed = _ext.point_rasterize_fixed(V, N, 16)
    assert torch.equal(_ext.fft3_r2c(fixed), _ext.fft3_r2c(_ext.grid_fixed_to_float(fixed)))


def test_unsupported_fft_size_raises(gpu_device):
    from slide_amd import _ext
    with pytest.raises(ValueError):
        _ext.fft3_r2c(torch.zeros(1, 24, 24, 24, device=gpu_device))
    with pytest.raises(ValueError):
        _ext.fft3_c2r(torch.zeros(1, 8, 8, 5, device=gpu_device, dtype=torch.complex64))


# ------------------------------------------------------------------------------------------------------------ interp
@pytest.mark.parametrize("r", (16, 32))
def test_grid_interp_against_the_fixture(r, golden, gpu_device):
    from dpsr_utils.utils import grid_interp
    V = golden["V_r%d" % r]
    grid = np.random.RandomState(int(golden["interp_seed"]) + r).standard_normal((len(V), r, r, r, 4)).astype(np.float32)
    got = grid_interp(_dev(grid, gpu_device), _dev(V, gpu_device))
    assert tuple(got.shape) == (len(V), V.shape[1], 4)
    err = np.abs(got.cpu().numpy().astype(np.float64) - golden["interp64_r%d" % r])
    bound = C.interp_bound(grid, V)
    print("grid_interp r%d: max err %.3e, max err / bound %.3f" % (r, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    one = grid_interp(_dev(grid[0], gpu_device), _dev(V[0], gpu_device), batched=False)
    assert torch.equal(one, got[0])


# ------------------------------------------------------------------------------------------------------------ DPSR.forward
def _check_phi(name, got, want_full, bound, golden=None, r=None, eref=None):
    err = np.abs(got.astype(np.float64) - want_full).reshape(len(bound), -1).max(1)
    msg = "%s: err %s, bound %s, err / bound %.3f" % (name, err, bound, (err / bound).max())
    if eref is not None:
        msg += ", err / e_ref %.2f" % (err.max() / eref)
    print(msg)
    assert np.isfinite(got).all() and (err <= bound).all(), name
    if golden is not None:
        e2 = np.abs(C.golden_cells(golden, name, r, got).astype(np.float64) - golden["phi64_" + name]).reshape(len(bound), -1).max(1)
        print("%s: against the recorded phi64 %s" % (name, e2))
        assert (e2 <= bound).all(), name


@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_forward_against_the_fixture(case, golden, gpu_device):
    name, r, sig, shift, scale = case
    V, N = golden["V_r%d" % r], golden["N_r%d" % r]
    want, d = C.restate(V, N, r, sig, shift, scale, detail=True)
    bound = C.phi_bound(r, sig, shift, scale, d)
    m = _dpsr(r, sig, shift, scale, gpu_device)
    got = m(_dev(V, gpu_device), _dev(N, gpu_device))
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(V), r, r, r)
    _check_phi(name, got.cpu().numpy(), want, bound, golden, r, float(golden["eref_" + name]))
    assert torch.equal(m(_dev(V, gpu_device), _dev(N, gpu_device)), got)


@pytest.mark.parametrize("r,B,n", [(64, 2, 4000), (128, 1, 20480)])
def test_forward_against_the_restatement(r, B, n, gpu_device):
    V, N = C.sphere_cloud(r, B, n)
    want, d = C.restate(V, N, r, 2, True, True, detail=True)
    bound = C.phi_bound(r, 2, True, True, d)
    m = _dpsr(r, 2, True, True, gpu_device)
    got = m(_dev(V, gpu_device), _dev(N, gpu_device))
    _check_phi("r%d" % r, got.cpu().numpy(), want, bound)
    assert torch.equal(m(_dev(V, gpu_device), _dev(N, gpu_device)), got)


def test_forward_is_independent_of_batch_position_and_chunk(golden, gpu_device):
    V, N = _dev(golden["V_r16"], gpu_device), _dev(golden["N_r16"], gpu_device)
    m = _dpsr(16, 2, True, True, gpu_device)
    both = m(V, N)
    pick = torch.tensor([1, 0, 0, 1, 0], device=gpu_device)
    Vp, Np = V[pick].contiguous(), N[pick].contiguous()
    for chunk in (None, 1, 2, 3, 5):
        got = m(Vp, Np, chunk=chunk)
        assert torch.equal(got, both[pick]), chunk
    assert torch.equal(m(V[1:].contiguous(), N[1:].contiguous())[0], both[1])


def test_composed_entry_point_equals_its_parts(golden, gpu_device):
    from slide_amd import _ext
    V, N = _dev(golden["V_r16"], gpu_device), _dev(golden["N_r16"], gpu_device)
    for shift, scale in ((True, True), (False, True), (True, False), (False, False)):
        m = _dpsr(16, 2, shift, scale, gpu_device)
        spec = _ext.fft3_r2c(_ext.point_rasterize_fixed(V, N, 16))
        phi = _ext.fft3_c2r(_ext.dpsr_spectral(spec, m.G), overwrite=True)
        if shift or scale:
            fv = _ext.grid_interp(phi.unsqueeze(-1), V).squeeze(-1)
            phi = _ext.dpsr_finish(phi, fv, shift=shift, scale=scale)
        assert torch.equal(m(V, N), phi), (shift, scale)


# ------------------------------------------------------------------------------------------------------------ error paths
def test_error_paths(golden, gpu_device):
    from dpsr_utils.utils import grid_interp, point_rasterize
    m = _dpsr(16, 2, True, True, gpu_device)
    V, N = golden["V_r16"].copy(), golden["N_r16"].copy()
    bad = V.copy()
    bad[1, 5, 2] = 1.0
    with pytest.raises(ValueError):
        m(_dev(bad, gpu_device), _dev(N, gpu_device))
    with pytest.raises(ValueError):
        point_rasterize(_dev(bad, gpu_device), _dev(N, gpu_device), (16, 16, 16))
    with pytest.raises(ValueError):
        grid_interp(torch.zeros(2, 16, 16, 16, 1, device=gpu_device), _dev(bad, gpu_device))
    for value in (np.nan, np.inf, 2.0 ** 20):
        badn = N.copy()
        badn[0, 3, 1] = value
        with pytest.raises(ValueError):
            m(_dev(V, gpu_device), _dev(badn, gpu_device))
    badv = V.copy()
    badv[0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        m(_dev(badv, gpu_device), _dev(N, gpu_device))
    with pytest.raises(ValueError):
        m(_dev(V, gpu_device), _dev(N[:, :-1], gpu_device))
    with pytest.raises(ValueError):
        point_rasterize(_dev(V, gpu_device), _dev(N[:1], gpu_device), (16, 16, 16))
    # a clean call still works afterwards
    assert torch.isfinite(m(_dev(V, gpu_device), _dev(N, gpu_device))).all()


# ------------------------------------------------------------------------------------------------------------ CLI
def test_psr_grid_cli(tmp_path, gpu_device):
    from dpsr_evaluation import points_to_dpsr_grid, shapenet_psr_normalize
    V, N = C.sphere_cloud(7, 3, 300)
    pts = ((V - 0.5) * 1.7).astype(np.float32)  # (some other scale and centre: the normalisation has work to do)
    src, dst = str(tmp_path / "clouds.npz"), str(tmp_path / "out" / "grid.npz")
    np.savez(src, points=np.concatenate([pts, N], axis=2))
    cli = [sys.executable, os.path.join(REPO, "pointnet2", "sampling_and_inference", "psr_grid.py"), "--points", src,
           "--split_points_to_normals", "--explicit_normalize", "--grid_res", "16", "--psr_sigma", "2", "--batch_size", "2", "--save", dst]
    r = subprocess.run(cli, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.load(dst)
    assert sorted(out.files) == ["normals", "points", "psr_grid"]
    assert out["psr_grid"].shape == (3, 16, 16, 16) and out["psr_grid"].dtype == np.float32
    assert out["points"].shape == (3, 300, 3) and out["normals"].shape == (3, 300, 3)
    assert np.array_equal(out["normals"], N)
    want_pts = torch.clamp(shapenet_psr_normalize(_dev(pts, gpu_device)) / 1.2 + 0.5, min=0, max=0.99)
    assert np.array_equal(out["points"], want_pts.cpu().numpy())
    assert out["points"].min() >= 0 and out["points"].max() <= 0.99
    m = _dpsr(16, 2, True, True, gpu_device)
    grid, p, _ = points_to_dpsr_grid(_dev(pts, gpu_device), _dev(N, gpu_device), m, explicit_normalize=True)
    assert np.array_equal(out["psr_grid"], grid.cpu().numpy()) and np.array_equal(out["psr_grid"], m(want_pts, _dev(N, gpu_device)).cpu().numpy())
