"""CPU: the DPSR fixture, the numpy restatement of tests/dpsr_cases.py, the wrong arithmetics and the bounds -- everything the GPU
tests of tests/test_hip_dpsr.py rely on, checked without a device."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, load_golden
import dpsr_cases as C

sys.path.insert(0, os.path.join(REPO, "pointnet2"))


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_dpsr.npz")


@pytest.fixture(scope="module")
def restated(golden):
    """{case: (phi, detail, bound (B,))} of the float64 restatement, computed once"""
    out = {}
    for name, r, sig, shift, scale in C.CASES:
        phi, d = C.restate(golden["V_r%d" % r], golden["N_r%d" % r], r, sig, shift, scale, detail=True)
        out[name] = (phi, d, C.phi_bound(r, sig, shift, scale, d))
    return out


def test_fixture_size_cap():
    assert os.path.getsize(os.path.join(GOLDEN, "golden_dpsr.npz")) <= C.SIZE_CAP


def test_fixture_holds_the_edge_points(golden):
    for r in (16, 32):
        V = golden["V_r%d" % r]
        q = V.astype(np.float64) * r
        assert V.min() >= 0 and V.max() < 1
        assert (V == 0).all(2).any(), "the point at 0"
        assert ((q == np.floor(q)).sum(2) == 1).any() and ((q == np.floor(q)).sum(2) == 3).any(), "points on lattice planes"
        assert all((V[:, :, d] > (r - 1) / r).any() for d in range(3)), "points in the last cell of each axis"
        assert max(int((V[b] == V[b, -1]).all(1).sum()) for b in range(len(V))) >= 40, "40 copies of one point"
    for name, *_ in C.CASES:
        assert float(golden["fv0_ratio_" + name]) >= 0.05


def test_restatement_equals_the_reference_in_float64(golden, restated):
    for name, r, sig, shift, scale in C.CASES:
        want = golden["phi64_" + name]
        assert want.dtype == np.float64
        got = C.golden_cells(golden, name, r, restated[name][0])
        err = float(np.abs(got - want).max())
        print("%s: restatement against phi64 %.2e" % (name, err))
        assert err <= 1e-12, name
    want = np.zeros(2 * 3 * 16 ** 3)
    want[golden["ras64_r16_idx"]] = golden["ras64_r16_val"]
    assert np.abs(C.rasterize(golden["V_r16"], golden["N_r16"], 16).reshape(-1) - want).max() <= 1e-14
    for r in (16, 32):
        V = golden["V_r%d" % r]
        grid = np.random.RandomState(int(golden["interp_seed"]) + r).standard_normal((len(V), r, r, r, 4)).astype(np.float32)
        assert np.abs(C.interp(grid, V) - golden["interp64_r%d" % r]).max() <= 1e-13


def test_module_constants_are_the_references_bit_for_bit(golden):
    from dpsr_utils.dpsr import DPSR
    from dpsr_utils.utils import fftfreqs, spec_gaussian_filter
    for r, sig in ((16, 2), (32, 2), (32, 10)):
        m = DPSR((r, r, r), sig=sig)
        assert m.G.dtype == torch.float32 and tuple(m.G.shape) == (r, r, r // 2 + 1, 1, 1)
        assert np.array_equal(m.G.numpy().reshape(r, r, r // 2 + 1), golden["G_r%d_s%d" % (r, sig)])
        assert spec_gaussian_filter((r, r, r), sig).dtype == torch.float64
        f = fftfreqs((r, r, r))
        assert f.dtype == torch.float32 and np.array_equal(f.numpy(), golden["freqs_r%d" % r])
    assert tuple(fftfreqs((16, 16, 16), exact=False).shape) == (16, 16, 8, 3)
    assert "G" in dict(DPSR((16, 16, 16)).named_buffers())


def test_bound_admits_the_reference_and_sees_every_wrong_arithmetic(golden, restated):
    """bound >= e_ref on every case (the reference's own float32 run passes), and every wrong arithmetic lies at least 10 bounds
    from phi64 on at least one case -- the corner mistake at the lattice-plane points, the wrap mistake at the last-cell points"""
    far = {w: 0.0 for w in C.WRONG}
    for name, r, sig, shift, scale in C.CASES:
        bound = restated[name][2]
        assert np.isfinite(bound).all()
        eref = float(golden["eref_" + name])
        e32 = np.abs(golden["phi32_" + name].astype(np.float64) - golden["phi64_" + name]).reshape(len(bound), -1).max(1)
        print("%s: bound %s, e_ref %.2e, bound / e_ref %.1f" % (name, bound, eref, bound.min() / eref))
        assert bound.min() >= eref and (e32 <= bound).all(), name
        want = golden["phi64_" + name]
        for w in C.WRONG:
            got = C.golden_cells(golden, name, r, C.restate(golden["V_r%d" % r], golden["N_r%d" % r], r, sig, shift, scale, wrong=w))
            dist = (np.abs(got - want).reshape(len(bound), -1).max(1) / bound).max()
            print("    %-8s %.1f bounds away" % (w, dist))
            far[w] = max(far[w], float(dist))
    assert all(v >= 10 for v in far.values()), far


def test_cell_mistakes_show_where_they_should(golden):
    """on the rasterized normals of the r 16 inputs: `corner` changes the cells of lattice-plane points, `nowrap` those of last-cell points"""
    V, N, r = golden["V_r16"][:1], golden["N_r16"][:1], 16
    q = V.astype(np.float64) * r
    plane = (q == np.floor(q)).any(2)[0] & ~(V == 0).all(2)[0]
    last = (V > (r - 1) / r).any(2)[0]
    inner = ~plane & ~last & ~(V == 0).any(2)[0]
    for w, where in (("corner", plane), ("nowrap", last)):
        assert where.any()
        assert np.abs(C.rasterize(V[:, where], N[:, where], r, w) - C.rasterize(V[:, where], N[:, where], r)).max() > 0.1
        assert np.array_equal(C.rasterize(V[:, inner], N[:, inner], r, w), C.rasterize(V[:, inner], N[:, inner], r))


def test_unsupported_sizes_and_cpu_tensors_raise():
    from dpsr_utils.dpsr import DPSR
    from dpsr_utils.utils import grid_interp, point_rasterize
    for res in ((24, 24, 24), (8, 8, 8), (512, 512, 512), (16, 16, 32), (16, 16)):
        with pytest.raises(ValueError):
            DPSR(res)
    m = DPSR((16, 16, 16), sig=2)
    V = torch.rand(1, 10, 3) * 0.9
    with pytest.raises(RuntimeError):
        m(V, V.clone())
    with pytest.raises(RuntimeError):
        point_rasterize(V, V.clone(), (16, 16, 16))
    with pytest.raises(RuntimeError):
        grid_interp(torch.zeros(1, 16, 16, 16, 2), V)
    with pytest.raises(ValueError):
        point_rasterize(V, V.clone(), (16, 16, 8))
