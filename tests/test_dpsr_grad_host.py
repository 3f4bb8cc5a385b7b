"""CPU: the DPSR gradient fixture, the numpy restatement of the backward in tests/dpsr_grad_cases.py, the wrong arithmetics and the
bounds -- everything the GPU tests of tests/test_hip_dpsr_backward.py rely on, checked without a device.

Condition (a): the reference's own float32 gradients pass the bound on every case.  Condition (b): every wrong arithmetic lies at
least 10 bounds from the float64 gradients in EVERY output it applies to, on every sample of every case it applies to
(dpsr_grad_cases.applies).  The table is in profiles/dpsr_backward.md."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import dpsr_cases as C
import dpsr_grad_cases as GC


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_dpsr.npz"), load_golden("golden_dpsr_grad.npz")


@pytest.fixture(scope="module")
def restated(golden):
    """{case: (g, dV, dN, bound dV (B,), bound dN (B,))} of the float64 restatement, computed once"""
    g0, _ = golden
    out = {}
    for index, (name, r, sig, shift, scale) in enumerate(GC.CASES):
        V, N = g0["V_r%d" % r], g0["N_r%d" % r]
        g = GC.upstream(index, C.restate(V, N, r, sig, shift, scale))
        dV, dN, d = GC.backward(V, N, r, sig, shift, scale, g, detail=True)
        bV, bN = GC.grad_bounds(V, N, r, sig, shift, scale, d, dV, dN)
        out[name] = (g, dV, dN, bV, bN)
    return out


def _mx(x, nb):
    return np.abs(x).reshape(nb, -1).max(1)


def test_fixture_size_cap():
    assert os.path.getsize(os.path.join(GOLDEN, "golden_dpsr_grad.npz")) <= C.SIZE_CAP


def test_upstream_recipe_reproduces_the_recorded_gradient(golden, restated):
    _, gg = golden
    for name, r, *_ in GC.CASES:
        g = restated[name][0]
        assert g.dtype == np.float32
        if r == 16:
            rec = gg["g_" + name]
            assert rec.dtype == np.float32 and rec.shape == g.shape
            # (tanh and the transforms of another numpy may differ in the last place of a double: a float32 ulp at the most)
            assert np.abs(g.astype(np.float64) - rec).max() <= 2.0 ** -22 * np.abs(rec).max(), name
        else:
            assert ("g_" + name) not in gg.files


def test_restatement_equals_the_reference_in_float64(golden, restated):
    _, gg = golden
    for name, *_ in GC.CASES:
        _, dV, dN, _, _ = restated[name]
        for what, got in (("dV", dV), ("dN", dN)):
            want = gg["%s64_%s" % (what, name)]
            assert want.dtype == np.float64 and want.shape == got.shape
            err = float(np.abs(got - want).max() / np.abs(want).max())
            print("%s %s: restatement against the reference's float64 autograd %.2e of the largest entry" % (name, what, err))
            assert err <= 1e-10, (name, what)


def test_bound_admits_the_references_float32_gradients(golden, restated):
    """condition (a)"""
    _, gg = golden
    for name, *_ in GC.CASES:
        _, _, _, bV, bN = restated[name]
        nb = len(bV)
        assert np.isfinite(bV).all() and np.isfinite(bN).all()
        for what, b in (("dV", bV), ("dN", bN)):
            want = gg["%s64_%s" % (what, name)]
            e32 = _mx(gg["%s32_%s" % (what, name)].astype(np.float64) - want, nb)
            print("%s %s: bound %s (%s of the largest entry), reference float32 error / bound %s" % (
                name, what, b, b / _mx(want, nb), e32 / b))
            assert (e32 <= b).all(), (name, what)


def test_bound_sees_every_wrong_arithmetic(golden, restated):
    """condition (b)"""
    g0, gg = golden
    for name, r, sig, shift, scale in GC.CASES:
        g, _, _, bV, bN = restated[name]
        nb = len(bV)
        V, N = g0["V_r%d" % r], g0["N_r%d" % r]
        for w in GC.WRONG:
            outs = [what for what in ("dV", "dN") if GC.applies(w, what, sig, shift, scale)]
            if not outs:
                continue
            wV, wN = GC.backward(V, N, r, sig, shift, scale, g, wrong=w)
            dist = {"dV": _mx(wV - gg["dV64_" + name], nb) / bV, "dN": _mx(wN - gg["dN64_" + name], nb) / bN}
            print("%s %-12s %s bounds away" % (name, w, {k: dist[k] for k in outs}))
            assert all((dist[k] >= 10).all() for k in outs), (name, w, dist)


def test_lattice_plane_points_tell_the_subgradient(golden, restated):
    """on the axis where a point sits on a lattice plane, sign(0) = 0 halves the derivative: `abs1` differs there and nowhere else"""
    g0, gg = golden
    name, r, sig, shift, scale = GC.CASES[3]
    V, N = g0["V_r16"], g0["N_r16"]
    g = restated[name][0]
    q = V.astype(np.float64) * r
    plane = q == np.floor(q)
    assert plane.any() and not plane.all()
    wV, _ = GC.backward(V, N, r, sig, shift, scale, g, wrong="abs1")
    diff = np.abs(wV - gg["dV64_" + name])
    assert (diff[~plane] <= 1e-12 * np.abs(gg["dV64_" + name]).max()).all()
    assert (diff[plane].max() >= 10 * restated[name][3]).all()
