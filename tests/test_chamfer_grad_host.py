"""CPU: tests/golden/golden_chamfer_grad.npz (the reference's calc_cd gradients from its own autograd,
tools/gen_golden_chamfer_grad.py) -- the fixture condition, the float64 restatement of slide_chamfer_cd_bwd's math
(tests/chamfer_grad_cases.py) against the recorded gradients, and the mutant check: wrong formulas must miss the GPU test's bound."""
import numpy as np
import pytest

from chamfer_grad_cases import MUTANTS, dred_of_loss, nearest, restate, tolerance
from conftest import load_golden

CASES = ("xyz", "feat", "fan")
GAP = 1e-4


def _case(g, name):
    return g[name + "_out"], g[name + "_gt"], g[name + "_i1"], g[name + "_i2"]


def _variants(g, name):
    """(tag, weight index, weight) of every recorded gradient of the case"""
    feat = g[name + "_out"].shape[2] > 3
    return [(tag, k, float(w)) for k, w in enumerate(g["weights"][:2 if feat else 1]) for tag in ("p", "t")]


@pytest.mark.parametrize("name", CASES)
def test_fixture_condition(name):
    """no zero distance or feature term, every neighbour ahead of its runner-up by a relative gap > 1e-4: an fp32 search must pick the
    recorded indices; the constructed fan-in is there"""
    g = load_golden("golden_chamfer_grad.npz")
    out, gt, i1, i2 = _case(g, name)
    j1, j2, D = nearest(gt, out)
    assert np.array_equal(j1, i1) and np.array_equal(j2, i2)
    for M, idx, own, other in ((D, i1, gt, out), (D.transpose(0, 2, 1), i2, out, gt)):
        srt = np.sort(M, axis=2)
        assert srt[:, :, 0].min() > 0
        assert ((srt[:, :, 1] - srt[:, :, 0]) / srt[:, :, 0]).min() > GAP
        if own.shape[2] > 3:
            near = np.take_along_axis(other.astype(np.float64), idx[:, :, None], axis=1)
            assert ((own[:, :, 3:] - near[:, :, 3:]) ** 2).sum(-1).min() > 0
    if name == "fan":
        indeg = np.bincount(i1[0], minlength=out.shape[1])
        assert indeg.max() >= 64 and (indeg == 0).any()
    assert g["weights"].tolist() == [0.0, 0.1]
    assert out.shape[1] != gt.shape[1]  # unequal point counts


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_gradients(name):
    g = load_golden("golden_chamfer_grad.npz")
    out, gt, i1, i2 = _case(g, name)
    B, n_gt, n_out = gt.shape[0], gt.shape[1], out.shape[1]
    for tag, k, w in _variants(g, name):
        dgt, dout, Sgt, Sout, _, _ = restate(gt, out, i1, i2, dred_of_loss(B, n_gt, n_out, tag, w))
        for got, S, key in ((dout, Sout, "gout"), (dgt, Sgt, "ggt")):
            want = g["%s_%s_%s_w%d" % (name, key, tag, k)]
            # float64 round-off: a few hundred units of 2^-53 on the magnitude sum (the fan-in point sums 160 terms)
            assert np.all(np.abs(got - want) <= 1e-13 * S + 1e-300), (name, tag, k, key, np.abs(got - want).max())


@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_formulas_miss_the_gpu_bound(mutant):
    """the scatter part dropped, its sign flipped, the factor 2 missing, the 1 / (2 sqrt) factor missing: each is outside the
    elementwise bound of tests/test_hip_chamfer_backward.py on every case it applies to (the missing 1 / (2 sqrt) factor only
    changes the cd_p form, whose dred has the square-root columns)"""
    g = load_golden("golden_chamfer_grad.npz")
    for name in CASES:
        out, gt, i1, i2 = _case(g, name)
        B, n_gt, n_out, F = gt.shape[0], gt.shape[1], out.shape[1], gt.shape[2] - 3
        for tag, k, w in _variants(g, name):
            if mutant == "no_sqrt_factor" and tag == "t":
                continue
            dred = dred_of_loss(B, n_gt, n_out, tag, w)
            _, _, Sgt, Sout, mgt, mout = restate(gt, out, i1, i2, dred)
            dgt, dout, _, _, _, _ = restate(gt, out, i1, i2, dred, mutant=mutant)
            worst = 0.0
            for got, S, m, key in ((dout, Sout, mout, "gout"), (dgt, Sgt, mgt, "ggt")):
                err, tol = np.abs(got - g["%s_%s_%s_w%d" % (name, key, tag, k)]), tolerance(S, m, F)
                worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))  # (tol == 0: the feature channels at w = 0)
            assert worst > 1.0, (mutant, name, tag, k, worst)
