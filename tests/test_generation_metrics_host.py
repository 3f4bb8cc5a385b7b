"""CPU: the all-pairs Chamfer entry point of include/slide_hip.h Part 4 is exported and checks its arguments on the host, and the
plain-torch halves of metrics_point_cloud.generation_metrics (lgan_mmd_cov, knn) reproduce the reference's results recorded in
tests/golden/golden_generation_metrics.npz (tools/gen_golden_generation_metrics.py) on the recorded float64 matrices."""
import ctypes
import os
import sys

import numpy as np
import torch

from conftest import REPO, load_golden

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

COUNTS = ("tp", "fp", "fn", "tn")


def test_pairwise_symbol_exported():
    from slide_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "slide_chamfer_pairwise")
    assert "slide_chamfer_pairwise" in _lib.EXPORTS


def test_pairwise_entry_point_rejects_bad_arguments_without_a_launch():
    """argument checks run on the host before any launch (no device needed): a point stride below 3 -> -2; the symmetric form with
    m != n or p != q -> -2; an empty set is a no-op"""
    from slide_amd import build
    lib = ctypes.CDLL(build.build())
    null = None
    f = lib.slide_chamfer_pairwise
    assert f(2, 2, 4, 4, null, 2, null, 3, 0, null, null) == -2
    assert f(2, 2, 4, 4, null, 3, null, 2, 0, null, null) == -2
    assert f(2, 3, 4, 4, null, 3, null, 3, 1, null, null) == -2
    assert f(2, 2, 4, 5, null, 3, null, 3, 1, null, null) == -2
    assert f(0, 2, 4, 4, null, 3, null, 3, 0, null, null) == 0
    assert f(2, 0, 4, 4, null, 3, null, 3, 0, null, null) == 0
    assert f(0, 0, 4, 4, null, 3, null, 3, 1, null, null) == 0


def _matrices(g):
    return [torch.from_numpy(g[k]) for k in ("M_rs", "M_rr", "M_ss")]


def test_lgan_mmd_cov_and_knn_reproduce_the_reference_on_the_recorded_matrices():
    """same arithmetic on the same float64 numbers: floats to 1e-12 relative, coverage and the confusion counts exactly"""
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_generation_metrics.npz")
    M_rs, M_rr, M_ss = _matrices(g)
    assert M_rs.dtype == torch.float64
    r = G.lgan_mmd_cov(M_rs.t())
    assert sorted(r) == ["lgan_cov", "lgan_mmd", "lgan_mmd_smp"]
    for k, v in r.items():
        want = float(g["mmd_cov_" + k])
        assert v.dim() == 0 and v.dtype == torch.float64
        if k == "lgan_cov":
            assert float(v) == want
        else:
            assert abs(float(v) - want) <= 1e-12 * abs(want), (k, float(v), want)
    s = G.knn(M_rr, M_rs, M_ss, 1, sqrt=False)
    assert sorted(s) == sorted(COUNTS + ("precision", "recall", "acc_t", "acc_f", "acc"))
    for k, v in s.items():
        want = float(g["knn_" + k])
        if k in COUNTS:
            assert float(v) == want, (k, float(v), want)
        else:
            assert abs(float(v) - want) <= 1e-12 * abs(want), (k, float(v), want)
    assert sum(float(s[k]) for k in COUNTS) == M_rr.shape[0] + M_ss.shape[0]
    # sqrt=True and k = 3 run and stay consistent (no recorded values: the reference's ranks are what the first part pins)
    s3 = G.knn(M_rr, M_rs, M_ss, 3, sqrt=True)
    assert sum(float(s3[k]) for k in COUNTS) == M_rr.shape[0] + M_ss.shape[0]


def test_ties_resolve_to_the_lowest_index():
    import metrics_point_cloud.generation_metrics as G
    d = torch.tensor([[1.0, 1.0, 2.0], [3.0, 1.0, 1.0]], dtype=torch.float64)  # sample 0 ties refs 0 / 1, sample 1 ties refs 1 / 2
    assert float(G.lgan_mmd_cov(d)["lgan_cov"]) == float(np.float32(2.0 / 3.0))  # refs {0, 1}; a float32 ratio, as in the reference
    # x0's nearest others tie (x1 and y0 at 1) -> x1 (index 1, label 1); y0's tie (x0 and y1 at 1) -> x0 (label 1): predicted x
    Mxx = torch.tensor([[0.0, 1.0], [1.0, 0.0]], dtype=torch.float64)
    Mxy = torch.tensor([[1.0, 5.0], [5.0, 5.0]], dtype=torch.float64)
    Myy = torch.tensor([[0.0, 1.0], [1.0, 0.0]], dtype=torch.float64)
    s = G.knn(Mxx, Mxy, Myy, 1)
    assert [float(s[k]) for k in COUNTS] == [2.0, 1.0, 0.0, 1.0]


def test_fixture_condition_every_deciding_minimum_is_separated():
    """in the float64 matrices the runner-up of every row / column whose arg-min decides coverage or a 1-NN vote exceeds the
    minimum by more than 1e-4 relative -- three orders above the fp32 error bound (8 eps ~ 1e-6), so an fp32 evaluation must
    reproduce coverage and the confusion counts exactly.  The cross matrix holds a zero off its diagonal (a cloud shared by
    both sets)."""
    g = load_golden("golden_generation_metrics.npz")
    M_rs, M_rr, M_ss = (g[k] for k in ("M_rs", "M_rr", "M_ss"))
    n_r, n_s = M_rr.shape[0], M_ss.shape[0]
    assert M_rs.shape == (n_r, n_s) and g["samples"].shape[0] == n_s and g["refs"].shape[0] == n_r
    cs, cr = (int(v) for v in g["copy_smp_ref"])
    assert np.array_equal(g["samples"][cs], g["refs"][cr]) and cr != cs
    assert abs(M_rs[cr, cs]) <= 1e-12 and M_rs[cr, cs] == M_rs.min()
    full = np.block([[M_rr, M_rs], [M_rs.T, M_ss]])
    np.fill_diagonal(full, np.inf)
    worst = np.inf
    for A in (M_rs, full):  # coverage: each sample's nearest reference; 1-NN: each element's nearest other element
        srt = np.sort(A, axis=0)
        lo, up = srt[0], srt[1]
        assert np.all(up - lo > 1e-4 * np.abs(lo))
        worst = min(worst, float(((up - lo) / np.maximum(np.abs(lo), 1e-300)).min()))
    assert worst > 1e-4 and abs(worst - float(g["min_gap"])) <= 1e-9 * worst
