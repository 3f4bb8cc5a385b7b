"""CPU: the float64 restatement of the approximate Earth Mover's Distance (tests/emd_cases.py::emd_ref, the yardstick of
tests/test_hip_emd.py) gives the reference's known answer, conserves mass and is not symmetric; the entry point of
include/slide_hip.h Part 4 is exported and checks its arguments on the host; tests/golden/golden_emd.npz
(tools/gen_golden_emd.py) separates every deciding minimum far enough for integer results to be compared exactly."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import emd_cases as E
from conftest import REPO, load_golden

sys.path.insert(0, os.path.join(REPO, "pointnet2"))


def test_known_answer_of_the_reference():
    """two points against two points: the match crosses, the cost is d(0,1) + d(1,0) = 0.30 + 0.41"""
    d = E.sqdist(E.KNOWN_XYZ1, E.KNOWN_XYZ2)
    assert abs(d[0, 1] + d[1, 0] - E.KNOWN_COST) <= 1e-6  # (float32 coordinates)
    cost, match = E.emd_ref(E.KNOWN_XYZ1, E.KNOWN_XYZ2, return_match=True)
    assert abs(cost - E.KNOWN_COST) <= 1e-6
    assert np.allclose(match, [[0, 1], [1, 0]], atol=1e-6)
    assert abs(E.emd_ref(E.KNOWN_XYZ1, E.KNOWN_XYZ2, np.float32) - E.KNOWN_COST) <= 1e-6
    assert E.case_reference("known", 2, 2)[0] == cost


def test_ten_levels_and_the_tolerance_constant():
    assert E.LEVELS == (-16384.0, -4096.0, -1024.0, -256.0, -64.0, -16.0, -4.0, -1.0, -0.25, 0.0)
    assert E.R == 8 * E.R_EMULATION and 1e-7 < E.R < 1e-4
    assert set(E.SIZES) == {(1, 1), (2, 2), (64, 64), (96, 48), (50, 130), (257, 255), (300, 1030), (1025, 1025)}
    assert len(E.CASES) == len(E.SIZES) * len(E.KINDS) + 1


@pytest.mark.parametrize("kind,n,m", [c for c in E.CASES if c[1] <= 257])
def test_float32_emulation_is_within_the_measured_ratio(kind, n, m):
    """R_EMULATION is what `python tests/emd_cases.py` measured over all of CASES; the smaller cases are re-measured here"""
    a, b = E.make_pair(kind, n, m)
    ref, S = E.case_reference(kind, n, m)
    assert abs(E.emd_ref(a, b, np.float32) - ref) <= E.R_EMULATION * 1.0001 * (abs(ref) + S)
    assert E.within(ref, ref, S)


@pytest.mark.parametrize("kind,n", [("cube", 64), ("gauss3", 64), ("dup", 257 - 2), ("apart", 96)])
def test_mass_conservation_when_the_clouds_have_equal_sizes(kind, n):
    """every point of either cloud ends fully matched: the last level (exp(0) = 1) hands out all that remains"""
    a, b = E.make_pair(kind, n, n)
    cost, match = E.emd_ref(a, b, return_match=True)
    assert match.min() >= 0
    assert np.allclose(match.sum(1), 1.0, atol=1e-6) and np.allclose(match.sum(0), 1.0, atol=1e-6)
    assert abs(cost - (match * E.sqdist(a, b)).sum()) <= 1e-9 * cost


def test_unequal_sizes_weigh_the_smaller_cloud():
    a, b = E.make_pair("cube", 96, 48)  # multiR = 2: a point of xyz2 takes the mass of two points of xyz1
    _, match = E.emd_ref(a, b, return_match=True)
    assert np.allclose(match.sum(1), 1.0, atol=1e-6) and np.allclose(match.sum(0), 2.0, atol=1e-6)


def test_the_argument_order_matters():
    a, b = E.make_pair("gauss3", 64, 64)
    ab, ba = E.emd_ref(a, b), E.emd_ref(b, a)
    assert abs(ab - ba) > 1e-4 * ab
    g = load_golden("golden_emd.npz")
    assert np.abs(g["M_rr"] - g["M_rr"].T).max() > 0.1  # on the fixture the two orders differ by up to 0.5


def test_identical_clouds_cost_nothing():
    a, _ = E.make_pair("gauss3", 64, 64)
    assert E.emd_ref(a, a) <= 1e-9 * E.scale(a, a)


def test_symbol_exported():
    from slide_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "slide_emd_pairwise")
    assert "slide_emd_pairwise" in _lib.EXPORTS
    assert ("emd_pairwise.hip", ["-ffp-contract=off"]) in build.SOURCES


def test_entry_point_rejects_bad_arguments_without_a_launch():
    """argument checks run on the host before any launch (no device needed): a point stride below 3 -> -2; the paired form with
    m != n -> -2; clouds whose mass vectors do not fit the LDS -> -2; an empty set is a no-op"""
    from slide_amd import build
    lib = ctypes.CDLL(build.build())
    null = None
    f = lib.slide_emd_pairwise
    assert f(2, 2, 4, 4, null, 2, null, 3, 0, null, null) == -2
    assert f(2, 2, 4, 4, null, 3, null, 2, 0, null, null) == -2
    assert f(2, 3, 4, 4, null, 3, null, 3, 1, null, null) == -2
    assert f(2, 2, 9729, 9728, null, 3, null, 3, 0, null, null) == -2  # 2 (p + q) floats + 8 KB > 160 KB
    assert f(1, 1, 1 << 30, 1 << 30, null, 3, null, 3, 0, null, null) == -2
    assert f(0, 2, 4, 4, null, 3, null, 3, 0, null, null) == 0
    assert f(2, 0, 4, 4, null, 3, null, 3, 0, null, null) == 0
    assert f(2, 2, 0, 4, null, 3, null, 3, 0, null, null) == 0
    assert f(0, 0, 4, 4, null, 3, null, 3, 1, null, null) == 0


def test_scope_errors_without_a_device():
    from metrics_point_cloud import emd, generation_metrics as G
    x = torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError):
        emd.earth_mover_distance(x, x)
    with pytest.raises(RuntimeError):
        emd.EMD_distance()(x[0], x[0])
    with pytest.raises(NotImplementedError):
        emd.earth_mover_distance(x, x, return_match=True)
    with pytest.raises(NotImplementedError):
        emd.earth_mover_distance(x.clone().requires_grad_(True), x)
    with pytest.raises(RuntimeError):
        G.pairwise_emd(x, x)
    with pytest.raises(NotImplementedError):
        G.pairwise_emd(x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        G.pairwise_emd(x[0], x)
    import generation_evaluate as cli
    assert cli.EMD_KEYS == ("lgan_mmd-EMD", "lgan_cov-EMD", "lgan_mmd_smp-EMD", "1-NN-EMD-acc_t", "1-NN-EMD-acc_f", "1-NN-EMD-acc")
    assert cli.build_parser().parse_args(["--samples", "a", "--ref", "b", "--emd"]).emd
    assert not cli.build_parser().parse_args(["--samples", "a", "--ref", "b"]).emd


def test_fixture_condition_every_deciding_minimum_is_separated():
    """before anything integer is compared: in the float64 matrices the runner-up of every column whose arg-min decides coverage
    or a 1-NN vote exceeds the minimum by at least 20 R relative, so a kernel within R reproduces coverage and the confusion counts
    exactly.  The recorded statistics are consistent with the recorded matrices."""
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_emd.npz")
    c = load_golden("golden_generation_metrics.npz")
    M_rs, M_rr, M_ss = (g[k] for k in ("M_rs", "M_rr", "M_ss"))
    n_r, n_s = c["refs"].shape[0], c["samples"].shape[0]
    assert M_rs.shape == (n_r, n_s) and M_rr.shape == (n_r, n_r) and M_ss.shape == (n_s, n_s) and M_rs.dtype == np.float64
    gap_nn, gap_cov = E.separation(M_rs, M_rr, M_ss)
    assert gap_nn == float(g["gap_nn"]) and gap_cov == float(g["gap_cov"])
    assert gap_nn >= 1.3e-4 and gap_cov >= 3e-3
    assert min(gap_nn, gap_cov) >= 20 * E.R
    # spot check of the recorded matrices against the restatement (one entry of each)
    P = c["refs"].shape[1]
    for M, a, b, (i, j) in ((M_rs, c["refs"], c["samples"], (7, 3)), (M_rr, c["refs"], c["refs"], (2, 11)),
                            (M_ss, c["samples"], c["samples"], (23, 0))):
        assert abs(E.emd_ref(a[i], b[j]) / P - M[i, j]) <= 1e-12 * M[i, j]
    t_rs, t_rr, t_ss = (torch.from_numpy(M) for M in (M_rs, M_rr, M_ss))
    r = G.lgan_mmd_cov(t_rs.t())
    for k, v in r.items():
        want = float(g["mmd_cov_" + k])
        assert float(v) == want if k == "lgan_cov" else abs(float(v) - want) <= 1e-12 * abs(want), k
    s = G.knn(t_rr, t_rs, t_ss, 1, sqrt=False)
    for k, v in s.items():
        want = float(g["knn_" + k])
        assert float(v) == want if k in ("tp", "fp", "fn", "tn") else abs(float(v) - want) <= 1e-12 * abs(want), k
