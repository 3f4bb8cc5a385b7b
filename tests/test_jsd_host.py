"""CPU: the host half of the JSD metric (metrics_point_cloud.generation_metrics: unit_cube_grid_point_cloud, the Bernoulli entropy,
jensen_shannon_divergence) against the reference's own results recorded in tests/golden/golden_jsd.npz (tools/gen_golden_jsd.py),
and the fixture's own conditions.  The float64 bounds are derived in tests/jsd_cases.py."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import REPO, load_golden
from jsd_cases import RESOLUTIONS, SETS, U, entropy_bound, jsd_bound

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

def test_fixture_holds_data_only_and_is_separated():
    g = load_golden("golden_jsd.npz")  # allow_pickle=False: arrays only
    assert float(g["min_margin"]) >= 1e-5
    for k in g.files:
        assert g[k].dtype in (np.float32, np.float64, np.int64), k
    s, c, o = g["pcs_sphere"], g["pcs_cube"], g["pcs_outside"]
    assert np.linalg.norm(s.astype(np.float64), axis=2).max() <= 0.5  # normalised into the sphere
    assert np.abs(c).max() <= 0.5 and np.linalg.norm(c.astype(np.float64), axis=2).max() > 0.5  # cube corners outside the sphere
    assert np.abs(o).max() > 0.5  # points outside the cube
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "golden_jsd.npz")) <= 781323  # the largest earlier fixture


@pytest.mark.parametrize("R", RESOLUTIONS)
def test_unit_cube_grid_is_the_reference_grid_bit_for_bit(R):
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_jsd.npz")
    grid, spacing = G.unit_cube_grid_point_cloud(R)
    assert grid.dtype == np.float32 and grid.shape == (R, R, R, 3) and spacing == 1.0 / float(R - 1)
    assert np.array_equal(grid.reshape(-1, 3).view(np.uint32), g["grid_%d_0" % R].view(np.uint32))
    clipped, spacing = G.unit_cube_grid_point_cloud(R, clip_sphere=True)
    assert clipped.dtype == np.float32 and spacing == 1.0 / float(R - 1)
    assert clipped.shape == g["grid_%d_1" % R].shape
    assert np.array_equal(clipped.view(np.uint32), g["grid_%d_1" % R].view(np.uint32))
    assert grid[3 % R, 1, R - 1, 0] == grid.reshape(-1, 3)[((3 % R) * R + 1) * R + R - 1, 0]  # flat index (i R + j) R + k
    import metrics_point_cloud as M
    assert M.unit_cube_grid_point_cloud is G.unit_cube_grid_point_cloud  # exported from the package
    assert M.jsd_between_point_cloud_sets is G.jsd_between_point_cloud_sets


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("R", RESOLUTIONS)
@pytest.mark.parametrize("clip", (0, 1))
def test_bernoulli_entropy_formula_on_the_recorded_counters(kind, R, clip):
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_jsd.npz")
    key = "%s_%d_%d" % (kind, R, clip)
    bern, n = g["bernoulli_" + key], g["pcs_" + kind].shape[0]
    assert len(bern) == len(g["grid_%d_%d" % (R, clip)]) == len(g["counters_" + key])
    assert g["counters_" + key].sum() == g["pcs_" + kind].shape[0] * g["pcs_" + kind].shape[1]
    total = G._bernoulli_entropy_sum(bern, n)
    want = float(g["entropy_" + key])
    got = total / len(bern)
    print("entropy", key, got, want, abs(got - want), entropy_bound(len(bern), total) / len(bern))
    assert abs(got - want) <= entropy_bound(len(bern), total) / len(bern)


@pytest.mark.parametrize("R", RESOLUTIONS)
def test_jensen_shannon_divergence_on_the_recorded_counters(R):
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_jsd.npz")
    for i, a in enumerate(SETS):
        for b in SETS[i + 1:]:
            P, Q = g["counters_%s_%d_1" % (a, R)], g["counters_%s_%d_1" % (b, R)]
            with warnings.catch_warnings():
                warnings.simplefilter("error")  # the two formulations agree: no warning
                got = G.jensen_shannon_divergence(P, Q)
            want = float(g["jsd_%s_%s_%d" % (a, b, R)])
            print("jsd", a, b, R, got, want, abs(got - want), jsd_bound(P, Q))
            assert isinstance(got, float) and 0.0 < got <= 1.0
            assert abs(got - want) <= jsd_bound(P, Q)
            assert abs(G._jsdiv(P, Q) - want) <= 1e-9  # the second formulation (the reference compares them at 1e-4)
    assert G.jensen_shannon_divergence(P, P) == 0.0


def test_jensen_shannon_divergence_errors_and_warning(monkeypatch):
    import metrics_point_cloud.generation_metrics as G
    with pytest.raises(ValueError, match="Negative values"):
        G.jensen_shannon_divergence(np.array([1.0, -1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match="Negative values"):
        G.jensen_shannon_divergence(np.array([1.0, 1.0]), np.array([-1.0, 1.0]))
    with pytest.raises(ValueError, match="Non equal size"):
        G.jensen_shannon_divergence(np.array([1.0, 1.0]), np.array([1.0, 1.0, 2.0]))
    assert abs(G.jensen_shannon_divergence(np.array([1.0, 0.0]), np.array([0.0, 3.0])) - 1.0) <= 4 * U  # disjoint supports: 1 bit
    monkeypatch.setattr(G, "_jsdiv", lambda P, Q: 0.5)
    with pytest.warns(UserWarning, match="don't agree"):
        G.jensen_shannon_divergence(np.array([1.0, 1.0]), np.array([1.0, 1.0]))


def test_cli_flags():
    import generation_evaluate as E
    a = E.build_parser().parse_args(["--samples", "a", "--ref", "b"])
    assert a.jsd is False and a.jsd_resolution == 28
    a = E.build_parser().parse_args(["--samples", "a", "--ref", "b", "--jsd", "--jsd_resolution", "9"])
    assert a.jsd is True and a.jsd_resolution == 9
    assert "JSD" not in E.KEYS
