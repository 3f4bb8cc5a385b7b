"""GPU: the occupancy-grid kernel (slide_amd/csrc/occupancy_grid.hip through _ext.occupancy_grid) and the JSD functions of
metrics_point_cloud.generation_metrics on it: the reference's counters recorded in tests/golden/golden_jsd.npz exactly, every point
of large random sets against a float64 brute force, constructed ties, the invariances of integer accumulation, scope and the CLI.

The float64 bound of the brute-force test (u = 2^-24, the unit roundoff of fp32).  The kernel's distance is
d32 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with dx = fl(p.x - axis[i]) etc.: every axis term passes one rounded subtraction (squared:
(1 + u)^2) and at most three more roundings (the product, two fused adds), so d32 lies in d [(1 - u)^5, (1 + u)^5] for the exact
squared distance d to the float32 cell centre.
  * scan step (the chosen cell minimises d32 over the admissible cells): d(chosen) (1 - u)^5 <= d32(chosen) <= d32(best)
    <= d(best) (1 + u)^5, so d(chosen) <= d(best) ((1 + u) / (1 - u))^5 <= d(best) (1 + 10.001 u);
  * lattice step (per axis the bracket end with the smaller |fl(p - axis)|; clamped axes are exact): per axis
    |dx(chosen)| (1 - u) <= |dx(other)| (1 + u), so d(chosen) <= d(any cell) ((1 + u) / (1 - u))^2 <= d (1 + 4.001 u).
Asserted: d(chosen) - d(best) <= 11 u d(best) + 1e-30 (the absolute term covers fp32 underflow of a squared difference below
1e-19; the float64 evaluation itself adds about 1e-16 d, inside the slack between 10.001 and 11)."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from jsd_cases import RESOLUTIONS, SETS, entropy_bound, jsd_bound

sys.path.insert(0, os.path.join(REPO, "pointnet2"))
pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
KEYS = ("lgan_mmd-CD", "lgan_cov-CD", "lgan_mmd_smp-CD", "1-NN-CD-acc_t", "1-NN-CD-acc_f", "1-NN-CD-acc")


def _grid(R, sphere):
    import metrics_point_cloud.generation_metrics as G
    return G._grid_axis_and_mask(R, sphere)


def _run(pts, R, sphere, cells=False):
    """pts: (S, P, C) numpy or CUDA tensor -> int64 numpy arrays (counts, clouds[, cells])"""
    from slide_amd import _ext
    axis, _, mask = _grid(R, sphere)
    t = pts if torch.is_tensor(pts) else torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
    out = _ext.occupancy_grid(t, torch.tensor(axis), torch.tensor(mask), return_cells=cells)
    assert all(o.dtype == torch.int32 for o in out)
    assert out[0].shape == out[1].shape == (R ** 3,)
    return tuple(o.cpu().numpy().astype(np.int64) for o in out)


def _clouds(rs, S, P, kind):
    """normalised: Gaussian blobs scaled into the sphere; wide: un-normalised (many points outside the sphere and the cube);
    mixed: alternating clouds of both"""
    x = rs.standard_normal((S, P, 3)) * rs.uniform(0.3, 1.0, (S, 1, 3))
    x = x / np.maximum(np.linalg.norm(x, axis=2).max(axis=1), 1e-9)[:, None, None] * 0.5
    if kind == "wide":
        x = x * 1.5 + rs.uniform(-0.2, 0.2, (S, 1, 3))
    elif kind == "mixed":
        x[1::2] = x[1::2] * rs.uniform(1.0, 3.0, (len(x[1::2]), 1, 1)) + rs.uniform(-0.3, 0.3, (len(x[1::2]), 1, 3))
    return x.astype(np.float32)


def _check_counters(counts, clouds, cells, S, P, mask):
    """the counters are the histogram of the per-point cells; sums and the admissibility mask"""
    R3 = len(mask)
    assert counts.sum() == S * P
    assert clouds.max(initial=0) <= S and counts.min(initial=0) >= 0
    assert np.array_equal(clouds > 0, counts > 0)
    assert not counts[~mask].any() and not clouds[~mask].any()
    if cells is not None:
        assert cells.shape == (S, P) and cells.min(initial=0) >= 0 and cells.max(initial=0) < R3
        assert np.array_equal(np.bincount(cells.reshape(-1), minlength=R3), counts)
        per_cloud = np.unique(cells + np.arange(S)[:, None] * R3)
        assert np.array_equal(np.bincount(per_cloud % R3, minlength=R3), clouds)


# ------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("R", RESOLUTIONS)
@pytest.mark.parametrize("clip", (0, 1))
def test_counters_equal_the_reference_fixture(gpu_device, kind, R, clip):
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_jsd.npz")
    key = "%s_%d_%d" % (kind, R, clip)
    pcs = g["pcs_" + kind]
    ent, counters = G.entropy_of_occupancy_grid(pcs, R, bool(clip))  # numpy input: moved to the current device
    assert isinstance(ent, float) and isinstance(counters, np.ndarray) and counters.dtype == np.float64
    assert counters.shape == g["counters_" + key].shape
    assert np.array_equal(counters, g["counters_" + key])
    bound = entropy_bound(len(counters), float(g["entropy_" + key]) * len(counters)) / len(counters)
    print("entropy", key, ent, float(g["entropy_" + key]), bound)
    assert abs(ent - float(g["entropy_" + key])) <= bound
    c2, b2 = G.occupancy_counters(torch.from_numpy(pcs).to(gpu_device), R, bool(clip))  # tensor input
    assert np.array_equal(c2, counters) and np.array_equal(b2, g["bernoulli_" + key])
    ent2, c3 = G.entropy_of_occupancy_grid(torch.from_numpy(pcs).to(gpu_device), R, in_sphere=bool(clip))
    assert ent2 == ent and np.array_equal(c3, counters)


@pytest.mark.parametrize("R", RESOLUTIONS)
def test_jsd_matches_the_reference_fixture(gpu_device, R):
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_jsd.npz")
    for i, a in enumerate(SETS):
        for b in SETS[i + 1:]:
            got = G.jsd_between_point_cloud_sets(g["pcs_" + a], torch.from_numpy(g["pcs_" + b]).to(gpu_device), R)
            want = float(g["jsd_%s_%s_%d" % (a, b, R)])
            bound = jsd_bound(g["counters_%s_%d_1" % (a, R)], g["counters_%s_%d_1" % (b, R)])
            print("jsd", a, b, R, got, want, bound)
            assert abs(got - want) <= bound
    got = G.jsd_between_point_cloud_sets(g["pcs_sphere"], g["pcs_cube"])  # the default resolution is 28
    assert abs(got - float(g["jsd_sphere_cube_28"])) <= jsd_bound(g["counters_sphere_28_1"], g["counters_cube_28_1"])


def test_verbose_warnings(gpu_device):
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_jsd.npz")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        G.entropy_of_occupancy_grid(g["pcs_sphere"], 9, True, verbose=True)
        G.entropy_of_occupancy_grid(g["pcs_outside"], 9, True)  # silent without verbose
    with pytest.warns(UserWarning, match="not in unit sphere"):
        G.entropy_of_occupancy_grid(g["pcs_cube"], 9, True, verbose=True)
    with pytest.warns(UserWarning, match="not in unit cube"):
        G.entropy_of_occupancy_grid(g["pcs_outside"], 9, False, verbose=True)


# ------------------------------------------------------------------ every point against float64
def _brute_excess(pts, cells, R, sphere, dev):
    """per point: (float64 squared distance to the chosen cell, float64 minimum over the admissible cells)"""
    axis, grid, mask = _grid(R, sphere)
    adm = torch.from_numpy(grid[mask].astype(np.float64)).to(dev)  # the float32 cell centres, exactly
    full = torch.from_numpy(grid.astype(np.float64)).to(dev)
    p = torch.from_numpy(pts.reshape(-1, 3).astype(np.float64)).to(dev)
    c = torch.from_numpy(cells.reshape(-1)).to(dev)
    d_chosen = ((p - full[c]) ** 2).sum(1)
    d_min = torch.empty_like(d_chosen)
    step = max(256, (1 << 26) // len(adm))  # at most 2^26 float64 distances (512 MB) at a time
    for s in range(0, len(p), step):
        q = p[s:s + step]
        d = (q[:, None, 0] - adm[None, :, 0]) ** 2
        d += (q[:, None, 1] - adm[None, :, 1]) ** 2
        d += (q[:, None, 2] - adm[None, :, 2]) ** 2
        d_min[s:s + step] = d.min(1)[0]
    return d_chosen.cpu().numpy(), d_min.cpu().numpy()


@pytest.mark.parametrize("S,P,R,sphere,kind", [(1000, 2048, 28, True, "mixed"), (300, 2048, 28, True, "normalised"),
                                               (37, 513, 9, True, "wide"), (64, 257, 17, False, "mixed"),
                                               (5, 300, 32, False, "wide"), (6, 1000, 32, True, "mixed"),
                                               (3, 1000, 2, False, "wide"), (2000, 1, 28, True, "wide"), (1, 5000, 3, True, "mixed")])
def test_every_point_against_a_float64_brute_force(gpu_device, S, P, R, sphere, kind):
    """bound: the module docstring.  No point is excluded: `cells` holds every point's choice, and the counters are checked to be
    exactly the histogram of those choices."""
    rs = np.random.RandomState(S * 31 + P * 7 + R)
    x = _clouds(rs, S, P, kind)
    counts, clouds, cells = _run(x, R, sphere, cells=True)
    mask = _grid(R, sphere)[2]
    _check_counters(counts, clouds, cells, S, P, mask)
    assert mask[cells].all()
    d_chosen, d_min = _brute_excess(x, cells, R, sphere, gpu_device)
    excess = d_chosen - d_min
    print("S %d P %d R %d sphere %s %s: max excess / d_min %.3e u, points off the float64 nearest cell %d, fraction of "
          "points outside the sphere %.3f" % (S, P, R, sphere, kind, float((excess / np.maximum(d_min, 1e-300)).max() / U32),
                                 int((excess > 0).sum()), float((np.linalg.norm(x.reshape(-1, 3), axis=1) > 0.5).mean())))
    assert np.all(excess <= 11 * U32 * d_min + 1e-30)
    # without the cells output the counters are the same numbers
    c2, b2 = _run(x, R, sphere)
    assert np.array_equal(c2, counts) and np.array_equal(b2, clouds)


# ------------------------------------------------------------------ constructed ties
def _exact_midpoints(axis):
    """indices i whose midpoint (axis[i] + axis[i + 1]) / 2 is a float32 number (then p - axis[i] and axis[i + 1] - p are equal
    exactly and so are their fp32 roundings), and those midpoints"""
    a = axis.astype(np.float64)
    m = (a[:-1] + a[1:]) / 2.0
    ok = m.astype(np.float32).astype(np.float64) == m
    return np.nonzero(ok)[0], m[ok].astype(np.float32)


def _expected_cells(pts, R, sphere):
    """exact rule in float64 on exactly representable inputs: nearest admissible cell, equal distances -> lowest flat index
    (equal |differences| give bitwise equal float64 sums, and numpy's argmin takes the first)"""
    _, grid, mask = _grid(R, sphere)
    flat, adm, p = np.nonzero(mask)[0], grid[mask].astype(np.float64), pts.astype(np.float64)
    return np.concatenate([flat[((p[s:s + 256, None, :] - adm[None]) ** 2).sum(-1).argmin(1)] for s in range(0, len(p), 256)])


@pytest.mark.parametrize("R", (28, 9, 32, 2))
def test_midpoints_take_the_lowest_flat_index(gpu_device, R):
    axis = _grid(R, False)[0]
    idx, mid = _exact_midpoints(axis)
    assert len(idx) >= 1, "no float32 midpoint at this resolution"
    rs = np.random.RandomState(R)
    pts, want = [], []
    for n, (i, m) in enumerate(zip(idx, mid)):
        j, k = rs.randint(0, R, 2)
        j2, k2 = idx[(n + 1) % len(idx)], idx[(n + 2) % len(idx)]
        pts += [(m, axis[j], axis[k]), (axis[j], m, axis[k]), (axis[j], axis[k], m),  # a face midpoint along each axis
                (m, mid[(n + 1) % len(idx)], axis[k]),  # an edge
                (m, mid[(n + 1) % len(idx)], mid[(n + 2) % len(idx)])]  # a cell corner: eight equidistant cells
        want += [(i * R + j) * R + k, (j * R + i) * R + k, (j * R + k) * R + i, (i * R + j2) * R + k, (i * R + j2) * R + k2]
    if R % 2 == 0 and axis[R // 2 - 1] == -axis[R // 2]:  # coordinate 0 is a midpoint in float32 at this even resolution
        h = R // 2 - 1
        pts += [(0.0, 0.0, 0.0), (0.0, axis[1], 0.0), (-0.0, 0.0, axis[0])]
        want += [(h * R + h) * R + h, (h * R + 1) * R + h, (h * R + h) * R + 0]
    pts, want = np.array(pts, np.float32), np.array(want, np.int64)
    assert np.array_equal(_expected_cells(pts, R, False), want)  # the construction is what it claims to be
    for shape in ((1, len(pts)), (len(pts), 1)):  # one cloud, and clouds of one point each
        cells = _run(pts.reshape(shape + (3,)), R, False, cells=True)[2]
        assert np.array_equal(cells.reshape(-1), want)


@pytest.mark.parametrize("R", (28, 9, 32))
def test_midpoints_at_the_sphere_surface(gpu_device, R):
    """in the clipped grid: midpoints between two admissible cells keep the lowest flat index; midpoints whose lower (or upper) cell
    is outside the sphere take the admissible one (the scan step)"""
    axis, _, mask = _grid(R, True)
    m3 = mask.reshape(R, R, R)
    idx, mid = _exact_midpoints(axis)
    pts, want, kinds = [], [], []
    for i, m in zip(idx, mid):
        for j in range(R):
            for k in range(R):
                for perm in range(3):
                    lo, hi = [i, j, k], [i + 1, j, k]
                    p = [m, axis[j], axis[k]]
                    for _ in range(perm):
                        lo, hi, p = lo[-1:] + lo[:-1], hi[-1:] + hi[:-1], p[-1:] + p[:-1]
                    a_lo, a_hi = m3[tuple(lo)], m3[tuple(hi)]
                    if not (a_lo or a_hi):
                        continue
                    c = lo if a_lo else hi
                    pts.append(p)
                    want.append((c[0] * R + c[1]) * R + c[2])
                    kinds.append(int(a_lo) + 2 * int(a_hi))
    pts, want, kinds = np.array(pts, np.float32), np.array(want, np.int64), np.array(kinds)
    assert (kinds == 3).any() and (kinds == 2).any() and (kinds == 1).any()
    rs = np.random.RandomState(R)  # at most 1000 of each kind (bounds the float64 brute force below)
    keep = np.concatenate([rs.permutation(np.nonzero(kinds == v)[0])[:1000] for v in (1, 2, 3)])
    pts, want = pts[keep], want[keep]
    assert np.array_equal(_expected_cells(pts, R, True), want)
    cells = _run(pts[None], R, True, cells=True)[2]
    assert np.array_equal(cells.reshape(-1), want)
    cells = _run(pts[:, None], R, True, cells=True)[2]
    assert np.array_equal(cells.reshape(-1), want)


# ------------------------------------------------------------------ integer accumulation: order, position, repeatability
def test_order_position_and_repeatability(gpu_device):
    rs = np.random.RandomState(4)
    S, P, R = 23, 700, 28
    x = _clouds(rs, S, P, "mixed")
    base = _run(x, R, True)
    _check_counters(base[0], base[1], None, S, P, _grid(R, True)[2])
    again = _run(x, R, True)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])  # two runs are equal
    xp = np.stack([c[rs.permutation(P)] for c in x])  # the points inside every cloud permuted
    got = _run(xp, R, True)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    got = _run(x[rs.permutation(S)], R, True)  # the clouds permuted
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    # a cloud's contribution does not depend on its position in the batch: the set without cloud i, plus cloud i alone
    for i in (0, 7, S - 1):
        rest = _run(np.delete(x, i, axis=0), R, True)
        one = _run(x[i:i + 1], R, True)
        assert np.array_equal(rest[0] + one[0], base[0]) and np.array_equal(rest[1] + one[1], base[1])
        assert one[1].max() == 1 and np.array_equal(one[1], (one[0] > 0).astype(np.int64))
    # features behind xyz are skipped through the point stride
    x6 = np.concatenate([x, rs.standard_normal((S, P, 3)).astype(np.float32)], axis=2)
    got = _run(x6, R, True)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


@pytest.mark.parametrize("R", (2, 3, 32))
def test_extreme_resolutions(gpu_device, R):
    rs = np.random.RandomState(R)
    x = _clouds(rs, 11, 400, "mixed")
    for sphere in (False, True):
        if R == 2 and sphere:
            continue  # its own case in test_error_cases: the eight cells of R = 2 are the cube's corners, none inside the sphere
        counts, clouds, cells = _run(x, R, sphere, cells=True)
        _check_counters(counts, clouds, cells, 11, 400, _grid(R, sphere)[2])
        d_chosen, d_min = _brute_excess(x, cells, R, sphere, gpu_device)
        assert np.all(d_chosen - d_min <= 11 * U32 * d_min + 1e-30)
    import metrics_point_cloud.generation_metrics as G
    ent, counters = G.entropy_of_occupancy_grid(x, R, False)
    assert counters.shape == (R ** 3,) and counters.sum() == 11 * 400 and 0.0 <= ent <= np.log(2.0)


def test_empty_inputs(gpu_device):
    from slide_amd import _ext
    axis, _, mask = _grid(28, True)
    a, m = torch.tensor(axis), torch.tensor(mask)
    for shape in ((0, 16, 3), (4, 0, 3), (0, 0, 3)):
        counts, clouds = _ext.occupancy_grid(torch.zeros(shape, device=gpu_device), a, m)
        assert counts.shape == clouds.shape == (28 ** 3,) and not counts.any() and not clouds.any()
    counts, clouds, cells = _ext.occupancy_grid(torch.zeros((0, 16, 3), device=gpu_device), a, m, return_cells=True)
    assert cells.shape == (0, 16)


def test_error_cases(gpu_device):
    import metrics_point_cloud.generation_metrics as G
    from slide_amd import _ext
    axis, _, mask = _grid(9, True)
    a, m = torch.tensor(axis), torch.tensor(mask)
    x = torch.rand(3, 16, 3, device=gpu_device) - 0.5
    with pytest.raises(RuntimeError):
        _ext.occupancy_grid(x.cpu(), a, m)  # CPU tensor
    with pytest.raises(RuntimeError):
        _ext.occupancy_grid(x.double(), a, m)  # wrong dtype
    with pytest.raises(RuntimeError):
        _ext.occupancy_grid(x[:, :, :2], a, m)  # wrong last dimension
    with pytest.raises(RuntimeError):
        _ext.occupancy_grid(x, a, m[:-1])  # a mask that is not R^3
    with pytest.raises(ValueError):
        _ext.occupancy_grid(x, torch.zeros(33), torch.ones(33 ** 3, dtype=torch.bool))  # R out of range
    with pytest.raises(ValueError):
        _ext.occupancy_grid(x, torch.zeros(1), torch.ones(1, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        G.entropy_of_occupancy_grid(x.cpu(), 9)
    with pytest.raises(ValueError):
        G.entropy_of_occupancy_grid(x[:, :, :2], 9)
    with pytest.raises(ValueError):
        G.entropy_of_occupancy_grid(x[0], 9)
    for R in (1, 33):
        with pytest.raises(ValueError):
            G.entropy_of_occupancy_grid(x, R)
        with pytest.raises(ValueError):
            G.jsd_between_point_cloud_sets(x, x, R)
    for bad in (float("nan"), float("inf"), -float("inf")):  # non-finite input: ValueError, whichever step the point would take
        y = x.clone()
        y[1, 5, 2] = bad
        with pytest.raises(ValueError, match="non-finite"):
            _ext.occupancy_grid(y, a, m)
        with pytest.raises(ValueError, match="non-finite"):
            G.entropy_of_occupancy_grid(y, 9, True)
    with pytest.raises(ValueError, match="admits no cell"):  # R = 2 clipped to the sphere: all eight corners are outside
        G.entropy_of_occupancy_grid(x, 2, True)
    assert _ext.occupancy_grid(x, a, m)[0].sum() == 48  # the device is fine afterwards


# ------------------------------------------------------------------ the CLI
def test_cli_jsd_flag_and_unchanged_default_output(gpu_device, tmp_path):
    """generation_evaluate.py in fresh child processes: with --jsd the JSON carries JSD, equal to the function's value on the same
    (normalised) sets; without it the saved file and the printed lines are, byte for byte, the six keys in the format recorded
    below (what the CLI printed and saved before the flag existed)"""
    import metrics_point_cloud.generation_metrics as G
    from load_evaluate import normalize_point_cloud
    rs = np.random.RandomState(8)
    a = (rs.standard_normal((14, 200, 3)) * rs.uniform(0.05, 0.2, (14, 1, 3))).astype(np.float32)
    b = (rs.standard_normal((10, 160, 3)) * rs.uniform(0.05, 0.2, (10, 1, 3)) + 0.05).astype(np.float32)
    pa, pb, pj = str(tmp_path / "a.npz"), str(tmp_path / "b.npz"), str(tmp_path / "m.json")
    np.savez(pa, points=a)
    np.savez(pb, points=b)
    cli = [sys.executable, os.path.join(REPO, "pointnet2", "generation_evaluate.py"), "--samples", pa, "--ref", pb, "--save", pj]

    def dev(v):
        return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(gpu_device)

    for extra, norm, res in ((["--jsd"], False, 28), (["--jsd", "--jsd_resolution", "9", "--normalize"], True, 9)):
        r = subprocess.run(cli + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        got = json.load(open(pj))
        assert list(got) == list(KEYS) + ["JSD"]
        sa, sb = (normalize_point_cloud(a), normalize_point_cloud(b)) if norm else (a, b)
        want = G.jsd_between_point_cloud_sets(dev(sa), dev(sb), res)
        assert got["JSD"] == want and 0.0 < want < 1.0
        assert ("%-16s %.9e" % ("JSD", want)) in r.stdout.split("\n")
        cd = G.compute_all_metrics(dev(sa), dev(sb))
        assert all(got[k] == float(cd[k]) for k in KEYS)
    r = subprocess.run(cli, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cd = {k: float(v) for k, v in G.compute_all_metrics(dev(a), dev(b)).items()}
    recorded_file = json.dumps({k: cd[k] for k in KEYS}, indent=1)
    assert open(pj).read() == recorded_file
    lines = r.stdout.split("\n")
    recorded_lines = ["14 samples x 10 references"] + ["%-16s %.9e" % (k, cd[k]) for k in KEYS]
    assert lines[:7] == recorded_lines and lines[7].startswith("wall time ") and lines[8:] == ["saved " + pj, ""]
    assert "JSD" not in r.stdout
