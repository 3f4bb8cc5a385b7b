"""pointnet2/load_evaluate.py (the reference's evaluation CLI, ported): flag parsing and normalize_point_cloud on the CPU against the
reference's formulas restated in numpy float64; on the GPU the CLI on two small npz files reproduces calc_cd pair by pair."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "pointnet2"))


def test_flags_and_the_type_bool_quirk():
    import load_evaluate as L
    a = L.build_parser().parse_args([])
    assert (a.dir1, a.dir2, a.threshold, a.device) == ('data/pointflow_1.npz', 'data/pointflow_2.npz', 0.0001, 'cuda:0')
    assert a.normalize is True and a.normalize_std_per_axis is True and a.normalize_per_shape is True and a.save is None
    # the reference's type=bool: any non-empty string is True, the empty string False
    a = L.build_parser().parse_args(['--normalize', 'False', '--normalize_per_shape', '', '--threshold', '0.01'])
    assert a.normalize is True and a.normalize_per_shape is False and a.threshold == 0.01
    assert "non-empty" in L.build_parser().format_help()


def test_normalize_point_cloud_matches_reference_formulas():
    import load_evaluate as L
    rs = np.random.RandomState(3)
    p = rs.standard_normal((4, 50, 3)) * np.array([1.0, 2.0, 0.5]) + 3.0
    B, N = p.shape[:2]
    want = {
        (True, True): (p - p.mean(1, keepdims=True)) / p.std(1, keepdims=True),
        (False, True): (p - p.mean(1, keepdims=True)) / p.reshape(B, -1).std(1).reshape(B, 1, 1),
        (True, False): (p - p.reshape(-1, 3).mean(0)) / p.reshape(-1, 3).std(0),
        (False, False): (p - p.reshape(-1, 3).mean(0)) / p.reshape(-1).std(),
    }
    for (per_axis, per_shape), w in want.items():
        got = L.normalize_point_cloud(p, per_axis, per_shape)
        assert np.allclose(got, w, rtol=1e-12, atol=1e-12), (per_axis, per_shape)
    box = L.normalize_point_cloud(p, True, False, box_per_shape=True)
    assert np.allclose(box.min(1), 0) and np.allclose(box.max(1), 1)
    m, s = np.float64(1.5), np.float64(2.0)
    assert np.array_equal(L.normalize_point_cloud(p, all_points_mean=m, all_points_std=s), (p - m) / s)


@pytest.mark.gpu
def test_cli_reproduces_calc_cd_per_pair(gpu_device, tmp_path):
    import torch
    import load_evaluate as L
    from metrics_point_cloud.chamfer_and_f1 import calc_cd
    rs = np.random.RandomState(8)
    a = rs.standard_normal((5, 300, 3)).astype(np.float32)
    b = (a + 0.05 * rs.standard_normal((5, 300, 3))).astype(np.float32)
    np.savez(tmp_path / "a.npz", points=a)
    np.savez(tmp_path / "b.npz", points=b)
    out = tmp_path / "m.npz"
    r = subprocess.run([sys.executable, os.path.join(REPO, "pointnet2", "load_evaluate.py"), "--dir1", str(tmp_path / "a.npz"),
                        "--dir2", str(tmp_path / "b.npz"), "--threshold", "0.01", "--batch", "2", "--save", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for k in ("cd_p", "cd_t", "f1"):
        assert ("%s: mean" % k) in r.stdout
    got = np.load(out)
    na, nb = L.normalize_point_cloud(a), L.normalize_point_cloud(b)
    with torch.no_grad():
        want = calc_cd(torch.from_numpy(na.astype(np.float32)).to(gpu_device), torch.from_numpy(nb.astype(np.float32)).to(gpu_device),
                       calc_f1=True, f1_threshold=0.01)
    for k in ("cd_p", "cd_t", "f1"):
        assert np.array_equal(got[k], want[k].cpu().numpy()), k
    assert got["f1"].min() > 0
