"""GPU: pointnet2/sampling_and_inference/mesh_reconstruction.py as a child process on three synthetic clouds, a temporary checkpoint of
synthetic weights and a reduced refine-and-upsample configuration (DPSR at 32^3, noise 0): every file it writes is byte-identical
between --batch_size 1 and --batch_size 3, shapes and keys are the documented ones, --largest_component is accepted and a
configuration that asks for the autoencoder branch is refused."""
import copy
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

pytestmark = pytest.mark.gpu

CLI = os.path.join(REPO, "pointnet2", "sampling_and_inference", "mesh_reconstruction.py")
N_SHAPES, N_POINTS, FACTOR = 3, 256, 5
VIS = "visualization_results_at_iteration_00000000_epoch_0000"


def _config():
    from slide_amd.configs import refine_and_upsample_config
    cfg = refine_and_upsample_config()
    cfg["pointnet_config"]["architecture"].update({"npoint": [128, 64, 32, 16], "nsample": [8, 8, 8, 8], "K": 4,
                                                   "feature_dim": [16, 32, 32, 64, 64], "decoder_feature_dim": [32, 32, 32, 64, 64]})
    cfg["dpsr_config"]["grid_res"] = 32
    cfg["shapenet_psr_dataset_config"]["augmentation"]["noise_magnitude"] = 0
    return cfg


def _clouds():
    """three ellipsoids with outward normals"""
    rs = np.random.RandomState(3)
    u = rs.standard_normal((N_SHAPES, N_POINTS, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    axes = np.array([[0.45, 0.3, 0.25], [0.3, 0.45, 0.35], [0.25, 0.35, 0.45]])[:, None, :]
    n = u / axes
    return (u * axes).astype(np.float32), (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from slide_amd.synth import synth_state_dict
    d = tmp_path_factory.mktemp("refine_cli")
    cfg = _config()
    with open(d / "config.json", "w") as f:
        json.dump(cfg, f)
    net = PointNet2CloudCondition(copy.deepcopy(cfg["pointnet_config"]))
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()])
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, d / "ckpt.pkl")
    p, n = _clouds()
    np.savez(d / "clouds.npz", points=p, normals=n, label=np.array([0, 4, 12], np.int64))
    return d


def _run(workdir, save, *extra, config="config.json"):
    cmd = [sys.executable, CLI, "-c", str(workdir / config), "--ckpt", str(workdir / "ckpt.pkl"), "--dataset_path",
           str(workdir / "clouds.npz"), "--save_dir", str(workdir / save), "--seed", "7"] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_cli_outputs_do_not_depend_on_the_batch_size(gpu_device, workdir):
    r1 = _run(workdir, "b1", "--batch_size", "1")
    assert r1.returncode == 0, r1.stderr[-3000:]
    r3 = _run(workdir, "b3", "--batch_size", "3")
    assert r3.returncode == 0, r3.stderr[-3000:]
    a, b = workdir / "b1" / "clouds" / VIS, workdir / "b3" / "clouds" / VIS
    names = _files(a)
    assert names == _files(b)
    assert names == sorted(["noisy_pcd.npz", "refined_pcd.npz", "points_sampled_from_mesh.npz", "uniform_points_sampled_from_mesh.npz"]
                           + [os.path.join("reconstructed_mesh", "reconstructed_mesh_%05d.ply" % i) for i in range(N_SHAPES)])
    for f in names:
        assert filecmp.cmp(a / f, b / f, shallow=False), "%s differs between --batch_size 1 and 3" % f
    for f in ("points_sampled_from_mesh.npz", "uniform_points_sampled_from_mesh.npz"):
        z = np.load(a / f)
        assert sorted(z.files) == ["label", "normals", "points"]
        assert z["points"].shape == (N_SHAPES, 2048, 3) and z["normals"].shape == (N_SHAPES, 2048, 3) and z["points"].dtype == np.float32
        assert np.array_equal(z["label"], [0, 4, 12]) and np.isfinite(z["points"]).all()
        # return_original_scale: the mesh's box is centred on the input cloud's and its longest edge is the input's longest edge, so
        # every sample lies within half that edge of the centre on every axis
        p, _ = _clouds()
        lo, hi = p.min(axis=1, keepdims=True), p.max(axis=1, keepdims=True)
        ctr, half = (hi + lo) / 2, (hi - lo).max(axis=2, keepdims=True) / 2
        assert np.all(np.abs(z["points"] - ctr) <= half + 1e-4)
    z = np.load(a / "noisy_pcd.npz")
    assert sorted(z.files) == ["normals", "points"] and z["points"].shape == (N_SHAPES, 2 * N_POINTS, 3)
    z = np.load(a / "refined_pcd.npz")
    assert sorted(z.files) == ["normals", "points"] and z["points"].shape == (N_SHAPES, 2 * N_POINTS * FACTOR, 3)
    assert z["points"].min() >= 0 and z["points"].max() <= np.float32(0.99)
    from slide_amd.mesh import load_ply
    v, f, n = load_ply(str(a / "reconstructed_mesh" / "reconstructed_mesh_00001.ply"))
    assert len(v) > 0 and len(f) > 0 and n is not None


def test_cli_largest_component_and_refusals(gpu_device, workdir):
    r = _run(workdir, "lc", "--batch_size", "3", "--largest_component")
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(_files(workdir / "lc" / "clouds" / VIS)) == 4 + N_SHAPES
    cfg = _config()
    cfg["autoencoder_config"] = {"config_file": "autoencoder.json"}
    with open(workdir / "config_ae.json", "w") as f:
        json.dump(cfg, f)
    r = _run(workdir, "ae", config="config_ae.json")
    assert r.returncode != 0 and "NotImplementedError" in r.stderr and "use_autoencoder" in r.stderr
    assert not os.path.exists(workdir / "ae")
