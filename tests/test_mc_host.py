"""CPU: the host side of the mesh path -- the PLY writer / reader of slide_amd/mesh.py, and the structure, scaling and file naming of
mc_from_psr / batch_mc_from_psr / save_mesh / export_mesh with the GPU call replaced by a hand-made mesh."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

VERTS = np.array([[0.25, 0, 0], [0, 0.5, 0], [0, 0, 0.75], [3, 3, 2.5]], dtype=np.float32)
FACES = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
NORMALS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.6, 0, -0.8]], dtype=np.float32)


def test_ply_round_trip(tmp_path):
    from slide_amd.mesh import load_ply, save_ply
    p = str(tmp_path / "m.ply")
    save_ply(p, VERTS, FACES, NORMALS)
    raw = open(p, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n")
    assert raw.startswith(header.encode("ascii"))
    assert len(raw) == len(header) + 4 * 6 * 4 + 2 * (1 + 3 * 4)
    body = raw[len(header):]
    assert np.array_equal(np.frombuffer(body[:24], "<f4"), np.concatenate([VERTS[0], NORMALS[0]]))
    assert body[96] == 3 and np.array_equal(np.frombuffer(body[97:109], "<i4"), FACES[0])
    v, f, n = load_ply(p)
    assert v.dtype == np.float32 and f.dtype == np.int32 and n.dtype == np.float32
    assert np.array_equal(v, VERTS) and np.array_equal(f, FACES) and np.array_equal(n, NORMALS)
    # without normals; tensors; int64 faces
    save_ply(p, torch.from_numpy(VERTS), torch.from_numpy(FACES).long())
    raw = open(p, "rb").read()
    assert b"nx" not in raw[:raw.index(b"end_header")] and len(raw) == raw.index(b"end_header\n") + 11 + 4 * 3 * 4 + 2 * 13
    v, f, n = load_ply(p)
    assert np.array_equal(v, VERTS) and np.array_equal(f, FACES) and n is None
    # an empty mesh
    save_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))
    v, f, n = load_ply(p)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    with pytest.raises(ValueError):
        save_ply(p, VERTS, FACES, NORMALS[:2])


@pytest.fixture
def fake_gpu(monkeypatch):
    """slide_amd.mesh.marching_cubes -> the hand-made mesh, once per grid (grid i's vertices shifted by i); records its calls"""
    from slide_amd import mesh
    calls = []

    def fake(psr_grid, level=0.0):
        calls.append((tuple(psr_grid.shape), level))
        return [(torch.from_numpy(VERTS + i), torch.from_numpy(FACES), torch.from_numpy(NORMALS)) for i in range(psr_grid.shape[0])]

    monkeypatch.setattr(mesh, "marching_cubes", fake)
    return calls


@pytest.mark.parametrize("B", [1, 2])
def test_mc_from_psr_structure_and_scaling(B, fake_gpu):
    from dpsr_utils.utils import mc_from_psr
    grid = torch.zeros(B, 8, 8, 8)
    v, f, n = mc_from_psr(grid)
    assert fake_gpu == [((B, 8, 8, 8), 0)]
    assert isinstance(v, list) and isinstance(f, list) and isinstance(n, list) and len(v) == len(f) == len(n) == B
    for i in range(B):
        assert isinstance(v[i], np.ndarray) and v[i].dtype == np.float32 and np.array_equal(v[i], (VERTS + i) / 8)
        assert f[i].dtype == np.int32 and np.array_equal(f[i], FACES) and np.array_equal(n[i], NORMALS)
    v, _, _ = mc_from_psr(grid, real_scale=True)
    assert all(np.array_equal(v[i], (VERTS + i) / 7) for i in range(B))
    v, f, n = mc_from_psr(grid, pytorchify=True)
    for i in range(B):
        assert all(isinstance(x[i], torch.Tensor) and x[i].dtype == torch.float32 for x in (v, f, n))
        assert np.array_equal(v[i].numpy(), (VERTS + i) / 8) and np.array_equal(f[i].numpy(), FACES.astype(np.float32))
        assert np.array_equal(n[i].numpy(), -NORMALS)
    # the reference honours zero_level for a batch of one only
    del fake_gpu[:]
    mc_from_psr(grid, zero_level=0.25)
    assert fake_gpu == [((B, 8, 8, 8), 0.25 if B == 1 else 0)]


def test_batch_mc_from_psr_files(tmp_path, fake_gpu):
    from dpsr_evaluation import batch_mc_from_psr, compute_center_and_max_length
    from slide_amd.mesh import load_ply
    grid = torch.zeros(2, 8, 8, 8)
    out = batch_mc_from_psr(grid, str(tmp_path), "shape", start_idx=7)
    assert out == ([], [], [], [])
    assert sorted(os.listdir(tmp_path)) == ["shape_00007.ply", "shape_00008.ply"]
    for i in range(2):
        v, f, n = load_ply(str(tmp_path / ("shape_%05d.ply" % (7 + i))))
        assert np.array_equal(v, (VERTS + i) / 8) and np.array_equal(f, FACES) and np.array_equal(n, NORMALS)
    batch_mc_from_psr(grid, str(tmp_path), "shape", batch_info=["chair", "table"])
    assert {"chair_00000.ply", "table_00001.ply"} <= set(os.listdir(tmp_path))
    # the original scale: the mesh's bounding box goes to the given centre and longest edge
    center = torch.tensor([[[1.0, 2.0, 3.0]], [[0.0, 0.0, 0.0]]])
    length = torch.tensor([[[2.0]], [[0.5]]])
    batch_mc_from_psr(grid, str(tmp_path), "orig", return_original_scale=True, original_center=center, original_max_length=length)
    for i in range(2):
        v, _, _ = load_ply(str(tmp_path / ("orig_%05d.ply" % i)))
        c, m = compute_center_and_max_length(torch.from_numpy(v)[None])
        assert torch.allclose(c, center[i:i + 1], atol=1e-6) and torch.allclose(m, length[i:i + 1], atol=1e-6)
        w = torch.from_numpy((VERTS + i) / 8)[None]
        wc, wm = compute_center_and_max_length(w)
        assert np.array_equal(v, ((w - wc) / wm * length[i:i + 1] + center[i:i + 1])[0].numpy())
    with pytest.raises(NotImplementedError):
        batch_mc_from_psr(grid, str(tmp_path), "x", sample_points_from_mesh=True)


def test_save_mesh_and_export_mesh(tmp_path):
    from dpsr_utils.io_utils import save_mesh
    from dpsr_utils.utils import export_mesh
    from slide_amd.mesh import load_ply
    p = str(tmp_path / "a.ply")
    save_mesh(p, torch.from_numpy(VERTS), FACES, normals=NORMALS)
    v, f, n = load_ply(p)
    assert np.array_equal(v, VERTS) and np.array_equal(f, FACES) and np.array_equal(n, NORMALS)
    save_mesh(p, VERTS, torch.from_numpy(FACES))
    assert load_ply(p)[2] is None
    export_mesh(p, torch.from_numpy(VERTS)[None], torch.from_numpy(FACES)[None])
    v, f, n = load_ply(p)
    assert np.array_equal(v, VERTS) and np.array_equal(f, FACES) and n is None
