"""GPU: marching cubes (slide_amd/csrc/marching_cubes.hip, slide_amd/mesh.py) against the float64 restatement of its definition in
tests/mc_cases.py and against scikit-image's meshes recorded in tests/golden/golden_mc.npz (tools/gen_golden_mc.py; the tests never
import skimage).  Every bound is derived in tests/mc_cases.py; every figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import mc_cases as C

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_mc.npz")


@pytest.fixture(scope="module")
def meshes(golden, gpu_device):
    """every fixture grid's mesh as numpy arrays (verts, faces, normals), each computed in a call of its own -- computed once"""
    from slide_amd.mesh import marching_cubes
    dev = gpu_device
    out = {}
    for name in golden["names"]:
        (v, f, n), = marching_cubes(torch.from_numpy(golden["grid_" + str(name)]).to(dev)[None])
        assert v.dtype == torch.float32 and n.dtype == torch.float32 and f.dtype == torch.int32
        assert v.dim() == 2 and v.size(1) == 3 and tuple(n.shape) == tuple(v.shape) and f.dim() == 2 and f.size(1) == 3
        out[str(name)] = (v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy())
    return out


def _mc(grid, dev, level=0.0):
    from slide_amd.mesh import marching_cubes
    return [tuple(x.cpu().numpy() for x in m) for m in marching_cubes(torch.from_numpy(np.ascontiguousarray(grid)).to(dev), level)]


def _check_vertices(what, grid, verts, level=0.0):
    """check 1: one vertex per sign-changing edge, each within the bound of the float64 crossing; -> the permutation onto crossings()"""
    r = grid.shape[0]
    x = C.crossings(grid, level)
    p = C.match_keys(C.vertex_keys(verts, r), x["keys"])
    err = np.abs(verts[p].astype(np.float64) - x["verts"]).max() if len(p) else 0.0
    print("%s: V %d, max |v - v64| %.3e, bound %.3e" % (what, len(p), err, C.vert_bound(r)))
    assert err <= C.vert_bound(r)
    return p, x


def _names(golden):
    return [str(n) for n in golden["names"]]


# ------------------------------------------------------------------------------------------------------------ 1. vertices
def test_vertices_are_the_sign_changing_edges(golden, meshes, gpu_device):
    strict = {str(s) for s in golden["strict"]}
    assert set(C.STRICT) <= strict
    for name in _names(golden):
        grid, (v, f, n) = golden["grid_" + name], meshes[name]
        r = grid.shape[0]
        p, x = _check_vertices(name, grid, v)
        # the bound tells the definition from the nearest wrong arithmetics on this grid
        for wrong in C.WRONG_T:
            off = np.abs(C.crossings(grid, wrong=wrong)["verts"] - x["verts"]).max()
            assert off > 100 * C.vert_bound(r), (name, wrong)
        if name in strict:
            sk = golden["sk_verts_" + name]
            q = C.match_keys(C.vertex_keys(sk, r), x["keys"])
            err = np.abs(v[p].astype(np.float64) - sk[q].astype(np.float64)).max()
            print("%s: max |v - skimage| %.3e, bound %.3e" % (name, err, C.skimage_vert_bound(r)))
            assert err <= C.skimage_vert_bound(r)


# ------------------------------------------------------------------------------------------------------------ 2. normals
def test_normals(golden, meshes, gpu_device):
    strict = {str(s) for s in golden["strict"]}
    for name in _names(golden):
        grid, (v, f, n) = golden["grid_" + name], meshes[name]
        r = grid.shape[0]
        x = C.crossings(grid)
        p = C.match_keys(C.vertex_keys(v, r), x["keys"])
        bound = C.normal_bound(x["M"], x["glen"])
        err = np.abs(n[p].astype(np.float64) - x["normals"]).max(axis=1)
        print("%s: max |n - n64| %.3e, max err / bound %.3f, finite bounds %d of %d" % (
            name, err.max(), (err / bound).max(), int(np.isfinite(bound).sum()), len(bound)))
        assert np.isfinite(bound).all() and (err <= bound).all()
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 6.01 * C.U  # (the normalisation's share of the bound)
        if name in strict:
            sk_n, sk_v = golden["sk_normals_" + name], golden["sk_verts_" + name]
            q = C.match_keys(C.vertex_keys(sk_v, r), x["keys"])
            dot = (n[p].astype(np.float64) * sk_n[q]).sum(1)
            print("%s: normal . skimage's normal: min %.3f, mean %.4f" % (name, dot.min(), dot.mean()))
            assert (dot > 0).all()


def test_exact_normals_and_the_zero_gradient(gpu_device):
    """grids whose gradients are exactly representable: the normals are then exact, and a vanishing gradient gives (0, 0, 0)"""
    # 2^3, -1 | +1 along k: every difference is one-sided, g = (0, 0, 2) everywhere, t = 0.5
    g = np.zeros((2, 2, 2), np.float32)
    g[..., 0], g[..., 1] = -1, 1
    (v, f, n), = _mc(g[None], gpu_device)
    assert len(v) == 4 and np.array_equal(n, np.tile(np.float32([0, 0, -1]), (4, 1))) and np.array_equal(v[:, 2], np.full(4, 0.5, np.float32))
    # 3^3, -1, +1, -1 along k: g_k = 2, 0, -2 (one-sided, central, one-sided); at t = 0.5 the two sheets get (0, 0, -1) and (0, 0, 1)
    h = np.zeros((3, 3, 3), np.float32)
    h[..., 0], h[..., 1], h[..., 2] = -1, 1, -1
    (v, f, n), = _mc(h[None], gpu_device)
    x = C.crossings(h)
    p = C.match_keys(C.vertex_keys(v, 3), x["keys"])
    assert np.array_equal(n[p].astype(np.float64), x["normals"]) and set(n[:, 2].tolist()) == {-1.0, 1.0}
    # 4^3, +1, -1, +1, -1 along k: the central differences at k = 1 and 2 vanish, so the 16 vertices between them have no direction
    c = np.zeros((4, 4, 4), np.float32)
    c[..., 0], c[..., 1], c[..., 2], c[..., 3] = 1, -1, 1, -1
    (v, f, n), = _mc(c[None], gpu_device)
    mid = C.vertex_keys(v, 4)[:, 2] == 1
    assert mid.sum() == 16 and np.array_equal(n[mid], np.zeros((16, 3), np.float32)) and np.isfinite(n).all()


# ------------------------------------------------------------------------------------------------------------ 3. faces, self-consistency
def test_faces_are_consistent(golden, meshes, gpu_device):
    for name in _names(golden):
        grid, (v, f, n) = golden["grid_" + name], meshes[name]
        C.check_faces(v, f, grid)
        print("%s: V %d F %d, ambiguous faces %d" % (name, len(v), len(f), C.ambiguous_faces(grid)))
    assert C.ambiguous_faces(golden["grid_noise"]) == 171


# ------------------------------------------------------------------------------------------------------------ 4. faces against the reference
def test_faces_against_skimage(golden, meshes, gpu_device):
    for name in (str(s) for s in golden["strict"]):
        grid, (v, f, n) = golden["grid_" + name], meshes[name]
        sk_v, sk_f = golden["sk_verts_" + name], golden["sk_faces_" + name]
        got = (len(f), C.euler(len(v), f), C.components(len(v), f))
        want = (len(sk_f), C.euler(len(sk_v), sk_f), C.components(len(sk_v), sk_f))
        o = C.orientation(v, f, grid)
        print("%s: (F, Euler, components) %s, skimage %s; min n . d %.3e" % (name, got, want, o.min()))
        assert got == want
        assert (o > 0).all()
        assert (C.orientation(sk_v, sk_f, grid) > 0).all()  # (the rule is the reference's own orientation)


# ------------------------------------------------------------------------------------------------------------ 5. batching
def test_a_mesh_does_not_depend_on_its_batch(golden, meshes, gpu_device):
    a, b = golden["grid_sphere"], golden["grid_torus"]
    for order in ((a, b), (b, a)):
        names = ("sphere", "torus") if order[0] is a else ("torus", "sphere")
        for _ in range(2):
            got = _mc(np.stack(order), gpu_device)
            assert len(got) == 2
            for name, m in zip(names, got):
                assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(m, meshes[name])), name
    # and whatever the chunking of the workspace
    from slide_amd import _ext
    t = torch.from_numpy(np.stack([a, b, a])).to(gpu_device)
    for chunk in (1, 2):
        got = _ext.marching_cubes(t, 0.0, chunk=chunk)
        for name, m in zip(("sphere", "torus", "sphere"), got):
            assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(m, meshes[name])), (chunk, name)


# ------------------------------------------------------------------------------------------------------------ 6. edges of the domain
def test_no_crossing_gives_an_empty_mesh(gpu_device):
    for grid in (np.ones((1, 16, 16, 16), np.float32), -np.ones((2, 5, 5, 5), np.float32), np.full((1, 4, 4, 4), np.nan, np.float32)):
        for v, f, n in _mc(grid, gpu_device):
            assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    from slide_amd.mesh import marching_cubes
    assert marching_cubes(torch.zeros((0, 8, 8, 8), device=gpu_device)) == []
    # an empty grid beside a full one
    s = load_golden("golden_mc.npz")["grid_sphere"]
    got = _mc(np.stack([np.ones_like(s), s, np.ones_like(s)]), gpu_device)
    assert [len(m[0]) for m in got] == [0, 522, 0] and [len(m[1]) for m in got] == [0, 1040, 0]


def test_a_single_cell(gpu_device):
    g = np.ones((2, 2, 2), np.float32)
    g[0, 0, 0] = -1
    (v, f, n), = _mc(g[None], gpu_device)
    assert v.shape == (3, 3) and f.shape == (1, 3)
    assert sorted(map(tuple, v.tolist())) == [(0.0, 0.0, 0.5), (0.0, 0.5, 0.0), (0.5, 0.0, 0.0)]
    assert (C.orientation(v, f, g) > 0).all()
    C.check_faces(v, f, g)
    # NaN is outside; the level moves the crossing
    g[1, 1, 1] = np.nan
    (v, f, n), = _mc(g[None], gpu_device, level=0.5)
    assert sorted(map(tuple, v.tolist())) == [(0.0, 0.0, 0.75), (0.0, 0.75, 0.0), (0.75, 0.0, 0.0)] and f.shape == (1, 3)


def test_a_size_that_is_no_power_of_two(golden, gpu_device):
    g = np.ascontiguousarray(golden["grid_sphere"][:13, :13, :13])
    (v, f, n), = _mc(g[None], gpu_device)
    _check_vertices("sphere cropped to 13^3", g, v)
    C.check_faces(v, f, g)


def test_many_bricks(gpu_device):
    """r = 64: 512 bricks per grid -- the per-grid scan and offsets beyond one workgroup; the second grid of the batch has its rows
    behind the first's"""
    g = C.sphere_grid(64)
    got = _mc(np.stack([g, g]), gpu_device)
    v, f, n = got[0]
    _check_vertices("sphere 64^3", g, v)
    C.check_faces(v, f, g)
    assert all(np.array_equal(x, y) for x, y in zip(got[0], got[1]))


def test_bad_arguments(gpu_device):
    from slide_amd.mesh import marching_cubes
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros((1, 8, 8, 4), device=gpu_device))
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros((1, 1, 1, 1), device=gpu_device))
    with pytest.raises(RuntimeError):
        marching_cubes(torch.zeros((1, 8, 8, 8)))
    with pytest.raises(RuntimeError):
        marching_cubes(torch.zeros((8, 8, 8), device=gpu_device))


# ------------------------------------------------------------------------------------------------------------ 7. mc_from_psr, CLI
@pytest.mark.parametrize("B", [1, 2])
def test_mc_from_psr(B, golden, meshes, gpu_device):
    from dpsr_utils.utils import mc_from_psr
    names = ("psr0", "psr1")[:B]
    grid = torch.from_numpy(np.stack([golden["grid_" + n] for n in names])).to(gpu_device)
    v, f, n = mc_from_psr(grid)
    assert all(isinstance(x, list) and len(x) == B for x in (v, f, n))
    for i, name in enumerate(names):
        mv, mf, mn = meshes[name]
        assert isinstance(v[i], np.ndarray) and np.array_equal(v[i], mv / 16) and v[i].dtype == np.float32
        assert np.array_equal(f[i], mf) and np.array_equal(n[i], mn)
    v1, _, _ = mc_from_psr(grid, real_scale=True)
    assert all(np.array_equal(v1[i], meshes[name][0] / 15) for i, name in enumerate(names))
    tv, tf, tn = mc_from_psr(grid, pytorchify=True)
    for i, name in enumerate(names):
        assert tv[i].device.type == "cuda" and tf[i].dtype == torch.float32
        assert np.array_equal(tv[i].cpu().numpy(), meshes[name][0] / 16) and np.array_equal(tn[i].cpu().numpy(), -meshes[name][2])
        assert np.array_equal(tf[i].cpu().numpy(), meshes[name][1].astype(np.float32))


def test_psr_grid_cli_writes_meshes(tmp_path, gpu_device):
    import dpsr_cases as D
    from slide_amd.mesh import load_ply, marching_cubes
    V, N = D.sphere_cloud(7, 3, 300)
    pts = ((V - 0.5) * 1.7).astype(np.float32)
    src, dst, mdir = str(tmp_path / "clouds.npz"), str(tmp_path / "out" / "grid.npz"), str(tmp_path / "meshes")
    np.savez(src, points=np.concatenate([pts, N], axis=2))
    cli = [sys.executable, os.path.join(REPO, "pointnet2", "sampling_and_inference", "psr_grid.py"), "--points", src,
           "--split_points_to_normals", "--explicit_normalize", "--grid_res", "16", "--psr_sigma", "2", "--batch_size", "2", "--save", dst,
           "--save_mesh_dir", mdir, "--mesh_prefix", "shape"]
    r = subprocess.run(cli, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.load(dst)
    assert sorted(out.files) == ["normals", "points", "psr_grid"]
    assert sorted(os.listdir(mdir)) == ["shape_%05d.ply" % i for i in range(3)]
    want = marching_cubes(torch.from_numpy(out["psr_grid"]).to(gpu_device))
    for i, (v, f, n) in enumerate(want):
        lv, lf, ln = load_ply(os.path.join(mdir, "shape_%05d.ply" % i))
        assert len(lv) > 0 and len(lf) > 0
        assert np.array_equal(lv, v.cpu().numpy() / 16) and np.array_equal(lf, f.cpu().numpy()) and np.array_equal(ln, n.cpu().numpy())
