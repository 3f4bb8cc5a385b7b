"""GPU: area-weighted point samples from triangle meshes (slide_amd/csrc/mesh_sample.hip, slide_amd/mesh.py) against the restatement
of the definition in tests/mesh_sample_cases.py: float32 areas bit for bit, the integer cdf and the selected faces exactly, points
and normals within the bounds derived there.  Every figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import mesh_sample_cases as C

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

pytestmark = pytest.mark.gpu

S_LIST = (1, 63, 64, 65, 2048)


def _dev(mesh, dev, normals=None):
    v, f = mesh
    out = (torch.from_numpy(np.ascontiguousarray(v)).to(dev), torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).to(dev))
    return out + (torch.from_numpy(normals).to(dev),) if normals is not None else out


def _unit_normals(n, seed):
    g = np.random.RandomState(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def _sample(meshes, S, **kw):
    from slide_amd.mesh import sample_points_from_meshes
    out = sample_points_from_meshes(meshes, S, return_normals=True, return_face_idx=True, **kw)
    return [t.cpu().numpy() for t in out]


def _check_mesh(what, got_p, got_n, got_f, ref, mode):
    """one mesh's samples against the restatement `ref` (mesh_sample_cases.sample)"""
    assert np.array_equal(got_f, ref["face"]), "%s: %d of %d faces differ" % (what, int((got_f != ref["face"]).sum()), len(got_f))
    if not ref["valid"]:
        assert not got_p.any() and not got_n.any() and (got_f == -1).all(), what
        return
    perr = np.abs(got_p.astype(np.float64) - ref["points"]).max(axis=1)
    pb = C.point_bound(ref["M"])
    if mode == "face":
        nb = C.face_normal_bound(ref["e1e2"], ref["nlen"])
        want = ref["normals_face"]
    else:
        nb = C.vertex_normal_bound(ref["G"], ref["glen"])
        want = ref["normals_vertex"]
    nerr = np.abs(got_n.astype(np.float64) - want).max(axis=1)
    fin = np.isfinite(nb)
    print("%s (%s normals): S %d, max point error / bound %.3f, max normal error / bound %.3f, %d normals undetermined"
          % (what, mode, len(got_f), (perr / pb).max(), (nerr[fin] / nb[fin]).max() if fin.any() else 0.0, int((~fin).sum())))
    assert (perr <= pb).all() and (nerr[fin] <= nb[fin]).all() and fin.mean() > 0.99


# ------------------------------------------------------------------------------------------------------------ 1. areas and cdf
def test_areas_and_cdf(gpu_device):
    """hand-made meshes packed into ONE call: areas bit-equal to the float32 restatement and within the bound of float64, the cdf
    equal to the integer restatement.  Face counts one below, at and one above the spans of the scan (a wave's and a workgroup
    pass's, read from the library) and one mesh of more than two passes"""
    from slide_amd import _ext
    wave, tile = _ext.mesh_cdf_span(1), _ext.mesh_cdf_span(2)
    assert _ext.mesh_cdf_span(0) * 64 == wave and wave < tile
    cases = [("single", C.single_face()), ("ratio", C.ratio_mesh()), ("empty", C.empty_mesh())]
    for k, nf in enumerate(dict.fromkeys((255, 256, 257, wave - 1, wave, wave + 1, tile - 1, tile, tile + 1, 2 * tile + 3))):
        cases.append(("random%d" % nf, C.random_mesh(nf, seed=10 + k, degenerate_every=7 if k % 2 else 0)))
    cases.append(("degenerate", C.degenerate_mesh()))
    voff = np.cumsum([0] + [len(m[0]) for _, m in cases]).tolist()
    foff = np.cumsum([0] + [len(m[1]) for _, m in cases]).tolist()
    verts = torch.from_numpy(np.concatenate([m[0] for _, m in cases])).to(gpu_device)
    faces = torch.from_numpy(np.concatenate([m[1] for _, m in cases])).to(gpu_device)
    areas, cdf, _, _ = _ext.mesh_face_cdf(verts, faces, voff, foff)
    areas, cdf = areas.cpu().numpy(), cdf.cpu().numpy()
    for k, (name, (v, f)) in enumerate(cases):
        a, c = areas[foff[k]:foff[k + 1]], cdf[foff[k]:foff[k + 1]]
        want = C.areas32(v, f)
        a64, e1e2 = C.areas64(v, f)
        err = np.abs(a.astype(np.float64) - a64)
        want_cdf, total = C.cdf_of(C.quantise(want))
        print("%s: F %d, areas bit-equal %s, max area error / (e |e1| |e2|) %.3f (bound %.2f), total %d, cdf equal %s"
              % (name, len(f), np.array_equal(a.view(np.uint32), want.view(np.uint32)),
                 (err[e1e2 > 0] / (C.E * e1e2[e1e2 > 0])).max() if (e1e2 > 0).any() else 0.0, C.AREA_C, total,
                 c.tolist() == want_cdf))
        assert np.array_equal(a.view(np.uint32), want.view(np.uint32)) and (err <= C.area_bound(e1e2)).all()
        assert c.tolist() == want_cdf


# ------------------------------------------------------------------------------------------------------------ 2. selection and points
@pytest.fixture(scope="module")
def batches():
    """three batches of three: an empty mesh in the middle, an all-degenerate mesh, live meshes on either side"""
    r257, ratio, mixed = C.random_mesh(257, seed=21), C.ratio_mesh(), C.random_mesh(64, 40, seed=2, degenerate_every=3)
    out = []
    for trio in ((r257, C.empty_mesh(), C.degenerate_mesh()), (C.degenerate_mesh(), C.empty_mesh(), ratio), (ratio, C.empty_mesh(), mixed)):
        out.append([(m, _unit_normals(len(m[0]), 40 + k)) for k, m in enumerate(trio)])
    return out


@pytest.mark.parametrize("S", S_LIST)
def test_selection_points_and_normals_with_philox(S, batches, gpu_device):
    for bi, batch in enumerate(batches):
        meshes = [_dev(m, gpu_device, g) for m, g in batch]
        for mode in ("face", "vertex"):
            p, n, fi = _sample(meshes, S, seed=1234 + (5 << 32), stream_id=3, normals=mode)
            assert p.shape == (3, S, 3) and n.shape == (3, S, 3) and fi.shape == (3, S) and p.dtype == np.float32 and fi.dtype == np.int32
            for k, (m, g) in enumerate(batch):
                ref = C.sample(m[0], m[1], S, seed=1234 + (5 << 32), mesh_id=k, stream_id=3, vnormals=g)
                _check_mesh("batch %d mesh %d" % (bi, k), p[k], n[k], fi[k], ref, mode)
    # valid: 0 for the empty and the degenerate mesh
    from slide_amd import _ext
    from slide_amd.mesh import pack_meshes
    v, f, _, voff, foff = pack_meshes([_dev(m, gpu_device) for m, _ in batches[0]])
    _, cdf, vo, fo = _ext.mesh_face_cdf(v, f, voff, foff)
    assert _ext.mesh_sample(v, f, vo, fo, cdf, S)[3].tolist() == [1, 0, 0]


# ------------------------------------------------------------------------------------------------------------ 3. explicit words
def _r_for(t, total):
    r = -((-t << 64) // total)  # the smallest r with mulhi64(r, total) = t
    assert (r * total) >> 64 == t and 0 <= r < 2 ** 64
    return r


def test_explicit_words_on_the_cdf_boundaries(gpu_device):
    """draws placed at r = 0, r = 2^64 - 1 and at t = cdf_f - 1, cdf_f (also across runs of zero-area faces), with u, v words of 0 and
    0xFFFFFFFF: the selection is exact, the points stay inside the triangle.  For the ratio mesh's right triangles the barycentric
    coordinates of a point p are (p - v0).e_i / |e_i|^2, each within sqrt(3) point_bound / |e_i| of the exact weight, plus 4e-7 for the
    angle between the float32 legs"""
    ends = (0, 0xFFFFFFFF)
    for name, (v, f) in (("ratio", C.ratio_mesh()), ("mixed", C.random_mesh(64, 40, seed=2, degenerate_every=3))):
        cdf, total = C.cdf_of(C.quantise(C.areas32(v, f)))
        rs = [0, 2 ** 64 - 1]
        for k in range(len(cdf)):
            rs += [_r_for(t, total) for t in (cdf[k] - 1, cdf[k]) if 0 <= t < total]
        words = np.array([[r >> 32, r & 0xFFFFFFFF, ends[i & 1], ends[(i >> 1) & 1]] for i, r in enumerate(rs)]
                         + [[0x12345678, 0x9ABCDEF0, a, b] for a in ends for b in ends], dtype=np.int64)
        p, n, fi = _sample([_dev((v, f), gpu_device)], len(words), words=torch.from_numpy(words)[None])
        ref = C.sample(v, f, len(words), words=words)
        lower = C.select(words.astype(np.uint64), cdf, total, wrong="lower_bound")
        print("%s: %d draws, faces %s ..., %d differ from the lower bound" % (name, len(words), fi[0][:12].tolist(), int((lower != ref["face"]).sum())))
        assert (lower != ref["face"]).sum() >= len(cdf) // 2  # (the draws do tell the two searches apart)
        _check_mesh(name, p[0], n[0], fi[0], ref, "face")
        q = C.quantise(C.areas32(v, f))
        assert all(q[k] > 0 for k in fi[0])
        # the float32 weights themselves
        u, w = C.uniforms(words.astype(np.uint64))
        su = np.sqrt(u)
        w32 = np.stack([np.float32(1) - su, su * (np.float32(1) - w), su * w])
        assert (w32 >= 0).all() and u.max() == 1.0 and u.min() > 0
        if name == "ratio":
            tri = v.astype(np.float64)[f[fi[0]]]
            e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
            d = p[0].astype(np.float64) - tri[:, 0]
            b1, b2 = (d * e1).sum(1) / (e1 * e1).sum(1), (d * e2).sum(1) / (e2 * e2).sum(1)
            tol = np.sqrt(3.0) * C.point_bound(ref["M"]) / np.minimum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)) + 4e-7
            print("ratio: min barycentric coordinates %.3e %.3e %.3e, tolerance %.3e" % (b1.min(), b2.min(), (1 - b1 - b2).min(), tol.max()))
            assert (b1 >= -tol).all() and (b2 >= -tol).all() and (1 - b1 - b2 >= -2 * tol).all()


# ------------------------------------------------------------------------------------------------------------ 4. independence
def test_a_mesh_draws_the_same_anywhere(gpu_device):
    x = _dev(C.random_mesh(257, seed=21), gpu_device, _unit_normals(300, 1))
    a = _dev(C.ratio_mesh(), gpu_device, _unit_normals(27, 2))
    b = _dev(C.single_face(), gpu_device, _unit_normals(3, 3))
    S = 300
    alone = _sample([x], S, seed=9, mesh_ids=[5], stream_id=2)
    again = _sample([x], S, seed=9, mesh_ids=[5], stream_id=2)
    assert all(np.array_equal(p, q) for p, q in zip(alone, again))
    for batch, ids, pos in (([a, x, b], [0, 5, 9], 1), ([x, a], [5, 1], 0), ([b, a, a, x], [7, 8, 9, 5], 3)):
        for mode in ("face", "vertex"):
            got = _sample(batch, S, seed=9, mesh_ids=ids, stream_id=2, normals=mode)
            want = _sample([x], S, seed=9, mesh_ids=[5], stream_id=2, normals=mode)
            assert all(np.array_equal(g[pos], w[0]) for g, w in zip(got, want)), (ids, mode)
    # the default id is the position
    assert np.array_equal(_sample([a, x], S, seed=9, stream_id=2)[2][1], _sample([x], S, seed=9, mesh_ids=[1], stream_id=2)[2][0])
    for kw in (dict(seed=10, mesh_ids=[5], stream_id=2), dict(seed=9 + (1 << 32), mesh_ids=[5], stream_id=2),
               dict(seed=9, mesh_ids=[5], stream_id=3), dict(seed=9, mesh_ids=[6], stream_id=2)):
        other = _sample([x], S, **kw)
        same = float((other[2] == alone[2]).mean())
        print("%s: %.3f of the faces coincide" % (kw, same))
        assert same < 0.1 and not np.array_equal(other[0], alone[0])


# ------------------------------------------------------------------------------------------------------------ 5. from marching cubes
def test_samples_of_marching_cubes_meshes(gpu_device):
    """sphere and torus of the marching-cubes fixture -> meshes -> 2048 samples: every sample lies on its face (the restatement's
    bound), and the unit face normal has ONE sign of dot product with the interpolated vertex normal over all samples.  That sign is
    NEGATIVE: marching_cubes winds its faces so that (v1 - v0) x (v2 - v0) points toward increasing phi, and its vertex normals point
    down the gradient (skimage's convention).  The sphere's samples fall into the octants around its centre evenly, 4 sigma."""
    from slide_amd.mesh import marching_cubes
    g = load_golden("golden_mc.npz")
    grids = torch.from_numpy(np.stack([g["grid_sphere"], g["grid_torus"]])).to(gpu_device)
    meshes = marching_cubes(grids)
    S = 2048
    pf, nf, fi = _sample(meshes, S, seed=3)
    pv, nv, fv = _sample(meshes, S, seed=3, normals="vertex")
    assert np.array_equal(pf, pv) and np.array_equal(fi, fv)
    for k, name in enumerate(("sphere", "torus")):
        v, f, n = (t.cpu().numpy() for t in meshes[k])
        ref = C.sample(v, f, S, seed=3, mesh_id=k, vnormals=n)
        _check_mesh(name, pf[k], nf[k], fi[k], ref, "face")
        _check_mesh(name, pv[k], nv[k], fv[k], ref, "vertex")
        dots = (nf[k].astype(np.float64) * nv[k]).sum(axis=1)
        print("%s: face normal . vertex normal in [%.4f, %.4f]" % (name, dots.min(), dots.max()))
        assert (dots < 0).all() or (dots > 0).all()
        assert dots.max() < 0
    centre = np.array([7.63, 7.63 + 0.21, 7.63 - 0.37])  # (mc_cases._coords)
    octant = ((pf[0] > centre) * np.array([4, 2, 1])).sum(axis=1)
    frac = np.bincount(octant, minlength=8) / S
    sigma = np.sqrt(0.125 * 0.875 / S)
    print("sphere: octant fractions %s, 1/8 +- 4 sigma = %.4f" % (np.round(frac, 4).tolist(), 4 * sigma))
    assert (np.abs(frac - 0.125) < 4 * sigma).all()


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(gpu_device):
    from slide_amd.mesh import sample_points_from_meshes
    v, f = C.random_mesh(100, 50, seed=5)
    good = _dev((v, f), gpu_device)
    bad_f = f.copy()
    bad_f[37, 1] = len(v)  # one past the mesh's last vertex: tested before it is used
    with pytest.raises(ValueError, match="index"):
        sample_points_from_meshes([good, _dev((v, bad_f), gpu_device)], 16)
    neg_f = f.copy()
    neg_f[3, 0] = -1
    with pytest.raises(ValueError, match="index"):
        sample_points_from_meshes([_dev((v, neg_f), gpu_device)], 16)
    # an index that is in range of the PACKED array but not of its own mesh
    with pytest.raises(ValueError, match="index"):
        sample_points_from_meshes([_dev((v[:40], np.minimum(f, 45)), gpu_device), good], 16)
    nan_v = v.copy()
    nan_v[f[11, 2], 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        sample_points_from_meshes([_dev((nan_v, f), gpu_device)], 16)
    nan_v = v.copy()
    unused = sorted(set(range(len(v))) - set(f.ravel().tolist()))
    if unused:  # a non-finite vertex no face refers to is nobody's business
        nan_v[unused[0]] = np.inf
        sample_points_from_meshes([_dev((nan_v, f), gpu_device)], 16)
    with pytest.raises(ValueError, match="vertex"):
        sample_points_from_meshes([good], 16, return_normals=True, normals="vertex")
    with pytest.raises(ValueError):
        sample_points_from_meshes([good], 16, normals="smooth")
    with pytest.raises(RuntimeError):
        sample_points_from_meshes([(torch.from_numpy(v), torch.from_numpy(f))], 16)
    vg = good[0].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        sample_points_from_meshes([(vg, good[1])], 16)
    with torch.no_grad():
        assert sample_points_from_meshes([(vg, good[1])], 16).shape == (1, 16, 3)
    # the device still answers
    assert sample_points_from_meshes([good], 0).shape == (1, 0, 3)
    assert torch.isfinite(sample_points_from_meshes([good], 16)).all()


# ------------------------------------------------------------------------------------------------------------ 7. batch_mc_from_psr
def test_batch_mc_from_psr_samples_points(gpu_device, tmp_path):
    import mc_cases
    from dpsr_evaluation import batch_mc_from_psr
    from slide_amd.mesh import load_ply, sample_points_from_meshes
    grids = torch.from_numpy(np.stack([mc_cases.sphere_grid(16, fr) for fr in (0.33, 0.25, 0.4)])).to(gpu_device)
    d = tmp_path / "all"
    d.mkdir()
    out = batch_mc_from_psr(grids, str(d), "s", start_idx=4, sample_points_from_mesh=True, seed=11, num_samples=256, num_dense=1024)
    assert len(out) == 4 and all(isinstance(a, np.ndarray) and a.shape == (3, 256, 3) and a.dtype == np.float32 for a in out)
    assert sorted(os.listdir(d)) == ["s_%05d.ply" % k for k in (4, 5, 6)]
    pts, nrm, upts, unrm = out
    assert np.allclose(np.linalg.norm(nrm, axis=2), 1, atol=1e-5) and np.allclose(np.linalg.norm(unrm, axis=2), 1, atol=1e-5)
    meshes = []
    for k in (4, 5, 6):
        v, f, n = load_ply(str(d / ("s_%05d.ply" % k)))
        meshes.append((torch.from_numpy(v).to(gpu_device), torch.from_numpy(f).to(gpu_device), torch.from_numpy(n).to(gpu_device)))
    plain, plain_n = sample_points_from_meshes(meshes, 256, return_normals=True, seed=11, mesh_ids=[4, 5, 6], stream_id=0)
    assert np.array_equal(plain.cpu().numpy(), pts) and np.array_equal(plain_n.cpu().numpy(), nrm)
    dense, dense_n = (t.cpu().numpy() for t in sample_points_from_meshes(meshes, 1024, return_normals=True, seed=11, mesh_ids=[4, 5, 6], stream_id=1))

    def min_dist(x):
        dd = np.linalg.norm(x[:, None] - x[None], axis=2)
        return dd[np.triu_indices(len(x), 1)].min()

    for k in range(3):
        rows = {r.tobytes(): i for i, r in enumerate(dense[k])}
        idx = [rows.get(r.tobytes()) for r in upts[k]]
        assert None not in idx and len(set(idx)) == 256 and idx[0] == 0
        assert np.array_equal(dense_n[k][idx], unrm[k])
        du, dp = min_dist(upts[k].astype(np.float64)), min_dist(pts[k].astype(np.float64))
        print("shape %d: minimum pairwise distance %.4f uniform, %.4f plain" % (k, du, dp))
        assert du > dp
    # another split of the same grids
    d2 = tmp_path / "split"
    d2.mkdir()
    a = batch_mc_from_psr(grids[:1], str(d2), "s", start_idx=4, sample_points_from_mesh=True, seed=11, num_samples=256, num_dense=1024)
    b = batch_mc_from_psr(grids[1:], str(d2), "s", start_idx=5, sample_points_from_mesh=True, seed=11, num_samples=256, num_dense=1024)
    for k in range(4):
        assert np.array_equal(np.concatenate([a[k], b[k]]), out[k]), k
    # without the flag: the four empty lists, as before
    assert batch_mc_from_psr(grids[:1], str(d2), "t") == ([], [], [], [])


# ------------------------------------------------------------------------------------------------------------ 8. the CLI
def test_psr_grid_cli_samples_points(gpu_device, tmp_path):
    rs = np.random.RandomState(0)
    u = rs.standard_normal((2, 600, 3)).astype(np.float32)
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    np.savez(tmp_path / "in.npz", points=(u * np.array([0.5, 0.4], np.float32)[:, None, None]), normals=u)
    cli = os.path.join(REPO, "pointnet2", "sampling_and_inference", "psr_grid.py")
    got = []
    for bs in (1, 2):
        d = tmp_path / ("bs%d" % bs)
        r = subprocess.run([sys.executable, cli, "--points", str(tmp_path / "in.npz"), "--grid_res", "32", "--batch_size", str(bs),
                            "--save", str(d / "grid.npz"), "--save_mesh_dir", str(d), "--sample_points_from_mesh", "--sample_seed", "5"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        files = []
        for name in ("points_sampled_from_mesh.npz", "uniform_points_sampled_from_mesh.npz"):
            z = np.load(d / name)
            assert sorted(z.files) == ["normals", "points"] and z["points"].shape == (2, 2048, 3) and z["normals"].shape == (2, 2048, 3)
            assert np.isfinite(z["points"]).all() and z["points"].any()
            files.append((z["points"], z["normals"]))
        assert {"mesh_00000.ply", "mesh_00001.ply"} <= set(os.listdir(d))
        got.append(files)
    for (p1, n1), (p2, n2) in zip(*got):
        assert np.array_equal(p1, p2) and np.array_equal(n1, n2)
    r = subprocess.run([sys.executable, cli, "--points", str(tmp_path / "in.npz"), "--save", str(tmp_path / "g.npz"), "--sample_points_from_mesh"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--save_mesh_dir" in r.stderr
