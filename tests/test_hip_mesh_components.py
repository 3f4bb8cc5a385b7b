"""GPU: connected components and the keep-largest filter of triangle meshes (slide_amd/csrc/mesh_components.hip, slide_amd/mesh.py)
against the numpy restatement of the definition in tests/mesh_cc_cases.py (a union-find on the host): labels, counts, vert_idx and
faces element for element, vertex and normal rows by their bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import mesh_cc_cases as C

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

pytestmark = pytest.mark.gpu


def _dev(mesh, dev, normals=None):
    v, f = mesh[0], mesh[1]
    out = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev).reshape(-1, 3),
           torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).to(dev).reshape(-1, 3))
    return out + (torch.from_numpy(np.ascontiguousarray(normals)).to(dev),) if normals is not None else out


def _normals(mesh, seed=3):
    return C.coords(len(mesh[0]), seed=seed, nan_every=7)


def _components(meshes, dev, **kw):
    from slide_amd.mesh import mesh_components
    return mesh_components([_dev(m, dev) for m in meshes], **kw)


def _check_components(what, got, mesh):
    cid, nverts, nfaces, _ = C.components(len(mesh[0]), mesh[1])
    lab, nv, nf = (t.cpu().numpy() for t in got)
    assert lab.dtype == np.int32 and nv.dtype == np.int32 and nf.dtype == np.int32, what
    assert np.array_equal(lab, cid), "%s: %d of %d labels differ" % (what, int((lab != cid).sum()) if lab.shape == cid.shape else -1, len(cid))
    assert np.array_equal(nv, nverts) and np.array_equal(nf, nfaces), what


def _check_filter(what, got, mesh, normals, sel):
    want_v, want_f, want_n, want_idx = C.filter_mesh(mesh[0], mesh[1], normals, **sel)
    v, f, n, idx = (None if t is None else t.cpu().numpy() for t in got)
    assert v.shape == want_v.shape and f.shape == want_f.shape and v.dtype == np.float32 and f.dtype == np.int32 and idx.dtype == np.int32, what
    assert np.array_equal(idx, want_idx) and np.array_equal(f, want_f), what
    assert v.tobytes() == want_v.tobytes(), what
    if normals is None:
        assert n is None, what
    else:
        assert n.tobytes() == want_n.tobytes(), what


def _filter_and_check(named, dev, sel, with_normals=True):
    """named: [(name, (verts, faces))] as ONE batch"""
    from slide_amd.mesh import filter_components
    normals = [_normals(m) if with_normals else None for _, m in named]
    got = filter_components([_dev(m, dev, g) for (_, m), g in zip(named, normals)], return_index=True, **sel)
    assert len(got) == len(named)
    for (name, m), g, one in zip(named, normals, got):
        _check_filter("%s %s" % (name, sel), one, m, g, sel)
    return got


# ------------------------------------------------------------------------------------------------------------ 1, 2. small graphs, selection
def test_small_graphs_and_selection_rules(gpu_device):
    cases = list(C.small_cases().items())
    got = _components([m for _, m in cases], gpu_device)
    for (name, m), one in zip(cases, got):
        _check_components(name, one, m)
    for sel in C.SELECTIONS:
        _filter_and_check(cases, gpu_device, sel)
    _filter_and_check(cases, gpu_device, dict(), with_normals=False)
    # each case alone as well (a batch of one; the empty ones included)
    for name, m in cases:
        _check_components(name + " alone", _components([m], gpu_device)[0], m)
        _filter_and_check([(name, m)], gpu_device, dict())
    # the rules, spelled out
    from slide_amd.mesh import filter_components
    named = dict(cases)
    idx = lambda name, **sel: filter_components([_dev(named[name], gpu_device)], return_index=True, **sel)[0][3].cpu().tolist()  # noqa: E731
    assert idx("equal_sizes") == [0, 1, 2, 3]  # a tie: the lowest cid
    assert idx("verts_vs_faces") == [0, 1, 2, 3, 4] and idx("verts_vs_faces", by="faces") == [5, 6, 7, 8]
    assert idx("several", keep="all", min_size=4) == [3, 4, 5, 6, 8, 9, 10, 11, 12] and idx("several", min_size=6) == []
    assert idx("several", keep="all") == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15]
    v, f, n = filter_components([_dev(named["only_unreferenced"], gpu_device)])[0]
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and n is None


# ------------------------------------------------------------------------------------------------------------ 3. long chains
def test_long_strips_converge_below_the_cap(gpu_device):
    """4096 triangles in a strip, vertices numbered in order, reversed and by the bit-reversal permutation: one component, in far fewer
    rounds than the cap of V + 1 (the rounds are printed; profiles/mesh_components.md records them)"""
    strips = [(order, C.strip(4096, order)) for order in ("forward", "reversed", "bitrev")]
    for order, m in strips:
        got, info = _components([m], gpu_device, return_info=True)
        print("strip of 4096 triangles, %s numbering: %d rounds lowered a label, %d issued, %d host reads" % (order, info["rounds"], info["issued"], info["reads"]))
        _check_components(order, got[0], m)
        assert got[0][1].tolist() == [4098] and got[0][2].tolist() == [4096]
        assert info["rounds"] < info["issued"] <= 4099  # (the cap is V + 1)
    _filter_and_check(strips, gpu_device, dict())
    # a cap below the rounds needed is reported, not looped on
    from slide_amd import _ext
    f = _dev(strips[2][1], gpu_device)[1]
    with pytest.raises(RuntimeError, match="rounds"):
        _ext.mesh_cc_label(f, [0, 4098], [0, 4096], 4098, group=1, max_rounds=1)
    labels = _ext.mesh_cc_label(f, [0, 4098], [0, 4096], 4098)[0]
    assert not labels.any()


# ------------------------------------------------------------------------------------------------------------ 4. size edges
def test_sizes_around_the_spans(gpu_device):
    """V and F one below, at and one above the workgroup size of the per-element launches and the pass size of the per-mesh scans, in
    disjoint triangles (many tiny components) plus vertices without a face to reach V exactly"""
    from slide_amd import _ext
    wg, wave, tile = (_ext.mesh_cc_span(k) for k in (0, 1, 2))
    assert wave <= tile and wg <= tile
    named = []
    for span in dict.fromkeys((wg, wave, tile)):
        for n in (span - 1, span, span + 1):
            named.append(("F=%d" % n, C.disjoint_triangles(n, extra_verts=1, seed=n)))            # F = n
            named.append(("V=%d" % n, C.disjoint_triangles(n // 3, extra_verts=n % 3, seed=n)))   # V = n
    named.append(("F=2tile+3", C.disjoint_triangles(2 * tile + 3, seed=5)))
    assert {len(m[0]) for _, m in named} >= {wg - 1, wg, wg + 1, tile - 1, tile, tile + 1}
    got = _components([m for _, m in named], gpu_device)
    for (name, m), one in zip(named, got):
        _check_components(name, one, m)
    for sel in (dict(), dict(keep="all"), dict(keep="all", min_size=4)):
        _filter_and_check(named, gpu_device, sel)
    # one mesh of a few components whose vertices and faces are scattered over more than two passes
    blobs = C.random_blobs((tile + 5, 3, 2 * tile - 1, 700, 3), unreferenced=9, seed=11)
    _check_components("blobs", _components([blobs], gpu_device)[0], blobs)
    for sel in (dict(), dict(by="faces"), dict(keep="all", min_size=4)):
        _filter_and_check([("blobs", blobs)], gpu_device, sel)


# ------------------------------------------------------------------------------------------------------------ 5. batch behaviour
def _bits(one):
    return [None if t is None else t.cpu().numpy().tobytes() for t in one]


def test_a_mesh_is_labelled_the_same_anywhere(gpu_device):
    from slide_amd.mesh import filter_components, mesh_components
    cases = C.small_cases()
    pool = [("blobs", C.random_blobs((40, 3, 300, 7), unreferenced=4, seed=2)), ("empty", cases["no_vertices"]),
            ("strip", C.strip(700, "bitrev")), ("several", cases["several"]), ("triangles", C.disjoint_triangles(300, 2, seed=4)),
            ("no_faces", cases["no_faces"])]
    dev = [_dev(m, gpu_device, _normals(m)) for _, m in pool]
    alone_f = [_bits(filter_components([d], return_index=True)[0]) for d in dev]
    alone_c = [_bits(mesh_components([d])[0]) for d in dev]
    for k, (name, m) in enumerate(pool):
        _check_components(name, mesh_components([dev[k]])[0], m)
    for order in ([0, 1, 2, 3, 4, 5], [5, 4, 2, 0, 3, 1, 2]):
        batch = [dev[k] for k in order]
        for rep in range(2):  # two runs of the same batch
            got_f, got_c = filter_components(batch, return_index=True), mesh_components(batch)
            for pos, k in enumerate(order):
                assert _bits(got_f[pos]) == alone_f[k] and _bits(got_c[pos]) == alone_c[k], (order, pos, rep)
    # every position of a batch of three
    x = dev[0]
    for pos in range(3):
        batch = [dev[4], dev[2]]
        batch.insert(pos, x)
        assert _bits(filter_components(batch, return_index=True)[pos]) == alone_f[0], pos


# ------------------------------------------------------------------------------------------------------------ 6. the fixture grids
def test_components_of_marching_cubes_meshes(gpu_device):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from slide_amd.mesh import filter_components, marching_cubes, mesh_components
    g = load_golden("golden_mc.npz")
    names = [str(s) for s in g["names"]]
    strict = {str(s) for s in g["strict"]}
    r16 = [n for n in names if g["grid_" + n].shape[0] == 16]
    meshes = marching_cubes(torch.from_numpy(np.stack([g["grid_" + n] for n in r16])).to(gpu_device))
    meshes += marching_cubes(torch.from_numpy(g["grid_noise"][None]).to(gpu_device))
    order = r16 + ["noise"]
    comps, info = mesh_components(meshes, return_info=True)
    kept = filter_components(meshes, return_index=True)
    print("fixture grids: %d rounds lowered a label, %d issued, %d host reads" % (info["rounds"], info["issued"], info["reads"]))
    for name, mesh, comp, one in zip(order, meshes, comps, kept):
        v, f, n = (t.cpu().numpy() for t in mesh)
        _check_components(name, comp, (v, f))  # on our own faces (on `noise` the only comparison: its topology may differ from skimage's)
        _check_filter(name, one, (v, f), n, dict())
        if name in strict:
            sf, nsv = g["sk_faces_" + name].astype(np.int64), len(g["sk_verts_" + name])
            i, j = np.concatenate([sf[:, 0], sf[:, 1], sf[:, 2]]), np.concatenate([sf[:, 1], sf[:, 2], sf[:, 0]])
            _, lab = connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(nsv, nsv)), directed=False)
            print("%s: component sizes %s" % (name, sorted(comp[1].cpu().tolist())))
            assert sorted(comp[1].cpu().tolist()) == sorted(np.bincount(lab).tolist()), name
    two = kept[order.index("two")]
    assert two[0].shape[0] == 170 and C.euler(170, two[1].cpu().numpy()) == 2


# ------------------------------------------------------------------------------------------------------------ 7. bad indices
def test_bad_indices_are_refused_and_the_next_call_is_right(gpu_device):
    """refusal only: the index is tested on the device before it is used as an address"""
    from slide_amd.mesh import filter_components, mesh_components
    good = [C.random_blobs((30, 5, 12), unreferenced=2, seed=s) for s in (1, 2, 3)]
    for pos in (0, 1, 2):
        for bad in ("V", -1, 2 ** 31 - 1):
            batch = [(v, f.copy()) for v, f in good]
            v, f = batch[pos]
            f[len(f) // 2, (pos + 1) % 3] = len(v) if bad == "V" else bad
            with pytest.raises(ValueError, match="index"):
                mesh_components([_dev(m, gpu_device) for m in batch])
            with pytest.raises(ValueError, match="index"):
                filter_components([_dev(m, gpu_device) for m in batch])
            # the flag is reset: a valid call directly afterwards is right
            got = _components(good, gpu_device)
            for k in range(3):
                _check_components("after the refusal", got[k], good[k])
    # an index in range of the PACKED array but not of its own mesh
    v, f = good[0]
    f = f.copy()
    f[0, 0] = len(v) + 3
    with pytest.raises(ValueError, match="index"):
        mesh_components([_dev((v, f), gpu_device), _dev(good[1], gpu_device)])
    with pytest.raises(RuntimeError):
        mesh_components([(torch.from_numpy(v), torch.from_numpy(good[0][1]))])
    vg = _dev(good[0], gpu_device)[0].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        filter_components([(vg, _dev(good[0], gpu_device)[1])])
    with pytest.raises(ValueError):
        filter_components([_dev(good[0], gpu_device)], keep="some")
    with pytest.raises(ValueError):
        filter_components([_dev(good[0], gpu_device)], by="area")
    _filter_and_check([("good", good[0])], gpu_device, dict())


# ------------------------------------------------------------------------------------------------------------ 8. integration
def test_batch_mc_from_psr_keeps_the_largest_component(gpu_device, tmp_path):
    import mc_cases
    from dpsr_evaluation import batch_mc_from_psr
    from dpsr_utils.utils import mc_from_psr, verts_on_largest_mesh
    from slide_amd.mesh import load_ply, save_ply
    g = load_golden("golden_mc.npz")
    grids = torch.from_numpy(np.stack([g["grid_two"], mc_cases.sphere_grid(16, 0.33)])).to(gpu_device)
    vs, fs, ns = mc_from_psr(grids, zero_level=0)
    kw = dict(start_idx=3, sample_points_from_mesh=True, seed=4, num_samples=256, num_dense=1024)
    d_on, d_off, d_want = tmp_path / "on", tmp_path / "off", tmp_path / "want"
    for d in (d_on, d_off, d_want):
        d.mkdir()
    on = batch_mc_from_psr(grids, str(d_on), "m", largest_component=True, **kw)
    off = batch_mc_from_psr(grids, str(d_off), "m", **kw)
    # `two`: the PLY holds the kept component, and every sample lies in its bounding box
    want = C.filter_mesh(vs[0], fs[0], ns[0])
    v, f, n = load_ply(str(d_on / "m_00003.ply"))
    assert len(v) == 170 and v.tobytes() == want[0].astype(np.float32).tobytes() and np.array_equal(f, want[1]) and n.tobytes() == want[2].tobytes()
    lo, hi = v.min(axis=0), v.max(axis=0)
    for arr in (on[0][0], on[2][0]):
        assert (arr >= lo).all() and (arr <= hi).all()
    whole_lo, whole_hi = vs[0].min(axis=0), vs[0].max(axis=0)
    assert ((off[0][0] < lo) | (off[0][0] > hi)).any() and (whole_lo < lo).any() | (whole_hi > hi).any()  # (the other blob does get samples by default)
    # the sphere is one component: with or without the filter the file and the samples are the same bytes
    assert (d_on / "m_00004.ply").read_bytes() == (d_off / "m_00004.ply").read_bytes()
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(on, off))
    # the default is what it was: the files are the extraction's meshes as written by save_ply
    for k in range(2):
        save_ply(str(d_want / ("m_%05d.ply" % (3 + k))), vs[k], fs[k], normals=ns[k])
        assert (d_off / ("m_%05d.ply" % (3 + k))).read_bytes() == (d_want / ("m_%05d.ply" % (3 + k))).read_bytes()
    again = batch_mc_from_psr(grids, str(d_want), "m", largest_component=False, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(off, again))
    # original scale: the kept component's bounding box is what gets mapped
    centre, length = torch.zeros(2, 1, 3, device=gpu_device), torch.ones(2, 1, 1, device=gpu_device)
    batch_mc_from_psr(grids, str(d_on), "s", return_original_scale=True, original_center=centre, original_max_length=length, largest_component=True)
    sv = load_ply(str(d_on / "s_00000.ply"))[0]
    assert len(sv) == 170 and abs((sv.max(axis=0) - sv.min(axis=0)).max() - 1) < 1e-5 and np.abs(sv.max(axis=0) + sv.min(axis=0)).max() < 1e-5
    # the reference's name, on numpy inputs and on tensors with a leading axis
    vl, fl = verts_on_largest_mesh(vs[0], fs[0])
    assert vl.dtype == np.float32 and vl.tobytes() == want[0].astype(np.float32).tobytes() and np.array_equal(fl, want[1])
    vl2, fl2 = verts_on_largest_mesh(torch.from_numpy(vs[0])[None], torch.from_numpy(fs[0])[None])
    assert vl2.tobytes() == vl.tobytes() and np.array_equal(fl2, fl)


def test_psr_grid_cli_largest_component(gpu_device, tmp_path):
    """two spheres apart in one cloud: two components.  With the flag the mesh is the larger sphere alone, which is the restatement's
    filter of the mesh written without the flag"""
    from slide_amd.mesh import load_ply
    rs = np.random.RandomState(0)
    u = rs.standard_normal((1, 1200, 3)).astype(np.float32)
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    pts = np.concatenate([u[:, :800] * 0.3 + np.array([-0.45, 0, 0], np.float32), u[:, 800:] * 0.2 + np.array([0.5, 0, 0], np.float32)], axis=1)
    np.savez(tmp_path / "in.npz", points=pts, normals=u)
    cli = os.path.join(REPO, "pointnet2", "sampling_and_inference", "psr_grid.py")
    meshes = {}
    for tag, extra in (("plain", []), ("largest", ["--largest_component"])):
        d = tmp_path / tag
        r = subprocess.run([sys.executable, cli, "--points", str(tmp_path / "in.npz"), "--grid_res", "32", "--save", str(d / "grid.npz"),
                            "--save_mesh_dir", str(d)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        meshes[tag] = load_ply(str(d / "mesh_00000.ply"))
    v, f, n = meshes["plain"]
    want = C.filter_mesh(v, f, n)
    got = meshes["largest"]
    print("psr_grid.py: %d vertices, %d with --largest_component, %d components" % (len(v), len(got[0]), len(C.components(len(v), f)[1])))
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
    assert len(C.components(len(v), f)[1]) >= 2 and len(C.components(len(got[0]), got[1])[1]) == 1 and 0 < len(got[0]) < len(v)
    r = subprocess.run([sys.executable, cli, "--points", str(tmp_path / "in.npz"), "--save", str(tmp_path / "g.npz"), "--largest_component"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--save_mesh_dir" in r.stderr
