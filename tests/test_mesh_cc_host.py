"""CPU: the numpy restatement of the mesh clean-up's definition (tests/mesh_cc_cases.py) against scipy's connected_components, on the
hand-made cases and on the skimage faces recorded in tests/golden/golden_mc.npz; its selection rules and its compaction."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from conftest import load_golden
import mesh_cc_cases as C


def _scipy(nv, faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    i = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    j = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    return connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(nv, nv)), directed=False)


def _all_cases():
    out = dict(C.small_cases())
    out["blobs"] = C.random_blobs((5, 3, 9, 4), unreferenced=3, seed=1)
    out["triangles"] = C.disjoint_triangles(50, extra_verts=2)
    for order in ("forward", "reversed", "bitrev"):
        out["strip_" + order] = C.strip(200, order)
    return out


def test_restatement_equals_scipy_on_every_case():
    for name, (v, f) in _all_cases().items():
        cid, nverts, nfaces, root = C.components(len(v), f)
        n, lab = _scipy(len(v), f)
        assert n == len(nverts) and np.array_equal(lab, cid), name
        assert nverts.sum() == len(v) and nfaces.sum() == len(f), name
        for c in range(n):  # the root is the component's smallest index
            assert root[cid == c].tolist() == [int(np.nonzero(cid == c)[0][0])] * int(nverts[c]), name
    # the strips are one component whatever the numbering; the bit-reversal numbering is a permutation
    for order in ("forward", "reversed", "bitrev"):
        v, f = C.strip(4096, order)
        assert sorted(np.unique(f).tolist()) == list(range(4098)) and len(C.components(len(v), f)[1]) == 1


def test_restatement_on_the_marching_cubes_fixture():
    g = load_golden("golden_mc.npz")
    want = {"two": [168, 170], "smooth1": [422, 480], "noise": [712, 4]}
    largest = {"two": (1, 170), "smooth0": (2, 277), "smooth1": (1, 480), "noise": (0, 712)}
    for name in (str(s) for s in g["names"]):
        nv, f = len(g["sk_verts_" + name]), g["sk_faces_" + name]
        cid, nverts, nfaces, _ = C.components(nv, f)
        n, lab = _scipy(nv, f)
        assert n == len(nverts) and np.array_equal(lab, cid), name
        if name in want:
            assert nverts.tolist() == want[name], name
        if name in largest:
            (c,) = C.select(nverts, nfaces)
            assert (c, int(nverts[c])) == largest[name], name
    nverts = C.components(len(g["sk_verts_smooth0"]), g["sk_faces_smooth0"])[1]
    assert len(nverts) == 5 and sorted(nverts.tolist(), reverse=True)[:4] == [277, 82, 74, 58]
    # the kept component of `two` is a closed surface of genus 0
    v, f, n, idx = C.filter_mesh(g["sk_verts_two"], g["sk_faces_two"], g["sk_normals_two"])
    assert len(v) == 170 and C.euler(len(v), f) == 2 and n.shape == v.shape


def test_selection_rules():
    cases = C.small_cases()
    v, f = cases["equal_sizes"]
    cid, nverts, nfaces, _ = C.components(len(v), f)
    assert nverts.tolist() == [4, 4] and C.select(nverts, nfaces) == [0]  # a tie goes to the lowest cid
    assert C.filter_mesh(v, f)[3].tolist() == [0, 1, 2, 3]
    v, f = cases["verts_vs_faces"]
    cid, nverts, nfaces, _ = C.components(len(v), f)
    assert (nverts.tolist(), nfaces.tolist()) == ([5, 4], [3, 4])
    assert C.select(nverts, nfaces, by="verts") == [0] and C.select(nverts, nfaces, by="faces") == [1]
    v, f = cases["several"]
    cid, nverts, nfaces, _ = C.components(len(v), f)
    assert nverts.tolist() == [3, 4, 1, 5, 3, 1] and nfaces.tolist() == [1, 2, 0, 3, 1, 0]
    assert C.select(nverts, nfaces, keep="all") == [0, 1, 3, 4]  # a component without a face is never selected
    assert C.select(nverts, nfaces, keep="all", min_size=4) == [1, 3] and C.select(nverts, nfaces, min_size=4) == [3]
    assert C.select(nverts, nfaces, min_size=6) == [] and C.select(nverts, nfaces, keep="all", min_size=6) == []
    # no face, never selected: also when it is the only and therefore the largest component
    for name in ("only_unreferenced", "no_faces", "no_vertices"):
        v, f = cases[name]
        ov, of, _, idx = C.filter_mesh(v, f)
        assert ov.shape == (0, 3) and of.shape == (0, 3) and len(idx) == 0, name
    # (a, a, a) has a face: a singleton WITH a face is a candidate
    v, f = C.mesh(2, [[1, 1, 1]])
    assert C.filter_mesh(v, f)[3].tolist() == [1] and C.filter_mesh(v, f)[1].tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("sel", C.SELECTIONS, ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()) or "default")
def test_compaction_yields_valid_meshes(sel):
    for name, (v, f) in _all_cases().items():
        normals = C.coords(len(v), seed=7)
        ov, of, on, idx = C.filter_mesh(v, f, normals, **sel)
        assert len(ov) == len(idx) and on.shape == ov.shape and (np.diff(idx) > 0).all(), name
        assert ov.tobytes() == v[idx].tobytes() and on.tobytes() == normals[idx].tobytes(), name  # bit for bit, NaN included
        if len(of):
            assert of.min() >= 0 and of.max() < len(ov), name
        assert sorted(np.unique(of).tolist()) == list(range(len(ov))), name  # every vertex is referenced
        # winding and order: mapped back, the kept faces are a subsequence of the input's faces
        back = idx[of] if len(of) else np.zeros((0, 3), np.int32)
        cid = C.components(len(v), f)[0]
        kept = np.isin(cid[f[:, 0]], np.unique(cid[idx])) if len(f) else np.zeros(0, bool)
        assert np.array_equal(back, f[kept]), name
