"""The definition of the mesh clean-up (include/slide_hip.h Part 8) restated in numpy, and the meshes the tests run it on.

  graph       nodes = the mesh's V vertices; two DISTINCT indices of one face are joined ((a, a, b): a-b; (a, a, a): nothing)
  root[v]     the smallest vertex index of v's component
  cid[v]      the rank of root[v] among the roots, ascending (scipy.sparse.csgraph.connected_components' numbering)
  counts      nverts[c]; nfaces[c] = the faces whose FIRST index is in c
  selection   candidates: nfaces >= 1 and size (by "verts" / "faces") >= min_size; "largest": the largest, ties to the lowest cid
              (numpy argmax); "all": every candidate; none: the empty mesh
  compaction  kept vertices / faces in their order, rows bit for bit, indices renumbered

The restatement is a union-find over the faces on the host: another algorithm than the kernels' label propagation."""
import numpy as np


def roots_of(nv, faces):
    """root (nv,) int64 by union-find with the smaller index as the parent"""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(nv)], dtype=np.int64)


def components(nv, faces):
    """-> (cid (nv,) int32, nverts (C,) int32, nfaces (C,) int32, root (nv,))"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    root = roots_of(nv, faces)
    uniq = np.unique(root)  # ascending
    cid = np.searchsorted(uniq, root).astype(np.int32)
    nverts = np.bincount(cid, minlength=len(uniq)).astype(np.int32)
    nfaces = np.bincount(cid[faces[:, 0]], minlength=len(uniq)).astype(np.int32) if len(faces) else np.zeros(len(uniq), np.int32)
    return cid, nverts, nfaces, root


def select(nverts, nfaces, keep="largest", by="verts", min_size=0):
    """-> the kept component ids, ascending"""
    size = nverts if by == "verts" else nfaces
    cand = [c for c in range(len(nverts)) if nfaces[c] >= 1 and size[c] >= min_size]
    if not cand or keep == "all":
        return cand
    best = max(size[c] for c in cand)
    return [min(c for c in cand if size[c] == best)]


def filter_mesh(verts, faces, normals=None, keep="largest", by="verts", min_size=0):
    """-> (verts', faces' int32, normals' or None, vert_idx int32)"""
    verts, faces = np.asarray(verts), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    cid, nverts, nfaces, _ = components(len(verts), faces)
    kept = np.zeros(len(nverts), dtype=bool)
    kept[select(nverts, nfaces, keep, by, min_size)] = True
    vkeep = kept[cid] if len(cid) else np.zeros(0, dtype=bool)
    fkeep = vkeep[faces[:, 0]] if len(faces) else np.zeros(0, dtype=bool)
    new = np.cumsum(vkeep) - 1
    out_f = new[faces[fkeep]].astype(np.int32).reshape(-1, 3)
    return verts[vkeep].reshape(-1, 3), out_f, (None if normals is None else np.asarray(normals)[vkeep].reshape(-1, 3)), np.nonzero(vkeep)[0].astype(np.int32)


def euler(nv, faces):
    """V - E + F with E = the distinct undirected edges"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return nv - len(np.unique(e, axis=0)) + len(f)


# ---------------------------------------------------------------------------------------------------------------- meshes
def coords(nv, seed=0, nan_every=0):
    """(nv, 3) float32 rows that tell the rows apart; every nan_every-th row holds a NaN with a payload"""
    v = np.random.RandomState(seed).standard_normal((nv, 3)).astype(np.float32)
    if nan_every:
        v.view(np.uint32)[::nan_every, 1] = 0x7FC00123
    return v


def mesh(nv, faces, seed=0, nan_every=0):
    return coords(nv, seed, nan_every), np.asarray(faces, dtype=np.int32).reshape(-1, 3)


def disjoint_triangles(n, extra_verts=0, seed=0):
    """n triangles (3k, 3k+1, 3k+2) and extra_verts vertices no face refers to at the end: n + extra_verts components"""
    return mesh(3 * n + extra_verts, np.arange(3 * n).reshape(n, 3), seed)


def strip(n, order="forward"):
    """a strip of n triangles (i, i+1, i+2) over n + 2 vertices, renumbered: "forward", "reversed" or "bitrev" (the bit-reversal
    permutation of the next power of two, compacted to 0 .. n+1)"""
    nv = n + 2
    if order == "forward":
        perm = np.arange(nv)
    elif order == "reversed":
        perm = np.arange(nv)[::-1].copy()
    else:
        bits = int(np.ceil(np.log2(nv)))
        rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(1 << bits)])
        perm = np.argsort(np.argsort(rev[:nv]))  # the ranks of the first nv bit-reversed numbers: a permutation of 0 .. nv-1
    i = np.arange(n)
    return mesh(nv, perm[np.stack([i, i + 1, i + 2], axis=1)], seed=n)


def random_blobs(sizes, unreferenced=0, seed=0):
    """fans of the given vertex counts (each one component, size >= 3), their vertices scattered by a random permutation together with
    `unreferenced` vertices no face refers to; the faces are shuffled"""
    rs = np.random.RandomState(seed)
    nv = sum(sizes) + unreferenced
    perm = rs.permutation(nv)
    faces, at = [], 0
    for s in sizes:
        ids = perm[at:at + s]
        faces += [(ids[0], ids[k], ids[k + 1]) for k in range(1, s - 1)]
        at += s
    faces = np.array(faces, dtype=np.int32).reshape(-1, 3)
    return coords(nv, seed, nan_every=5), faces[rs.permutation(len(faces))]


# name -> (verts, faces): the small graphs of the issue's case 1 and the selection cases of 2
def small_cases():
    return {
        "one_triangle": mesh(3, [[0, 1, 2]]),
        "two_disjoint": mesh(6, [[3, 4, 5], [0, 1, 2]]),
        "share_vertex": mesh(5, [[0, 1, 2], [2, 3, 4]]),
        "share_edge": mesh(4, [[0, 1, 2], [2, 1, 3]]),
        "degenerate_aab": mesh(5, [[3, 3, 1], [0, 2, 4]]),
        "degenerate_aaa": mesh(4, [[2, 2, 2], [0, 1, 3]]),
        "unref_front_middle_end": mesh(9, [[1, 2, 3], [5, 6, 7], [7, 6, 5]], nan_every=2),
        "only_unreferenced": mesh(4, np.zeros((0, 3))),
        "no_faces": mesh(7, np.zeros((0, 3))),
        "no_vertices": mesh(0, np.zeros((0, 3))),
        # selection: equal sizes (the lowest cid wins)
        "equal_sizes": mesh(8, [[4, 5, 6], [6, 5, 7], [0, 1, 2], [2, 1, 3]]),
        # by verts: the fan of 5 vertices / 3 faces (cid 0); by faces: 4 vertices carrying 4 faces (cid 1)
        "verts_vs_faces": mesh(9, [[0, 1, 2], [0, 2, 3], [0, 3, 4], [5, 6, 7], [5, 7, 8], [5, 8, 6], [6, 8, 7]]),
        # sizes 3, 4, 5, 3 and two vertices without a face
        "several": mesh(17, [[0, 1, 2], [3, 4, 5], [3, 5, 6], [8, 9, 10], [8, 10, 11], [8, 11, 12], [13, 14, 15]]),
    }


SELECTIONS = (dict(), dict(by="faces"), dict(keep="all"), dict(min_size=4), dict(min_size=4, keep="all"), dict(min_size=4, keep="all", by="faces"),
              dict(min_size=100), dict(min_size=100, keep="all"), dict(min_size=2, by="faces"))
