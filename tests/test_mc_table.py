"""CPU: the generated marching-cubes table (tools/gen_mc_table.py -> slide_amd/csrc/marching_cubes_table.h): the committed header is
what the generator writes, and every one of the 256 cases is a consistent piece of surface -- it covers the crossed edges, is
closed inside the cell, open exactly along the cell's faces, and what it leaves on a face depends on that face's four signs only
(two cells that share a face meet without a crack)."""
import os
import sys

import numpy as np

from conftest import REPO
import mc_cases as C

sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_mc_table as G  # noqa: E402


def _case_tris(case):
    ntri, tri, _ = C.load_table()
    return [tuple(int(e) for e in t) for t in tri[case][:ntri[case]]]


def test_generator_reproduces_the_committed_header():
    text = G.render(G.table())
    assert open(C.TABLE_HEADER).read() == text
    ntri, tri, corner = C.load_table()
    assert ntri.shape == (256,) and tri.shape[0] == 256 and tri.shape[1] == ntri.max() == 5
    assert list(corner) == G.EDGE_CORNER
    for case, want in enumerate(G.table()):
        assert _case_tris(case) == want
        assert (tri[case][ntri[case]:] == 255).all()


def test_edge_numbering():
    """edge e = 4 axis + 2 bu + bv joins MC_EDGE_CORNER[e] to the corner one step along the axis; corner c = 4 bi + 2 bj + bk"""
    _, _, corner = C.load_table()
    seen = set()
    for e in range(12):
        a = e >> 2
        c0 = int(corner[e])
        off = [(c0 >> 2) & 1, (c0 >> 1) & 1, c0 & 1]
        assert off[a] == 0
        u, v = [x for x in range(3) if x != a]
        assert 2 * off[u] + off[v] == (e & 3)
        assert G.EDGES[e] == (c0, c0 | (4 >> a))
        seen.add(G.EDGES[e])
    assert len(seen) == 12


def test_every_case_is_a_consistent_surface_patch():
    for case in range(256):
        tris = _case_tris(case)
        crossed = {e for e, (a, b) in enumerate(G.EDGES) if ((case >> a) & 1) != ((case >> b) & 1)}
        assert {e for t in tris for e in t} == crossed, case
        assert all(len(set(t)) == 3 for t in tris), case
        count = {}
        for t in tris:
            for q in range(3):
                k = (t[q], t[(q + 1) % 3])
                count[k] = count.get(k, 0) + 1
        for (a, b), n in count.items():
            assert n == 1, (case, a, b)
            if G.on_one_face(a, b):  # on a face of the cube: open here, the neighbouring cell closes it
                assert (b, a) not in count, (case, a, b)
            else:  # inside the cell: used twice, in opposite directions
                assert count.get((b, a), 0) == 1, (case, a, b)
    assert _case_tris(0) == [] and _case_tris(255) == []


def test_triangles_face_toward_the_outside_corners():
    """with every vertex at its edge's midpoint: (v1 - v0) x (v2 - v0) . (sum of the steps from the inside to the outside end) > 0"""
    for case in range(256):
        for t in _case_tris(case):
            p = [G.edge_midpoint(e) for e in t]
            d = np.zeros(3)
            for e in t:
                a, b = G.EDGES[e]
                d += (G.corner_offset(b) - G.corner_offset(a)) * (1 if (case >> a) & 1 else -1)
            assert np.dot(np.cross(p[1] - p[0], p[2] - p[0]), d) > 0, (case, t)


def _segments_on_face(case, cyc):
    """the directed triangle edges of a case that lie on the face with corners cyc"""
    on = {G.EDGE_OF[frozenset((cyc[q], cyc[(q + 1) % 4]))] for q in range(4)}
    out = set()
    for t in _case_tris(case):
        for q in range(3):
            a, b = t[q], t[(q + 1) % 3]
            if a in on and b in on:
                out.add((a, b))
    return out


def test_a_face_depends_on_its_four_signs_only():
    """no cracks: for each of the 6 x 16 face sign patterns, all 16 cases that share the pattern leave the same directed segments on
    the face -- and the opposite face of the neighbouring cell, which is the same grid face seen from the other side, carries the
    same segments reversed (every mesh edge is then used once in each direction)"""
    for axis, side, _, cyc in G.FACES:
        other = [q for q in range(8) if q not in cyc]
        per_pattern = {}
        for pattern in range(16):
            segs = None
            for rest in range(16):
                case = sum(((pattern >> q) & 1) << cyc[q] for q in range(4)) | sum(((rest >> q) & 1) << other[q] for q in range(4))
                s = _segments_on_face(case, cyc)
                assert segs is None or s == segs, (axis, side, pattern, rest)
                segs = s
            n_in = bin(pattern).count("1")
            diagonal = n_in == 2 and ((pattern & 1) == ((pattern >> 2) & 1))
            assert len(segs) == (0 if n_in in (0, 4) else 2 if diagonal else 1), (axis, side, pattern)
            per_pattern[pattern] = segs
        if side == 0:
            low = per_pattern
        else:  # edge e of the side-0 face is edge e + (the step along the axis) of the side-1 face: same bu, bv, other lower corner
            shift = {G.EDGE_OF[frozenset((c, d))]: G.EDGE_OF[frozenset((c | (4 >> axis), d | (4 >> axis)))]
                     for c, d in (G.EDGES[e] for e in range(12)) if not (c & (4 >> axis)) and not (d & (4 >> axis))}
            for pattern in range(16):
                assert per_pattern[pattern] == {(shift[b], shift[a]) for a, b in low[pattern]}, (axis, pattern)
