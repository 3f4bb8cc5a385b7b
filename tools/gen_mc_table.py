#!/usr/bin/env python
"""Derives the 256-case marching-cubes triangle table and writes slide_amd/csrc/marching_cubes_table.h.

Nothing is copied from a published table: every case is traced on the cube's six faces and closed into loops.

Numbering (what csrc/marching_cubes.hip and tests/mc_cases.py use):
  corner c = 4 bi + 2 bj + bk        the cell's corner at offset (bi, bj, bk) from its lowest-index corner; flat grid index
                                      (i r + j) r + k, so bk is the fastest axis
  case     = sum_c 2^c [corner c is inside]          inside: phi < level
  edge e   = 4 a + 2 bu + bv         the edge along axis a (0 = i, 1 = j, 2 = k) whose lower end sits at offsets (bu, bv) on the
                                      other two axes u < v; EDGE_CORNER[e] is that lower end's corner number

A face of the cube has four corners.  Its segments join the crossed edges of the face:
  one corner differs from the other three   one segment, cutting that corner off
  two adjacent corners inside               one segment between the two opposite crossed edges
  two diagonal corners inside (AMBIGUOUS)   two segments, each cutting off one INSIDE corner -- the rule reads the face's four signs
                                            only, so the two cells that share the face trace the same segments: no cracks
Every segment is directed so that, seen from outside the cube, the inside corners lie to its right; the neighbouring cell sees the
same face from the other side and walks the same segment the other way.  Each crossed edge then has one segment arriving (on one
of its two faces) and one leaving (on the other): following them closes loops whose right-hand normal points from inside to
outside, toward increasing phi.  Loops are taken in the order of their lowest-numbered edge and fan-triangulated from it -- or,
for the 18 loops where that fan would lay a chord INSIDE a cube face, from the lowest-numbered edge whose fan does not (fan_apex).

  python tools/gen_mc_table.py            rewrite the header, print the largest triangle count
  python tools/gen_mc_table.py --check    compare with the committed header instead (exit status 1 when it differs)
"""
import os
import sys

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slide_amd", "csrc", "marching_cubes_table.h")


def corner_offset(c):
    return np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1])


def _edges():
    """[(lower corner, upper corner)] of the 12 edges, in the numbering above"""
    out = []
    for a in range(3):
        u, v = [x for x in range(3) if x != a]
        for bu in range(2):
            for bv in range(2):
                off = np.zeros(3, dtype=int)
                off[u], off[v] = bu, bv
                c0 = int(off[0] * 4 + off[1] * 2 + off[2])
                off[a] = 1
                out.append((c0, int(off[0] * 4 + off[1] * 2 + off[2])))
    return out


EDGES = _edges()
EDGE_CORNER = [c0 for c0, _ in EDGES]
EDGE_OF = {frozenset(e): n for n, e in enumerate(EDGES)}


def faces():
    """[(axis, side, outward normal, the four corners in cyclic order)] of the six faces"""
    out = []
    for a in range(3):
        u, v = [x for x in range(3) if x != a]
        for side in range(2):
            cyc = []
            for bu, bv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = np.zeros(3, dtype=int)
                off[a], off[u], off[v] = side, bu, bv
                cyc.append(int(off[0] * 4 + off[1] * 2 + off[2]))
            n = np.zeros(3)
            n[a] = 1.0 if side else -1.0
            out.append((a, side, n, cyc))
    return out


FACES = faces()


def edge_midpoint(e):
    c0, c1 = EDGES[e]
    return (corner_offset(c0) + corner_offset(c1)) / 2.0


def face_segments(case, face):
    """directed segments (from edge, to edge) of one face for one case"""
    _, _, normal, cyc = face
    inside = [(case >> c) & 1 for c in cyc]
    n_in = sum(inside)
    if n_in in (0, 4):
        return []

    def around(q):  # the two face edges that meet at cyclic corner q
        return EDGE_OF[frozenset((cyc[q], cyc[(q - 1) % 4]))], EDGE_OF[frozenset((cyc[q], cyc[(q + 1) % 4]))]

    if n_in == 1:
        pairs = [around(inside.index(1))]
    elif n_in == 3:
        pairs = [around(inside.index(0))]
    elif inside[0] == inside[2]:  # ambiguous: the inside corners are diagonal; cut each of them off
        pairs = [around(q) for q in range(4) if inside[q]]
    else:  # two adjacent inside corners: the crossed edges are the two that join an inside to an outside corner
        crossed = [EDGE_OF[frozenset((cyc[q], cyc[(q + 1) % 4]))] for q in range(4) if inside[q] != inside[(q + 1) % 4]]
        pairs = [tuple(crossed)]
    out = []
    for e1, e2 in pairs:
        m1, m2 = edge_midpoint(e1), edge_midpoint(e2)
        toward_inside = np.zeros(3)
        for e, m in ((e1, m1), (e2, m2)):
            c_in = [c for c in EDGES[e] if (case >> c) & 1][0]
            toward_inside += corner_offset(c_in) - m
        left = np.cross(normal, m2 - m1)  # the left of the direction m1 -> m2, seen from outside the cube
        s = float(np.dot(left, toward_inside))
        assert abs(s) > 1e-9
        out.append((e1, e2) if s < 0 else (e2, e1))  # inside on the right
    return out


def case_loops(case):
    nxt = {}
    for face in FACES:
        for e1, e2 in face_segments(case, face):
            assert e1 not in nxt
            nxt[e1] = e2
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop, cur = [], e
        while cur not in seen:
            seen.add(cur)
            loop.append(cur)
            cur = nxt[cur]
        assert cur == e and len(loop) >= 3
        loops.append(loop)
    return loops


def on_one_face(e1, e2):
    """do the two cube edges lie on a common face of the cube?"""
    return any(set(EDGES[e1]) | set(EDGES[e2]) <= set(cyc) for _, _, _, cyc in FACES)


def fan_apex(loop):
    """the loop rotated to the edge its fan starts from: the lowest-numbered edge whose fan chords all run through the cell's
    interior.  A chord between two crossed edges of one (ambiguous) face would lie IN that face, where the neighbouring cell may lay
    the same chord: 18 loops of the 256 cases have such a chord from their lowest edge, and every one has an apex without."""
    n = len(loop)
    for e in sorted(loop):
        s = loop.index(e)
        rot = loop[s:] + loop[:s]
        if not any(on_one_face(rot[0], rot[q]) for q in range(2, n - 1)):
            return rot
    raise AssertionError("no fan without a chord in a cube face: %s" % (loop,))


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        loop = fan_apex(loop)
        for q in range(1, len(loop) - 1):
            tris.append((loop[0], loop[q], loop[q + 1]))
    return tris


def table():
    return [case_triangles(case) for case in range(256)]


def render(tab):
    mt = max(len(t) for t in tab)
    lines = ["// marching_cubes_table.h -- GENERATED by tools/gen_mc_table.py (the numbering and the rule of ambiguous faces are written out",
             "// there); do not edit.  MC_NTRI[case] triangles per case, MC_TRI[case] their 3 * MC_NTRI[case] cube edges (255 = unused),",
             "// MC_EDGE_CORNER[e] the corner at the lower end of edge e (its axis is e >> 2).",
             "#ifndef SLIDE_MARCHING_CUBES_TABLE_H", "#define SLIDE_MARCHING_CUBES_TABLE_H", "",
             "#define MC_MAX_TRIS %d" % mt, "",
             "__device__ const unsigned char MC_EDGE_CORNER[12] = {%s};" % ", ".join(str(c) for c in EDGE_CORNER), "",
             "__device__ const unsigned char MC_NTRI[256] = {"]
    for row in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tab[row:row + 32]) + ",")
    lines += ["};", "", "__device__ const unsigned char MC_TRI[256][MC_MAX_TRIS * 3] = {"]
    for case, t in enumerate(tab):
        flat = [e for tri in t for e in tri]
        flat += [255] * (mt * 3 - len(flat))
        lines.append("    {%s},  // %d" % (", ".join("%d" % e for e in flat), case))
    lines += ["};", "", "#endif", ""]
    return "\n".join(lines)


def main():
    tab = table()
    text = render(tab)
    if "--check" in sys.argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("marching_cubes_table.h is %s" % ("up to date" if same else "STALE"))
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote %s: 256 cases, largest triangle count %d" % (os.path.relpath(HEADER), max(len(t) for t in tab)))


if __name__ == "__main__":
    main()
