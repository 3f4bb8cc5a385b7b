"""Marching-cubes test cases: the grids, a numpy float64 restatement of the definition in slide_amd/csrc/marching_cubes.hip, the mesh
checks and the bounds.  numpy only -- tools/gen_golden_mc.py imports this file under the one interpreter that has scikit-image.

Definition (include/slide_hip.h Part 6).  A grid point is inside iff phi < level.  Every grid edge (p, p + e_axis) whose ends differ
in that predicate carries one vertex at p + t e_axis, t = (level - a) / (b - a), a = phi[p], b = phi[p + e_axis]; its normal is
-g / |g| with g = g(p) + t (g(p + e_axis) - g(p)), g(q) the central difference of phi at q, one-sided on the border
(numpy.gradient).  A vertex is KEYED by (floor(v), axis): the lower end of its edge and the one coordinate that is not an integer.

Bounds.  u = 2^-24.

Vertex.  a and b are float32 values of opposite side of level.  fl(level - a) and fl(b - a) carry one rounding each, the quotient a
third: t^ = t (1 + d), |d| <= 3.01 u.  0 <= t <= 1 (|level - a| <= |b - a| when level lies between a and b, and rounding is
monotone: t^ <= 1).  The coordinate p + t^ with p an integer <= r - 1 is rounded once more, to a value <= r: at most u r.  So
      |v - v64| <= 3.01 u t + u r   <=  VERT_BOUND(r) = (3.01 + r) u                           (5.7e-7 + 6e-8 r)
Against skimage's float32 vertices: skimage interpolates in float64 and rounds once, a further half ulp of a value <= r: u r.
The wrong arithmetics the bound must exclude on the test grids (WRONG_T): `other_end` t measured from the far end (1 - t),
`midpoint` t = 0.5.

Normal.  With M = max |phi| over the stencil of the edge (the 10 neighbours of its two ends): a difference fl(x - y) has absolute
error u |x - y| <= 2 u M and the scale by 0.5 is exact, so each component of g(p), g(p + e) is within 2 u M.  g1 - g0 rounds once
(<= u 4 M on values <= 2 M each), times t^ (relative 4.01 u of a product <= 4 M, plus the 4 u M already there), plus g0 rounds
once more: each component of g^ is within E = (2 + 4 + 4 + 16.04 + 6) u M <= 33 u M of g.  Normalising: the squared length of three
rounded squares and two sums (relative 3 u, 1.5 u after the root), the root and the division within one ulp each (2 u): relative
5.5 u per component; and for unit vectors |g^ / |g^| - g / |g|| <= 2 |g^ - g| / |g|.  So per component
      |n - n64| <= 2 sqrt(3) E / |g| + 6.01 u        =: normal_bound(M, |g|) = 115 u M / |g| + 6.01 u
(infinite where |g| <= sqrt(3) E: the direction is not determined there).
"""
import os
import re

import numpy as np

U = 2.0 ** -24
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_HEADER = os.path.join(REPO, "slide_amd", "csrc", "marching_cubes_table.h")
WRONG_T = ("other_end", "midpoint")

# the cases compared with skimage (no ambiguous face: Lewiner's and the classic tables agree in vertex count and topology there)
STRICT = ("sphere", "torus", "two", "cut", "smooth0", "smooth1")


def vert_bound(r):
    return (3.01 + r) * U


def skimage_vert_bound(r):
    return vert_bound(r) + r * U


def normal_bound(M, glen):
    E = 33.0 * U * M
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(glen > np.sqrt(3.0) * E, 2.0 * np.sqrt(3.0) * E / glen + 6.01 * U, np.inf)


# ------------------------------------------------------------------------------------------------------------ grids
def _coords(r=16):
    g = np.mgrid[0:r, 0:r, 0:r].astype(np.float64)
    c = 7.63
    return g[0] - c, g[1] - c - 0.21, g[2] - c + 0.37


def _lowpass(seed):
    k = np.fft.fftfreq(16)
    k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, :] ** 2
    noise = np.random.default_rng(seed).standard_normal((16, 16, 16))
    return np.fft.ifftn(np.fft.fftn(noise) * np.exp(-150.0 * k2)).real


def synthetic_grids():
    """name -> float32 grid, the cases of the fixture that are defined by a formula"""
    x, y, z = _coords()
    out = {"sphere": np.sqrt(x * x + y * y + z * z) - 5.3,
           "torus": (np.sqrt(x * x + y * y) - 4.2) ** 2 + z * z - 2.1 ** 2,
           "two": np.minimum(np.sqrt((x - 3.6) ** 2 + y * y + z * z) - 3.0, np.sqrt((x + 3.7) ** 2 + y * y + z * z) - 3.0),
           "cut": np.sqrt(x * x + y * y + z * z) - 9.0,
           "smooth0": _lowpass(10), "smooth1": _lowpass(11),
           "noise": np.random.default_rng(1).standard_normal((8, 8, 8))}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def sphere_grid(r, radius_frac=0.33):
    """an r^3 sphere off the lattice (the r = 64 case and the timing tool's grids)"""
    g = np.mgrid[0:r, 0:r, 0:r].astype(np.float64)
    c = (r - 1) / 2 + 0.13
    return (np.sqrt((g[0] - c) ** 2 + (g[1] - c - 0.21) ** 2 + (g[2] - c + 0.37) ** 2) - radius_frac * r).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ restatement
def inside(phi, level=0.0):
    return np.asarray(phi) < np.float32(level)  # (a NaN compares false: outside)


def ambiguous_faces(phi, level=0.0):
    """the number of cell faces whose four corners alternate diagonally"""
    s, n = inside(phi, level), 0
    for ax in range(3):
        a = np.moveaxis(s, ax, 0)
        p00, p01, p10, p11 = a[:, :-1, :-1], a[:, :-1, 1:], a[:, 1:, :-1], a[:, 1:, 1:]
        n += int(((p00 == p11) & (p01 == p10) & (p00 != p01)).sum())
    return n


def gradient64(phi):
    """(r, r, r, 3) float64: central differences, one-sided on the border (numpy.gradient, edge_order 1)"""
    return np.stack(np.gradient(np.asarray(phi, np.float64)), axis=-1)


def crossings(phi, level=0.0, wrong=None):
    """every sign-changing grid edge, in float64: keys (n, 4) int (i, j, k, axis) sorted lexicographically, vertices (n, 3),
    normals (n, 3), t (n,), and for the normal bound M (n,) = max |phi| over the stencil and |g| (n,)"""
    phi32 = np.asarray(phi, np.float32)
    phi64 = phi32.astype(np.float64)
    r = phi32.shape[0]
    s = inside(phi32, level)
    grad = gradient64(phi32)
    # max |phi| over a point's own 7-point stencil; an edge's stencil is the union of its two ends'
    pad = np.pad(np.abs(phi64), 1, mode="edge")
    m7 = np.abs(phi64).copy()
    for ax in range(3):
        for sh in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[ax] = slice(sh, sh + r)
            m7 = np.maximum(m7, pad[tuple(sl)])
    keys, verts, normals, ts, Ms, gl = [], [], [], [], [], []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, r - 1), slice(1, r)
        lo, hi = tuple(lo), tuple(hi)
        m = s[lo] != s[hi]
        idx = np.argwhere(m)
        a, b = phi64[lo][m], phi64[hi][m]
        t = (float(np.float32(level)) - a) / (b - a)
        if wrong == "other_end":
            t = 1.0 - t
        elif wrong == "midpoint":
            t = np.full_like(t, 0.5)
        v = idx.astype(np.float64)
        v[:, ax] += t
        g0, g1 = grad[lo][m], grad[hi][m]
        g = g0 + t[:, None] * (g1 - g0)
        ln = np.linalg.norm(g, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.where(ln[:, None] > 0, -g / ln[:, None], 0.0)
        keys.append(np.concatenate([idx, np.full((len(idx), 1), ax)], axis=1))
        verts.append(v)
        normals.append(n)
        ts.append(t)
        Ms.append(np.maximum(m7[lo][m], m7[hi][m]))
        gl.append(ln)
    keys = np.concatenate(keys).astype(np.int64)
    order = np.lexsort(keys.T[::-1])
    pick = lambda xs: np.concatenate(xs)[order]  # noqa: E731
    return {"keys": keys[order], "verts": pick(verts), "normals": pick(normals), "t": pick(ts), "M": pick(Ms), "glen": pick(gl)}


def vertex_keys(verts, r):
    """(V, 4) int (i, j, k, axis) of float32 vertices: floor and the non-integer coordinate.  A vertex whose t rounded to 0 or 1 has no
    fractional coordinate and cannot be keyed: ValueError (the fixture's grids keep |phi| away from the level)"""
    v = np.asarray(verts, np.float64)
    base = np.floor(v)
    frac = v - base
    nz = frac > 0
    if not (nz.sum(1) == 1).all():
        raise ValueError("%d vertices do not lie strictly inside exactly one grid edge" % int((nz.sum(1) != 1).sum()))
    return np.concatenate([base.astype(np.int64), np.argmax(nz, axis=1)[:, None]], axis=1)


def match_keys(keys, want_keys):
    """the permutation p with keys[p] == want_keys (both (n, 4)); AssertionError unless keys is one-to-one onto want_keys"""
    assert keys.shape == want_keys.shape, "%d vertices for %d sign-changing edges" % (len(keys), len(want_keys))
    p = np.lexsort(keys.T[::-1])
    assert np.array_equal(keys[p], want_keys), "the vertices are not one-to-one with the sign-changing edges"
    return p


# ------------------------------------------------------------------------------------------------------------ table
def load_table():
    """the committed header -> (ntri (256,), tri (256, MAX, 3) edges, edge_corner (12,))"""
    text = open(TABLE_HEADER).read()
    text = re.sub(r"//[^\n]*", "", text)

    def body(name):
        m = re.search(r"%s\s*(?:\[[^\]]*\])+\s*=\s*\{(.*?)\};" % name, text, flags=re.S)
        return np.array([int(x) for x in re.findall(r"\d+", m.group(1))], dtype=np.int64)

    mt = int(re.search(r"#define MC_MAX_TRIS (\d+)", text).group(1))
    return body("MC_NTRI"), body("MC_TRI").reshape(256, mt, 3), body("MC_EDGE_CORNER")


def cell_cases(phi, level=0.0):
    """(r-1, r-1, r-1) case numbers: bit c = 4 bi + 2 bj + bk set when that corner is inside"""
    s = inside(phi, level)
    r = s.shape[0]
    out = np.zeros((r - 1,) * 3, dtype=np.int64)
    for c in range(8):
        bi, bj, bk = (c >> 2) & 1, (c >> 1) & 1, c & 1
        out |= s[bi:r - 1 + bi, bj:r - 1 + bj, bk:r - 1 + bk].astype(np.int64) << c
    return out


def table_face_count(phi, level=0.0):
    return int(load_table()[0][cell_cases(phi, level)].sum())


# ------------------------------------------------------------------------------------------------------------ mesh checks
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def check_faces(verts, faces, phi, level=0.0):
    """the self-consistency of an indexed mesh on a grid: indices in range, no repeated index in a face, every directed edge once,
    its reverse once unless both ends lie on one boundary plane of the grid, F = the table's count"""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    r = np.asarray(phi).shape[0]
    V = len(v)
    assert f.ndim == 2 and f.shape[1] == 3
    if len(f):
        assert f.min() >= 0 and f.max() < V
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    e = directed_edges(f)
    code = e[:, 0] * max(V, 1) + e[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    has_rev = np.isin(e[:, 1] * max(V, 1) + e[:, 0], code)
    p, q = v[e[:, 0]], v[e[:, 1]]
    on_border = (((p == 0) & (q == 0)) | ((p == r - 1) & (q == r - 1))).any(axis=1)
    assert (has_rev | on_border).all(), "%d interior edges have no reverse" % int((~(has_rev | on_border)).sum())
    assert len(f) == table_face_count(phi, level), "F %d, the table gives %d" % (len(f), table_face_count(phi, level))


def euler(n_verts, faces):
    e = np.sort(directed_edges(faces), axis=1)
    return int(n_verts) - len(np.unique(e, axis=0)) + len(faces)


def components(n_verts, faces):
    """connected components of the vertex graph (isolated vertices count)"""
    parent = np.arange(n_verts)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in np.sort(directed_edges(faces), axis=1):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[rb] = ra
    return len({find(x) for x in range(n_verts)})


def orientation(verts, faces, phi, level=0.0):
    """per face n . d: n = (v1 - v0) x (v2 - v0), d = the sum over its three vertices of the unit step from the inside end to the
    outside end of the vertex's grid edge"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    keys = vertex_keys(verts, np.asarray(phi).shape[0])
    s0 = inside(phi, level)[keys[:, 0], keys[:, 1], keys[:, 2]]
    step = np.zeros((len(v), 3))
    step[np.arange(len(v)), keys[:, 3]] = np.where(s0, 1.0, -1.0)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    d = step[f[:, 0]] + step[f[:, 1]] + step[f[:, 2]]
    return (n * d).sum(1)
