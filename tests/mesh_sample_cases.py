"""Mesh-sampling test cases: the meshes, a restatement of the definition in slide_amd/csrc/mesh_sample.hip (include/slide_hip.h
Part 7) in numpy float32 / float64 / exact integers, the wrong arithmetics next to it, and the bounds.  numpy only.

Definition.  A mesh is verts (V, 3) float32 and faces (F, 3) integers.
  face vector  n_f = (v1 - v0) x (v2 - v0) in float32, each component a*b - c*d as two products and one subtraction
  area         area_f = 0.5f * sqrtf((nx*nx + ny*ny) + nz*nz);  0 for a face with an index outside [0, V) or a non-finite vertex
  amax         the largest finite area
  quantised    q_f = floor(float64(area_f) * 2^32 / float64(amax)), 0 for a zero or non-finite area or amax = 0
  cdf          the inclusive prefix sum of q, exact integers; total = cdf[-1]
  words        (c0, c1, c2, c3) = Philox4x32-10(counter (s, mesh_id, stream_id, 0x13198A2E), key (seed_lo, seed_hi)), or given
  face         r = c0 << 32 | c1, t = (r * total) >> 64, face = the number of cdf entries <= t
  weights      u = ((c2 >> 8) + 0.5) * 2^-24 in float32 (so in (0, 1]), v likewise from c3; su = sqrt(u), w0 = 1 - su, w1 = su (1 - v),
               w2 = su v
  point        w0 v0 + w1 v1 + w2 v2
  normal       face:   n_f / max(|n_f|, FLT_EPSILON);   vertex: g / max(|g|, FLT_EPSILON), g = w0 g0 + w1 g1 + w2 g2
  empty        F = 0 or total = 0: zeros, face -1, valid 0
The areas are restated in float32, bit for bit; everything after the words in exact integers (the selection) and float64 (points and
normals, from the float32 u and v, which are exact).

Bounds.  e = 2^-24 (the unit roundoff of float32), coordinates of normal magnitude (no underflow).

Area.  e1 = fl(v1 - v0), e2 likewise: relative e per component.  A product of two of them then carries (1 + e)^3: 3.01 e.  A component
fl(a - b) of n: |error| <= 3.01 e (|a| + |b|) + e |a - b| <= 4.02 e (|a| + |b|), and by Cauchy-Schwarz |a| + |b| <= |e1| |e2| for each of
the three components: |n^ - n| <= sqrt(3) 4.02 e |e1| |e2| = 6.97 e |e1| |e2|.  The length: two squares and two sums of positive terms
(relative 3 e, 1.5 e after the root), the root itself (e): 2.51 e |n| <= 2.51 e |e1| |e2|; the factor 0.5 is exact.
      |area - area64| <= AREA_C e |e1| |e2|,   AREA_C = 0.5 (6.97 + 2.51) rounded up = 4.75
relative to |e1| |e2| and NOT to the area: the cross product cancels, a sliver's area has no relative accuracy.

Point.  M = the largest |coordinate| of the face's three vertices.  su = fl(sqrt(u)): e.  w0 = fl(1 - su): 2 e absolute (values <= 1);
1 - v: e; w1 = fl(su (1 - v)): 3 e; w2 = fl(su v): 2 e.  Each product w_i x_i adds relative e (in sum e (w0 + w1 + w2) M = e M), the
two additions round once each (e M each, partial sums <= M):
      |p - p64| <= POINT_C e M,   POINT_C = (2 + 3 + 2) + 1 + 2 = 10, taken as 10.1 for the second-order terms
The wrong arithmetics it must exclude (WRONG_POINT): `u_for_sqrt` su = u, `rotated` the weights attached to (v1, v2, v0),
`v_swapped` v and 1 - v exchanged.  Each moves a sample by a fraction of the triangle's size.

Normal (unit vectors, per component).  Face mode: for unit vectors |a^/|a^| - a/|a|| <= 2 |a^ - a| / |a|; the computed length carries
2.51 e, the division e:
      |n - n64| <= 2 * 6.97 e |e1| |e2| / |n_f| + 3.6 e          = face_normal_bound
(it needs |n_f| >= 2 FLT_EPSILON: below, the clamp decides).  The wrong arithmetic: `flipped` (v2 - v0) x (v1 - v0), off by 2 |n|.
Vertex mode: g's components carry the point's error with G = the largest |component| of the three vertex normals, so
      |n - n64| <= 2 sqrt(3) 10.1 e G / |g| + 3.6 e             = vertex_normal_bound   (infinite where |g| <= sqrt(3) 10.1 e G)

Selection is exact: face indices are compared with ==.  Its wrong arithmetics (WRONG_SELECT): `lower_bound` the number of entries
< t, `exclusive` the exclusive prefix sum: both change the chosen face of a draw that lands on a boundary or next to a face with
q = 0, and `exclusive` shifts every draw's face by construction on a mesh whose first face has q > 0.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from update_cases import philox4x32_10  # noqa: E402

F32 = np.float32
E = 2.0 ** -24
FLT_EPSILON = 2.0 ** -23
PHILOX_K = 0x13198A2E
AREA_C, POINT_C = 4.75, 10.1
WRONG_POINT = ("u_for_sqrt", "rotated", "v_swapped")
WRONG_SELECT = ("lower_bound", "exclusive")
CHI2_7_0999 = 24.32  # the 0.999 quantile of chi^2 with 7 degrees of freedom


# ------------------------------------------------------------------------------------------------------------ meshes
def single_face():
    v = np.array([[0.25, -1.0, 0.5], [2.0, 0.5, 0.75], [-0.5, 1.5, 3.0]], F32)
    return v, np.array([[0, 1, 2]], np.int32)


def ratio_mesh():
    """8 faces with areas in ratio 1 : 2 : ... : 8 (each a right triangle with legs 1 and k, in a plane of its own) and one zero-area
    face (three collinear vertices) in the middle, row 4: 9 faces, 27 vertices"""
    verts, k = [], 1
    for row in range(9):
        o = np.array([3.0 * row, -0.5 * row, 0.25 * row])
        if row == 4:
            verts += [o, o + [1.0, 1.0, 0.5], o + [2.0, 2.0, 1.0]]
            continue
        a = 0.3 * k
        verts += [o, o + [np.cos(a), np.sin(a), 0.0], o + k * np.array([-np.sin(a) * 0.6, np.cos(a) * 0.6, 0.8])]
        k += 1
    return np.array(verts, F32), np.arange(27, dtype=np.int32).reshape(9, 3)


def random_mesh(n_faces, n_verts=300, seed=0, degenerate_every=0):
    """random triangles over random vertices; with degenerate_every = d every d-th face repeats a vertex (area 0)"""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-1.0, 1.0, (n_verts, 3)).astype(F32)
    f = np.stack([rs.permutation(n_verts)[:3] for _ in range(n_faces)]).astype(np.int32) if n_faces else np.zeros((0, 3), np.int32)
    if degenerate_every:
        f[::degenerate_every, 2] = f[::degenerate_every, 0]
    return v, f


def degenerate_mesh(n_faces=5):
    """every face has a repeated vertex: total = 0"""
    v, f = random_mesh(n_faces, 12, seed=3)
    f[:, 1] = f[:, 0]
    return v, f


def empty_mesh():
    return np.zeros((4, 3), F32) + F32(0.5), np.zeros((0, 3), np.int32)


# ------------------------------------------------------------------------------------------------------------ restatement
def face_vectors32(verts, faces, flipped=False):
    """(F, 3) float32, the stated operation order"""
    v = np.asarray(verts, F32)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    e1, e2 = (c - a, b - a) if flipped else (b - a, c - a)
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(F32)


def length32(n):
    n = np.asarray(n, F32)
    return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(F32)


def refused(verts, faces):
    """(F,) flag bits: 1 an index outside [0, V), 2 a non-finite coordinate of a referenced vertex"""
    f = np.asarray(faces, np.int64)
    out = np.where(((f < 0) | (f >= len(verts))).any(axis=1), 1, 0)
    ok = out == 0
    fin = np.isfinite(np.asarray(verts, F32)).all(axis=1)
    out[ok] = np.where(fin[f[ok]].all(axis=1), 0, 2)
    return out


def areas32(verts, faces):
    """(F,) float32, bit for bit what the kernel stores"""
    bad = refused(verts, faces)
    out = np.zeros(len(faces), F32)
    ok = bad == 0
    with np.errstate(over="ignore", invalid="ignore"):
        out[ok] = F32(0.5) * length32(face_vectors32(verts, np.asarray(faces)[ok]))
    return out


def areas64(verts, faces):
    """(area (F,), |e1| |e2| (F,)) in float64 from the float32 vertices"""
    v = np.asarray(verts, np.float64)
    e1, e2 = v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
    return 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1), np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)


def quantise(areas):
    """list of Python ints"""
    a = np.asarray(areas, F32).astype(np.float64)
    fin = np.isfinite(a)
    amax = a[fin].max() if fin.any() else 0.0
    if not amax > 0:
        return [0] * len(a)
    return [int(np.floor(x * 4294967296.0 / amax)) if (f and x > 0) else 0 for x, f in zip(a, fin)]


def cdf_of(q, exclusive=False):
    """the prefix sums as Python ints; (cdf list, total)"""
    out, run = [], 0
    for x in q:
        out.append(run if exclusive else run + x)
        run += x
    return out, run


def philox_words(n, seed, mesh_id, stream_id):
    """(n, 4) uint64 holding the 32-bit words of samples 0 .. n - 1"""
    s = np.arange(n, dtype=np.uint64)
    full = lambda x: np.full(n, x & 0xFFFFFFFF, np.uint64)  # noqa: E731
    return np.stack(philox4x32_10(s, full(mesh_id), full(stream_id), full(PHILOX_K), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), axis=1)


def select(words, cdf, total, wrong=None):
    """(S,) int64 face rows from the first two words, exact integers"""
    import bisect
    out = np.empty(len(words), np.int64)
    for i, w in enumerate(words):
        t = (((int(w[0]) << 32) | int(w[1])) * total) >> 64
        out[i] = bisect.bisect_left(cdf, t) if wrong == "lower_bound" else bisect.bisect_right(cdf, t)
    return out


def uniforms(words):
    """(u, v) float32 -- exact values of the kernel's"""
    return [((np.asarray(words)[:, k].astype(np.uint64) >> np.uint64(8)).astype(F32) + F32(0.5)) * F32(1.0 / 16777216.0) for k in (2, 3)]


def weights64(words, wrong=None):
    u, v = (x.astype(np.float64) for x in uniforms(words))
    if wrong == "v_swapped":
        v = 1.0 - v
    su = u if wrong == "u_for_sqrt" else np.sqrt(u)
    return np.stack([1.0 - su, su * (1.0 - v), su * v], axis=1)


def sample(verts, faces, n, seed=0, mesh_id=0, stream_id=0, words=None, vnormals=None, wrong=None):
    """the restatement for ONE mesh -> dict: face (S,), points (S, 3) float64, normals_face, normals_vertex (or None), valid, words,
    and the per-sample quantities of the bounds: M, e1e2, nlen (face mode), G, glen (vertex mode)"""
    verts, faces = np.asarray(verts, F32), np.asarray(faces, np.int64)
    words = philox_words(n, seed, mesh_id, stream_id) if words is None else np.asarray(words, np.uint64)
    n = len(words)
    q = quantise(areas32(verts, faces)) if len(faces) else []
    cdf, total = cdf_of(q, exclusive=(wrong == "exclusive"))
    zero = np.zeros((n, 3))
    if total == 0:
        return {"face": np.full(n, -1, np.int64), "points": zero, "normals_face": zero, "normals_vertex": zero, "valid": 0, "words": words}
    face = select(words, cdf, total, wrong)
    if wrong in WRONG_SELECT:
        return {"face": face, "valid": 1, "words": words}
    w = weights64(words, wrong)
    tri = verts.astype(np.float64)[faces[face]]  # (S, 3 vertices, 3)
    if wrong == "rotated":
        tri = tri[:, [1, 2, 0]]
    pts = (w[:, :, None] * tri).sum(axis=1)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nf = np.cross(e2, e1) if wrong == "flipped" else np.cross(e1, e2)
    nlen = np.linalg.norm(nf, axis=1)
    out = {"face": face, "points": pts, "valid": 1, "words": words, "weights": w, "M": np.abs(tri).max(axis=(1, 2)),
           "e1e2": np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1), "nlen": nlen,
           "normals_face": nf / np.maximum(nlen, FLT_EPSILON)[:, None], "normals_vertex": None}
    if vnormals is not None:
        gt = np.asarray(vnormals, F32).astype(np.float64)[faces[face]]
        g = (w[:, :, None] * gt).sum(axis=1)
        out["glen"], out["G"] = np.linalg.norm(g, axis=1), np.abs(gt).max(axis=(1, 2))
        out["normals_vertex"] = g / np.maximum(out["glen"], FLT_EPSILON)[:, None]
    return out


# ------------------------------------------------------------------------------------------------------------ bounds
def area_bound(e1e2):
    return AREA_C * E * np.asarray(e1e2)


def point_bound(M):
    return POINT_C * E * np.asarray(M)


def face_normal_bound(e1e2, nlen):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(nlen >= 2 * FLT_EPSILON, 2 * 6.97 * E * e1e2 / nlen + 3.6 * E, np.inf)


def vertex_normal_bound(G, glen):
    err = np.sqrt(3.0) * POINT_C * E * np.asarray(G)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(glen > err, 2 * err / glen + 3.6 * E, np.inf)


def triangle_variance(a, b, c):
    """per coordinate, the variance of a uniform point of the triangle (a, b, c)"""
    return (a * a + b * b + c * c - a * b - b * c - c * a) / 18.0
