"""The case tables of the point ops (csrc/point_ops.hip behind slide_amd/_ext.py), their references and a mirror of the host dispatch
-- shared by tests/test_point_ops_host.py (the tables and the references themselves, no GPU) and tests/test_hip_point_ops.py (every
row through slide_amd._ext on the GPU).  tests/test_hip_ops.py keeps the golden fixtures and the full-size properties; the rows here
are the smallest shapes that reach each kernel variant and each edge of the dispatch.

References
  (a) oracle.ops, the plain-C oracle: the exact reference of every index op (and of three_interpolate, bit for bit) on any input.
  (b) numpy float64 restatements on DYADIC LATTICE inputs: every coordinate is k / 8 (k / 16 for the off-lattice queries of the
      empty-ball rows), |k| <= 8 (17).  A difference is then a multiple of 1/16 below 2.2, its square a multiple of 1/256 below 4.8
      and a sum of three squares a multiple of 1/256 below 14.4: 12 bits -- exact in fp32 and in float64, in any order, fused or not.
      Kernel, oracle and the restatement below must therefore agree BIT FOR BIT, ties and points on the sphere included (a k / 6
      lattice would not do: 1/6 is not exact).
        ball query              nonzero(d < float64(float32(r) * float32(r)))[:ns], padded with the first hit
        kNN, three_nn           argsort(d, kind="stable")[..., :K]
        sample_farthest_points  running minimum, argmax (lowest index wins)
      furthest_point_sampling keeps the oracle alone: its tie order is the reference's reduction tree.
  (c) gather_points / group_points / gather_rows: numpy indexing (exact).  three_interpolate: the oracle bit for bit, and float64 numpy
      at 3 u sum|p_i w_i| (u = 2^-24): the kernel's fmaf(p3, w3, fmaf(p2, w2, p1 * w1)) rounds three times, each time a value whose
      magnitude is at most sum|p_i w_i| (1 + 2 u).
  (d) the three atomic backward ops against a float64 scatter-add (scatter_ref) at the ORDER-FREE bound
        b = (k + 1) u sum|term|,   k = the number of terms that land on the element,
      derived as follows.  The output starts at 0 and the k atomic additions arrive in an order nobody fixes.  The first addition,
      0 + t, is exact; each of the other k - 1 rounds a partial sum whose magnitude is at most sum|term| (1 + u)^k, so whatever the
      order the additions contribute at most (k - 1) u sum|term| to first order.  three_interpolate_grad's terms are products
      go * w rounded once before they are added: one more u sum|term|, together k u sum|term|.  The last of the k + 1 covers the
      second-order terms (k u << 1 for every row here: k < 2^16) -- so one formula serves the three ops.  k and sum|term| come from
      the same scatter-add run on ones and on absolute values.  k = 0: b = 0, the element must still be exactly 0.
      test_point_ops_host.py checks the bound against fp32 sequential scatter-adds in shuffled orders (it holds) and against the
      sum with its largest term dropped (it is refused).

The dispatch mirror (expected_variant) restates the `if` ladders of the host wrappers in point_ops.hip so that every row can state
the kernel variant it is there for and the host test can assert that the tables reach ALL of them (VARIANTS).  It is a second copy of
the C code and can drift from it: a change to the dispatch in point_ops.hip must change the mirror with it (each predicate names the
line of point_ops.hip it restates, as of this writing).  Pointers are taken as 16-byte aligned -- torch's allocator guarantees it --
except for the operands a row lists as `misaligned`.
"""
import zlib

import numpy as np

from oracle import ops as O

U = 2.0 ** -24


def rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def lattice(rs, *shape, scale=8, lim=8):
    """(*shape, 3) float32 coordinates k / scale, integer |k| <= lim"""
    return (rs.randint(-lim, lim + 1, tuple(shape) + (3,)).astype(np.float64) / scale).astype(np.float32)


def uniform(rs, *shape):
    return rs.uniform(-1, 1, tuple(shape) + (3,)).astype(np.float32)


def misaligned(t):
    """a contiguous copy of the torch tensor t whose data pointer is 4 bytes past a 16-byte boundary (the alignment fallbacks of the
    wrappers: every `(uintptr_t) & 15` test)"""
    flat = t.new_empty(t.numel() + 1)
    flat[1:].copy_(t.reshape(-1))
    return flat[1:].view(t.shape)


# ================================================================================================ the dispatch mirror
def _ceil(a, b):
    return (a + b - 1) // b


def group_lds_plan(b, c, n, slots):
    """launch_group_lds: (qpt, wide, tile, cchunk)"""
    qpt = 4 if slots >= 4096 else (2 if slots >= 2048 else 1)          # point_ops.hip:841  `int qpt = ...`
    while qpt < 16 and qpt * 1024 < 4 * n and slots >= qpt * 2048:      # point_ops.hip:842  the `while`
        qpt *= 2
    wide = qpt == 16 and n >= 8192 and slots >= 65536                   # point_ops.hip:843  `const bool wide`
    tile = qpt * (2048 if wide else 1024)                               # point_ops.hip:844  `const int tile`
    gx = _ceil(slots, tile)                                             # point_ops.hip:845
    chunks = min(max(_ceil(1024, gx * b), 1), c)                        # point_ops.hip:846-847  `int chunks`, clamped to [1, c]
    return qpt, wide, tile, _ceil(c, chunks)                            # point_ops.hip:848  `const int cchunk`


def _lds_name(qpt, wide):
    return "lds_wide" if wide else "lds_q%d" % qpt


def _gather_like(min_slots, b, c, n, slots, mis):
    """gather_points_kernel_wrapper (min_slots 1024) and group_points_kernel_wrapper (2048): the same ladder"""
    if slots % 4 == 0 and not mis & {"idx", "points"} and n <= 16384 and slots >= min_slots:   # point_ops.hip:863 / 955  row-in-LDS
        return _lds_name(*group_lds_plan(b, c, n, slots)[:2])
    if slots % 4 == 0 and "idx" not in mis:                                                     # point_ops.hip:866 / 958  v4
        return "v4"
    return "scalar"                                                                             # point_ops.hip:874 / 965


def three_interpolate_lds_plan(b, c, n):
    """three_interpolate_kernel_wrapper, the LDS branch: (tile, cchunk)"""
    gx = _ceil(n, 2048)                                                 # point_ops.hip:1041
    chunks = min(max(_ceil(1024, gx * b), 1), c)                        # point_ops.hip:1042-1043
    return 2048, _ceil(c, chunks)                                       # point_ops.hip:1044


def _three_interpolate(b, c, m, n, mis):
    """three_interpolate_kernel_wrapper"""
    all_aligned = not mis & {"idx", "weight", "points"}
    if n % 4 == 0 and all_aligned and m <= 16384 and n >= 2048:                                 # point_ops.hip:1039-1040  LDS
        return "lds"
    if n in (256, 512, 1024) and all_aligned and m <= 8192 and \
            (1024 // n) * (((m + 3) & ~3) + 4) * 4 <= 64 * 1024:                                # point_ops.hip:1051-1052  rows, R = 1024 / n
        return "rows_r%d" % (1024 // n)
    if n % 4 == 0 and not mis & {"idx", "weight"}:                                              # point_ops.hip:1063  v4
        return "v4"
    return "scalar"


def fps_class(n):
    """fps_launch: the FPS_LAUNCH ladder and use_lds"""
    if n > 8192:                                                                                 # point_ops.hip:909-911
        return "large"
    for lim, ppt, nt in ((64, 1, 64), (256, 1, 256), (512, 2, 256), (1024, 4, 256), (2048, 8, 256), (4096, 16, 256), (8192, 32, 256)):
        if n <= lim:                                                                             # point_ops.hip:898-908
            return "ppt%d_nt%d_%s" % (ppt, nt, "lds" if n * 12 <= 60000 else "global")             # point_ops.hip:893  `const int use_lds`


def _ball_query(n, ns):
    """query_ball_point_kernel_wrapper"""
    if ns <= 32 and n < 65536:                                          # point_ops.hip:933
        return "staged"
    return "unstaged_ns" if ns > 32 else "unstaged_n"


def _knn(n1, K):
    """slide_knn_points: the KNN_KEY table"""
    if K > 64:                                                          # point_ops.hip:1090  status -2
        return "error"
    if n1 > 64:                                                         # point_ops.hip:1097-1102
        return "nt%d_kt%d" % ((256, 4) if K <= 4 else (256, 8) if K <= 8 else (256, 16) if K <= 16 else (256, 32) if K <= 32 else (128, 64))
    return "nt64_kt%d" % (4 if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64)


def expected_variant(op, misaligned=(), **s):
    """the kernel variant the host dispatch of point_ops.hip launches for a shape (see the module docstring: a mirror, kept in step by
    hand).  `misaligned`: the operands whose pointer is not a multiple of 16."""
    mis = set(misaligned)
    if op == "gather":
        return _gather_like(1024, s["B"], s["C"], s["n"], s["m"], mis)
    if op == "group":
        return _gather_like(2048, s["B"], s["C"], s["n"], s["npoint"] * s["ns"], mis)
    if op == "three_interpolate":
        return _three_interpolate(s["B"], s["C"], s["m"], s["n"], mis)
    if op == "gather_rows":                                                                      # point_ops.hip:1121  `const bool v4`
        return "v4" if s["C"] % 4 == 0 and "points" not in mis else "scalar"
    if op in ("fps", "sfp"):
        return fps_class(s["n"])
    if op == "ball_query":
        return _ball_query(s["n"], s["ns"])
    if op == "knn":
        return _knn(s["n1"], s["K"])
    raise KeyError(op)


VARIANTS = {
    "gather": {"scalar", "v4", "lds_q1"},
    "group": {"scalar", "v4", "lds_q2", "lds_q4", "lds_q8", "lds_q16", "lds_wide"},
    "three_interpolate": {"scalar", "v4", "rows_r4", "rows_r2", "rows_r1", "lds"},
    "ball_query": {"staged", "unstaged_ns", "unstaged_n"},
    "knn": {"nt%d_kt%d" % p for p in ((256, 4), (256, 8), (256, 16), (256, 32), (128, 64), (64, 4), (64, 8), (64, 16), (64, 32), (64, 64))},
    "fps": {"ppt1_nt64_lds", "ppt1_nt256_lds", "ppt2_nt256_lds", "ppt4_nt256_lds", "ppt8_nt256_lds", "ppt16_nt256_lds", "ppt32_nt256_lds",
            "ppt32_nt256_global", "large"},
}
VARIANTS["sfp"] = VARIANTS["fps"]


class Row(dict):
    """a table row: a dict with attribute access; `id` names it in the parametrisation, `target` says what it is there for"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def ids(rows):
    return [r.id for r in rows]


# ================================================================================================ gather / group
def _idx(rs, n, shape):
    """random indices with 0 and n - 1 forced in (first and last slot of every batch element)"""
    idx = rs.randint(0, n, shape).astype(np.int32)
    flat = idx.reshape(shape[0], -1)
    flat[:, 0] = n - 1
    flat[:, -1] = 0
    return idx


def _gg(op, target, variant, B, C, n, npoint, ns=1, ragged=False, cchunk_ragged=False):
    r = Row(op=op, target=target, variant=variant, B=B, C=C, n=n, npoint=npoint, ns=ns, m=npoint, ragged=ragged, cchunk_ragged=cchunk_ragged)
    r["id"] = "%s-%s-B%d-C%d-n%d-%dx%d" % (op, variant, B, C, n, npoint, ns)
    return r


GATHER_ROWS = [
    _gg("gather", "row-in-LDS, one quad per thread, ragged second block, scalar staging (n & 3 != 0)", "lds_q1", 2, 3, 1023, 1028, ragged=True),
    _gg("gather", "row-in-LDS, one quad per thread, one exact tile, 16-byte staging", "lds_q1", 2, 5, 100, 1024),
    _gg("gather", "v4: m % 4 == 0 below the LDS threshold", "v4", 3, 4, 300, 1020),
    _gg("gather", "v4: a single quad", "v4", 1, 2, 5, 4),
    _gg("gather", "scalar: m % 4 != 0, two blocks", "scalar", 2, 3, 77, 257),
    _gg("gather", "scalar: m % 4 != 0 above the LDS threshold", "scalar", 1, 2, 1023, 1029),
]
GROUP_ROWS = [
    _gg("group", "LDS QPT 2, ragged, scalar staging", "lds_q2", 2, 3, 255, 171, 12, ragged=True),
    _gg("group", "LDS QPT 4, ragged, 16-byte staging", "lds_q4", 2, 3, 516, 1025, 4, ragged=True),
    _gg("group", "LDS QPT 8, ragged, scalar staging", "lds_q8", 1, 2, 2050, 683, 12, ragged=True),
    _gg("group", "LDS QPT 16, ragged, 16-byte staging", "lds_q16", 1, 2, 2052, 4097, 4, ragged=True),
    _gg("group", "the wide form <16, 512>, ragged third block", "lds_wide", 1, 2, 8192, 16385, 4, ragged=True),
    _gg("group", "a row of exactly 64 KB of LDS", "lds_q2", 1, 2, 16384, 64, 32),
    _gg("group", "n > 16384 falls to v4", "v4", 1, 2, 16388, 64, 32),
    _gg("group", "LDS with a channel chunk > 1 that does not divide C", "lds_q2", 8, 130, 255, 513, 4, ragged=True, cchunk_ragged=True),
    _gg("group", "v4: slots % 4 == 0 below the LDS threshold", "v4", 2, 5, 300, 51, 20),
    _gg("group", "scalar: slots % 4 != 0", "scalar", 2, 3, 7, 5, 3),
    _gg("group", "scalar: slots % 4 != 0 above the LDS threshold, several blocks", "scalar", 1, 2, 64, 683, 3),
]


def gather_inputs(r):
    """-> points (B,C,n), idx (B,m) for gather or (B,npoint,ns) for group, grad_out of the output's shape"""
    rs = rng(r.id)
    shape = (r.B, r.npoint) if r.op == "gather" else (r.B, r.npoint, r.ns)
    pts = rs.standard_normal((r.B, r.C, r.n)).astype(np.float32)
    idx = _idx(rs, r.n, shape)
    g = rs.standard_normal((r.B, r.C) + shape[1:]).astype(np.float32)
    return pts, idx, g


def gather_ref(pts, idx):
    """out[b, c, ...] = pts[b, c, idx[b, ...]]"""
    B, C = pts.shape[:2]
    flat = idx.reshape(B, 1, -1).astype(np.int64)
    return np.take_along_axis(pts, np.broadcast_to(flat, (B, C, flat.shape[2])), axis=2).reshape((B, C) + idx.shape[1:])


def scatter_ref(terms, idx, n):
    """float64 scatter-add with its bound: terms (B,C,S) float64, idx (B,S) -> (sum (B,C,n), bound (B,C,n)); see (d) above"""
    B, C, S = terms.shape
    bi = np.arange(B)[:, None, None]
    ci = np.arange(C)[None, :, None]
    ii = np.broadcast_to(idx.reshape(B, 1, S).astype(np.int64), (B, C, S))
    out, mag, k = (np.zeros((B, C, n)) for _ in range(3))
    np.add.at(out, (bi, ci, ii), terms)
    np.add.at(mag, (bi, ci, ii), np.abs(terms))
    np.add.at(k, (bi, ci, ii), 1.0)
    return out, np.where(k > 0, (k + 1) * U * mag, 0.0)


def gather_grad_ref(g, idx, n):
    B, C = g.shape[:2]
    return scatter_ref(g.reshape(B, C, -1).astype(np.float64), idx.reshape(B, -1), n)


# ================================================================================================ three_interpolate
def _ti(target, variant, B, C, m, n, ragged=False, cchunk_ragged=False):
    r = Row(op="three_interpolate", target=target, variant=variant, B=B, C=C, m=m, n=n, ragged=ragged, cchunk_ragged=cchunk_ragged)
    r["id"] = "ti-%s-B%d-C%d-m%d-n%d" % (variant, B, C, m, n)
    return r


INTERP_ROWS = [
    _ti("LDS, one exact block, 16-byte staging", "lds", 2, 3, 100, 2048),
    _ti("LDS, scalar staging (m & 3 != 0), ragged second block", "lds", 2, 3, 1023, 2052, ragged=True),
    _ti("LDS, a row of exactly 64 KB", "lds", 1, 2, 16384, 2048),
    _ti("m > 16384 falls to v4", "v4", 1, 2, 16388, 2048),
    _ti("LDS with a channel chunk > 1 that does not divide C", "lds", 8, 130, 255, 2052, ragged=True, cchunk_ragged=True),
    _ti("rows kernel R = 4: m % 4 != 0, C % 4 != 0", "rows_r4", 2, 7, 101, 256),
    _ti("rows kernel R = 2: m % 4 != 0, C odd", "rows_r2", 2, 5, 203, 512),
    _ti("rows kernel R = 1: m % 4 != 0", "rows_r1", 2, 3, 75, 1024),
    _ti("v4", "v4", 2, 4, 100, 300),
    _ti("scalar", "scalar", 1, 3, 3, 5),
    _ti("scalar, several blocks", "scalar", 2, 2, 40, 513),
]


def interp_inputs(r):
    """-> points (B,C,m) N(0,1), idx (B,n,3) random (0 and m - 1 forced in), weight (B,n,3) U(0,1), grad_out (B,C,n)"""
    rs = rng(r.id)
    pts = rs.standard_normal((r.B, r.C, r.m)).astype(np.float32)
    idx = _idx(rs, r.m, (r.B, r.n, 3))
    w = rs.uniform(0, 1, (r.B, r.n, 3)).astype(np.float32)
    g = rs.standard_normal((r.B, r.C, r.n)).astype(np.float32)
    return pts, idx, w, g


def interp_ref(pts, idx, w):
    """float64: (out (B,C,n), bound = 3 u sum|p_i w_i|)"""
    p = gather_ref(pts.astype(np.float64), idx)                    # (B,C,n,3)
    t = p * w.astype(np.float64)[:, None]
    return t.sum(-1), 3 * U * np.abs(t).sum(-1)


def interp_grad_ref(g, idx, w, m):
    """terms go * w, three per output, scattered to idx"""
    B, C, n = g.shape
    t = g.astype(np.float64)[:, :, :, None] * w.astype(np.float64)[:, None]
    return scatter_ref(t.reshape(B, C, n * 3), idx.reshape(B, n * 3), m)


# ================================================================================================ misaligned operands
def _mis(base, op, operand):
    r = Row(base)
    r["op"] = op
    r["misaligned"] = operand
    r["aligned_variant"] = base["variant"]
    kw = dict(r)
    r["variant"] = expected_variant(op, misaligned=(operand,), **{k: kw[k] for k in ("B", "C", "n", "m", "npoint", "ns") if k in kw})
    r["id"] = "%s-mis-%s" % (base["id"] if "id" in base else op, operand)
    return r


_GR = [Row(op="gather_rows", variant="v4", B=2, n=100, m=37, C=8, id="gather_rows-B2-n100-m37-C8")]
# one LDS-eligible and one v4-eligible shape per op, each operand in turn 4 bytes off
MISALIGNED_ROWS = (
    [_mis(GATHER_ROWS[1], "gather", o) for o in ("points", "idx")] + [_mis(GATHER_ROWS[2], "gather", o) for o in ("points", "idx")] +
    [_mis(GROUP_ROWS[0], "group", o) for o in ("points", "idx")] + [_mis(GROUP_ROWS[8], "group", o) for o in ("points", "idx")] +
    [_mis(INTERP_ROWS[0], "three_interpolate", o) for o in ("points", "idx", "weight")] +
    [_mis(INTERP_ROWS[8], "three_interpolate", o) for o in ("points", "idx", "weight")] +
    [_mis(INTERP_ROWS[5], "three_interpolate", o) for o in ("points",)] +
    [_mis(_GR[0], "gather_rows", o) for o in ("points", "idx")])
# what each of them must fall back to
MISALIGNED_EXPECT = {("gather", "lds_q1", "points"): "v4", ("gather", "lds_q1", "idx"): "scalar", ("gather", "v4", "points"): "v4",
                     ("gather", "v4", "idx"): "scalar", ("group", "lds_q2", "points"): "v4", ("group", "lds_q2", "idx"): "scalar",
                     ("group", "v4", "points"): "v4", ("group", "v4", "idx"): "scalar",
                     ("three_interpolate", "lds", "points"): "v4", ("three_interpolate", "lds", "idx"): "scalar",
                     ("three_interpolate", "lds", "weight"): "scalar", ("three_interpolate", "v4", "points"): "v4",
                     ("three_interpolate", "v4", "idx"): "scalar", ("three_interpolate", "v4", "weight"): "scalar",
                     ("three_interpolate", "rows_r4", "points"): "v4",
                     ("gather_rows", "v4", "points"): "scalar", ("gather_rows", "v4", "idx"): "v4"}

GATHER_ROWS_ROWS = _GR + [Row(op="gather_rows", variant="scalar", B=3, n=64, m=300, C=5, id="gather_rows-B3-n64-m300-C5")]


def gather_rows_inputs(r):
    rs = rng(r.id)
    return rs.standard_normal((r.B, r.n, r.C)).astype(np.float32), _idx(rs, r.n, (r.B, r.m))


# ================================================================================================ ball query
def _bq(target, B, n, m, r, ns, kind="lattice"):
    row = Row(op="ball_query", target=target, B=B, n=n, m=m, r=r, ns=ns, kind=kind)
    row["variant"] = _ball_query(n, ns)
    row["id"] = "bq-%s-B%d-n%d-m%d-r%g-ns%d-%s" % (row["variant"], B, n, m, r, ns, kind)
    return row


EDGES = (1, 63, 64, 65, 255, 256, 257)
BALL_ROWS = (
    [_bq("staged, nsample sweep", 2, 300, 70, 0.25, ns) for ns in (1, 3, 8, 32)] +
    [_bq("unstaged, nsample sweep (100: the l += 64 padding loop)", 2, 777, 130, 0.5 if ns < 100 else 0.75, ns) for ns in (33, 48, 64, 100)] +
    [_bq("unstaged, sparse balls: more than 64 unused slots repeat the first hit", 1, 777, 70, 0.25, 100)] +
    [_bq("mostly full balls: truncation at nsample, the r < nsample cut inside a 64-wide step", 1, 1500, 70, 0.25, 3),
     _bq("full and partial balls mixed", 1, 777, 130, 0.5, 33)] +
    [_bq("every 64-step overflows the ball: the cnt >= nsample skip, the wave's early break", 2, 300, 70, 4.0, ns) for ns in (3, 32, 33, 100)] +
    [_bq("empty balls: queries off the lattice points", 2, 300, 200, 2.0 ** -10, ns, "offset") for ns in (32, 33)] +
    [_bq("wave and workgroup edges in m", 1, 300, m, 0.375, ns) for m in EDGES for ns in (5, 40)] +
    [_bq("search-set edges in n (64-wide steps, 256-point chunks)", 1, n, 70, 0.5, ns) for n in EDGES for ns in (5, 40)] +
    [_bq("search-block map: B > 8 and not a multiple of 8", B, 40, 5, 0.5, ns) for B in (9, 17) for ns in (4, 36)] +
    [_bq("16-bit staging at its size boundary: indices above 32767, n - 1 among them", 1, 65535, 3, 0.05, 32, "copies"),
     _bq("n = 65536: unstaged by size", 1, 65536, 3, 0.05, 32, "copies")])


def ball_inputs(row):
    """-> new_xyz (B,m,3), xyz (B,n,3).  lattice: both on the k / 8 lattice; offset: the queries on the k / 8 lattice + 1/16 in every
    coordinate (no search point within 2^-10); copies: the queries are the search points 3, 40000 and n - 1"""
    rs = rng(row.id)
    xyz = lattice(rs, row.B, row.n)
    if row.kind == "copies":
        q = np.ascontiguousarray(xyz[:, [3, 40000, row.n - 1]])
    else:
        q = lattice(rs, row.B, row.m)
        if row.kind == "offset":
            q = q + np.float32(1 / 16)
    return q, xyz


def sqdist64(a, b):
    """(B,p,3), (B,q,3) -> (B,p,q) float64 squared distances (exact on the lattice inputs)"""
    d = a.astype(np.float64)[:, :, None, :] - b.astype(np.float64)[:, None, :, :]
    return (d * d).sum(-1)


def ball_query_np(q, xyz, r, ns):
    d = sqdist64(q, xyz)
    r2 = np.float64(np.float32(r) * np.float32(r))
    B, m = q.shape[:2]
    idx = np.zeros((B, m, ns), np.int32)
    cnt = np.zeros((B, m), np.int32)
    for b in range(B):
        for j in range(m):
            hits = np.nonzero(d[b, j] < r2)[0][:ns]
            if len(hits):
                idx[b, j] = hits[0]
                idx[b, j, :len(hits)] = hits
                cnt[b, j] = len(hits)
    return idx, cnt


def on_sphere_pairs(q, xyz, r):
    return int((sqdist64(q, xyz) == np.float64(np.float32(r) * np.float32(r))).sum())


# ================================================================================================ kNN
K_SWEEP = (1, 3, 4, 5, 8, 9, 12, 16, 17, 20, 32, 33, 50, 64)
_NORM_POINTS = {}
for _a in range(9):
    for _b in range(9):
        for _c in range(9):
            _NORM_POINTS.setdefault(_a * _a + _b * _b + _c * _c, []).append((_a, _b, _c))
N_NORMS = len(_NORM_POINTS)      # 116 distinct squared norms on the lattice: the longest search set without two equal norms


def _kn(target, B, n1, n2, K, kind="lattice", lengths2=None):
    row = Row(op="knn", target=target, B=B, n1=n1, n2=n2, K=K, kind=kind, lengths2=lengths2)
    row["variant"] = _knn(n1, K)
    row["id"] = "knn-%s-B%d-n1_%d-n2_%d-K%d-%s%s" % (row["variant"], B, n1, n2, K, kind, "-len" if lengths2 else "")
    return row


KNN_ROWS = (
    [_kn("n1 <= 64: 64-thread workgroups, K sweep", 2, 64, 517, K) for K in K_SWEEP] +
    [_kn("n1 > 64 with one busy lane in the second tile, K sweep; two tiles and a padded 7-point chunk", 2, 65, 1031, K) for K in K_SWEEP] +
    [_kn("n1 > 64, mid-size, K sweep", 2, 300, 517, K) for K in K_SWEEP] +
    [_kn("ragged lengths2 in one batch: 0, 1, K - 1, K, 513, n2", 6, 65, 1031, 12, lengths2=(0, 1, 11, 12, 513, 1031)),
     _kn("ragged lengths2, 64-thread workgroups, K = 33", 6, 30, 1031, 33, lengths2=(0, 1, 32, 33, 513, 1031)),
     _kn("search-block map", 9, 5, 40, 3), _kn("search-block map", 17, 70, 40, 9)] +
    [_kn("flush order A: p2 by descending norm, queries next to the origin: queues flush at a high rate", 2, 65, 1031, K, "descending")
     for K in (8, 20, 32)] +
    [_kn("flush order B: p2 by ascending norm: next to no flush before the last", 2, 65, 1031, K, "ascending") for K in (8, 20, 32)] +
    [_kn("flush order A, one point per norm: at the origin EVERY candidate beats the K-th, the maximum flush rate", 2, 65, N_NORMS, K,
         "descending_distinct") for K in (8, 20, 32)] +
    [_kn("flush order B, one point per norm: at the origin no candidate past the K-th is queued", 2, 65, N_NORMS, K, "ascending_distinct")
     for K in (8, 20, 32)])
KNN_GATHER_ROW = KNN_ROWS[len(K_SWEEP) + 6]        # n1 65, n2 1031, K 12
KNN_GATHER_U = (1, 11)


def knn_inputs(row):
    """-> p1 (B,n1,3), p2 (B,n2,3), lengths2 (B,) int64 or None; all on the lattice.  descending / ascending: the queries have
    |k| <= 1 and p2 is sorted by its norm; *_distinct: p2 holds one point of every norm the lattice has and every other query is the
    origin itself"""
    rs = rng(row.id)
    if row.kind.endswith("_distinct"):
        p2 = np.array([[_NORM_POINTS[v][rs.randint(len(_NORM_POINTS[v]))] for v in sorted(_NORM_POINTS)] for _ in range(row.B)], np.float64)
        p2 = (p2 * rs.choice([-1.0, 1.0], p2.shape) / 8).astype(np.float32)
    else:
        p2 = lattice(rs, row.B, row.n2)
    if row.kind == "lattice":
        p1 = lattice(rs, row.B, row.n1)
    else:
        p1 = lattice(rs, row.B, row.n1, lim=1)
        if row.kind.endswith("_distinct"):
            p1[:, 0::2] = 0
        nrm = (p2.astype(np.float64) ** 2).sum(-1)
        order = np.argsort(-nrm if row.kind.startswith("descending") else nrm, axis=1, kind="stable")
        p2 = np.ascontiguousarray(np.take_along_axis(p2, order[:, :, None], axis=1))
    l2 = None if row.lengths2 is None else np.array(row.lengths2, np.int64)
    return p1, p2, l2


def knn_np(p1, p2, K, lengths2=None):
    B, n1 = p1.shape[:2]
    d = sqdist64(p1, p2)
    dists = np.zeros((B, n1, K), np.float32)
    idx = np.zeros((B, n1, K), np.int64)
    for b in range(B):
        ln = p2.shape[1] if lengths2 is None else int(lengths2[b])
        c = min(K, ln)
        o = np.argsort(d[b, :, :ln], axis=1, kind="stable")[:, :c]
        idx[b, :, :c] = o
        dists[b, :, :c] = np.take_along_axis(d[b, :, :ln], o, axis=1)
    return dists, idx


def tied_fraction(dists, valid):
    """the share of adjacent output slots (both valid) that hold the same distance"""
    both = valid[..., 1:] & valid[..., :-1]
    return float(((dists[..., 1:] == dists[..., :-1]) & both).sum()) / max(int(both.sum()), 1)


# ================================================================================================ three_nn
def _tn(target, B, n, m, kind="lattice"):
    row = Row(op="three_nn", target=target, B=B, n=n, m=m, kind=kind)
    row["id"] = "tn-B%d-n%d-m%d-%s" % (B, n, m, kind)
    return row


THREE_NN_ROWS = (
    [_tn("tile edge in m (1024 known points per tile)", 2, 70, m) for m in (3, 4, 1024, 1025, 2049)] +
    [_tn("workgroup edge in n", 2, n, 600) for n in (1, 255, 256, 257)] +
    [_tn("search-block map", B, 5, 7) for B in (9, 17)] +
    [_tn("the best three lie in the last, 3-point tile: known by descending norm, unknown at the origin", 2, 70, 2051, "descending")])


def three_nn_inputs(row):
    """-> unknown (B,n,3), known (B,m,3)"""
    rs = rng(row.id)
    known = lattice(rs, row.B, row.m)
    if row.kind == "descending":
        known[:, :3] = np.array([[0, 0, 0.125], [0, 0.125, 0], [0.125, 0, 0]], np.float32)   # the three nearest to the origin ...
        known[:, 3:][(known[:, 3:].astype(np.float64) ** 2).sum(-1) < 0.02] = 1.0          # ... and nothing else as near
        order = np.argsort(-(known.astype(np.float64) ** 2).sum(-1), axis=1, kind="stable")
        known = np.ascontiguousarray(np.take_along_axis(known, order[:, :, None], axis=1))
        unknown = np.zeros((row.B, row.n, 3), np.float32)
        unknown[:, 1::2] = lattice(rs, row.B, row.n, lim=1)[:, 1::2]
    else:
        unknown = lattice(rs, row.B, row.n)
    return unknown, known


def three_nn_np(unknown, known):
    d = sqdist64(unknown, known)
    o = np.argsort(d, axis=2, kind="stable")[:, :, :3]
    return np.take_along_axis(d, o, axis=2).astype(np.float32), o.astype(np.int32)


# ================================================================================================ FPS
def _fp(op, target, B, n, m, kind):
    row = Row(op=op, target=target, B=B, n=n, m=m, kind=kind)
    row["variant"] = fps_class(n)
    row["id"] = "%s-%s-B%d-n%d-m%d-%s" % (op, row["variant"], B, n, m, kind)
    return row


FPS_BOUNDARIES = (64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 5000, 5001, 8192, 8193)
FPS_CLASS_N = (50, 200, 400, 800, 1500, 3000, 4500, 6000, 9000)      # one n inside every class (4500 / 6000: PPT 32 with / without LDS)
FPS_ROWS = (
    [_fp("fps", "class boundary, lattice: ties decided by the reduction tree's order", 3, n, 24, "lattice") for n in FPS_BOUNDARIES] +
    [_fp("fps", "uniform cloud, two points inside the origin ball", 2, n, 24, "uniform") for n in FPS_CLASS_N] +
    [_fp("fps", "exhaustion with an invalid point 0: 0 5 9 20 20 20 20 20", 1, 40, 8, "exhaust_small"),
     _fp("fps", "exhaustion, 512 lanes: 0 300 9 577 5 300 300 300 (bit-reversed lane order alone)", 1, 600, 8, "exhaust_large"),
     _fp("fps", "every point inside the origin ball: all zeros", 2, 100, 8, "all_inside")])
FPS_EXHAUST = {"exhaust_small": (0, 5, 9, 20, 20, 20, 20, 20), "exhaust_large": (0, 300, 9, 577, 5, 300, 300, 300),
               "all_inside": (0,) * 8}
SFP_ROWS = (
    [_fp("sfp", "lattice cloud, starts 0 / n - 1 / random", 3, n, 24, "lattice") for n in FPS_CLASS_N] +
    [_fp("sfp", "uniform cloud, starts 0 / n - 1 / random", 3, n, 24, "uniform") for n in FPS_CLASS_N])


def fps_inputs(row):
    """-> points (B,n,3), and for sample_farthest_points the start indices (B,) int32 = 0, n - 1, random"""
    rs = rng(row.id)
    B, n = row.B, row.n
    if row.kind == "lattice":
        p = lattice(rs, B, n)
    elif row.kind == "uniform":
        p = uniform(rs, B, n)
        if row.op == "fps":
            p[:, 3] = 0.001
            p[:, n // 2] = -0.01
    else:                                                  # everything inside the origin ball (|p|^2 <= 1e-3) ...
        p = (rs.uniform(-0.01, 0.01, (B, n, 3))).astype(np.float32)
        if row.kind == "exhaust_small":                    # ... except three / four points, ever nearer to point 0
            p[:, 5], p[:, 9], p[:, 20] = (1, 0, 0), (-0.875, 0, 0), (0, 0.75, 0)
        elif row.kind == "exhaust_large":
            p[:, 300], p[:, 9], p[:, 577], p[:, 5] = (1, 0, 0), (-0.875, 0, 0), (0, 0.75, 0), (0, -0.5, 0)
    start = np.array([0, n - 1, rs.randint(0, n)][:B], np.int32) if row.op == "sfp" else None
    return p, start


def sfp_np(points, K, start):
    """plain farthest point sampling: running minimum of the squared distances, argmax (the lowest index wins a tie)"""
    B, n = points.shape[:2]
    p = points.astype(np.float64)
    idx = np.zeros((B, K), np.int64)
    for b in range(B):
        md = np.full(n, 1e10)
        old = int(start[b])
        idx[b, 0] = old
        for j in range(1, K):
            md = np.minimum(md, ((p[b] - p[b, old]) ** 2).sum(-1))
            old = int(np.argmax(md))
            idx[b, j] = old
    return idx


# ================================================================================================ references, computed once
_CACHE = {}


def reference(row):
    """the oracle's answer for a row (every op but the float64-bounded backward ops), computed once and shared; the arrays are
    read-only"""
    if row.id in _CACHE:
        return _CACHE[row.id]
    op = row.op
    if op == "ball_query":
        q, xyz = ball_inputs(row)
        ref = O.ball_query(q, xyz, row.r, row.ns)
    elif op == "knn":
        p1, p2, l2 = knn_inputs(row)
        ref = O.knn_points(p1, p2, row.K, l2)
    elif op == "three_nn":
        ref = O.three_nn(*three_nn_inputs(row))
    elif op == "fps":
        ref = (O.furthest_point_sampling(fps_inputs(row)[0], row.m),)
    elif op == "sfp":
        p, start = fps_inputs(row)
        ref = (O.sample_farthest_points(p, row.m, start)[1],)
    elif op == "three_interpolate":
        pts, idx, w, _ = interp_inputs(row)
        ref = (O.three_interpolate(pts, idx, w),)
    else:
        raise KeyError(op)
    for a in ref:
        a.setflags(write=False)
    _CACHE[row.id] = ref
    return ref
