"""The tables and references of tests/point_ops_cases.py, checked without a GPU: on the lattice rows the numpy restatements equal the
oracle bit for bit; the tables reach every kernel variant the dispatch mirror knows and stay inside the caps that keep them hard
(full / partial / empty balls, points on the sphere, tied neighbours); the ragged rows are ragged; the misaligned helper misaligns;
the scatter-add bound holds for shuffled fp32 sums and refuses a dropped term."""
import numpy as np
import pytest
import torch

import point_ops_cases as PC
from oracle import ops as O


# ------------------------------------------------------------------------------------------------ numpy restatements == oracle
@pytest.mark.parametrize("row", PC.BALL_ROWS, ids=PC.ids(PC.BALL_ROWS))
def test_ball_query_numpy_equals_oracle(row):
    q, xyz = PC.ball_inputs(row)
    idx, cnt = PC.ball_query_np(q, xyz, row.r, row.ns)
    ri, rc = PC.reference(row)
    assert np.array_equal(idx, ri) and np.array_equal(cnt, rc), (row.id, row.target)


@pytest.mark.parametrize("row", PC.KNN_ROWS, ids=PC.ids(PC.KNN_ROWS))
def test_knn_numpy_equals_oracle(row):
    p1, p2, l2 = PC.knn_inputs(row)
    d, i = PC.knn_np(p1, p2, row.K, l2)
    rd, ri = PC.reference(row)
    assert np.array_equal(i, ri) and np.array_equal(d, rd), (row.id, row.target)


@pytest.mark.parametrize("row", PC.THREE_NN_ROWS, ids=PC.ids(PC.THREE_NN_ROWS))
def test_three_nn_numpy_equals_oracle(row):
    u, k = PC.three_nn_inputs(row)
    d, i = PC.three_nn_np(u, k)
    rd, ri = PC.reference(row)
    assert np.array_equal(i, ri) and np.array_equal(d, rd), (row.id, row.target)
    if row.kind == "descending":          # the best three are the last three known points, in the last (3-point) tile
        assert row.m % 1024 == 3 and np.array_equal(ri[:, 0], np.broadcast_to(np.arange(row.m - 3, row.m), (row.B, 3)))


@pytest.mark.parametrize("row", [r for r in PC.SFP_ROWS if r.kind == "lattice"], ids=PC.ids([r for r in PC.SFP_ROWS if r.kind == "lattice"]))
def test_sample_farthest_points_numpy_equals_oracle(row):
    p, start = PC.fps_inputs(row)
    assert start[0] == 0 and start[1] == row.n - 1
    assert np.array_equal(PC.sfp_np(p, row.m, start), PC.reference(row)[0]), row.id


def test_gather_and_interpolate_references_equal_oracle():
    """numpy indexing == the oracle's loops; the float64 three_interpolate holds the oracle's fp32 result inside its bound"""
    for r in PC.GATHER_ROWS + PC.GROUP_ROWS:
        pts, idx, _ = PC.gather_inputs(r)
        assert np.array_equal(PC.gather_ref(pts, idx), (O.gather_points if r.op == "gather" else O.group_points)(pts, idx)), r.id
    for r in PC.GATHER_ROWS_ROWS:
        pts, idx = PC.gather_rows_inputs(r)
        assert np.array_equal(np.take_along_axis(pts, idx[:, :, None].astype(np.int64), axis=1), O.gather_rows(pts, idx)), r.id
    for r in PC.INTERP_ROWS:
        pts, idx, w, _ = PC.interp_inputs(r)
        ref, bound = PC.interp_ref(pts, idx, w)
        assert (np.abs(PC.reference(r)[0] - ref) <= bound).all(), r.id


# ------------------------------------------------------------------------------------------------ the tables stay hard
def _ball_stats(rows):
    full = partial = empty = total = sphere = 0
    for row in rows:
        q, xyz = PC.ball_inputs(row)
        cnt = PC.reference(row)[1]
        full += int((cnt == row.ns).sum())
        empty += int((cnt == 0).sum())
        partial += int(((cnt > 0) & (cnt < row.ns)).sum())
        total += cnt.size
        sphere += PC.on_sphere_pairs(q, xyz, row.r)
    return full / total, partial / total, empty / total, sphere


@pytest.mark.parametrize("staged", [True, False], ids=["staged", "unstaged"])
def test_ball_tables_fill_truncate_and_miss(staged):
    """across the staged rows, and across the unstaged ones: >= 10 % of the balls full, >= 10 % partial, >= 10 % empty, and at least 50
    (query, point) pairs exactly on the sphere"""
    rows = [r for r in PC.BALL_ROWS if (r.variant == "staged") == staged]
    full, partial, empty, sphere = _ball_stats(rows)
    print("ball rows staged=%s: full %.3f partial %.3f empty %.3f on-sphere pairs %d" % (staged, full, partial, empty, sphere))
    assert full >= 0.10 and partial >= 0.10 and empty >= 0.10 and sphere >= 50


def test_ball_named_rows_are_what_they_say():
    by = {}
    for r in PC.BALL_ROWS:
        by.setdefault(r.target.split(":")[0], []).append(r)
    (mostly,) = by["mostly full balls"]
    assert (PC.reference(mostly)[1] == mostly.ns).mean() >= 0.9
    (mix,) = by["full and partial balls mixed"]
    c = PC.reference(mix)[1]
    assert (c == mix.ns).mean() >= 0.25 and ((c > 0) & (c < mix.ns)).mean() >= 0.25
    for r in by["every 64-step overflows the ball"]:
        assert (PC.reference(r)[1] == r.ns).all()
    for r in by["empty balls"]:
        assert (PC.reference(r)[1] == 0).all() and not PC.reference(r)[0].any()
    for r in PC.BALL_ROWS:
        if r.kind == "copies":        # indices beyond 15 bits, the last point among them
            idx = PC.reference(r)[0]
            assert idx.max() == r.n - 1 and (idx > 32767).sum() >= 3 and r.n in (65535, 65536)
    assert any(r.ns > 64 and ((PC.reference(r)[1] > 0) & (PC.reference(r)[1] < r.ns - 64)).any() for r in PC.BALL_ROWS), \
        "no row pads more than 64 slots of a ball"


def test_knn_and_three_nn_tables_are_full_of_ties():
    """>= 30 % of adjacent output slots tied, across the kNN rows and across the three_nn rows"""
    num = den = 0
    for row in PC.KNN_ROWS:
        d = PC.reference(row)[0]
        ln = np.full(row.B, row.n2) if row.lengths2 is None else np.array(row.lengths2)
        valid = np.arange(row.K)[None, None, :] < np.minimum(ln, row.K)[:, None, None]
        valid = np.broadcast_to(valid, d.shape)
        both = valid[..., 1:] & valid[..., :-1]
        num += int(((d[..., 1:] == d[..., :-1]) & both).sum())
        den += int(both.sum())
    print("kNN rows: tied adjacent slots %.3f" % (num / den))
    assert num / den >= 0.30
    num = den = 0
    for row in PC.THREE_NN_ROWS:
        d = PC.reference(row)[0]
        num += int((d[..., 1:] == d[..., :-1]).sum())
        den += d[..., 1:].size
    print("three_nn rows: tied adjacent slots %.3f" % (num / den))
    assert num / den >= 0.30


def test_knn_flush_order_rows():
    """the share of candidates past the first K that beat the K-th best of those before them (an up-to-date version of what the
    kernel queues).  One point per norm and a query at the origin: all of them (descending), none (ascending).  The 1031-point rows
    have shells of equal norms and queries next to the origin, so they are measured against a random order of the same points, where
    candidate j beats the K-th best with probability K / j: E = K (H(n2) - H(K)) / (n2 - K); descending >= 3 E, ascending <= E / 3"""
    assert PC.N_NORMS == 116
    for row in PC.KNN_ROWS:
        if row.kind == "lattice":
            continue
        p1, p2, _ = PC.knn_inputs(row)
        d = PC.sqdist64(p1[:1], p2[:1])[0]
        beats = np.array([d[:, j] < np.partition(d[:, :j], row.K - 1, axis=1)[:, row.K - 1] for j in range(row.K, row.n2)])  # (j, query)
        print(row.id, "candidates that beat the K-th best so far: %.3f" % beats.mean())
        if row.kind.endswith("_distinct"):
            assert row.n2 == PC.N_NORMS and not p1[:, 0::2].any()
            assert beats[:, 0::2].all() if row.kind.startswith("descending") else not beats[:, 0::2].any()
        else:
            E = row.K * sum(1.0 / j for j in range(row.K + 1, row.n2 + 1)) / (row.n2 - row.K)
            assert beats.mean() >= 3 * E if row.kind == "descending" else beats.mean() <= E / 3


def test_fps_exhaustion_rows():
    for row in PC.FPS_ROWS:
        if row.kind in PC.FPS_EXHAUST:
            ref = PC.reference(row)[0]
            assert all(tuple(r) == PC.FPS_EXHAUST[row.kind] for r in ref.tolist()), (row.id, ref)
        if row.kind == "uniform":
            p = PC.fps_inputs(row)[0].astype(np.float64)
            assert (((p ** 2).sum(-1) <= 1e-3).sum(1) >= 2).all()


# ------------------------------------------------------------------------------------------------ coverage of the dispatch
def _variant(r):
    return PC.expected_variant(r.op, **{k: r[k] for k in ("B", "C", "n", "m", "npoint", "ns", "n1", "K") if k in r})


@pytest.mark.parametrize("op,rows", [("gather", PC.GATHER_ROWS), ("group", PC.GROUP_ROWS), ("three_interpolate", PC.INTERP_ROWS),
                                     ("ball_query", PC.BALL_ROWS), ("knn", PC.KNN_ROWS), ("fps", PC.FPS_ROWS), ("sfp", PC.SFP_ROWS)],
                         ids=["gather", "group", "three_interpolate", "ball_query", "knn", "fps", "sfp"])
def test_tables_reach_every_variant(op, rows):
    """every row reaches the variant it names, and together the rows reach all of them"""
    for r in rows:
        assert _variant(r) == r.variant, (r.id, r.target)
    assert {r.variant for r in rows} == PC.VARIANTS[op]


def test_variant_lists():
    assert len(PC.VARIANTS["knn"]) == 10 and len(PC.VARIANTS["fps"]) == 9
    assert {PC.fps_class(n) for n in PC.FPS_BOUNDARIES} == PC.VARIANTS["fps"]          # both sides of every switch
    assert {PC.fps_class(n) for n in PC.FPS_CLASS_N} == PC.VARIANTS["fps"]
    for lo in (64, 256, 512, 1024, 2048, 4096, 5000, 8192):
        assert PC.fps_class(lo) != PC.fps_class(lo + 1) and {lo, lo + 1} <= set(PC.FPS_BOUNDARIES)
    for n1 in (64, 65, 300):
        assert {PC.expected_variant("knn", n1=n1, K=K) for K in PC.K_SWEEP} == \
            {"nt%d_kt%d" % (64 if n1 <= 64 else 128 if kt == 64 else 256, kt) for kt in (4, 8, 16, 32, 64)}
    assert PC.expected_variant("knn", n1=5, K=65) == "error"
    assert PC.expected_variant("ball_query", n=65535, ns=32) == "staged" and PC.expected_variant("ball_query", n=65536, ns=32) == "unstaged_n"


def test_ragged_rows_are_ragged():
    n_staging = set()
    for r in PC.GATHER_ROWS + PC.GROUP_ROWS:
        if not r.variant.startswith("lds"):
            continue
        slots = r.npoint * r.ns
        qpt, wide, tile, cchunk = PC.group_lds_plan(r.B, r.C, r.n, slots)
        n_staging.add((r.op, r.n & 3 == 0))
        assert r.n <= 16384
        if r.ragged:
            assert 0 < slots % tile < tile and slots > tile, r.id      # a last block with fewer slots than its tile, after a whole one
        else:
            assert slots % tile == 0, r.id
        assert r.cchunk_ragged == (cchunk > 1 and r.C % cchunk != 0), (r.id, cchunk)
    assert n_staging == {("gather", True), ("gather", False), ("group", True), ("group", False)}
    assert any(r.cchunk_ragged for r in PC.GROUP_ROWS)
    m_staging = set()
    for r in PC.INTERP_ROWS:
        if r.variant != "lds":
            continue
        tile, cchunk = PC.three_interpolate_lds_plan(r.B, r.C, r.n)
        m_staging.add(r.m & 3 == 0)
        assert r.ragged == (r.n % tile != 0), r.id
        assert r.cchunk_ragged == (cchunk > 1 and r.C % cchunk != 0), (r.id, cchunk)
    assert m_staging == {True, False} and any(r.cchunk_ragged for r in PC.INTERP_ROWS)
    for r in PC.INTERP_ROWS:
        if r.variant.startswith("rows"):
            R = int(r.variant[-1])
            assert r.m % 4 != 0 and (R == 1 or r.C % R != 0), r.id
    # the 64 KB rows and their neighbours on the other side of the limit
    assert {(r.n, r.variant) for r in PC.GROUP_ROWS if r.n >= 16384} == {(16384, "lds_q2"), (16388, "v4")}
    assert {(r.m, r.variant) for r in PC.INTERP_ROWS if r.m >= 16384} == {(16384, "lds"), (16388, "v4")}


def test_misaligned_rows():
    t = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    assert t.data_ptr() % 16 == 0
    u = PC.misaligned(t)
    assert u.data_ptr() % 16 == 4 and u.is_contiguous() and torch.equal(u, t) and u.shape == t.shape
    i = PC.misaligned(torch.arange(8, dtype=torch.int32).view(2, 4))
    assert i.data_ptr() % 16 == 4 and i.dtype == torch.int32
    seen = set()
    for r in PC.MISALIGNED_ROWS:
        key = (r.op, r.aligned_variant, r.misaligned)
        assert r.variant == PC.MISALIGNED_EXPECT[key], r.id
        seen.add(key)
    assert seen == set(PC.MISALIGNED_EXPECT)
    for op in ("gather", "group", "three_interpolate"):   # one LDS-eligible and one v4-eligible shape each
        assert {k[1][:3] for k in seen if k[0] == op} >= {"lds", "v4"}


# ------------------------------------------------------------------------------------------------ the scatter-add bound
def _shuffled_f32_scatter(terms, idx, n, rs):
    """fp32 scatter-add of terms (B,C,S) to idx (B,S), one addition at a time in a shuffled order: a stand-in for the atomics' order"""
    B, C, S = terms.shape
    out = np.zeros((B, C, n), np.float32)
    order = rs.permutation(S)
    bi = np.arange(B)[:, None, None]
    ci = np.arange(C)[None, :, None]
    ii = np.broadcast_to(idx.reshape(B, 1, S).astype(np.int64)[:, :, order], (B, C, S))
    np.add.at(out, (bi, ci, ii), terms[:, :, order].astype(np.float32))
    return out


def _bound_cases():
    for r in (PC.GATHER_ROWS[0], PC.GROUP_ROWS[0], PC.GROUP_ROWS[10]):
        _, idx, g = PC.gather_inputs(r)
        yield r.id, g.reshape(r.B, r.C, -1), idx.reshape(r.B, -1), r.n
    for r in (PC.INTERP_ROWS[1], PC.INTERP_ROWS[8]):
        _, idx, w, g = PC.interp_inputs(r)
        t = (g[:, :, :, None] * w[:, None]).astype(np.float32)           # the kernel's rounded products
        yield r.id, t.reshape(r.B, r.C, -1), idx.reshape(r.B, -1), r.m


def test_scatter_bound_holds_and_bites():
    rs = np.random.RandomState(3)
    worst = 0.0
    for name, terms, idx, n in _bound_cases():
        if "ti-" in name:      # the reference multiplies in float64; the fp32 products above carry the term's own rounding
            r = next(r for r in PC.INTERP_ROWS if r.id == name)
            _, ii, w, g = PC.interp_inputs(r)
            ref, bound = PC.interp_grad_ref(g, ii, w, n)
        else:
            ref, bound = PC.scatter_ref(terms.astype(np.float64), idx, n)
        assert (bound[ref == 0] >= 0).all() and (bound > 0).any()
        for _ in range(3):
            got = _shuffled_f32_scatter(terms, idx, n, rs)
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
            assert (got[bound == 0] == 0).all()
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        # a sum that lost its largest term is outside the bound
        b, c, s = np.unravel_index(np.argmax(np.abs(terms)), terms.shape)
        mutant = ref.copy()
        mutant[b, c, idx[b, s]] -= np.float64(terms[b, c, s])
        assert np.abs(mutant - ref)[b, c, idx[b, s]] > bound[b, c, idx[b, s]], name
    print("shuffled fp32 scatter-adds: worst err / bound %.3f" % worst)
    assert 0.0 < worst <= 1.0     # the roundings are there, and inside the bound
