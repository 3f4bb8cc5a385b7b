"""The SLIDE_OP_TRANSPOSE / SLIDE_OP_GROUPNORM_NCHW case tables without a GPU (tests/nchw_cases.py): the mutants each expected
result must tell apart, the shapes the tables reach.  The GPU half is tests/test_hip_nchw_ops.py."""
import numpy as np

import nchw_cases as nc
from op_harness import SENTINEL, bits


def test_transpose_expectations_see_the_mutants():
    seen = set()
    for c in nc.TR_CASES:
        d = nc.tr_data(c)
        want = nc.tr_expected(c, d, SENTINEL)
        n_in, n_out = nc.tr_sizes(c)
        assert d["buf"].size == n_in and want.size == n_out
        assert int((bits(want) != bits(want.dtype.type(SENTINEL))).sum()) <= c["B"] * c["R"] * c["C"]
        for m in nc.tr_mutants(c):
            got = nc.tr_expected(c, d, SENTINEL, mutant=m)
            assert got is None or (bits(got) != bits(want)).any(), (c["name"], m)
            seen.add(m)
    assert seen == {"swap_ld", "batch_stride_of_other_side", "tile_edge_off_by_one", "truncate_fp16"}


def test_transpose_matrix_reaches_every_shape():
    shapes = {(c["B"], c["R"], c["C"]) for c in nc.TR_CASES}
    assert {(1, 1, 1), (2, 33, 31), (3, 32, 64), (2, 65, 40), (1, 16, 1568)} <= shapes
    assert all({c["f16"] for c in nc.TR_CASES if (c["B"], c["R"], c["C"]) == s} == {False, True} for s in shapes)
    assert any(c["in_ld"] > c["C"] for c in nc.TR_CASES) and any(c["out_ld"] > c["R"] for c in nc.TR_CASES)
    assert any(c["in_bs"] > c["R"] * c["in_ld"] and c["out_bs"] > c["C"] * c["out_ld"] for c in nc.TR_CASES)
    # HipConv1x1.forward: i = (B, C, P, P, kp, C P, P kp, half) and (B, P, O, op_, P, P op_, O P)
    B, C, O, P = 2, 35, 51, 50
    a, b = nc.TR_BY_NAME["conv_in_f16"], nc.TR_BY_NAME["conv_out_f32"]
    assert [a[k] for k in ("B", "R", "C", "in_ld", "out_ld", "in_bs", "out_bs")] == [B, C, P, P, nc.ru(C), C * P, P * nc.ru(C)]
    assert [b[k] for k in ("B", "R", "C", "in_ld", "out_ld", "in_bs", "out_bs")] == [B, P, O, nc.ru(O), P, P * nc.ru(O), O * P]


def test_transpose_data_holds_the_rounding_edges():
    """ties both ways, subnormals, the largest finite value, the tie that becomes inf, -0.0 and NaN are among the fp16 results"""
    c = nc.TR_BY_NAME["b2_33x31_f16"]
    x = nc.tr_data(c)["x"].reshape(-1)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    hb = set(bits(h).tolist())
    assert {0x3c00, 0x3c02, 0xbc00, 0x6800, 0x6802, 0x0000, 0x0001, 0x0002, 0x7bff, 0xfbff, 0x7c00, 0x8000, 0x7e00} <= hb, sorted(hb)[:8]
    assert np.isnan(x).sum() == 1 and (bits(x) == 0x80000000).sum() == 1


def test_groupnorm_bounds_see_the_mutants():
    seen = {}
    for c in nc.GN_CASES:
        d = nc.gn_data(c)
        ref = nc.gn_forward(c, d)
        n_norm = c["n_norm"]
        assert np.isfinite(ref["b"]).all() and (ref["b"][:, :n_norm] > 0).all() and (ref["b"][:, n_norm:] == 0).all()
        assert nc.ratio(ref, ref["stored"]).max() <= 1
        tail = d["x"][:, n_norm:].astype(np.float64)
        assert (ref["y"][:, n_norm:] == (np.maximum(tail, 0) if c["relu"] else tail)).all()
        for m in nc.gn_mutants(c):
            seen[(c["name"], m)] = float(nc.ratio(ref, nc.gn_forward(c, d, mutant=m)["stored"]).max())
    assert {m for _, m in seen} == {"unbiased_var", "tail_normalised", "tail_relu_dropped", "neighbour_sample", "gamma_within_group",
                                    "count_hw_only"}
    unseen = []
    for (name, m), r in seen.items():
        if (name, m) in nc.GN_EXEMPT:
            assert seen[(nc.GN_EXEMPT[(name, m)], m)] > 1, (name, m)
        elif not r > 1:
            unseen.append((name, m, round(r, 3)))
    assert not unseen, "the bound does not see (case, mutant, max deviation / bound): %s" % unseen
    assert not [k for k in nc.GN_EXEMPT if k not in seen], "stale exemptions"


def test_groupnorm_matrix_reaches_every_branch():
    cs = nc.GN_CASES
    n = lambda c: c["n_norm"] // c["G"] * c["HW"]
    assert {64, 300, 4096} <= {n(c) for c in cs}
    assert any(c["HW"] == 1 and c["n_norm"] // c["G"] == 4 for c in cs) and any(c["G"] == 1 for c in cs) and any(c["B"] == 3 for c in cs)
    assert {(c["n_norm"] < c["C"], c["relu"]) for c in cs} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c["dist"] for c in cs} == {"normal", "common", "const"}
    # the constant group: variance exactly 0 in the reference, output beta, and a bound that says how near
    c = nc.GN_BY_NAME["const_group"]
    d = nc.gn_data(c)
    ref = nc.gn_forward(c, d)
    gs = c["n_norm"] // c["G"]
    assert np.allclose(ref["y"][:, gs:2 * gs], d["beta"][gs:2 * gs, None].astype(np.float64), rtol=0, atol=1e-12)
    # (rstd = 1 / sqrt(eps), x = m = 3.7, d = ceil(log2 200) + 2 = 10: |gamma| rstd (12 u 3.7) + 3 u (2 * 3.7 |gamma| rstd + |beta|) + u |beta|)
    gmax, bmax, rstd = np.abs(d["gamma"][gs:2 * gs]).max(), np.abs(d["beta"][gs:2 * gs]).max(), 1 / np.sqrt(nc.EPS)
    assert 0 < ref["b"][:, gs:2 * gs].max() <= (18 * 3.7 * gmax * rstd + 4 * bmax) * nc.U * (1 + 1e-6)
