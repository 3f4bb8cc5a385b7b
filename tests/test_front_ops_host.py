"""The step-front launches on the CPU (tests/front_cases.py): the case tables reach every listed edge, the tied / excluded shares of
the committed seeds hold, every mutant misses its check and the references agree with the oracle where there is one.
(tests/test_hip_front_ops.py holds the kernels to the same references and bounds.)"""
import numpy as np
import pytest

import front_cases as fc
from front_cases import F16, F32

MAX_EXCLUDED = 0.01  # the share of Gaussian slots whose order the distances do not decide (the issue's limit)


# ------------------------------------------------------------------------------------------------------------ PREP_POINTS
def test_prep_table_reaches_every_listed_edge():
    col = lambda k: {c[k] for c in fc.PREP_CASES}
    assert col("B") == {1, 3, 17} and col("cx") == {3, 6, 51} and col("f16") == {False, True} and col("cm") == {False, True}
    assert col("copies") == {"none", "one", "three"} and col("kw") == {False, True} and col("cloud") == {"lattice", "lattice64", "gauss"}
    for c in fc.PREP_CASES:
        assert c["ldf"] > c["cx"]
        cps = fc.prep_copies(c)
        assert all(n < c["cx"] for n, _, kind in cps if kind == 0) and all(n == 3 for n, _, kind in cps if kind == 1)
        assert all(ld >= n for n, ld, _ in cps)
    assert [k for _, _, k in fc.prep_copies(fc.PREP_CASES[2])] == [0, 1, 0]


@pytest.mark.parametrize("c", [c for c in fc.PREP_CASES if c["cloud"] in fc.LATTICES], ids=lambda c: c["name"])
def test_prep_lattice_reference_is_the_oracle_and_full_of_ties(c):
    from oracle import ops as O
    x = fc.prep_inputs(c)
    ref = fc.prep_reference(c, x)
    xyz = np.ascontiguousarray(x[:, :, :3])
    dists, idx = O.knn_points(xyz, xyz, 16)
    assert (ref["kidx"] == idx).all() and (ref["kd2"].view(np.uint32) == dists.view(np.uint32)).all()
    assert (ref["kd2"].astype(np.float64) == ref["kd2_64"]).all()  # (the float32 distances are exact on the lattice)
    share = fc.tied_share(ref["kd2"])
    dup = float((ref["kd2"][..., 1] == 0).mean())
    print("prep %s: tied adjacent slots %.3f, points with a duplicate %.3f" % (c["name"], share, dup))
    assert share > 0.25 and dup >= 3 / 16


@pytest.mark.parametrize("c", [c for c in fc.PREP_CASES if c["cloud"] == "gauss"], ids=lambda c: c["name"])
def test_prep_gauss_excluded_share(c):
    ref = fc.prep_reference(c, fc.prep_inputs(c))
    ok = fc.decided_slots(ref["kd2_64"])
    excl = 1.0 - float(ok.mean())
    print("prep %s: excluded slots %.5f" % (c["name"], excl))
    assert excl <= MAX_EXCLUDED
    # the float32 restatement of the kernel's distances is inside the bound it is held to
    d32 = np.take_along_axis(fc.d2_f32(fc.prep_inputs(c)[:, :, :3]).astype(np.float64), ref["kidx_64"].astype(np.int64), -1)
    assert (np.abs(d32 - ref["kd2_64"]) <= fc.d2_bound(ref["kd2_64"])).all()


@pytest.mark.parametrize("c", fc.PREP_CASES, ids=lambda c: c["name"])
def test_prep_checks_see_the_mutants(c):
    x = fc.prep_inputs(c)
    ref = fc.prep_reference(c, x)
    if c["cloud"] in fc.LATTICES:
        m = fc.prep_reference(c, x, "tie_larger_index")
        assert (m["kidx"] != ref["kidx"]).any() and (m["kd2"] == ref["kd2"]).all()  # (only the order of the ties differs)
    for mut in ("kw_over_16", "kw_by_neighbour"):
        m = fc.prep_reference(c, x, mut)
        r = np.abs(m["kw"] - ref["kw"])[..., :8] / (fc.KW_ULPS * fc.U * ref["kw"][..., :8])
        print("prep %s %s: %.3g bounds" % (c["name"], mut, r.max()))
        if mut == "kw_by_neighbour" or c["cloud"] == "lattice64":  # (kw_over_16 elsewhere: front_cases.LATTICES)
            assert r.max() > 1, (mut, r.max())
    if c["cx"] > 3:  # (cx 3: there are no features, the two halves are the same three columns)
        m = fc.prep_reference(c, x, "feat_halves_swapped")
        assert (m["feat0"] != ref["feat0"]).any() and (m["feat0_cm"] != ref["feat0_cm"]).any()
        assert any((a != b).any() for a, b, (_, _, kind) in zip(m["copies"], ref["copies"], fc.prep_copies(c)) if kind == 0) or c["copies"] == "none"


# ------------------------------------------------------------------------------------------------------------ TEMB / COND
def test_temb_and_cond_tables_reach_every_listed_edge():
    col = lambda k: {c[k] for c in fc.TEMB_CASES}
    assert col("nsamp") == {1, 5} and col("t_dim") == {32, 128} and col("n_out") == {40, 600}
    assert 4 * 32 < 256 < 4 * 128  # H = 4 t_dim fits one pass of 256 threads and exceeds it
    ts = {t for c in fc.TEMB_CASES if c["ts"] for t in c["ts"]}
    assert {0.0, 1.0, 999.0} <= ts and any(c["ts"] is None for c in fc.TEMB_CASES)
    col = lambda k: {c[k] for c in fc.COND_CASES}
    assert col("B") == {1, 5} and col("dim") == {8, 128} and col("n_out") == {40, 600}
    labels = {int(v) for c in fc.COND_CASES for v in fc.cond_inputs(c)["label"]}
    assert {0, fc.NCLS - 1} <= labels


@pytest.mark.parametrize("c", fc.TEMB_CASES, ids=lambda c: c["name"])
def test_temb_bound_sees_the_mutants(c):
    d = fc.temb_inputs(c)
    ref, b = fc.temb_forward(c, d)
    assert np.isfinite(ref).all() and (b > 0).all()
    for m in fc.TEMB_MUTANTS:
        r = (np.abs(fc.temb_forward(c, d, m)[0].astype(F32).astype(np.float64) - ref) / b).max()
        print("temb %s %s: %.3g bounds" % (c["name"], m, r))
        assert r > 1, (m, r)
    # a float32 evaluation in the kernel's order of operations is inside the bound
    assert (np.abs(_temb_f32(c, d) - ref) <= b).all()


def _temb_f32(c, d):
    t = np.array(c["ts"] if c["ts"] is not None else [float(fc.T_DEV0)], F32)
    arg = t[:, None] * d["freq"][None, :]
    x = np.concatenate([np.sin(arg), np.cos(arg)], 1).astype(F32)
    sw = lambda v: (v * (F32(1) / (F32(1) + np.exp(-v)))).astype(F32)
    h1 = sw(d["b1"] + x @ d["w1"])
    h2 = sw(d["b2"] + h1 @ d["w2"])
    return (d["bfc"] + h2 @ d["wfc"]).astype(np.float64)


@pytest.mark.parametrize("c", fc.COND_CASES, ids=lambda c: c["name"])
def test_cond_bound_sees_the_mutants(c):
    d = fc.cond_inputs(c)
    ref, b = fc.cond_forward(c, d)
    for m in fc.COND_MUTANTS:
        r = (np.abs(fc.cond_forward(c, d, m)[0].astype(F32).astype(np.float64) - ref) / b).max()
        print("cond %s %s: %.3g bounds" % (c["name"], m, r))
        assert r > 1, (m, r)
    got = (d["bfc"] + d["emb"][d["label"]] @ d["wfc"]).astype(np.float64)
    assert (np.abs(got - ref) <= b).all()


# ------------------------------------------------------------------------------------------------------------ FINALIZE_GN
@pytest.mark.parametrize("c", fc.FIN_CASES, ids=lambda c: c["name"])
def test_finalize_bound_sees_the_mutants(c):
    d = fc.fin_inputs(c)
    scl, sft, dscl, dsft, var = fc.fin_forward(c, d)  # (asserts the first-order regime)
    assert fc.FIN_BS > fc.FIN_C and (d["gid"] == -1).any()
    lens = [b - a for a, b in fc.FIN_RUNS]
    assert len(set(lens)) > 2 and any(a // fc.PRODUCER != (b - 1) // fc.PRODUCER for a, b in fc.FIN_RUNS)  # unequal, straddling
    assert (var[:, fc.FIN_CONST] == 0).all() and (var[:, [g for g in range(len(lens)) if g != fc.FIN_CONST]] > 0).all()
    off = d["gid"] < 0
    assert (scl[:, off] == 1).all() and (sft[:, off] == 0).all() and (dscl[:, off] == 0).all()
    on = ~off
    for m in fc.FIN_MUTANTS:
        ms, mf = fc.fin_forward(c, d, m)[:2]
        r = max((np.abs(ms - scl)[:, on] / dscl[:, on]).max(), (np.abs(mf - sft)[:, on] / dsft[:, on]).max())
        print("finalize_gn %s %s: %.3g bounds" % (c["name"], m, r))
        assert r > 1, (m, r)


# ------------------------------------------------------------------------------------------------------------ COPY_COLS
def test_copy_table_and_edge_values():
    assert {(c["src_f16"], c["dst_f16"]) for c in fc.COPY_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for c in fc.COPY_CASES:
        assert c["n"] < min(c["src_ld"], c["dst_ld"])
    e = fc.COPY_EDGES
    with np.errstate(over="ignore"):
        h = e.astype(F16)
    back = h.astype(np.float64)
    fin = np.isfinite(e)
    assert (back[fin] != e[fin].astype(np.float64)).sum() >= 10  # most edge values do round
    assert h[0] == F16(1.0) and h[1] == F16(1 + 2.0 ** -9)  # ties go to the even neighbour, in both directions
    assert h[5] == 0 and h[6] == F16(2.0 ** -23) and h[7] == F16(2.0 ** -24)  # 2^-25: a tie to zero; just above it: up
    assert h[10] == F16(65504.0) and np.isinf(h[11])  # 65520 is the tie that overflows


# ------------------------------------------------------------------------------------------------------------ ASSEMBLE
def test_assemble_table_reaches_every_listed_edge():
    run = [c for c in fc.ASM_CASES if c["status"] == 0]
    for fp in (False, True):
        cs = [c for c in run if c["fp"] == fp]
        assert {c["K"] for c in cs} == {8, 16} and {c["f16"] for c in cs} == {False, True} and {c["C"] for c in cs} == {48, 51}
        assert any(fc.asm_nbulk(c) == 0 for c in cs) and any(fc.asm_nbulk(c) == c["C"] // 8 for c in cs)
        assert any(c["c_begin"] == 32 and c["ld_out"] < c["ldg"] and c["ld_out"] > c["ldg"] - 32 for c in cs)
    for c in run:
        assert c["c_begin"] <= 8 * fc.asm_nbulk(c) and c["ldg"] % 8 == 0 and c["ldg"] >= c["C"] + (11 if c["fp"] else 9) + 8
        kidx = fc.asm_inputs(c)["kidx"][:, :c["K"]]
        assert (np.sort(kidx, 1)[:, 1:] == np.sort(kidx, 1)[:, :-1]).any(1).mean() > 0.3  # repeated neighbours
    assert [c["status"] for c in fc.ASM_CASES if c["status"]] == [-3, -3]
    assert all(c["c_begin"] > 8 * fc.asm_nbulk(c) for c in fc.ASM_CASES if c["status"])


@pytest.mark.parametrize("c", [c for c in fc.ASM_CASES if c["status"] == 0], ids=lambda c: c["name"])
def test_assemble_checks_see_the_mutants(c):
    d = fc.asm_inputs(c)
    g, bnd, exact = fc.asm_forward(c, d)
    dt = F16 if c["f16"] else F32
    assert (g[:, c["C"] + (11 if c["fp"] else 9):] == 0).all()
    for m in fc.asm_mutants(c):
        gm = fc.asm_forward(c, d, m)[0]
        moved = (gm.astype(dt)[:, exact] != g.astype(dt)[:, exact]).any()
        r = (np.abs(gm.astype(dt).astype(np.float64) - g)[:, ~exact] / bnd[:, ~exact]).max() if (~exact).any() else 0.0
        print("assemble %s %s: exact columns differ %s, weight column %.3g bounds" % (c["name"], m, moved, r))
        assert (r > 1) if m == "w_over_16" else moved, m
    assert set(fc.asm_mutants(c)) <= set(fc.ASM_MUTANTS)
