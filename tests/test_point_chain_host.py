"""SLIDE_OP_POINT_CHAIN on the CPU: the case table of tests/chain_cases.py reaches every listed edge, every case stays inside the
first-order regime of its GroupNorm bounds, every mutant misses the bound of every case it applies to and the non-mutant stays
inside.  (tests/test_hip_point_chain.py holds the kernel to the same references and bounds.)"""
import numpy as np
import pytest

import chain_cases as cc

DENSE = [c for c in cc.CASES if not c["probe"]]
IDS = ["%s-%s" % (c["name"], f) for c in cc.CASES for f in cc.FORMS]
PAIRS = [(c, f) for c in cc.CASES for f in cc.FORMS]


def test_case_table_reaches_every_listed_edge():
    col = lambda k: {c[k] for c in DENSE}
    assert col("rows") == {16, 32, 48, 112} and col("kz") == {32, 96, 192} and col("k0") == {160} and col("x_ld") == {160, 168}
    assert {c["z_ld"] - c["kz"] for c in DENSE} == {0, 8}
    assert {(c["n1c"], c["eps_ld"]) for c in DENSE} == {(1, 20), (1, 32), (2, 52), (2, 64)}
    assert col("tvec") == {None, "shared", "sample"} and col("cvec") == {False, True}
    assert col("dist") == {"normal", "common", "gnmean"}
    for kz in (32, 96, 192):  # every input width with and without a padded leading dimension somewhere in the table
        assert {c["z_ld"] - c["kz"] for c in DENSE if c["kz"] == kz} & {0, 8}
    # the leading dimensions of the vectors exceed 128 and the pointers are offset into them, inside the tables
    assert min(cc.T_STRIDE, cc.T_BS, cc.C_BS) > 128 and min(cc.T_COFF, cc.T_BS_COFF, cc.C_COFF) > 0
    assert cc.T_COFF + 128 <= cc.T_STRIDE and cc.T_BS_COFF + 128 <= cc.T_BS and cc.C_COFF + 128 <= cc.C_BS and 0 < cc.T_ROW < cc.T_ROWS
    assert {c["probe"] for c in cc.CASES} == {0, 2, 3, 4}
    # every mutant of the list applies somewhere
    seen = {m for c, f in PAIRS for m in cc.mutants(c, f)}
    assert seen == set(cc.MUTANT_DOC), set(cc.MUTANT_DOC) ^ seen


def test_gnmean_case_has_a_group_far_above_its_spread():
    """the group that carries GNMEAN: its mean is more than 20 x its spread in both layers, and (forward() asserts it through
    pair_cases._norm_fin) still inside the first-order regime"""
    c = cc.CASE_BY_NAME["r16_kz96_gnmean"]
    d = cc.make_data(c)
    v1 = d["Z"].astype(np.float64) @ cc.split(d["Wz"])[0][:128].astype(np.float64).T + d["vz"][0]
    g = v1[:, 20:24]
    assert abs(g.mean()) > 20 * g.std(), (g.mean(), g.std())
    for form in cc.FORMS:
        cc.forward(c, d, form)


@pytest.mark.parametrize("c,form", PAIRS, ids=IDS)
def test_bounds_see_the_mutants(c, form):
    d = cc.make_data(c)
    ref = cc.forward(c, d, form)  # (asserts the GroupNorm regime of every layer)
    for k in ("X", "eps"):
        assert np.isfinite(ref[k][0]).all() and (ref[k][2] > 0).all() and np.isfinite(ref[k][2]).all()
    assert ref["eps"][0].shape == (c["rows"], c["eps_ld"]) and ref["X"][0].shape == (c["rows"], 128)
    for nm in cc.NON_MUTANTS:
        r = cc.ratios(cc.forward(c, d, form, nm), ref)
        print("%s %s %s: X %.3f eps %.3f of the bound" % (c["name"], form, nm, r["X"], r["eps"]))
        assert max(r.values()) <= 1.0, (nm, r)
    for m in cc.mutants(c, form):
        r = cc.ratio(cc.forward(c, d, form, m), ref)
        print("%s %s %s: %.3g bounds" % (c["name"], form, m, r))
        assert r > 1.0, (m, r)

