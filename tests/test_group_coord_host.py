"""CPU: the yardstick of the grouping layer's coordinate gradient is checked against itself (tests/group_coord_cases.py).  The
float64 torch restatement of the reference's operators (autograd) equals the closed formulas of include/slide_train.h written as
explicit loops; every wrong variant of the formulas misses the GPU test's bound; the right formulas evaluated in float32, in the
kernel's order of operations, stay inside it -- the bound is neither loose nor unattainable."""
import numpy as np

import group_coord_cases as G

# (case, mutant) pairs on which the wrong formula is right to within rounding, with the reason; another case must show the mutant
EXEMPT = {
    # every centre is its own first neighbour: its weight is 1 - O(1e-8) and (q - c) = 0 for it, the other neighbours' r^2 / S is
    # O(1e-6) or less, so the coupling term moves no element by more than its bound
    ("fp-coincident-C5", "no_w_coupling"): "fp-base8-C5",
}


def _bounds(d, Sx, Sc, indeg):
    K = d["K"]
    return G.tolerance(Sx, indeg, d["flags"], K), G.tolerance(Sc, np.full(Sc.shape[:2], K), d["flags"], K)


def test_autograd_restatement_equals_the_closed_formulas():
    """on the smallest case of each form (and the ball case, for the empty-ball rule): the two float64 statements agree to float64
    rounding, far inside the fp32 bound"""
    for name in ("sa-clamp-C5", "sa_abs_ctr-clamp-C5", "fp-clamp-C5", "sa_abs_ctr-ball-C5", "fp-coincident-C5"):
        d = G.make_data(name)
        ox, oc = G.oracle_grads(d)
        dx, dc, Sx, Sc, indeg = G.closed_form(d)
        tx, tc = _bounds(d, Sx, Sc, indeg)
        for got, want, tol in ((dx, ox, tx), (dc, oc, tc)):
            assert np.isfinite(want).all()
            assert np.all(np.abs(got - want) <= 1e-6 * tol), name  # 2^-53 against 2^-24: nine decimal digits between them
        if d["counts"] is not None:  # no source point received anything from an empty centre
            b, p = np.nonzero(d["counts"] == 0)
            assert len(b) and indeg.sum() == (d["counts"] > 0).sum() * d["K"]


def test_every_mutant_misses_the_bound():
    shown = set()
    for c in G.CASES:
        d = G.make_data(c["name"])
        ox, oc = G.oracle_grads(d)
        _, _, Sx, Sc, indeg = G.closed_form(d)
        tx, tc = _bounds(d, Sx, Sc, indeg)
        for m in G.MUTANTS:
            if not G.applies(m, d):
                continue
            mx, mc, _, _, _ = G.closed_form(d, mutant=m)
            r = max(G.worst(mx, ox, tx), G.worst(mc, oc, tc))
            if (c["name"], m) in EXEMPT:
                assert EXEMPT[(c["name"], m)] in G.CASE_BY_NAME
                continue
            assert r > 1, "case %s: the bound does not see mutant %s (max deviation / bound %.3g)" % (c["name"], m, r)
            shown.add((c["name"], m))
    assert {m for _, m in shown} == set(G.MUTANTS)
    for (_, m), other in EXEMPT.items():
        assert (other, m) in shown


def test_float32_evaluation_stays_inside_the_bound():
    w = 0.0
    for c in G.CASES:
        d = G.make_data(c["name"])
        ox, oc = G.oracle_grads(d)
        fx, fc, Sx, Sc, indeg = G.closed_form(d, dtype=np.float32)
        tx, tc = _bounds(d, Sx, Sc, indeg)
        r = max(G.worst(fx, ox, tx), G.worst(fc, oc, tc))
        assert r <= 1, (c["name"], r)
        w = max(w, r)
    print("float32 closed formulas: worst err / tol %.3f" % w)
    assert w > 0.01  # the bound is within two orders of what fp32 arithmetic does: not loose


def test_case_matrix_reaches_what_it_claims():
    """C in {0, 5, 29, 32}: the coordinate columns start a row, straddle an 8-column piece and a 32-column pad boundary, start a fresh
    pad block; K clamps to N; in-degree 300; one centre; an empty and a partly filled ball; d2 = 0"""
    lds = {c["C"]: G.make_data(c["name"])["ldg"] for c in G.CASES if c["form"] == "fp" and c["shape"] == "base8"}
    assert lds == {0: 32, 5: 32, 29: 64, 32: 64}
    d = G.make_data("sa-clamp-C5")
    assert d["K"] == d["N"] == 5
    d = G.make_data("fp-fan300-C5")
    assert (G.closed_form(d)[4] == 300).all()
    assert G.make_data("fp-one-C5")["np"] == 1
    d = G.make_data("sa-ball-C5")
    assert d["idx"].dtype == np.int32 and (d["counts"] == 0).any()
    assert (G.make_data("fp-coincident-C5")["d2"] == 0).any()
