"""The SLIDE_OP_GEMM_ATTEND case table without a GPU (tests/attend_cases.py): every bound against the mutants it must see, the
branches the table reaches, the counts and the NaN guards of the physical layouts.  The GPU half is tests/test_hip_attend.py."""
import numpy as np

import attend_cases as ac
from attend_cases import CASES, CASE_BY_NAME, EXEMPT, forward, make_data, mutants, physical, ratio, reach

ALL_MUTANTS = ("scores_fp16", "k_tail", "affine_sample", "add_all_columns", "aff_relu_dropped", "slot_past_count", "zero_count_empty",
               "count_unclamped_high", "no_max_shift", "vss_sample_of_tile", "v_relu_dropped", "pad_channels_not_zeroed")


def test_bounds_see_the_mutants():
    """the unmutated reference (rounded to fp16) is inside its own bound everywhere; each mutant a case can express leaves the bound
    in that case, or the exemption names a case where it does; scores_fp16 -- the two-launch form's arithmetic -- is seen unexempted"""
    seen = {}
    for c in CASES:
        d = make_data(c)
        ref = forward(c, d)
        assert np.isfinite(ref["y"]).all() and np.isfinite(ref["b"]).all() and (ref["b"] >= 0).all(), c["name"]
        assert (ref["b"][:, :c["C"]] > 0).all() or c["dist"] in ("onehot", "w0"), c["name"]
        assert (ref["b"][:, c["C"]:] == 0).all() and (ref["y"][:, c["C"]:] == 0).all()
        assert ratio(ref, ref["stored"]).max() <= 1, c["name"]
        for m in mutants(c):
            seen[(c["name"], m)] = float(ratio(ref, forward(c, d, mutant=m)["stored"]).max())
    assert {m for _, m in seen} == set(ALL_MUTANTS)
    unseen = []
    for (name, m), r in seen.items():
        if (name, m) in EXEMPT:
            assert seen[(EXEMPT[(name, m)], m)] > 1, (name, m, EXEMPT[(name, m)])
        elif not r > 1:
            unseen.append((name, m, round(r, 3)))
    assert not unseen, "the bound does not see (case, mutant, max deviation / bound): %s" % unseen
    assert not [k for k in EXEMPT if k not in seen], "stale exemptions"
    unexempt = [n for (n, m), r in seen.items() if m == "scores_fp16" and (n, m) not in EXEMPT and r > 1]
    assert "ties8" in unexempt, unexempt
    print("scores_fp16 seen in", unexempt)


def test_a_wrong_bias_cancels_in_the_soft_max():
    """the one mutant of the issue's list that no data can express (attend_cases.INEXPRESSIBLE): with distinct per-channel biases
    in every block, taking block 0's bias for all blocks stays inside the bound of every case with more than one block"""
    assert set(ac.INEXPRESSIBLE) == {"bias_block0"} and not set(ac.INEXPRESSIBLE) & set(ALL_MUTANTS)
    n = 0
    for c in CASES:
        if c["n_cob"] > 1 and c["dist"] != "onehot":
            d = make_data(c)
            assert len(set(d["bias"].tolist())) == c["n_cob"] * 32 and (d["bias"][32:64] != d["bias"][:32]).all()
            assert ratio(forward(c, d), forward(c, d, mutant="bias_block0")["stored"]).max() <= 1, c["name"]
            n += 1
    assert n >= 8


def test_case_matrix_reaches_every_branch():
    """from the table alone: both instantiations, and every K, n_cob, k_pad, tile count, counts / vss / affine form of the issue"""
    R = [reach(c) for c in CASES]
    S = lambda k, f=lambda r: True: {r[k] for r in R if f(r)}
    assert S("AFF") == {False, True}
    assert S("K") == {4, 8, 16, 32}
    assert S("n_cob") == {1, 2, 3} and S("half_tile") == {False, True}
    assert S("k_pad") == {32, 64, 96, 1536}
    assert S("k_pad", lambda r: r["AFF"]) >= {64, 96, 1536} and 1536 in S("k_pad", lambda r: not r["AFF"])
    assert {1, 2, 9} <= S("tiles", lambda r: not r["ragged"])
    assert any(r["ragged"] and not r["AFF"] and r["K"] == 32 for r in R) and not any(r["ragged"] and r["AFF"] for r in R)
    assert any(r["tiles"] == 9 and r["idle"] == 7 * ((r["n_cob"] + 1) // 2) for r in R)
    assert S("counts") == {False, True}
    assert S("vss") == {None, "relu", "plain"} and {64, 512} <= S("vss_span")
    assert S("tps", lambda r: r["AFF"]) == {1, 2} and all(r["samples"] >= 3 for r in R if r["AFF"])
    assert S("aff_form", lambda r: r["AFF"]) == {"add_relu", "add", "relu", "common", "plain"}
    assert any(r["aff_form"] == "add_relu" and r["add_short"] for r in R)
    assert S("dist") == {"normal", "common", "pm100", "ties8", "w0", "onehot"}
    assert S("pad_channels") == {False, True} and S("packed") == {False, True}
    assert all(S(k) == {False, True} for k in ("x_gap", "v_gap", "o_gap"))
    for c in CASES:  # the affine form is never built on a ragged or sub-sample row count (run_gemm_attend refuses it)
        assert not c["aff"] or c["rows"] % (256 * c["tps"]) == 0


def test_counts_hold_every_clamp_edge():
    n = 0
    for c in CASES:
        if c["counts"]:
            cnt, K = make_data(c)["counts"], c["K"]
            assert cnt.dtype == np.int32 and {0, 1, K, K + 5, -3} <= set(cnt.tolist()), c["name"]
            n += 1
    assert n >= 3


def test_physical_layouts_guard_what_must_not_be_read():
    """pad columns the kernel multiplies are zero, everything past them is NaN, and the logical part is what the reference reads"""
    for c in CASES:
        d = make_data(c)
        p = physical(c, d)
        kp, nch = c["k_pad"], c["n_cob"] * 32
        assert (p["X"][:, c["kl"]:kp] == 0).all() and np.isnan(p["X"][:, kp:]).all() and np.isfinite(p["X"][:, :kp]).all()
        assert (p["W"][c["C"]:] == 0).all() and (p["W"][:, c["kl"]:] == 0).all() and p["W"].shape == (nch, kp)
        assert np.isfinite(p["V"][:, :nch]).all() and np.isnan(p["V"][:, nch:]).all()
        assert (p["X"][:, :c["kl"]].astype(np.float64) == ac.r16(d["X"])).all()
        if c["vss"]:
            assert np.isnan(p["vss"][:, :, nch:]).all() and p["vss"].shape[0] * c["pps"] >= c["rows"] // c["K"]
        if c["aff"]:
            assert p["ss"].shape == (ac.n_smp(c), 2, kp)


def test_probe_bounds_are_the_derived_ones():
    """the one-hot probe is exact everywhere; the W = 0 probe allows half an fp16 ulp and K 2^-13 of one"""
    c = CASE_BY_NAME["onehot"]
    ref = forward(c, make_data(c))
    assert (ref["b"] == 0).all() and (np.abs(ref["y"]) > 0).any()
    c = CASE_BY_NAME["w0_mean"]
    d = make_data(c)
    ref = forward(c, d)
    n = np.clip(d["counts"], 1, c["K"])
    v = ac.r16(d["V"]).reshape(-1, c["K"], c["n_cob"] * 32)
    mean = np.stack([v[p, :n[p]].mean(0) for p in range(len(n))])
    assert np.allclose(ref["y"][:, :c["C"]], mean[:, :c["C"]], rtol=1e-13, atol=0)
    mabs = np.stack([np.abs(v[p, :n[p]]).mean(0) for p in range(len(n))])[:, :c["C"]]
    assert (ref["b"][:, :c["C"]] <= 2.0 ** -11 * np.abs(mean[:, :c["C"]]) + 2.0 ** -25 + c["K"] * 2.0 ** -24 * mabs * (1 + 2.0 ** -10)).all()
