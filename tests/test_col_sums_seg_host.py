"""CPU: the case matrix of slide_col_sums_seg (tests/col_sums_seg_cases.py) -- the restated order of additions stays inside the bound
derived from its longest chain, the bound does not grow with S, and it refuses the nearest wrong variants."""
import numpy as np
import pytest

import col_sums_seg_cases as K


def test_matrix_reaches_both_forms_and_every_layout():
    maps = {c["name"]: K.seg_map(c["S"], c["ld"]) for c in K.CASES}
    assert {m["stages"] for m in maps.values()} == {1, 2}
    assert maps["s127_ld32"]["stages"] == 1 and maps["s128_ld32"]["stages"] == 2       # the threshold between the two forms
    assert {m["rt"] for m in maps.values()} == {32, 10, 1}                              # ld 96: 16 idle threads per workgroup
    assert any(m["rpc"] * m["nchunk"] != c["S"] for c, m in zip(K.CASES, maps.values()))  # a ragged last chunk
    for c in K.CASES:
        m = maps[c["name"]]
        assert m["rpc"] * (m["nchunk"] - 1) < c["S"] <= m["rpc"] * m["nchunk"] and m["nchunk"] <= 256
        assert c["B"] * m["scratch_floats"] <= K.scratch_floats(c["B"], c["S"], c["ld"])  # the documented size covers the launch


def test_chain_does_not_grow_with_the_rows():
    assert K.seg_map(8195, 32)["chain"] == 3 + 32 + 4 + 32
    assert K.seg_map(8195, 1024)["chain"] == 65 + 1 + 127 + 1                               # (127 chunks of 65 rows)
    assert K.seg_map(1 << 24, 32)["chain"] == 2048 + 32 + 8 + 32                        # 2^24 rows: 2120 links, not 2^24
    assert max(K.seg_map(c["S"], c["ld"])["chain"] for c in K.CASES) < 256


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_restated_order_is_inside_the_bound_and_mutants_are_outside(case):
    B, S, ld = case["B"], case["S"], case["ld"]
    x = K.make_data(case, "normal")
    ref = x.astype(np.float64).reshape(B, S, ld).sum(axis=1)
    bnd = K.bound(x, B, S, ld)
    assert K.ratio(K.ordered_sums(x, B, S, ld), ref, bnd) <= 1.0
    xi = K.make_data(case, "ints")
    assert np.array_equal(K.ordered_sums(xi, B, S, ld), xi.astype(np.float64).reshape(B, S, ld).sum(axis=1))
    for mutant in K.MUTANTS:
        got = K.ordered_sums(x, B, S, ld, mutant=mutant)
        assert K.ratio(got, ref, bnd) > 1.0, mutant


def test_a_sample_does_not_depend_on_its_batch():
    case = dict(name="alone", B=3, S=130, ld=96)
    x = K.make_data(case, "normal")
    full = K.ordered_sums(x, 3, 130, 96)
    alone = K.ordered_sums(x[130:260], 1, 130, 96)
    assert np.array_equal(full[1:2], alone)
