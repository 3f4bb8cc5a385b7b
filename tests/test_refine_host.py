"""CPU: the numpy float32 restatement of the refine-and-upsample front (tests/refine_cases.py) equals the reference's own outputs
(tests/golden/golden_refine.npz, tools/gen_golden_refine.py) bit for bit on every case; each of the nearest wrong arithmetics differs
from them somewhere, so the GPU tests' bit equality with the restatement tells them apart; and the wrappers' argument errors."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import refine_cases as C


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _golden_refine(g, name):
    return tuple(g["refine_%s_%s" % (name, k)] for k in ("points", "normals", "bbox"))


def _restated_refine(name, wrong=None):
    X, disp = C.refine_inputs(name)
    p, n, bbox = C.refine_to_dpsr(X, disp, wrong=wrong, **C.refine_kwargs(name))
    if name == C.BIG:
        sel = C.big_rows(p.shape[1])
        p, n = p[:, sel], n[:, sel]
    return p, n, bbox


@pytest.mark.parametrize("name", list(C.REFINE_CASES))
def test_refine_restatement_equals_reference_bitwise(name):
    g = load_golden("golden_refine.npz")
    p, n, bbox = _restated_refine(name)
    gp, gn, gb = _golden_refine(g, name)
    assert p.shape == gp.shape, (name, p.shape, gp.shape)
    assert _same(p, gp), "%s: %d point elements differ" % (name, int((_bits(p) != _bits(gp)).sum()))
    assert _same(n, gn), "%s: %d normal elements differ" % (name, int((_bits(n) != _bits(gn)).sum()))
    assert _same(bbox, gb), name


def test_scale_mode_cases_clamp_at_both_ends():
    g = load_golden("golden_refine.npz")
    for name, c in C.REFINE_CASES.items():
        if c["mode"] == "scale":
            p = g["refine_%s_points" % name]
            assert (p == 0).sum() >= 10 and (p == np.float32(0.99)).sum() >= 10, name


def test_big_case_has_its_extremes_in_the_first_and_the_last_tile():
    X, disp = C.refine_inputs(C.BIG)
    child = C.point_upsample(X, disp, C.REFINE_CASES[C.BIG]["factor"])
    R = child.shape[1]
    assert R == 7000 and R % C.TILE != 0
    for b in range(child.shape[0]):
        lo, hi = child[b, :, 0:3].argmin(axis=0), child[b, :, 0:3].argmax(axis=0)
        first = [(lo[k] < C.TILE, hi[k] < C.TILE) for k in range(3)]
        last = [(lo[k] >= R - R % C.TILE, hi[k] >= R - R % C.TILE) for k in range(3)]
        for k in range(3):  # one extreme of the axis in the first tile, the other in the last, ragged one
            assert (first[k][0] and last[k][1]) or (first[k][1] and last[k][0]), (b, k, lo, hi)


@pytest.mark.parametrize("name", list(C.MIRROR_CASES))
def test_mirror_restatement_equals_reference_bitwise(name):
    g = load_golden("golden_refine.npz")
    c = C.MIRROR_CASES[name]
    perm = g["mirror_%s_perm" % name] if c["perm"] else None
    out = C.mirror_concat(C.mirror_inputs(name), g["mirror_%s_center" % name], axis=c["axis"], attach_label=c["label"], perm=perm)
    assert _same(out, g["mirror_%s_out" % name]), name


def test_recorded_permutation_is_refine_permutation():
    from slide_amd.refine import refine_permutation
    g = load_golden("golden_refine.npz")
    for name, c in C.MIRROR_CASES.items():
        if c["perm"]:
            assert np.array_equal(refine_permutation(2 * c["N"], C.MIRROR_PERM_SEED).numpy(), g["mirror_%s_perm" % name]), name
    assert np.array_equal(refine_permutation(len(g["net_perm"]), int(g["net_seed"])).numpy(), g["net_perm"])
    p = refine_permutation(10, 3)
    assert p.dtype == torch.int32 and sorted(p.tolist()) == list(range(10))


WRONG_REFINE = {"fma": None, "gs": None, "rsqrtf": None, "centroid": "normalize", "rcp12": None, "parent_box": "normalize"}


@pytest.mark.parametrize("wrong", list(WRONG_REFINE))
def test_nearest_wrong_arithmetic_differs_from_the_reference(wrong):
    g = load_golden("golden_refine.npz")
    differing = []
    for name, c in C.REFINE_CASES.items():
        if WRONG_REFINE[wrong] not in (None, c["mode"]):
            continue
        p, n, bbox = _restated_refine(name, wrong=wrong)
        gp, gn, gb = _golden_refine(g, name)
        if not (_same(p, gp) and _same(n, gn)):
            differing.append(name)
    print("%s differs on %s" % (wrong, differing))
    assert differing, wrong


def test_mirror_without_the_round_trip_differs_from_the_reference():
    g = load_golden("golden_refine.npz")
    differing = []
    for name, c in C.MIRROR_CASES.items():
        perm = g["mirror_%s_perm" % name] if c["perm"] else None
        out = C.mirror_concat(C.mirror_inputs(name), g["mirror_%s_center" % name], axis=c["axis"], attach_label=c["label"], perm=perm,
                              wrong="no_roundtrip")
        if not _same(out, g["mirror_%s_out" % name]):
            differing.append(name)
    assert differing


def test_network_bound_is_derived_and_small():
    g = load_golden("golden_refine.npz")
    hp_factor, s = 5, 0.001
    X, disp = g["net_X"], g["net_disp"]
    child = C.point_upsample(X[:, :, 0:6], disp, hp_factor, out_scale=s)
    p, n, bbox = C.refine_to_dpsr(X, disp, hp_factor, out_scale=s, mode="normalize", ldx=7)
    assert _same(p, g["net_points"]) and _same(n, g["net_normals"])
    L = (bbox[:, 1] - bbox[:, 0]).max(axis=1)
    bound, e_c = C.network_point_bound(disp, np.abs(child).max(), L, hp_factor, s)
    assert bound.shape == (2,) and np.all(bound < 1e-5) and np.all(bound > 5 * C.EPS) and e_c < 1e-5


def test_wrapper_argument_errors():
    """raised before any device is touched"""
    from slide_amd import refine
    x6, x7 = torch.zeros(2, 8, 6), torch.zeros(2, 8, 7)
    with pytest.raises(ValueError, match="at least 3 channels"):
        refine.mirror_and_concat(torch.zeros(2, 8, 2))
    with pytest.raises(ValueError, match="axis"):
        refine.mirror_and_concat(x6, axis=3)
    with pytest.raises(ValueError, match="perm"):
        refine.mirror_and_concat(x6, perm=torch.zeros(15, dtype=torch.int32))
    with pytest.raises(ValueError, match="perm"):
        refine.mirror_and_concat(x6, perm=torch.zeros(16))
    with pytest.raises(RuntimeError, match="float"):
        refine.mirror_and_concat(x6.double())
    with pytest.raises(RuntimeError, match="CUDA"):
        refine.mirror_and_concat(x6)
    d = torch.zeros(2, 8, 30)
    with pytest.raises(ValueError, match="channels"):
        refine.refine_to_dpsr_points(x7, d, 5)
    with pytest.raises(ValueError, match="channels"):
        refine.refine_to_dpsr_points(x6, d, 5, last_dim_as_indicator=True)
    with pytest.raises(ValueError, match="disagree"):
        refine.refine_to_dpsr_points(x6, d[:, :7], 5)
    with pytest.raises(ValueError, match="form needs 36"):
        refine.refine_to_dpsr_points(x6, d, 5, first_refine_coarse_points=True)
    with pytest.raises(ValueError, match="form needs 24"):
        refine.refine_to_dpsr_points(x6, d, 4)
    with pytest.raises(ValueError, match="first_refine_coarse_points"):
        refine.refine_to_dpsr_points(x6, d, 5, include_displacement_center_to_final_output=True)
    with pytest.raises(ValueError, match="at least 1"):
        refine.refine_to_dpsr_points(x6, d[:, :, :0], 0)
    with pytest.raises(ValueError, match="last_dim_as_indicator"):
        refine.refine_to_dpsr_points(x6, d, 5, only_original_points_split=True)
    with pytest.raises(ValueError, match="scale"):
        refine.refine_to_dpsr_points(x6, d, 5, scale=0)
    with pytest.raises(RuntimeError, match="CUDA"):
        refine.refine_to_dpsr_points(x6, d, 5)
