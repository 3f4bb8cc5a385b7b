"""GPU: the refine-and-upsample front (slide_amd/csrc/refine_front.hip, slide_amd/refine.py) against the reference's own outputs
(tests/golden/golden_refine.npz) and the numpy float32 restatement that tests/test_refine_host.py pins to them: bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_spec, load_golden
import refine_cases as C

sys.path.insert(0, os.path.join(REPO, "pointnet2"))

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == np.float32 and np.array_equal(_bits(a), _bits(b))


def _run_refine(name, dev, sl=slice(None)):
    from slide_amd.refine import refine_to_dpsr_points
    c = C.REFINE_CASES[name]
    X, disp = C.refine_inputs(name)
    first, center = C.form_flags(c["form"])
    out = refine_to_dpsr_points(T(X[sl], dev), T(disp[sl], dev), c["factor"], first_refine_coarse_points=first,
                                include_displacement_center_to_final_output=center, output_scale_factor=c["out_scale"], scale=c["scale"],
                                explicit_normalize=c["mode"] == "normalize", last_dim_as_indicator=c["ldx"] == 7,
                                only_original_points_split=c["only_orig"])
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("name", list(C.REFINE_CASES))
def test_refine_equals_reference_bitwise(gpu_device, name):
    """points, normals and bbox equal the golden (the big case: its recorded rows) and the restatement on every row; a sample alone
    equals the sample in the batch; two runs are equal"""
    g = load_golden("golden_refine.npz")
    p, n, bbox = _run_refine(name, gpu_device)
    X, disp = C.refine_inputs(name)
    wp, wn, wb = C.refine_to_dpsr(X, disp, **C.refine_kwargs(name))
    assert _same(p, wp), "%s: %d point elements differ from the restatement" % (name, int((_bits(p) != _bits(wp)).sum()) if p.shape == wp.shape else -1)
    assert _same(n, wn) and _same(bbox, wb), name
    sel = C.big_rows(p.shape[1]) if name == C.BIG else slice(None)
    assert _same(np.ascontiguousarray(p[:, sel]), g["refine_%s_points" % name]), name
    assert _same(np.ascontiguousarray(n[:, sel]), g["refine_%s_normals" % name]) and _same(bbox, g["refine_%s_bbox" % name]), name
    last = p.shape[0] - 1
    p1, n1, b1 = _run_refine(name, gpu_device, slice(last, last + 1))
    assert _same(p1, p[last:]) and _same(n1, n[last:]) and _same(b1, bbox[last:]), name
    p2, n2, b2 = _run_refine(name, gpu_device)
    assert _same(p2, p) and _same(n2, n) and _same(b2, bbox), name


@pytest.mark.parametrize("name", list(C.MIRROR_CASES))
def test_mirror_equals_reference_bitwise(gpu_device, name):
    from slide_amd.refine import mirror_and_concat
    g = load_golden("golden_refine.npz")
    c = C.MIRROR_CASES[name]
    x = C.mirror_inputs(name)
    perm = g["mirror_%s_perm" % name] if c["perm"] else None

    def run(sl=slice(None)):
        out, center = mirror_and_concat(T(x[sl], gpu_device), axis=c["axis"], attach_label=c["label"],
                                        perm=None if perm is None else torch.from_numpy(perm))
        return out.cpu().numpy(), center.cpu().numpy()

    out, center = run()
    assert out.shape == (c["B"], 2 * c["N"], c["C"] + int(c["label"])) and center.shape == (c["B"], 3)
    # the centre: within 1 ulp of the float32 rounding of the float64 mean
    want_c = C.mirror_center(x)
    assert np.all(np.abs(center.astype(np.float64) - want_c) <= np.spacing(np.abs(want_c))), (name, center, want_c)
    # the rows, given the kernel's own centre
    assert _same(out, C.mirror_concat(x, center, axis=c["axis"], attach_label=c["label"], perm=perm)), name
    # ... and the reference's rows where the centres agree (its float32 mean may differ from ours by rounding)
    ref_c, ref = g["mirror_%s_center" % name], g["mirror_%s_out" % name]
    agree = (_bits(center) == _bits(ref_c)).all(axis=1)
    print("mirror %s: centre bit-equal to the reference's float32 mean in %d of %d samples" % (name, int(agree.sum()), len(agree)))
    assert _same(np.ascontiguousarray(out[agree]), np.ascontiguousarray(ref[agree])), name
    last = c["B"] - 1
    o1, c1 = run(slice(last, last + 1))
    assert _same(o1, out[last:]) and _same(c1, center[last:]), name
    o2, c2 = run()
    assert _same(o2, out) and _same(c2, center), name


def test_flag_errors(gpu_device):
    """NaN input, a coincident cloud with zero displacement and a bad perm are ValueErrors; nothing faults and the next call is clean"""
    from slide_amd.refine import mirror_and_concat, refine_to_dpsr_points
    name = "n37_plain_norm"
    X, disp = C.refine_inputs(name)
    Xn = X.copy()
    Xn[1, 5, 1] = np.nan
    with pytest.raises(ValueError, match="sample 1 has a non-finite"):
        refine_to_dpsr_points(T(Xn, gpu_device), T(disp, gpu_device), 5, explicit_normalize=True)
    with pytest.raises(ValueError, match="sample 1 has a non-finite"):
        refine_to_dpsr_points(T(Xn, gpu_device), T(disp, gpu_device), 5, explicit_normalize=False)
    Xi = X.copy()
    Xi[2, 0, 0] = np.inf
    with pytest.raises(ValueError, match="sample 2"):
        refine_to_dpsr_points(T(Xi, gpu_device), T(disp, gpu_device), 5, explicit_normalize=True)
    Xc = X.copy()
    Xc[0, :, 0:3] = np.float32(0.25)
    dz = disp.copy()
    dz[0] = 0
    with pytest.raises(ValueError, match="sample 0 coincide"):
        refine_to_dpsr_points(T(Xc, gpu_device), T(dz, gpu_device), 5, explicit_normalize=True)
    p, _, _ = refine_to_dpsr_points(T(Xc, gpu_device), T(dz, gpu_device), 5, explicit_normalize=False)  # (fine in scale mode)
    assert torch.isfinite(p).all()
    x = C.mirror_inputs("a2_c6_l")
    n2 = 2 * x.shape[1]
    for bad in (n2, -1, 2 ** 31 - 1):
        perm = torch.arange(n2, dtype=torch.int32)
        perm[7] = bad
        with pytest.raises(ValueError, match="perm has an entry outside"):
            mirror_and_concat(T(x, gpu_device), perm=perm)
    out, _ = mirror_and_concat(T(x, gpu_device), perm=torch.arange(n2, dtype=torch.int32))
    assert torch.isfinite(out).all()
    p, n, bbox = _run_refine(name, gpu_device)
    assert _same(p, C.refine_to_dpsr(X, disp, **C.refine_kwargs(name))[0])


def test_reference_names(gpu_device):
    """data_utils.mirror_partial.mirror_and_concat and dpsr_evaluation.network_output_to_dpsr_grid return the reference's tuples"""
    from data_utils.mirror_partial import down_sample_points, mirror, mirror_and_concat
    from dpsr_evaluation import network_output_to_dpsr_grid
    from slide_amd.refine import refine_permutation
    g = load_golden("golden_refine.npz")
    x = T(g["net_x"], gpu_device)
    seed = int(g["net_seed"])
    full, d48, d24 = mirror_and_concat(x, axis=2, num_points=[48, 24], attach_label=True, permute=True, seed=seed)
    assert full.shape == (2, 80, 7) and d48.shape == (2, 48, 7) and d24.shape == (2, 24, 7)
    assert np.array_equal(refine_permutation(80, seed).numpy(), g["net_perm"])
    X = g["net_X"]
    got = full.cpu().numpy()
    assert np.abs(got - X).max() <= 2 * np.spacing(np.float32(np.abs(X[:, :, 0:3]).max()))  # (the centres may differ by rounding)
    assert np.array_equal(got[:, :, 3:], X[:, :, 3:])
    # the down-sampled clouds are rows of the full one, the first being row 0 (farthest point sampling starts there)
    rows = {tuple(r) for r in got[0].tolist()}
    assert all(tuple(r) in rows for r in d48[0].cpu().numpy().tolist()) and np.array_equal(d48[0, 0].cpu().numpy(), got[0, 0])
    assert down_sample_points(full, 24).shape == (2, 24, 7)
    m = mirror(x, axis=1).cpu().numpy()
    assert np.array_equal(m[:, :, 4], -g["net_x"][:, :, 4]) and np.array_equal(m[:, :, 3], g["net_x"][:, :, 3])
    (only,) = mirror_and_concat(x, axis=2, num_points=[], attach_label=False, permute=False)
    assert only.shape == (2, 80, 6) and np.array_equal(only[:, :40].cpu().numpy(), g["net_x"])
    hp = json.loads(str(g["net_config_json"]))
    seen = {}

    def dpsr(p, n):
        seen["p"], seen["n"] = p, n
        return "grid"

    grid, p, n = network_output_to_dpsr_grid(T(X, gpu_device), T(g["net_disp"], gpu_device), dpsr, 1, hp, last_dim_as_indicator=True,
                                             explicit_normalize=True)
    assert grid == "grid" and seen["p"] is p and seen["n"] is n
    assert _same(p.cpu().numpy(), g["net_points"]) and _same(n.cpu().numpy(), g["net_normals"])


def test_network_case(gpu_device):
    """the reduced refinement network on the module path: its displacement within 2e-4 of the reference's (max-norm, relative to the
    largest entry -- test_denoiser_parent_project_switches_match_reference's tolerance), the refined points and normals within the
    bound refine_cases.network_point_bound derives from it"""
    from dpsr_evaluation import network_output_to_dpsr_grid
    from models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from slide_amd.synth import synth_state_dict
    g = load_golden("golden_refine.npz")
    hp = json.loads(str(g["net_config_json"]))
    spec = golden_spec(g, "net_spec")
    net = PointNet2CloudCondition(json.loads(str(g["net_config_json"])))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(spec)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec).items()})
    net = net.to(gpu_device).eval()
    X = T(g["net_X"], gpu_device)
    with torch.no_grad():
        disp = net(X, None, ts=None, label=T(g["net_label"], gpu_device))
    ref = g["net_disp"]
    err = np.abs(disp.cpu().numpy() - ref).max() / np.abs(ref).max()
    _, p, n = network_output_to_dpsr_grid(X, disp.contiguous(), lambda a, b: None, 1, hp, last_dim_as_indicator=True, explicit_normalize=True)
    child = C.point_upsample(g["net_X"][:, :, 0:6], ref, hp["point_upsample_factor"], out_scale=hp["output_scale_factor"])
    L = (child[:, :, 0:3].max(axis=1) - child[:, :, 0:3].min(axis=1)).max(axis=1)
    bound, bound_n = C.network_point_bound(ref, np.abs(child).max(), L, hp["point_upsample_factor"], hp["output_scale_factor"])
    ep = np.abs(p.cpu().numpy().astype(np.float64) - g["net_points"]).reshape(len(L), -1).max(axis=1)
    en = np.abs(n.cpu().numpy().astype(np.float64) - g["net_normals"]).max()
    print("refine network case: displacement error / tolerance %.3f (%.2e of %.0e); points error / bound %s (bound %s); "
          "normals error / bound %.3f (bound %.2e)" % (err / C.NET_DISP_TOL, err, C.NET_DISP_TOL, np.round(ep / bound, 3).tolist(),
                                                       ["%.2e" % b for b in bound], en / bound_n, bound_n))
    assert disp.shape == ref.shape and err <= C.NET_DISP_TOL, err
    assert np.all(ep <= bound), (ep, bound)
    assert en <= bound_n, (en, bound_n)
