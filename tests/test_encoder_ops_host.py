"""CPU: the encode-side training kernels' entry points (include/slide_train.h, csrc/encoder_ops.hip) are exported and mirrored in
slide_amd/abi.py, their argument checks run before any launch, the float64 references of tests/encoder_ops_cases.py agree with
torch's float64 autograd of the reference's expression (DiagonalGaussianDistribution; max over the points), and the derived bounds
are tight enough to refuse the nearest wrong arithmetic.  No device is needed."""
import ctypes

import numpy as np
import pytest
import torch

import encoder_ops_cases as K
from slide_amd import _lib, abi, build

NEW = {"slide_col_max_seg": "iiiipppp", "slide_col_max_seg_bwd": "iiipppp", "slide_gauss_posterior_fwd": "iiiiippppp",
       "slide_gauss_posterior_bwd": "iiiiipppppp"}


@pytest.fixture(scope="module")
def lib():
    return abi.bind(ctypes.CDLL(build.build()), False)


def test_new_symbols_are_exported_and_mirrored(lib):
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
        restype, argtypes = abi.PROTOTYPES[name]
        assert restype is ctypes.c_int
        assert argtypes == tuple({"i": ctypes.c_int, "p": ctypes.c_void_p}[c] for c in sig), name


def _ptrs(names, null):
    buf = ctypes.create_string_buffer(64)  # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    return [None if n in null else p for n in names], buf


def test_status_codes_without_a_launch(lib):
    for name, kw, null, status in K.COL_MAX_STATUS:
        a, _keep = _ptrs(("x", "out", "arg"), null)
        assert lib.slide_col_max_seg(kw["B"], kw["S"], kw["C"], kw["ld"], *a, None) == status, name
    for (B, S, ld), null, status in (((2, 4, 48), (), -3), ((2, 4, 0), (), -3), ((2, 0, 32), (), -3), ((-1, 4, 32), (), -3),
                                     ((2, 4, 32), ("dy",), -3), ((2, 4, 32), ("arg",), -3), ((2, 4, 32), ("dx",), -3),
                                     ((0, 4, 32), ("arg", "dy", "dx"), 0)):
        a, _keep = _ptrs(("arg", "dy", "dx"), null)
        assert lib.slide_col_max_seg_bwd(B, S, ld, *a, None) == status, (B, S, ld, null)
    for name, kw, null, status in K.POSTERIOR_STATUS:
        a, _keep = _ptrs(("params", "eps", "z", "kl"), null)
        assert lib.slide_gauss_posterior_fwd(kw["B"], kw["S"], kw["C"], kw["ldp"], kw["ldz"], *a, None) == status, name
        b, _keep = _ptrs(("params", "eps", "dz", "dkl", "dparams"), {"dparams" if n == "z" else n for n in null})
        assert lib.slide_gauss_posterior_bwd(kw["B"], kw["S"], kw["C"], kw["ldp"], kw["ldz"], *b, None) == status, name


@pytest.mark.parametrize("case", K.POSTERIOR_CASES, ids=[c["name"] for c in K.POSTERIOR_CASES])
def test_posterior_reference_is_torch_autograd_of_the_reference_expression(case):
    B, S, C = case["B"], case["S"], case["C"]
    params, eps, dz, dkl = K.posterior_data(case)
    p = torch.from_numpy(params[:, :2 * C]).double().requires_grad_(True)
    mean, logvar = torch.chunk(p, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    z = mean + torch.exp(0.5 * logvar) * torch.from_numpy(eps[:, :C]).double()
    kl = 0.5 * torch.sum((torch.pow(mean, 2) + torch.exp(logvar) - 1.0 - logvar).reshape(B, S * C), dim=1)
    zr, klr, _, _ = K.posterior_fwd_ref(params, eps, B, S, C)
    assert np.allclose(z.detach().numpy(), zr, rtol=1e-13, atol=0) and np.allclose(kl.detach().numpy(), klr, rtol=1e-13, atol=0)
    (z * torch.from_numpy(dz[:, :C]).double()).sum().backward(retain_graph=True)
    (kl * torch.from_numpy(dkl).double()).sum().backward()
    gr, _ = K.posterior_bwd_ref(params, eps, dz, dkl, B, S, C)
    assert np.allclose(p.grad.numpy(), gr, rtol=1e-12, atol=1e-300)
    if case["kind"] == "edges":  # the cases do sit on and outside the clamps, and the gradient passes AT them
        raw = params[:, C:2 * C]
        assert (raw == -30).any() and (raw == 20).any() and (raw == 40).any() and (raw == -40).any()
        assert (gr[:, C:][(raw == -30) | (raw == 20)] != 0).all() and (gr[:, C:][np.abs(raw) == 40] == 0).all()


def test_bounds_refuse_the_nearest_wrong_arithmetic():
    """each wrong variant, evaluated exactly, misses the right reference by more than the bound somewhere in the edge cases; the right
    arithmetic rounded to fp32 at every step stays inside"""
    worst = {}
    for case in (c for c in K.POSTERIOR_CASES if c["kind"] == "edges"):
        B, S, C = case["B"], case["S"], case["C"]
        params, eps, dz, dkl = K.posterior_data(case)
        z, kl, bz, bkl = K.posterior_fwd_ref(params, eps, B, S, C)
        g, bg = K.posterior_bwd_ref(params, eps, dz, dkl, B, S, C)
        for v in ("no_clamp", "var_for_std", "dropped_half", "dropped_row"):
            zv, klv, _, _ = K.posterior_fwd_ref(params, eps, B, S, C, variant=v)
            worst.setdefault("fwd " + v, []).append(max(K.ratio(zv, z, bz), K.ratio(klv, kl, bkl)))
        for v in ("dropped_half", "masked_at_bounds", "neighbour_dkl"):
            gv, _ = K.posterior_bwd_ref(params, eps, dz, dkl, B, S, C, variant=v)
            worst.setdefault("bwd " + v, []).append(K.ratio(gv, g, bg))
        # the right arithmetic in fp32 (numpy float32 steps; numpy's exp is correctly rounded within an ulp)
        f = np.float32
        mean, raw = params[:, :C], params[:, C:2 * C]
        lv = np.clip(raw, f(-30), f(20))
        z32 = mean + np.exp(f(0.5) * lv) * eps[:, :C]
        kl32 = f(0.5) * (mean * mean + np.exp(lv) - f(1) - lv).reshape(B, -1).sum(axis=1, dtype=np.float32)
        assert K.ratio(z32, z, bz) <= 1.0
        assert K.ratio(kl32, kl, bkl * (S * C / 8.0)) <= 1.0  # (numpy's pairwise sum is not the kernel's order: only a sanity check)
    for name, rs in worst.items():
        assert min(rs) > 1.0, (name, rs)


@pytest.mark.parametrize("case", K.COL_MAX_CASES[::7], ids=[c["name"] for c in K.COL_MAX_CASES[::7]])
def test_col_max_reference_is_torch_max_pool(case):
    """the reference of the GPU test against torch on the CPU: values and ROUTING of max over dim 2 (Pnet2Stage's f.max(dim=2))"""
    B, S, C, ld = case["B"], case["S"], case["C"], case["ld"]
    x = K.col_max_data(case)
    out, arg = K.col_max_ref(x.copy(), B, S, C)
    t = torch.from_numpy(x).reshape(B, S, ld).permute(0, 2, 1)[:, :C].double().contiguous().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(t.unsqueeze(-1), kernel_size=(S, 1)).reshape(B, C)
    assert np.array_equal(y.detach().numpy().astype(np.float32), out[:, :C])
    dy = np.arange(1, B * ld + 1, dtype=np.float32).reshape(B, ld)
    (y * torch.from_numpy(dy[:, :C]).double()).sum().backward()
    dx = K.col_max_bwd_ref(arg, dy, S).reshape(B, S, ld)
    assert np.array_equal(t.grad.permute(0, 2, 1).numpy().astype(np.float32), dx[:, :, :C]) and not dx[:, :, C:].any()
