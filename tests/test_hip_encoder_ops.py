"""GPU: slide_col_max_seg(_bwd) and slide_gauss_posterior_fwd / _bwd (csrc/encoder_ops.hip) on the case matrices of
tests/encoder_ops_cases.py, and the autograd Functions on top of them (functions.col_max_seg, functions.gauss_posterior).

Column max: integer-valued data, so values, first indices and the scattered gradient are compared for equality; B = 3 against every
sample alone, bit for bit.  Posterior: against the float64 evaluation of the same fp32 inputs (which the host test pins to torch's
float64 autograd of the reference expression) inside the derived bounds; kl bit-equal over runs and batch positions.  Each posterior
case prints "WORST posterior <case> <z> <kl> <dparams>" as fractions of the bounds (recorded in profiles/encoder_training.md)."""
import ctypes

import numpy as np
import pytest

import encoder_ops_cases as K

pytestmark = pytest.mark.gpu
PREFILL = -77.0


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _col_max(x, B, S, C, ld, device):
    import torch
    from slide_amd._lib import lib
    xd = _dev(x, device)
    out = torch.full((B, ld), PREFILL, dtype=torch.float32, device=device)
    arg = torch.full((B, ld), -7, dtype=torch.int32, device=device)
    st = lib().slide_col_max_seg(B, S, C, ld, _P(xd), _P(out), _P(arg), _stream())
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), arg.cpu().numpy()


@pytest.mark.parametrize("case", K.COL_MAX_CASES, ids=[c["name"] for c in K.COL_MAX_CASES])
def test_col_max_seg_case(case, gpu_device):
    import torch
    from slide_amd._lib import lib
    B, S, C, ld = case["B"], case["S"], case["C"], case["ld"]
    x = K.col_max_data(case)
    want_out, want_arg = K.col_max_ref(x.copy(), B, S, C)
    st, out, arg = _col_max(x, B, S, C, ld, gpu_device)
    assert st == 0
    assert np.array_equal(out, want_out)
    assert np.array_equal(arg, want_arg)            # numpy's argmax: the first maximum; -1 in the pad columns
    if case["kind"] == "negative" and C:
        assert (out[:, :C] < 0).all()
    # every sample alone: the bits it has inside the batch
    for b in range(B):
        s1, o1, a1 = _col_max(x[b * S:(b + 1) * S], 1, S, C, ld, gpu_device)
        assert s1 == 0 and np.array_equal(o1[0], out[b]) and np.array_equal(a1[0], arg[b])
    # the backward: the scatter, every other element written as zero
    dy = np.random.RandomState(S).randint(-5, 6, size=(B, ld)).astype(np.float32)
    dx = torch.full((B * S, ld), PREFILL, dtype=torch.float32, device=gpu_device)
    arg_d, dy_d = _dev(arg, gpu_device), _dev(dy, gpu_device)   # (named: a temporary's memory is reused by the next allocation)
    st = lib().slide_col_max_seg_bwd(B, S, ld, _P(arg_d), _P(dy_d), _P(dx), _stream())
    torch.cuda.synchronize()
    assert st == 0 and np.array_equal(dx.cpu().numpy(), K.col_max_bwd_ref(want_arg, dy, S))


def test_col_max_seg_function_routes_like_max_pool(gpu_device):
    import torch
    from slide_amd.train import functions as F
    case = dict(B=3, S=17, C=40, ld=64, kind="mixed")
    x = K.col_max_data(case)
    xd = _dev(x, gpu_device).requires_grad_(True)
    out, arg = F.col_max_seg(xd, 3, 17, 40)
    w = torch.arange(1, 3 * 64 + 1, device=gpu_device, dtype=torch.float32).reshape(3, 64)
    (out * w).sum().backward()
    t = torch.from_numpy(x).reshape(3, 17, 64).permute(0, 2, 1).contiguous().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(t.unsqueeze(-1), kernel_size=(17, 1)).reshape(3, 64)
    (y[:, :40] * w.cpu()[:, :40]).sum().backward()
    assert torch.equal(out.detach().cpu()[:, :40], y.detach()[:, :40]) and not out.detach()[:, 40:].any()
    assert torch.equal(xd.grad.cpu().reshape(3, 17, 64), t.grad.permute(0, 2, 1))


def _posterior(params, eps, B, S, C, device, want_kl=True):
    import torch
    from slide_amd._lib import lib
    ldp, ldz = params.shape[1], K.ru(C)
    z = torch.full((B * S, ldz), PREFILL, dtype=torch.float32, device=device)
    kl = torch.full((B,), PREFILL, dtype=torch.float32, device=device) if want_kl else None
    pd, ed = _dev(params, device), _dev(eps, device)
    st = lib().slide_gauss_posterior_fwd(B, S, C, ldp, ldz, _P(pd), _P(ed), _P(z), _P(kl), _stream())
    torch.cuda.synchronize()
    return st, z.cpu().numpy(), None if kl is None else kl.cpu().numpy()


def _posterior_bwd(params, eps, dz, dkl, B, S, C, device):
    import torch
    from slide_amd._lib import lib
    ldp, ldz = params.shape[1], K.ru(C)
    dp = torch.full((B * S, ldp), PREFILL, dtype=torch.float32, device=device)
    pd, ed, zd, kd = (_dev(a, device) for a in (params, eps, dz, dkl))
    st = lib().slide_gauss_posterior_bwd(B, S, C, ldp, ldz, _P(pd), _P(ed), _P(zd), _P(kd), _P(dp), _stream())
    torch.cuda.synchronize()
    return st, dp.cpu().numpy()


@pytest.mark.parametrize("case", K.POSTERIOR_CASES, ids=[c["name"] for c in K.POSTERIOR_CASES])
def test_gauss_posterior_case(case, gpu_device):
    B, S, C = case["B"], case["S"], case["C"]
    params, eps, dz, dkl = K.posterior_data(case)
    worst = [0.0, 0.0, 0.0]
    for e in (eps, None):                                        # a sample, and the mode
        zr, klr, bz, bkl = K.posterior_fwd_ref(params, e, B, S, C)
        st, z, kl = _posterior(params, e, B, S, C, gpu_device)
        assert st == 0 and not z[:, C:].any()
        worst[0] = max(worst[0], K.ratio(z[:, :C], zr, bz))
        worst[1] = max(worst[1], K.ratio(kl, klr, bkl))
        if e is None:
            assert np.array_equal(z[:, :C], params[:, :C])
        # kl: two runs and every batch position give the same bits; without kl the same z
        st2, z2, kl2 = _posterior(params, e, B, S, C, gpu_device)
        assert np.array_equal(kl2, kl) and np.array_equal(z2, z)
        for b in range(B):
            rows = slice(b * S, (b + 1) * S)
            s1, z1, k1 = _posterior(params[rows], None if e is None else e[rows], 1, S, C, gpu_device)
            assert s1 == 0 and np.array_equal(k1[0], kl[b]) and np.array_equal(z1, z[rows])
        s3, z3, _ = _posterior(params, e, B, S, C, gpu_device, want_kl=False)
        assert s3 == 0 and np.array_equal(z3, z)
        for g_z, g_k in ((dz, dkl), (None, dkl), (dz, None)):     # dz / dkl each NULL
            gr, bg = K.posterior_bwd_ref(params, e, g_z, g_k, B, S, C)
            st, dp = _posterior_bwd(params, e, g_z, g_k, B, S, C, gpu_device)
            assert st == 0 and not dp[:, 2 * C:].any()
            worst[2] = max(worst[2], K.ratio(dp[:, :2 * C], gr, bg))
    print("WORST posterior %s z %.3g kl %.3g dparams %.3g" % ((case["name"],) + tuple(worst)))
    assert max(worst) <= 1.0, worst


def test_gauss_posterior_function_against_float64_autograd(gpu_device):
    """functions.gauss_posterior: (z, kl) and the gradient of a loss that uses both, only z, and only kl, against float64 torch
    autograd of DiagonalGaussianDistribution's expression"""
    import torch
    from slide_amd.train import functions as F
    case = K.POSTERIOR_CASES[3]  # S16_C32_edges
    B, S, C = case["B"], case["S"], case["C"]
    params, eps, dz, dkl = K.posterior_data(case)
    for use_z, use_k in ((True, True), (True, False), (False, True)):
        p = _dev(params, gpu_device).requires_grad_(True)
        z, kl = F.gauss_posterior(p, _dev(eps, gpu_device), B, S, C)
        loss = 0
        if use_z:
            loss = loss + (z * _dev(dz, gpu_device)).sum()
        if use_k:
            loss = loss + (kl * _dev(dkl, gpu_device)).sum()
        loss.backward()
        gr, bg = K.posterior_bwd_ref(params, eps, dz if use_z else None, dkl if use_k else None, B, S, C)
        assert K.ratio(p.grad.cpu().numpy()[:, :2 * C], gr, bg) <= 1.0
    zr, klr, bz, bkl = K.posterior_fwd_ref(params, None, B, S, C)
    z, kl = F.gauss_posterior(_dev(params, gpu_device), None, B, S, C)
    assert K.ratio(z.cpu().numpy()[:, :C], zr, bz) <= 1.0 and K.ratio(kl.cpu().numpy(), klr, bkl) <= 1.0


def test_status_codes_write_nothing(gpu_device):
    import torch
    from slide_amd._lib import lib
    buf = torch.full((8192,), PREFILL, dtype=torch.float32, device=gpu_device)
    pick = lambda names, null: [None if n in null else _P(buf) for n in names]
    for name, kw, null, status in K.COL_MAX_STATUS:
        assert lib().slide_col_max_seg(kw["B"], kw["S"], kw["C"], kw["ld"], *pick(("x", "out", "arg"), null), _stream()) == status, name
    for name, kw, null, status in K.POSTERIOR_STATUS:
        assert lib().slide_gauss_posterior_fwd(kw["B"], kw["S"], kw["C"], kw["ldp"], kw["ldz"],
                                               *pick(("params", "eps", "z", "kl"), null), _stream()) == status, name
    torch.cuda.synchronize()
    assert bool((buf == PREFILL).all())
