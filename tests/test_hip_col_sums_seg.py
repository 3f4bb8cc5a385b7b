"""GPU: slide_col_sums_seg (csrc/train_ops.hip) on the case matrix of tests/col_sums_seg_cases.py -- exact on integer data, inside
the chain-length bound of float64 on normal data, bit-equal over runs and for a sample alone against the same sample in a batch,
the status codes, and functions.add_vec_rows against torch's autograd of the broadcast expression.  Each case prints
"WORST col_sums_seg <case> <err / bound>"."""
import ctypes

import numpy as np
import pytest

import col_sums_seg_cases as K

pytestmark = pytest.mark.gpu
PREFILL = -77.0


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _run(x, B, S, ld, device, scratch=True):
    """one call on explicit prefilled buffers -> (status, out [B, ld] float32 numpy)"""
    import torch
    from slide_amd._lib import lib
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    out = torch.full((max(B, 1), ld), PREFILL, dtype=torch.float32, device=device)
    n = K.scratch_floats(B, S, ld)
    sc = torch.full((max(n, 1),), PREFILL, dtype=torch.float32, device=device) if scratch else None
    st = lib().slide_col_sums_seg(B, S, ld, _P(xd), _P(out), _P(sc), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_col_sums_seg_case(case, gpu_device):
    B, S, ld = case["B"], case["S"], case["ld"]
    # integers of [-8, 8]: every partial sum is exact in fp32, so the result is exact in any order
    xi = K.make_data(case, "ints")
    st, got = _run(xi, B, S, ld, gpu_device)
    assert st == 0
    assert np.array_equal(got, xi.reshape(B, S, ld).sum(axis=1, dtype=np.float64).astype(np.float32))
    # normal data: inside the bound of the longest chain of additions, and the restated order bit for bit
    x = K.make_data(case, "normal")
    ref = x.astype(np.float64).reshape(B, S, ld).sum(axis=1)
    st, got = _run(x, B, S, ld, gpu_device)
    assert st == 0
    r = K.ratio(got, ref, K.bound(x, B, S, ld))
    print("WORST col_sums_seg %s %.3g" % (case["name"], r))
    assert r <= 1.0
    assert np.array_equal(got, K.ordered_sums(x, B, S, ld))
    # two runs are bit-equal; a sample alone gives the bits it has inside the batch
    assert np.array_equal(_run(x, B, S, ld, gpu_device)[1], got)
    st1, alone = _run(x[S:2 * S], 1, S, ld, gpu_device)
    assert st1 == 0 and np.array_equal(alone[0], got[1])


def test_col_sums_seg_status_codes(gpu_device):
    import torch
    from slide_amd._lib import lib
    buf = torch.full((4096,), PREFILL, dtype=torch.float32, device=gpu_device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, kw, status in K.STATUS_CASES:
        args = [_P(buf) if kw.get(k, True) else None for k in ("x", "out", "scratch")]
        assert lib().slide_col_sums_seg(kw["B"], kw["S"], kw["ld"], *args, st) == status, name
    torch.cuda.synchronize()
    assert bool((buf == PREFILL).all())                       # nothing written by any of them
    # S = 0 with B > 0: out zero-filled, status 0, x and scratch not needed
    assert lib().slide_col_sums_seg(3, 0, 32, None, _P(buf), None, st) == 0
    torch.cuda.synchronize()
    assert bool((buf[:96] == 0).all()) and bool((buf[96:] == PREFILL).all())
    # S < 128 runs without scratch
    x = K.make_data(dict(name="noscratch", B=2, S=127, ld=32), "ints")
    s, got = _run(x, 2, 127, 32, gpu_device, scratch=False)
    assert s == 0 and np.array_equal(got, x.reshape(2, 127, 32).sum(axis=1))


@pytest.mark.parametrize("S,ld,C", [(5, 32, 20), (130, 96, 96), (1000, 32, 32)])
def test_add_vec_rows_gradients(S, ld, C, gpu_device):
    import torch
    from slide_amd.train import functions as F
    B = 3
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B * S, ld, generator=g).to(gpu_device).requires_grad_(True)
    vec = torch.randn(B, C, generator=g).to(gpu_device).requires_grad_(True)
    w = torch.randn(B * S, ld, generator=g).to(gpu_device)
    y = F.add_vec_rows(x, vec, B, S)
    want = (x.view(B, S, ld) + torch.nn.functional.pad(vec, (0, ld - C))[:, None, :]).reshape(B * S, ld)
    assert torch.equal(y, want)
    gx, gv = torch.autograd.grad((y * w).sum(), (x, vec))
    rx, rv = torch.autograd.grad((want.double() * w.double()).sum(), (x, vec))
    assert torch.equal(gx, rx)
    bnd = K.bound(w.cpu().numpy(), B, S, ld)[:, :C]
    ref = w.double().view(B, S, ld).sum(1)[:, :C].cpu().numpy()
    assert gv.shape == (B, C) and K.ratio(gv.cpu().numpy(), ref, bnd) <= 1.0
    assert np.abs(rv.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()   # torch's own gradient is that sum
