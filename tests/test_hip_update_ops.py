"""The DDPM update launches against numpy float32 restatements, BITWISE (tests/update_cases.py has the restatements, the case list
and the derivation of the noise bound).  The ops are hand-built SlideOps run through slide_run_ops on synthetic tables (T = 8); no
denoiser is involved.

  feature / position update   every case of update_cases with an explicit noise tensor; afterwards the key-point channels equal the
                              condition, t_dev[0..2] == [t - 1, step + 1, 0], t_dev[3..4] unchanged, columns a copy does not own untouched
  hand-over                   five launches back to back on one stream with no host synchronisation, eagerly and as a captured graph
                              replayed five times, on grids of one workgroup and of many: the state equals five sequential numpy steps,
                              t_dev[0..2] == [t0 - 5, 5, 0]
  in-kernel noise             the Philox path of both kernels equals the explicit-noise path fed with slide_philox_normal_selftest's
                              output for the same (seed, nonce, step, global element offset); the self-test's output is within
                              NORMAL_BOUND of the float64 restatement, and on the CPU a generator with two counter words swapped is not."""
import numpy as np
import pytest

import update_cases as uc
from op_harness import Dev as _Dev, bits as _bits, run as _run
from update_cases import C, F32, KDIM

SEED = (0x9E3779B9, 0x7F4A7C15)  # (seed_lo, seed_hi): both above 2^31, so the words cross the int ABI as bit patterns


# ------------------------------------------------------------------------------------------------------------ CPU
def test_restated_uniforms_are_open_unit_interval():
    u1, u2 = uc.philox_uniforms(*SEED, step=3, nonce=7, elem0=2 ** 32 - 100, n=4096)  # (the element number wraps at 2^32)
    for u in (u1, u2):
        assert u.dtype == F32 and u.min() > 0 and u.max() < 1.0 + 2.0 ** -24
    # Philox4x32-10's published known-answer vector for the all-zero counter and key (Random123's kat_vectors)
    w = uc.philox4x32_10(*[np.zeros(1, np.uint64)] * 4, 0, 0)
    assert [int(v[0]) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_noise_bound_rejects_a_swapped_counter_word():
    """the bound the GPU test asserts is met by the restatement rounded to float32 and missed by every mutant that swaps two of the
    four counter words"""
    n = 4096
    z, bound = uc.philox_normal_ref(*SEED, step=5, nonce=0x1234, elem0=777, n=n)
    assert bound.max() < 7e-6 and np.abs(z).max() < 6.0
    assert (np.abs(z.astype(F32).astype(np.float64) - z) <= bound).all()  # (one rounding is inside the four the bound allows)
    for a in range(4):
        for b in range(a + 1, 4):
            order = list(range(4))
            order[a], order[b] = order[b], order[a]
            zm, _ = uc.philox_normal_ref(*SEED, step=5, nonce=0x1234, elem0=777, n=n, order=tuple(order))
            assert (np.abs(zm - z) > bound).mean() > 0.99, order


def test_feature_restatement_keeps_the_condition_and_skips_noise_at_t0():
    x, eps, kp, cx0, km = uc.feat_inputs(16, 0, True, 1)
    tabs = uc.feat_tables()
    out = uc.feat_step(x, eps, kp, tabs, 0, None, 1.5, cx0, km)
    assert (out[:, :KDIM] == kp).all()
    pinned = km == 0  # mask 0: the predicted x0 is complete_x0, whatever the prediction says
    want = tabs[2][0] * cx0[pinned][:, KDIM:] + tabs[3][0] * x[pinned][:, KDIM:]
    assert (out[pinned][:, KDIM:] == want).all()


# ------------------------------------------------------------------------------------------------------------ GPU helpers
def _feat_op(d, x, eps, eps_ld, noise, t_dev, keypoint, tabs, clamp=0.0, cx0=None, kmask=None, feat0=None, ldf=0, half_out=0, copies=None,
             n_copies=0, seed=SEED):
    from slide_amd import abi
    p = lambda t: None if t is None else t.data_ptr()
    return abi.make_op(abi.OP_UPDATE_FEAT,
                       i=(x.shape[0], C, KDIM, uc.as_i32(seed[0]), uc.as_i32(seed[1]), eps_ld, ldf, half_out, n_copies), f=(clamp,),
                       p=(p(x), p(eps), p(noise), p(t_dev), p(keypoint)) + tuple(p(t) for t in tabs) + (p(cx0), p(kmask), p(feat0), p(copies)))


def _pos_op(d, x, eps, eps_ld, noise, t_dev, tabs, seed=SEED):
    from slide_amd import abi
    p = lambda t: None if t is None else t.data_ptr()
    return abi.make_op(abi.OP_UPDATE_POS, i=(x.numel(), eps_ld, uc.as_i32(seed[0]), uc.as_i32(seed[1])),
                       p=(p(x), p(eps), p(noise), p(t_dev)) + tuple(p(t) for t in tabs))


SENTINEL = 1234.5  # (exact in fp16 and fp32)


# ------------------------------------------------------------------------------------------------------------ feature update
@pytest.mark.gpu
@pytest.mark.parametrize("case", uc.FEAT_CASES, ids=[c[0] for c in uc.FEAT_CASES])
def test_feature_update_is_bitwise_the_restatement(gpu_device, case):
    import torch
    from slide_amd import abi
    name, npts, eps_ld, clamp, t, resample, f0, copies = case
    step, nonce, offset = 2, 0xCAFE, 3
    x, eps, kp, cx0, km = uc.feat_inputs(npts, eps_ld, resample, seed=100 + npts + eps_ld)
    tabs = uc.feat_tables()
    noise = np.random.RandomState(5).standard_normal((step + 1, npts * C)).astype(F32)
    d = _Dev(gpu_device)
    dx, deps, dkp, dnoise = d.put(x), d.put(eps), d.put(kp), d.put(noise)
    dtabs = [d.put(a) for a in tabs]
    dt = d.t_dev(t, step, nonce, offset)
    dcx0, dkm = (d.put(cx0), d.put(km)) if resample else (None, None)
    tdt = None if f0 is None else (torch.float16 if f0 == "f16" else torch.float32)
    ldf = 64
    feat0 = None if f0 is None else torch.full((npts, ldf), SENTINEL, dtype=tdt, device=gpu_device)
    bufs, tab = [], None
    if copies:
        assert f0 is not None
        tab = (abi.SlidePrepCopy * len(copies))()
        for q, (n, ld, kind) in enumerate(copies):
            bufs.append(torch.full((npts, ld), SENTINEL, dtype=tdt, device=gpu_device))
            tab[q].dst, tab[q].ld, tab[q].kind, tab[q].n = bufs[q].data_ptr(), ld, kind, n
        tab = d.put(np.frombuffer(bytes(tab), np.uint8).copy())
    _run([_feat_op(d, dx, deps, eps_ld, dnoise, dt, dkp, dtabs, clamp, dcx0, dkm, feat0, ldf if f0 else 0, int(f0 == "f16"), tab,
                   len(copies))])
    want = uc.feat_step(x, eps, kp, tabs, t, noise[step].reshape(npts, C) if t > 0 else None, clamp, cx0, km)
    got = dx.cpu().numpy()
    assert (_bits(got) == _bits(want)).all(), "max |diff| %g" % np.abs(got - want).max()
    assert (got[:, :KDIM] == kp).all()
    assert dt.cpu().numpy().tolist() == [t - 1, step + 1, 0, 0xCAFE, offset, 0, 0, 0]
    if f0 is not None:
        npd = np.float16 if f0 == "f16" else F32
        feat = want[:, KDIM:].astype(npd)

        def check(buf, n, what):
            b = buf.cpu().numpy()
            assert (_bits(b[:, :n]) == _bits(feat[:, :n])).all(), what
            assert (b[:, n:] == npd(SENTINEL)).all(), what + ": columns beyond the copy were written"
        check(feat0, C - KDIM, "feat0")
        for q, (n, ld, kind) in enumerate(copies):
            check(bufs[q], n if kind == 0 else 0, "copy %d" % q)


# ------------------------------------------------------------------------------------------------------------ position update
def _eps_rows(rs, n, eps_ld):
    """the prediction as the plan's last GEMM leaves it: rows of 3 (eps_ld == 0) or padded rows of eps_ld; and gathered per element"""
    eps = rs.standard_normal((n // 3, eps_ld or 3)).astype(F32)
    return eps, np.ascontiguousarray(eps[:, :3]).reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("n,eps_ld,t", uc.POS_CASES)
def test_position_update_is_bitwise_the_restatement(gpu_device, n, eps_ld, t):
    step = 1
    rs = np.random.RandomState(n + eps_ld)
    x = rs.standard_normal(n).astype(F32)
    eps, eps_flat = _eps_rows(rs, n, eps_ld)
    noise = rs.standard_normal((step + 1, n)).astype(F32)
    tabs = uc.pos_tables()
    d = _Dev(gpu_device)
    dx, deps, dnoise, dtabs, dt = d.put(x), d.put(eps), d.put(noise), [d.put(a) for a in tabs], d.t_dev(t, step, 9, 2)
    _run([_pos_op(d, dx, deps, eps_ld, dnoise, dt, dtabs)])
    want = uc.pos_step(x, eps_flat, tabs, t, noise[step] if t > 0 else None)
    assert (_bits(dx.cpu().numpy()) == _bits(want)).all()
    assert dt.cpu().numpy().tolist() == [t - 1, step + 1, 0, 9, 2, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ hand-over
T0, LAUNCHES = 4, 5  # t = 4, 3, 2, 1, 0: the last launch is the noise-free one and leaves t = -1


@pytest.mark.gpu
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "graph"))
@pytest.mark.parametrize("npts", (4, 336), ids=("one_workgroup", "many_workgroups"))
def test_feature_hand_over_five_launches(gpu_device, npts, graph):
    x, eps, kp, _, _ = uc.feat_inputs(npts, 0, False, seed=npts)
    tabs = uc.feat_tables()
    noise = np.random.RandomState(8).standard_normal((LAUNCHES, npts * C)).astype(F32)
    d = _Dev(gpu_device)
    dx, deps, dkp, dnoise, dtabs, dt = d.put(x), d.put(eps), d.put(kp), d.put(noise), [d.put(a) for a in tabs], d.t_dev(T0, 0)
    _run([_feat_op(d, dx, deps, 0, dnoise, dt, dkp, dtabs, 1.5)], times=LAUNCHES, graph=graph)
    want = x
    for k in range(LAUNCHES):
        want = uc.feat_step(want, eps, kp, tabs, T0 - k, noise[k].reshape(npts, C), 1.5)
    assert (_bits(dx.cpu().numpy()) == _bits(want)).all()
    assert dt.cpu().numpy().tolist()[:3] == [T0 - LAUNCHES, LAUNCHES, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "graph"))
@pytest.mark.parametrize("n", (48, 2400), ids=("one_workgroup", "many_workgroups"))
def test_position_hand_over_five_launches(gpu_device, n, graph):
    rs = np.random.RandomState(n)
    x = rs.standard_normal(n).astype(F32)
    eps, eps_flat = _eps_rows(rs, n, 8)
    noise = rs.standard_normal((LAUNCHES, n)).astype(F32)
    tabs = uc.pos_tables()
    d = _Dev(gpu_device)
    dx, deps, dnoise, dtabs, dt = d.put(x), d.put(eps), d.put(noise), [d.put(a) for a in tabs], d.t_dev(T0, 0)
    _run([_pos_op(d, dx, deps, 8, dnoise, dt, dtabs)], times=LAUNCHES, graph=graph)
    want = x
    for k in range(LAUNCHES):
        want = uc.pos_step(want, eps_flat, tabs, T0 - k, noise[k])
    assert (_bits(dx.cpu().numpy()) == _bits(want)).all()
    assert dt.cpu().numpy().tolist()[:3] == [T0 - LAUNCHES, LAUNCHES, 0]


# ------------------------------------------------------------------------------------------------------------ in-kernel noise
def _selftest(device, step, nonce, elem0, n):
    import torch
    from slide_amd import _lib
    out = torch.full((n,), float("nan"), device=device)
    _lib.check(_lib.lib().slide_philox_normal_selftest(uc.as_i32(SEED[0]), uc.as_i32(SEED[1]), uc.as_i32(step), uc.as_i32(nonce),
                                                       uc.as_i32(elem0), n, _lib.ptr(out), _lib.stream_of()), "slide_philox_normal_selftest")
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
def test_selftest_noise_is_within_the_derived_bound(gpu_device):
    n, step, nonce, elem0 = 20000, 3, 0xBEEF0001, 2 ** 32 - 5000  # (several workgroups; the element number wraps)
    got = _selftest(gpu_device, step, nonce, elem0, n).cpu().numpy().astype(np.float64)
    z, bound = uc.philox_normal_ref(*SEED, step=step, nonce=nonce, elem0=elem0, n=n)
    err = np.abs(got - z)
    print("philox_normal: max |kernel - float64| = %.3e (bound there %.3e), max error / bound = %.3f"
          % (err.max(), bound[err.argmax()], (err / bound).max()))
    assert (err <= bound).all()
    assert abs(got.mean()) < 0.03 and abs(got.std() - 1.0) < 0.03  # (20000 standard normals: 4 sigma of the mean is 0.028)


@pytest.mark.gpu
def test_selftest_rejects_bad_arguments(gpu_device):
    import torch
    from slide_amd import _lib
    buf = torch.zeros(4, device=gpu_device)
    L = _lib.lib()
    assert L.slide_philox_normal_selftest(0, 0, 0, 0, 0, -1, _lib.ptr(buf), _lib.stream_of()) == -2
    assert L.slide_philox_normal_selftest(0, 0, 0, 0, 0, 4, None, _lib.stream_of()) == -2
    assert L.slide_philox_normal_selftest(0, 0, 0, 0, 0, 0, None, _lib.stream_of()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("npts", (16, 336))
def test_feature_philox_path_equals_the_explicit_noise_path(gpu_device, npts):
    import torch
    t, step, nonce, offset = 5, 2, 0x51DE, 7  # (offset: t_dev[4], the global index of the chain's first sample)
    x, eps, kp, _, _ = uc.feat_inputs(npts, 64, False, seed=npts + 1)
    tabs = uc.feat_tables()
    z = _selftest(gpu_device, step, nonce, offset * 16 * C, npts * C)
    noise = torch.zeros((step + 1, npts * C), device=gpu_device)
    noise[step] = z
    outs = []
    for nz in (None, noise):
        d = _Dev(gpu_device)
        dx, deps, dkp, dtabs, dt = d.put(x), d.put(eps), d.put(kp), [d.put(a) for a in tabs], d.t_dev(t, step, nonce, offset)
        _run([_feat_op(d, dx, deps, 64, nz, dt, dkp, dtabs, 1.5)])
        outs.append(dx.cpu().numpy())
    assert (_bits(outs[0]) == _bits(outs[1])).all()
    want = uc.feat_step(x, eps, kp, tabs, t, z.cpu().numpy().reshape(npts, C), 1.5)
    assert (_bits(outs[0]) == _bits(want)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", (48, 2400))
def test_position_philox_path_equals_the_explicit_noise_path(gpu_device, n):
    import torch
    t, step, nonce, offset = 6, 1, 0x0DDBA11, 5
    rs = np.random.RandomState(n + 2)
    x = rs.standard_normal(n).astype(F32)
    eps, eps_flat = _eps_rows(rs, n, 0)
    tabs = uc.pos_tables()
    z = _selftest(gpu_device, step, nonce, offset * 48, n)
    noise = torch.zeros((step + 1, n), device=gpu_device)
    noise[step] = z
    outs = []
    for nz in (None, noise):
        d = _Dev(gpu_device)
        dx, deps, dtabs, dt = d.put(x), d.put(eps), [d.put(a) for a in tabs], d.t_dev(t, step, nonce, offset)
        _run([_pos_op(d, dx, deps, 0, nz, dt, dtabs)])
        outs.append(dx.cpu().numpy())
    assert (_bits(outs[0]) == _bits(outs[1])).all()
    assert (_bits(outs[0]) == _bits(uc.pos_step(x, eps_flat, tabs, t, z.cpu().numpy()))).all()
