"""SLIDE_OP_POINT_CHAIN (slide_amd/csrc/point_chain.hip), ONE launch at a time on synthetic data: hand-built SlidePointChainArgs run
through slide_run_ops; no engine and no sampler is involved.  tests/chain_cases.py has the case table, the float64 reference and the
derivation of the bounds; tests/test_point_chain_host.py checks on the CPU that the bounds reject the mutants.

  arithmetic      every case in both forms (fp16, and WIDE = all four *_lo pointers set): X[:, :128] and eps within the derived bound of
                  the float64 reference (max |kernel - ref| / bound is printed: profiles/point_chain_arith.md); the eps entries the
                  launch does not own (rows past `rows` of an over-allocated buffer) keep a sentinel, X[:, 128:] and the pads of X are
                  unchanged, the NaN in the pads of Z reaches no output
  fused update    fuse_update = 1: eps bit-equal to the plain launch, x BITWISE update_cases.feat_step of that eps, the key-point
                  channels equal the condition, t_dev handed over; the Philox path equals the explicit-noise path; three launches back
                  to back (eagerly and as one captured graph replayed three times) read the t their predecessor left
  refusals        -3 and nothing launched for a partly set *_lo quartet, kz 200, k0 128, eps_ld 6, C > 32 n1c with fuse_update"""
import ctypes

import numpy as np
import pytest

import chain_cases as cc
import update_cases as uc
from op_harness import SENTINEL, Dev, bits, run, status

F32, F16 = np.float32, np.float16
SEED = (0x9E3779B9, 0x7F4A7C15)


class _Chain:
    """the device buffers of one case and its SlidePointChainArgs"""

    def __init__(self, device, c, d, form, t_dev=None):
        from slide_amd import abi
        self.c, self.dev = c, Dev(device)
        put = self.dev.put
        rows, kz, k0 = c["rows"], c["kz"], c["k0"]
        ra = rows + cc.EXTRA_ROWS
        Z = np.full((ra, c["z_ld"]), np.nan, F16)  # NaN in the pads and in the rows past `rows`
        Z[:rows, :kz] = d["Z"]
        X = np.full((ra, c["x_ld"]), SENTINEL, F16)
        X[:rows, 128:k0] = d["Xin"]
        self.X0 = X
        self.Z, self.X = put(Z), put(X)
        self.eps = put(np.full(ra * c["eps_ld"], SENTINEL, F32))
        a = self.args = abi.SlidePointChainArgs()
        a.Z, a.X, a.eps = self.Z.data_ptr(), self.X.data_ptr(), self.eps.data_ptr()
        for k in ("Wz", "W2", "W0", "W1"):
            hi, lo = cc.split(d[k])
            setattr(a, k, put(hi.astype(F16)).data_ptr())
            if form == "wide":
                setattr(a, k + "_lo", put(lo.astype(F16)).data_ptr())
        a.vz, a.v2, a.v0, a.b1 = (put(d[k].reshape(-1)).data_ptr() for k in ("vz", "v2", "v0", "b_out"))
        a.rows, a.z_ld, a.kz, a.x_ld, a.k0, a.n1c, a.eps_ld = rows, c["z_ld"], kz, c["x_ld"], k0, c["n1c"], c["eps_ld"]
        self.t_dev = t_dev if t_dev is not None else self.dev.t_dev(cc.T_ROW, 0)
        if c["tvec"] == "shared":
            a.tvec, a.t_idx, a.t_stride, a.t_bs = put(d["ttab"]).data_ptr() + 4 * cc.T_COFF, self.t_dev.data_ptr(), cc.T_STRIDE, 0
        elif c["tvec"] == "sample":
            a.tvec, a.t_idx, a.t_stride, a.t_bs = put(d["ttab"]).data_ptr() + 4 * cc.T_BS_COFF, None, 0, cc.T_BS
        if c["cvec"]:
            a.cvec, a.c_bs = put(d["ctab"]).data_ptr() + 4 * cc.C_COFF, cc.C_BS

    def op(self):
        from slide_amd import abi
        return abi.make_op(abi.OP_POINT_CHAIN, p=(ctypes.addressof(self.args),))

    def outputs(self):
        c = self.c
        X = self.X.cpu().numpy()
        eps = self.eps.cpu().numpy()
        n = c["rows"] * c["eps_ld"]
        return X, eps[:n].reshape(c["rows"], c["eps_ld"]), eps[n:]

    def check_poison(self):
        """what the launch does not own is untouched; returns (X[:, :128] as float64, eps)"""
        c = self.c
        X, eps, tail = self.outputs()
        assert (tail == F32(SENTINEL)).all(), "eps rows past `rows` were written"
        assert (bits(X[:, 128:]) == bits(self.X0[:, 128:])).all(), "X[:, 128:] or the pad of X changed"
        assert (X[c["rows"]:] == F16(SENTINEL)).all(), "X rows past `rows` were written"
        assert np.isfinite(X[:c["rows"], :128].astype(F32)).all() and np.isfinite(eps).all(), "a NaN of the pads of Z reached an output"
        return X[:c["rows"], :128].astype(np.float64), eps


_REF = {}


def _ref(name, form):
    """(data, float64 reference) of a case, computed once and shared (read-only) by the tests that need it"""
    if (name, form) not in _REF:
        c = cc.CASE_BY_NAME[name]
        d = _REF[name, None] = _REF.get((name, None)) or cc.make_data(c)
        _REF[name, form] = (d, cc.forward(c, d, form))
    return _REF[name, form]


# ------------------------------------------------------------------------------------------------------------ arithmetic
@pytest.mark.gpu
@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("name", [c["name"] for c in cc.CASES])
def test_point_chain_is_within_the_derived_bound(gpu_device, name, form):
    c = cc.CASE_BY_NAME[name]
    d, ref = _ref(name, form)
    ch = _Chain(gpu_device, c, d, form)
    run([ch.op()])
    X, eps = ch.check_poison()
    r = cc.ratios(dict(X=X, eps=eps.astype(np.float64)), ref)
    print("point_chain %s %s: max |kernel - float64| / bound: X %.3f, eps %.3f (max bound X %.2e, eps %.2e)"
          % (name, form, r["X"], r["eps"], ref["X"][2].max(), ref["eps"][2].max()))
    assert r["X"] <= 1.0 and r["eps"] <= 1.0, r


# ------------------------------------------------------------------------------------------------------------ fused update
T = uc.T
KDIM = 3
# name, case of chain_cases (n1c / eps_ld / rows / tvec form), C, t, clamp, resample, eps set
FUSED = [
    ("r16_c19_t5", "r16_kz32", 19, 5, 0.0, False, True),
    ("r16_c19_t0_clamp_rs_noeps", "r16_kz32", 19, 0, 1.5, True, False),
    ("r48_c51_t3_clamp_rs", "r48_kz192_common", 51, 3, 1.5, True, True),
    ("r48_c51_t0_noeps", "r48_kz192_common", 51, 0, 0.0, False, False),
    ("r48_c19_t7_noeps", "r48_kz32_pad_common", 19, 7, 1.5, False, False),
    ("r16_c51_t2", "r16_kz96_gnmean", 51, 2, 0.0, True, True),
]


def _feat_inputs(npts, C, resample, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((npts, C)).astype(F32)
    kp = rs.uniform(-1, 1, (npts, KDIM)).astype(F32)
    cx0 = rs.standard_normal((npts, C)).astype(F32) if resample else None
    km = (rs.uniform(size=npts) < 0.5).astype(F32) if resample else None
    return x, kp, cx0, km


def _fuse(ch, C, x, kp, tabs, clamp=0.0, cx0=None, km=None, noise=None, eps=True):
    """turns the chain's launch into the fused one; returns the device state x"""
    put = ch.dev.put
    a, u = ch.args, ch.args.upd
    a.fuse_update = 1
    if not eps:
        a.eps = None
    u.kind, u.C, u.kdim, u.clamp, u.seed_lo, u.seed_hi = 1, C, KDIM, clamp, SEED[0], SEED[1]
    dx = put(x)
    u.x, u.t_dev, u.keypoint = dx.data_ptr(), ch.t_dev.data_ptr(), put(kp).data_ptr()
    u.t0, u.t1, u.t2, u.t3, u.t4 = (put(t).data_ptr() for t in tabs)
    if cx0 is not None:
        u.complete_x0, u.kmask = put(cx0).data_ptr(), put(km).data_ptr()
    if noise is not None:
        u.noise = (noise if hasattr(noise, "data_ptr") else put(noise)).data_ptr()
        ch.dev.keep.append(noise)
    return dx


def _plain_eps(device, c, d, form, t):
    """eps of the plain (fuse_update = 0) launch at timestep t, [rows][eps_ld]"""
    ch = _Chain(device, c, d, form, t_dev=Dev(device).t_dev(t, 0))
    run([ch.op()])
    return ch.outputs()[1]


@pytest.mark.gpu
@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("case", FUSED, ids=[f[0] for f in FUSED])
def test_fused_update_is_bitwise_the_restatement(gpu_device, case, form):
    _, name, C, t, clamp, resample, eps_set = case
    c = cc.CASE_BY_NAME[name]
    assert C <= c["eps_ld"] and C <= 32 * c["n1c"]
    d = _ref(name, form)[0]
    npts, step, nonce, offset = c["rows"], 2, 0xCAFE, 3
    eps0 = _plain_eps(gpu_device, c, d, form, t)
    x, kp, cx0, km = _feat_inputs(npts, C, resample, seed=npts + C)
    tabs = uc.feat_tables()
    noise = np.random.RandomState(5).standard_normal((step + 1, npts * C)).astype(F32)
    ch = _Chain(gpu_device, c, d, form, t_dev=Dev(gpu_device).t_dev(t, step, nonce, offset))
    dx = _fuse(ch, C, x, kp, tabs, clamp, cx0, km, noise, eps_set)
    run([ch.op()])
    _, eps1, tail = ch.outputs()
    if eps_set:
        assert (bits(eps1) == bits(eps0)).all(), "eps of the fused launch differs from the plain launch's"
    else:
        assert (eps1 == F32(SENTINEL)).all(), "eps NULL: the buffer the test kept was written"
    assert (tail == F32(SENTINEL)).all()
    want = uc.feat_step(x, eps0, kp, tabs, t, noise[step].reshape(npts, C) if t > 0 else None, clamp, cx0, km, kdim=KDIM)
    got = dx.cpu().numpy()
    assert (bits(got) == bits(want)).all(), "max |diff| %g" % np.abs(got - want).max()
    assert (got[:, :KDIM] == kp).all()
    assert ch.t_dev.cpu().numpy().tolist() == [t - 1, step + 1, 0, 0xCAFE, offset, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("name,C", [("r16_kz32", 19), ("r48_kz192_common", 51)])
def test_fused_philox_path_equals_the_explicit_noise_path(gpu_device, name, C):
    import torch
    from slide_amd import _lib
    c = cc.CASE_BY_NAME[name]
    d = _ref(name, "wide")[0]
    npts, t, step, nonce, offset = c["rows"], 5, 2, 0x51DE, 7  # (offset: t_dev[4], the global index of the chain's first sample)
    z = torch.full((npts * C,), float("nan"), device=gpu_device)
    _lib.check(_lib.lib().slide_philox_normal_selftest(uc.as_i32(SEED[0]), uc.as_i32(SEED[1]), step, uc.as_i32(nonce), offset * 16 * C,
                                                       npts * C, _lib.ptr(z), _lib.stream_of()), "slide_philox_normal_selftest")
    torch.cuda.synchronize()
    noise = torch.zeros((step + 1, npts * C), device=gpu_device)
    noise[step] = z
    x, kp, _, _ = _feat_inputs(npts, C, False, seed=npts + C + 1)
    tabs = uc.feat_tables()
    outs = []
    for nz in (None, noise):
        ch = _Chain(gpu_device, c, d, "wide", t_dev=Dev(gpu_device).t_dev(t, step, nonce, offset))
        dx = _fuse(ch, C, x, kp, tabs, 1.5, noise=nz)
        run([ch.op()])
        outs.append(dx.cpu().numpy())
    assert (bits(outs[0]) == bits(outs[1])).all()
    eps0 = _plain_eps(gpu_device, c, d, "wide", t)
    want = uc.feat_step(x, eps0, kp, tabs, t, z.cpu().numpy().reshape(npts, C), 1.5, kdim=KDIM)
    assert (bits(outs[0]) == bits(want)).all()


T0, LAUNCHES = 2, 3  # t = 2, 1, 0: the last launch is the noise-free one and leaves t = -1


@pytest.mark.gpu
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "graph"))
@pytest.mark.parametrize("name,C", [("r16_kz96_gnmean", 51), ("r112_kz192_pad", 19)], ids=("one_workgroup", "four_workgroups"))
def test_fused_hand_over_three_launches(gpu_device, name, C, graph):
    """the shared-row tvec form reads row t_idx[0] = t_dev[0]: every launch must see the t its predecessor handed over"""
    c = cc.CASE_BY_NAME[name]
    assert c["tvec"] == "shared"
    d = _ref(name, "wide")[0]
    npts = c["rows"]
    x, kp, _, _ = _feat_inputs(npts, C, False, seed=npts + C + 2)
    tabs = uc.feat_tables()
    noise = np.random.RandomState(8).standard_normal((LAUNCHES, npts * C)).astype(F32)
    ch = _Chain(gpu_device, c, d, "wide", t_dev=Dev(gpu_device).t_dev(T0, 0))
    dx = _fuse(ch, C, x, kp, tabs, 1.5, noise=noise)
    run([ch.op()], times=LAUNCHES, graph=graph)
    want = x
    eps_t = [_plain_eps(gpu_device, c, d, "wide", T0 - k) for k in range(LAUNCHES)]
    assert not (bits(eps_t[0]) == bits(eps_t[1])).all()  # (the prediction does depend on the t row)
    for k in range(LAUNCHES):
        want = uc.feat_step(want, eps_t[k], kp, tabs, T0 - k, noise[k].reshape(npts, C), 1.5, kdim=KDIM)
    assert (bits(dx.cpu().numpy()) == bits(want)).all()
    assert ch.t_dev.cpu().numpy().tolist()[:3] == [T0 - LAUNCHES, LAUNCHES, 0]
    assert (bits(ch.outputs()[1]) == bits(eps_t[-1])).all()  # (eps of the last launch: t = 0)


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
@pytest.mark.parametrize("what", ("lo_quartet", "kz_200", "k0_128", "eps_ld_6", "fuse_C_over_32_n1c"))
def test_launcher_refuses(gpu_device, what):
    c = cc.CASE_BY_NAME["r16_kz32"]
    d = _ref("r16_kz32", "wide")[0]
    ch = _Chain(gpu_device, c, d, "wide")
    a = ch.args
    if what == "lo_quartet":
        a.W0_lo = None
    elif what == "kz_200":
        a.kz, a.z_ld = 200, 200
    elif what == "k0_128":
        a.k0 = 128
    elif what == "eps_ld_6":
        a.eps_ld = 6
    else:
        x, kp, _, _ = _feat_inputs(c["rows"], 33, False, seed=1)
        _fuse(ch, 33, x, kp, uc.feat_tables())
    assert status(ch.op()) == -3 * 1000  # (slide_run_ops: status * 1000 - index of the failing op)
    X, eps, tail = ch.outputs()
    assert (eps == F32(SENTINEL)).all() and (tail == F32(SENTINEL)).all() and (X[:, :128] == F16(SENTINEL)).all(), "a kernel ran"
