"""SLIDE_OP_TRANSPOSE and SLIDE_OP_GROUPNORM_NCHW (csrc/engine.hip; slide_amd.nn_ops.HipConv1x1 / HipGroupNorm), one launch at a time:
the transpose bit for bit against numpy, GroupNorm against float64 at the derived bound of tests/nchw_cases.py (cases, references,
mutants; CPU half: tests/test_nchw_ops_host.py) -- hand-built SlideOps through slide_run_ops (tests/op_harness.py).  And every
refusal of the two launches' argument checks, by status with the outputs untouched."""
import numpy as np
import pytest

import nchw_cases as nc
from op_harness import SENTINEL, Dev, bits, run, status

F16, F32 = np.float16, np.float32
GUARD = 64


def _tr_op(c, src, dst, over=()):
    from slide_amd import abi
    i = dict(B=c["B"], R=c["R"], C=c["C"], in_ld=c["in_ld"], out_ld=c["out_ld"], in_bs=c["in_bs"], out_bs=c["out_bs"], f16=int(c["f16"]))
    p = dict(src=src.data_ptr(), dst=dst.data_ptr())
    for k, v in dict(over).items():
        (i if k in i else p)[k] = v
    return abi.make_op(abi.OP_TRANSPOSE, i=list(i.values()), p=[p["src"], p["dst"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in nc.TR_CASES])
def test_transpose_is_bit_exact(gpu_device, name):
    c = nc.TR_BY_NAME[name]
    d = Dev(gpu_device)
    dat = nc.tr_data(c)
    dt = F16 if c["f16"] else F32
    want = nc.tr_expected(c, dat, SENTINEL)
    src = d.put(dat["buf"])
    dst = d.put(np.full(want.size + GUARD, SENTINEL, dt))
    run([_tr_op(c, src, dst)])
    got = dst.cpu().numpy()
    assert (bits(got[want.size:]) == bits(dt(SENTINEL))).all(), "written past the last matrix"
    bad = np.flatnonzero(bits(got[:want.size]) != bits(want))
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


def _gn_op(c, t, over=()):
    from slide_amd import abi
    i = dict(B=c["B"], C=c["C"], HW=c["HW"], G=c["G"], n_norm=c["n_norm"], relu=int(c["relu"]))
    p = {k: t[k].data_ptr() for k in ("x", "gamma", "beta", "y")}
    for k, v in dict(over).items():
        (i if k in i else p)[k] = v
    return abi.make_op(abi.OP_GROUPNORM_NCHW, i=list(i.values()), p=[p[k] for k in ("x", "gamma", "beta", "y")])


def _gn_upload(d, c, dat):
    n = c["B"] * c["C"] * c["HW"]
    return dict(x=d.put(dat["x"]), gamma=d.put(dat["gamma"]), beta=d.put(dat["beta"]), y=d.put(np.full(n + GUARD, SENTINEL, F32)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in nc.GN_CASES])
def test_groupnorm_nchw_matches_float64(gpu_device, name):
    c = nc.GN_BY_NAME[name]
    d = Dev(gpu_device)
    dat = nc.gn_data(c)
    t = _gn_upload(d, c, dat)
    run([_gn_op(c, t)])
    got = t["y"].cpu().numpy()
    n = c["B"] * c["C"] * c["HW"]
    assert (bits(got[n:]) == bits(F32(SENTINEL))).all(), "written past the tensor"
    ref = nc.gn_forward(c, dat)
    g = got[:n].reshape(c["B"], c["C"], c["HW"])
    r = nc.ratio(ref, g)
    k = np.unravel_index(np.argmax(r), r.shape)
    print("groupnorm_nchw %s: worst err/bound %.4f at %s (err %.3g, |ref| %.3g)" % (name, r[k], k, abs(g[k] - ref["y"][k]), abs(ref["y"][k])))
    assert r.max() <= 1, (name, float(r.max()), k)
    tail = g[:, c["n_norm"]:]
    assert (bits(tail) == bits(ref["stored"][:, c["n_norm"]:].astype(F32))).all(), "the pass-through channels are a copy (or max(x, 0))"


# ------------------------------------------------------------------------------------------------------------------ refusals
TR_REFUSALS = dict(b0=dict(B=0), b_neg=dict(B=-1), b_past_grid_z=dict(B=65536), r0=dict(R=0), c0=dict(C=0), c_neg=dict(C=-3),
                   in_ld_narrow=dict(in_ld=30), out_ld_narrow=dict(out_ld=32), null_in=dict(src=None), null_out=dict(dst=None))


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("what", sorted(TR_REFUSALS))
def test_transpose_refuses(gpu_device, what, f16):
    c = nc.TR_BY_NAME["b2_33x31_" + ("f16" if f16 else "f32")]
    d = Dev(gpu_device)
    dt = F16 if f16 else F32
    src = d.put(nc.tr_data(c)["buf"])
    dst = d.put(np.full(nc.tr_sizes(c)[1], SENTINEL, dt))
    assert status(_tr_op(c, src, dst, TR_REFUSALS[what])) == -3000  # (slide_run_ops: status * 1000 - index of the failing op)
    assert (bits(dst.cpu().numpy()) == bits(dt(SENTINEL))).all(), "a kernel ran"


GN_REFUSALS = dict(b0=dict(B=0), b_past_grid_y=dict(B=65536), c0=dict(C=0), hw0=dict(HW=0), hw_neg=dict(HW=-1), g0=dict(G=0), g_neg=dict(G=-2),
                   n_norm_mod_g=dict(n_norm=5), n_norm_past_c=dict(n_norm=10), n_norm0=dict(n_norm=0), null_x=dict(x=None),
                   null_gamma=dict(gamma=None), null_beta=dict(beta=None), null_y=dict(y=None))


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(GN_REFUSALS))
def test_groupnorm_nchw_refuses(gpu_device, what):
    c = nc.GN_BY_NAME["n300_tail_relu"]  # C = 8, G = 2, n_norm = 6
    d = Dev(gpu_device)
    t = _gn_upload(d, c, nc.gn_data(c))
    assert status(_gn_op(c, t, GN_REFUSALS[what])) == -3000
    assert (bits(t["y"].cpu().numpy()) == bits(F32(SENTINEL))).all(), "a kernel ran"
