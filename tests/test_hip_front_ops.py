"""The launches that open a denoiser step (slide_amd/csrc/engine.hip), ONE launch at a time: hand-built SlideOps run through
slide_run_ops on synthetic data; no engine and no sampler is involved.  tests/front_cases.py has the case tables, the references and
the derivation of every bound; tests/test_front_ops_host.py checks on the CPU that the checks reject the mutants.

  PREP_POINTS    lattice clouds: kidx / kd2 bit-equal to the stable (float32 d2, index) sort, every copy exact; Gaussian clouds: kd2
                 within the derived bound of float64, kidx a valid sort of the kernel's own kd2 and the reference's order wherever the
                 distances decide it; kw within its bound; nothing written outside what a copy owns
  TEMB / COND    within the derived bound of float64
  FINALIZE_GN    within the derived bound; gid -1: scale 1, shift 0 exactly; columns past C untouched
  COPY_COLS      exact in all four type pairs (round-to-nearest-even ties, subnormals, overflow); columns past n untouched
  ASSEMBLE_*     feature / coordinate columns exact, rel one fp32 subtraction, the FP weight within its bound, pads zero, nothing
                 written outside the rows; c_begin beyond the whole-vector pieces: -3"""
import ctypes

import numpy as np
import pytest

import front_cases as fc
from front_cases import F16, F32, U
from op_harness import SENTINEL, Dev, bits, run, status


def _full(d, shape, dt):
    return d.put(np.full(shape, SENTINEL, dt))


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------ PREP_POINTS
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in fc.PREP_CASES])
def test_prep_points(gpu_device, name):
    from slide_amd import abi
    c = fc.PREP_BY_NAME[name]
    B, cx, ldf = c["B"], c["cx"], c["ldf"]
    dt = F16 if c["f16"] else F32
    x = fc.prep_inputs(c)
    ref = fc.prep_reference(c, x)
    d = Dev(gpu_device)
    n = B * 16
    xyz, feat0 = _full(d, (n, 3), F32), _full(d, (n, ldf), dt)
    kidx, kd2 = d.put(np.full((n, 16), -7, np.int32)), _full(d, (n, 16), F32)
    nch = (cx + 31) // 32
    cm = _full(d, (nch, n, 32), dt) if c["cm"] else None
    kw = _full(d, (n, 16), F32) if c["kw"] else None
    cps = fc.prep_copies(c)
    bufs, tab = [], None
    if cps:
        t = (abi.SlidePrepCopy * len(cps))()
        for q, (cn, ld, kind) in enumerate(cps):
            bufs.append(_full(d, (n, ld), dt))
            t[q].dst, t[q].ld, t[q].kind, t[q].n = bufs[q].data_ptr(), ld, kind, cn
        tab = d.put(np.frombuffer(bytes(t), np.uint8).copy())
    run([abi.make_op(abi.OP_PREP_POINTS, i=(B, cx, ldf, abi.PREC_F16 if c["f16"] else abi.PREC_F32, len(cps)),
                     p=(d.put(x).data_ptr(), xyz.data_ptr(), feat0.data_ptr(), kidx.data_ptr(), kd2.data_ptr(), _ptr(cm), _ptr(tab), _ptr(kw)))])
    assert (bits(xyz.cpu().numpy()) == bits(ref["xyz"])).all()
    f0 = feat0.cpu().numpy()
    assert (bits(f0[:, :cx]) == bits(ref["feat0"])).all() and (f0[:, cx:] == dt(SENTINEL)).all()
    if cm is not None:
        got = cm.cpu().numpy()
        v = np.broadcast_to(ref["cm_valid"], got.shape)
        assert (bits(got)[v] == bits(ref["feat0_cm"])[v]).all() and (got[~v] == dt(SENTINEL)).all()
    for buf, want, (cn, ld, kind) in zip(bufs, ref["copies"], cps):
        got = buf.cpu().numpy()
        assert (bits(got[:, :cn]) == bits(want)).all() and (got[:, cn:] == dt(SENTINEL)).all(), (cn, ld, kind)
    gi, gd = kidx.cpu().numpy().reshape(B, 16, 16), kd2.cpu().numpy().reshape(B, 16, 16)
    if c["cloud"] in fc.LATTICES:
        assert (gi == ref["kidx"]).all() and (bits(gd) == bits(ref["kd2"])).all()
    else:
        assert (np.sort(gi, -1) == np.arange(16)).all(), "kidx is no permutation"
        dk = np.take_along_axis(ref["d64"], gi.astype(np.int64), -1)  # the float64 distance to the neighbour each slot names
        err = np.abs(gd.astype(np.float64) - dk) / np.maximum(fc.d2_bound(dk), 2.0 ** -149)
        print("prep_points %s: max |kd2 - float64| / bound %.3f" % (name, err.max()))
        assert (err <= 1).all()
        srt = (gd[..., 1:] > gd[..., :-1]) | ((gd[..., 1:] == gd[..., :-1]) & (gi[..., 1:] > gi[..., :-1]))
        assert srt.all(), "kidx is no (distance, index) sort of the kernel's own kd2"
        ok = fc.decided_slots(ref["kd2_64"])
        assert (gi[ok] == ref["kidx_64"][ok]).all()
    if kw is not None:
        gw = kw.cpu().numpy().reshape(B, 16, 16).astype(np.float64)
        assert (gw[..., 8:] == 0).all()
        r = np.abs(gw - ref["kw"])[..., :8] / (fc.KW_ULPS * U * ref["kw"][..., :8] * (1 + 64 * U))
        print("prep_points %s: max |kw - float64| / bound %.3f" % (name, r.max()))
        assert (r <= 1).all()


# ------------------------------------------------------------------------------------------------------------ TEMB / COND
@pytest.mark.gpu
@pytest.mark.parametrize("c", fc.TEMB_CASES, ids=lambda c: c["name"])
def test_temb(gpu_device, c):
    from slide_amd import abi
    dat = fc.temb_inputs(c)
    ref, bnd = fc.temb_forward(c, dat)
    d = Dev(gpu_device)
    ns, no = c["nsamp"], c["n_out"]
    out = _full(d, (ns + 1, no), F32)
    ts = None if c["ts"] is None else d.put(np.array(c["ts"], F32))
    t_dev = d.t_dev(fc.T_DEV0, 0)
    p = [_ptr(ts), t_dev.data_ptr()] + [d.put(dat[k]).data_ptr() for k in ("w1", "b1", "w2", "b2", "wfc", "bfc")] + [out.data_ptr(),
                                                                                                                  d.put(dat["freq"]).data_ptr()]
    run([abi.make_op(abi.OP_TEMB, i=(ns, c["t_dim"], no), p=p)])
    got = out.cpu().numpy()
    assert (got[ns] == F32(SENTINEL)).all()
    r = np.abs(got[:ns].astype(np.float64) - ref) / bnd
    print("temb %s: max |kernel - float64| / bound %.4f" % (c["name"], r.max()))
    assert (r <= 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("c", fc.COND_CASES, ids=lambda c: c["name"])
def test_cond(gpu_device, c):
    from slide_amd import abi
    dat = fc.cond_inputs(c)
    ref, bnd = fc.cond_forward(c, dat)
    d = Dev(gpu_device)
    B, no = c["B"], c["n_out"]
    out = _full(d, (B + 1, no), F32)
    run([abi.make_op(abi.OP_COND, i=(B, c["dim"], no), p=[d.put(dat[k]).data_ptr() for k in ("label", "emb", "wfc", "bfc")] + [out.data_ptr()])])
    got = out.cpu().numpy()
    assert (got[B] == F32(SENTINEL)).all()
    r = np.abs(got[:B].astype(np.float64) - ref) / bnd
    print("cond %s: max |kernel - float64| / bound %.4f" % (c["name"], r.max()))
    assert (r <= 1).all()


# ------------------------------------------------------------------------------------------------------------ FINALIZE_GN
@pytest.mark.gpu
@pytest.mark.parametrize("c", fc.FIN_CASES, ids=lambda c: c["name"])
def test_finalize_gn(gpu_device, c):
    from slide_amd import abi
    dat = fc.fin_inputs(c)
    scl, sft, dscl, dsft, _ = fc.fin_forward(c, dat)
    d = Dev(gpu_device)
    B, C, bs = c["B"], fc.FIN_C, fc.FIN_BS
    scale, shift = _full(d, (B, bs), F32), _full(d, (B, bs), F32)
    p = [d.put(dat[k]).data_ptr() for k in ("sum", "sq", "gid", "gstart", "gend", "gamma", "beta")] + [scale.data_ptr(), shift.data_ptr()]
    run([abi.make_op(abi.OP_FINALIZE_GN, i=(B, C, bs), f=(float(dat["inv_count"]),), p=p)])
    gs, gf = scale.cpu().numpy(), shift.cpu().numpy()
    assert (gs[:, C:] == F32(SENTINEL)).all() and (gf[:, C:] == F32(SENTINEL)).all()
    off = dat["gid"] < 0
    assert (gs[:, :C][:, off] == 1).all() and (gf[:, :C][:, off] == 0).all()
    on = ~off
    r = max((np.abs(gs[:, :C] - scl)[:, on] / dscl[:, on]).max(), (np.abs(gf[:, :C] - sft)[:, on] / dsft[:, on]).max())
    print("finalize_gn %s: max |kernel - float64| / bound %.4f" % (c["name"], r))
    assert r <= 1


# ------------------------------------------------------------------------------------------------------------ COPY_COLS
@pytest.mark.gpu
@pytest.mark.parametrize("c", fc.COPY_CASES, ids=lambda c: c["name"])
def test_copy_cols(gpu_device, c):
    from slide_amd import abi
    src = fc.copy_inputs(c)
    td = F16 if c["dst_f16"] else F32
    d = Dev(gpu_device)
    dst = _full(d, (c["rows"] + 1, c["dst_ld"]), td)
    run([abi.make_op(abi.OP_COPY_COLS, i=(c["rows"], c["n"], c["src_ld"], c["dst_ld"], c["src_f16"], c["dst_f16"]),
                     p=(d.put(src).data_ptr(), dst.data_ptr()))])
    got = dst.cpu().numpy()
    with np.errstate(over="ignore"):
        want = src[:, :c["n"]].astype(F32).astype(td)
    assert (bits(got[:c["rows"], :c["n"]]) == bits(want)).all()
    assert (got[:c["rows"], c["n"]:] == td(SENTINEL)).all() and (got[c["rows"]] == td(SENTINEL)).all()


# ------------------------------------------------------------------------------------------------------------ ASSEMBLE
GUARD = 64  # elements in front of and behind the output that must keep the sentinel


def _assemble(device, c):
    from slide_amd import abi
    dat = fc.asm_inputs(c)
    dt = F16 if c["f16"] else F32
    d = Dev(device)
    rows = c["B"] * 16 * c["K"]
    buf = _full(d, (GUARD + rows * c["ld_out"] + GUARD,), dt)
    out = buf.data_ptr() + GUARD * np.dtype(dt).itemsize
    p = [d.put(dat["xyz"]).data_ptr(), d.put(dat["feat"]).data_ptr(), d.put(dat["kidx"]).data_ptr()]
    p += [d.put(dat["kd2"]).data_ptr(), out] if c["fp"] else [out]
    op = abi.make_op(abi.OP_ASSEMBLE_FP if c["fp"] else abi.OP_ASSEMBLE_SA,
                     i=(c["B"], c["C"], c["ldf"], c["ldg"], c["K"], abi.PREC_F16 if c["f16"] else abi.PREC_F32, c["c_begin"],
                        c["ld_out"] if c["c_begin"] else 0), p=p)
    return d, dat, buf, op, rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in fc.ASM_CASES if c["status"] == 0])
def test_assemble(gpu_device, name):
    c = fc.ASM_BY_NAME[name]
    d, dat, buf, op, rows = _assemble(gpu_device, c)
    run([op])
    g, bnd, exact = fc.asm_forward(c, dat)
    dt = F16 if c["f16"] else F32
    got = buf.cpu().numpy()
    assert (got[:GUARD] == dt(SENTINEL)).all() and (got[-GUARD:] == dt(SENTINEL)).all(), "written outside the rows"
    got = got[GUARD:-GUARD].reshape(rows, c["ld_out"])
    w = c["ldg"] - c["c_begin"]  # the columns the launch owns: [c_begin, ldg) of the source layout
    assert (got[:, w:] == dt(SENTINEL)).all(), "columns past the source layout were written"
    got, g, bnd, exact = got[:, :w], g[:, c["c_begin"]:], bnd[:, c["c_begin"]:], exact[c["c_begin"]:]
    assert (bits(got[:, exact]) == bits(g.astype(dt)[:, exact])).all()
    assert (got[:, c["C"] - c["c_begin"] + (11 if c["fp"] else 9):] == 0).all(), "the pad columns are not zero"
    if c["fp"]:
        r = (np.abs(got.astype(np.float64) - g)[:, ~exact] / bnd[:, ~exact]).max()
        print("assemble %s: max |w - float64| / bound %.3f" % (name, r))
        assert r <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in fc.ASM_CASES if c["status"]])
def test_assemble_refuses_a_c_begin_beyond_the_vector_pieces(gpu_device, name):
    c = fc.ASM_BY_NAME[name]
    d, dat, buf, op, rows = _assemble(gpu_device, c)
    assert status(op) == c["status"] * 1000
    assert (buf.cpu().numpy() == (F16 if c["f16"] else F32)(SENTINEL)).all(), "a kernel ran"
