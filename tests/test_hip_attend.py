"""SLIDE_OP_GEMM_ATTEND, one launch at a time, against float64 at the elementwise bound of tests/attend_cases.py (the case matrix, the
reference, the derivation and the mutants; its CPU half is tests/test_attend_host.py): hand-built SlideOps through slide_run_ops
(tests/op_harness.py), no module, engine or sampler -- the per-launch companion of
tests/test_hip_modules.py::test_attention_fused_score_gemm_and_attend, which holds a whole AttentionModule to a relative L2 norm.
Also: slide_amd.rows.conv_attend packs the same op as the hand-built one, and every refusal of run_gemm_attend by status with the
output untouched."""
import types

import numpy as np
import pytest

import attend_cases as ac
from attend_cases import CASES, CASE_BY_NAME, forward, make_data, physical, ratio
from op_harness import SENTINEL, Dev, bits, run, status

F16 = np.float16


def _epi(d, bias, n_cob, packed):
    """the descriptor array of the launch (only the bias is read), with the packed [bias | gamma | beta] vectors behind it or without"""
    from slide_amd import abi
    bt = d.put(bias.astype(np.float32))
    tab = (abi.SlideEpi * n_cob)()
    for j in range(n_cob):
        tab[j].mode, tab[j].out_ld, tab[j].bias = abi.EPI_RAW, n_cob * 32, bt.data_ptr() + 4 * 32 * j
    raw = np.frombuffer(bytes(tab), dtype=np.uint8)
    if packed:
        pv = np.zeros((n_cob, 3, 32), np.float32)
        pv[:, 0] = bias.reshape(n_cob, 32)
        raw = np.concatenate([raw, pv.reshape(-1).view(np.uint8)])
    return d.put(raw.copy()).data_ptr() | (abi.EPI_PACKED_VECS if packed else 0)


def _out(d, c):
    """[points + 1][ldo] of SENTINEL: the last row and the columns past n_cob * 32 belong to nobody"""
    return d.put(np.full((c["rows"] // c["K"] + 1, c["ldo"]), SENTINEL, F16))


def _op(c, t, out, over=()):
    """the SlideOp of a case from its device tensors t (X, W, V, epi and, where the case has them, counts, vss, ss, add)"""
    from slide_amd import abi
    ptr = lambda k: None if t.get(k) is None else t[k].data_ptr()
    kp = c["k_pad"]
    i = dict(rows=c["rows"], x_ld=c["x_ld"], k_pad=kp, n_cob=c["n_cob"], K=c["K"], in_bs=0, ldv=c["ldv"], ldo=c["ldo"], pps=c["pps"],
             v_relu=int(c["vss"] == "relu"), C=c["C"])
    f = [0.0, 0.0, 0.0, 0.0]
    p = dict(X=ptr("X"), W=ptr("W"), epi=t["epi"], sc=None, sh=None, V=ptr("V"), out=out.data_ptr(), counts=ptr("counts"), vss=ptr("vss"),
             add=None)
    if c["aff"]:
        i["in_bs"] = 2 * kp
        p["sc"], p["sh"] = t["ss"].data_ptr(), t["ss"].data_ptr() + 4 * kp
        add_bs = t["add"].shape[1] if t.get("add") is not None else 0
        p["add"] = ptr("add")
        f = [0.0, float(c["tps"]), float(add_bs), float(2 * c["add_n"] + int(c["aff_relu"]))]
    for k, v in dict(over).items():
        (i if k in i else p)[k] = v
    return abi.make_op(abi.OP_GEMM_ATTEND, i=[i[k] for k in ("rows", "x_ld", "k_pad", "n_cob", "K", "in_bs", "ldv", "ldo", "pps", "v_relu", "C")],
                       f=f, p=[p[k] for k in ("X", "W", "epi", "sc", "sh", "V", "out", "counts", "vss")] + [None, None, p["add"]])


def _upload(d, c, dat):
    p = physical(c, dat)
    t = {k: d.put(p[k]) for k in ("X", "W", "V", "counts", "vss", "ss", "add") if k in p}
    t["epi"] = _epi(d, p["bias"], c["n_cob"], c["packed"])
    return t


def _check(c, ref, got, what=""):
    """got: the whole output buffer [points + 1][ldo]"""
    pts, nch = c["rows"] // c["K"], c["n_cob"] * 32
    assert (bits(got[pts]) == bits(F16(SENTINEL))).all() and (bits(got[:, nch:]) == bits(F16(SENTINEL))).all(), "written outside the output"
    g = got[:pts, :nch].astype(np.float64)
    assert np.isfinite(g).all()
    r = ratio(ref, g)
    k = np.unravel_index(np.argmax(r), r.shape)
    print("%s%s [AFF=%s]: worst err/bound %.4f at %s (err %.3g, |ref| %.3g), exact elements %d" %
          (c["name"], what, c["aff"], r[k], k, abs(g[k] - ref["y"][k]), abs(ref["y"][k]), int((ref["b"] == 0).sum())))
    assert r.max() <= 1, (c["name"], float(r.max()), k)
    assert (g[:, c["C"]:] == 0).all(), "pad channels must be zero"


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_gemm_attend_matches_float64(gpu_device, name):
    c = CASE_BY_NAME[name]
    d = Dev(gpu_device)
    dat = make_data(c)
    t = _upload(d, c, dat)
    out, out2 = _out(d, c), _out(d, c)
    assert status(_op(c, t, out)) == 0
    got = out.cpu().numpy()
    _check(c, forward(c, dat), got)
    run([_op(c, t, out2)])  # (no atomics, no order-dependent sums: a second launch reproduces every bit)
    assert (bits(out2.cpu().numpy()) == bits(got)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("base", ["ties8", "aff_tps1_add_relu"])
def test_conv_attend_packs_the_same_op(gpu_device, monkeypatch, base):
    """slide_amd.rows.conv_attend on a plain and on a deferred input: the op it launches has the i / f fields of the hand-built op of
    the same tensors, and the same output bits (and that output is inside the float64 bound)"""
    import torch
    from slide_amd import rows as R
    c0 = CASE_BY_NAME[base]
    B = ac.n_smp(c0) if c0["aff"] else 1
    S = c0["rows"] // B
    c = dict(c0, name=base + "_module", pps=S // c0["K"], packed=True)  # (conv_attend: value-samples are the input's samples)
    assert c["x_ld"] == c["k_pad"] == ac.ru(c["kl"]) and c["ldo"] == c["n_cob"] * 32 == ac.ru(c["C"])
    d = Dev(gpu_device)
    dat = make_data(c)
    p = physical(c, dat)
    t = _upload(d, c, dat)
    if c["add_n"]:
        t["add"] = d.put(p["add"][:, :c["add_n"]])  # [samples][add_n], as norm_act hands the embedding over: add_bs = add_n
    u = R.Rows(t["X"], B, S, c["kl"])
    if c["aff"]:
        u.pending = (t["ss"], c["aff_relu"], t.get("add"))
    values = R.Rows(t["V"], B, S, c["C"])
    if c["vss"]:
        values.pending = (t["vss"], c["vss"] == "relu", None)
    mod = types.SimpleNamespace(weight=d.put(dat["W"].reshape(c["C"], c["kl"], 1, 1)), bias=d.put(dat["bias"][:c["C"]]))
    counts = t["counts"].reshape(B, -1) if c["counts"] else None
    seen = []
    real_run = R._run
    monkeypatch.setattr(R, "_run", lambda op: (seen.append(op), real_run(op))[1])
    monkeypatch.setenv("SLIDE_MODULE_FUSE_ATTEND", "1")
    res = R.conv_attend(u, mod, values, c["K"], counts)
    torch.cuda.synchronize()
    assert [o.kind for o in seen] == [R.OP_GEMM_ATTEND]
    out = _out(d, c)
    mine = _op(c, t, out)
    assert list(seen[0].i) == list(mine.i) and list(seen[0].f) == list(mine.f)
    for k in (0, 3, 4, 5, 7, 8, 11):  # X, scale, shift, V, counts, vss, add: the very same tensors
        assert seen[0].p[k] == mine.p[k], k
    run([mine])
    got = out.cpu().numpy()
    assert (bits(res.data.cpu().numpy()) == bits(got[:-1])).all()
    assert (res.B, res.S, res.C) == (B, S // c["K"], c["C"])
    _check(c, forward(c, dat), got, " via conv_attend")


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refusal_base(gpu_device, name):
    c = CASE_BY_NAME[name]
    d = Dev(gpu_device)
    t = _upload(d, c, make_data(c))
    return c, d, t, _out(d, c)


def _refused(op, out, want):
    assert status(op) == want * 1000  # (slide_run_ops: status * 1000 - index of the failing op)
    assert (bits(out.cpu().numpy()) == bits(F16(SENTINEL))).all(), "a kernel ran"


REFUSALS = dict(k5=dict(K=5), rows_mod_k=dict(rows=256 - 2), k_pad_mod32=dict(k_pad=48), x_ld_mod8=dict(x_ld=100), n_cob0=dict(n_cob=0),
                null_x=dict(X=None), null_w=dict(W=None), null_epi=dict(epi=None), null_v=dict(V=None), null_out=dict(out=None),
                ldv_mod4=dict(ldv=98), ldo_narrow=dict(ldo=32))


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_gemm_attend_refuses(gpu_device, what):
    c, d, t, out = _refusal_base(gpu_device, "k4_counts")
    _refused(_op(c, t, out, REFUSALS[what]), out, -3)


@pytest.mark.gpu
def test_gemm_attend_refuses_a_scale_without_a_shift(gpu_device):
    c, d, t, out = _refusal_base(gpu_device, "aff_tps1_add_relu")
    _refused(_op(c, t, out, dict(sh=None)), out, -3)


@pytest.mark.gpu
def test_gemm_attend_refuses_an_affine_beyond_its_lds(gpu_device):
    """k_pad = 2048 with the input affine: three fp16 vectors of k_pad behind the two-stage ring pass the 53 KB of three workgroups
    per CU -- status -8 from the launcher, nothing launched (1536, the widest the module sends, fits: case kp1536_aff)"""
    c = dict(CASE_BY_NAME["aff_tps1_add_relu"], name="aff_kp2048", kl=2048, k_pad=2048, x_ld=2048, add_n=0)
    d = Dev(gpu_device)
    t = _upload(d, c, make_data(c))
    out = _out(d, c)
    _refused(_op(c, t, out), out, -8)


@pytest.mark.gpu
@pytest.mark.parametrize("what,rows,tps", [("ragged", 256 + 8, 1), ("tiles_not_whole_samples", 768, 2), ("below_one_sample", 256, 2)])
def test_gemm_attend_refuses_the_affine_on_partial_samples(gpu_device, what, rows, tps):
    """with in_scale the kernel takes a tile's sample from the tile index: rows must be a multiple of 256 * tiles-per-sample (a ragged
    last tile would silently take the previous sample's affine, fewer rows than one sample index sample -1).  Status only: the shape
    is never launched."""
    c, d, t, out = _refusal_base(gpu_device, "aff_tps1_add_relu")
    assert rows <= c["rows"] and rows % c["K"] == 0 and rows % (256 * tps) != 0
    _refused(_op(dict(c, tps=tps), t, out, dict(rows=rows)), out, -3)
