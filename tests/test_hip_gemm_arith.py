"""SLIDE_OP_GEMM in all three arithmetics (exact fp32, fp16 operands, two-term fp16 split) against float64, elementwise, at
bounds derived from the arithmetic (tests/gemm_cases.py: the case matrix, the reference, the derivation of the bounds and the
mutants they must see).

Every product-build branch of run_gemm (csrc/gemm_ring.hip) has a case:
  branch                                               | cases
  launch_gemm<F32, 4 / 7 / 8, 2>                       | f32_n4_*, f32_n7_*, f32_n8_*
  launch_gemm<SPLIT, 7 / 8, 2>                         | split_n7_norm, split_n7_stats, split_n8_raw, split_n8_norm_aff
  gemm_split_small_kernel<4>                           | split_n4_raw, split_n4_norm_aff (k_pad 544), split_n4_stats_wide (1568)
  launch_gemm<SPLIT, 4, 2> (input affine, k_pad>=736) | split_n4_raw_aff_wide (the small kernel's 64 KB of LDS do not fit)
  launch_gemm<SPLIT, 8 / 7, 2, true> (pair residual)   | split_n8_pair (F_RES_PAIR), split_n7_pair_nbr (F_RES_PAIR_NBR)
  gemm_small_kernel<2, false / true>                   | f16_n4_raw, f16_n4_norm / f16_n4_norm_aff
  the same with gn_fin                                 | f16_n4_gnfin, f16_n4_gnfin_1024 (1024 tiles), f16_n4_gnfin_1025 (-10)
  gemm_glds_occ3_kernel<8, false / true, false>        | f16_n8_norm, f16_n8_stats / f16_n8_norm_aff
  gemm_glds_kernel<8, 2, 3, 32, true>                  | f16_n8_raw_aff_wide (k_pad 2048: occ3's 53 KB check declines)
  gemm_glds_kernel<7, 2, 3, 32, true>                  | f16_n7_norm_aff
  gemm_glds_kernel<8 / 7, 2, 3, 32, false, false, true>| f16_n8_pair, f16_n7_pair_nbr
Across them: RAW / NORM / STATS epilogues, ragged GroupNorm layouts (N = 51, 111) and N < 32, PRE / POST ReLU, fp32 output of an
fp16 GEMM, addvec with and without a device-side row index, residual, pre_add per point / per sample and through the
neighbour table; K in {3, 35, 96, 544, 1568, 2021}, N in {3, 32, 51, 64, 111, 512}, 1 / 3 / 17 / 37 samples; inputs N(0, 1),
mean 30 (GroupNorm's cancellation), scale 1e-3 (the split's low terms must stay normal fp16) and split weights up to |w| = 64.
The padded X columns hold large finite values (the kernels must ignore them); padded output columns must come out zero.

The module path (slide_amd.rows: from_ncx -> norm_act(defer=True) -> conv) is checked the same way, output and the per-tile
statistics its GEMM publishes."""
import ctypes

import numpy as np
import pytest

from gemm_cases import CASES, CASE_BY_NAME, EPI_NORM, EPI_STATS, EXEMPT, U, fin_scale_shift, forward, gn_params, make_data, \
    mutants, r16, ru


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_bounds_see_the_mutants():
    """every case's bound is tighter than the deviation of each of its mutants in at least one element (or the exemption names
    a case of the same kernel where that mutant is visible)"""
    seen = {}
    for c in CASES:
        d = make_data(c)
        ref = forward(c, d)
        assert np.isfinite(ref["b"]).all() and (ref["b"] > 0).all()
        for m in mutants(c):
            dev = np.abs(forward(c, d, mutant=m)["stored"] - ref["y"])
            seen[(c["name"], m)] = float((dev / ref["b"]).max())
    for (name, m), r in seen.items():
        if (name, m) in EXEMPT:
            other = EXEMPT[(name, m)]
            assert CASE_BY_NAME[other]["kernel"] == CASE_BY_NAME[name]["kernel"], (name, other)
            assert seen[(other, m)] > 1, (name, m, other, seen[(other, m)])
        else:
            assert r > 1, "case %s: the bound does not see mutant %s (max deviation / bound %.3g)" % (name, m, r)


def test_case_matrix_reaches_every_branch():
    """the kernels named in the module docstring's table all have a case"""
    kernels = {c["kernel"] for c in CASES}
    for k in ("gemm_kernel<0, 4, 2, false>", "gemm_kernel<0, 7, 2, false>", "gemm_kernel<0, 8, 2, false>",
              "gemm_kernel<2, 4, 2, false>", "gemm_kernel<2, 7, 2, false>", "gemm_kernel<2, 8, 2, false>",
              "gemm_kernel<2, 7, 2, true>", "gemm_kernel<2, 8, 2, true>", "gemm_split_small_kernel<4>",
              "gemm_small_kernel<2, false>", "gemm_small_kernel<2, true>", "gemm_glds_occ3_kernel<8, false, false, false>",
              "gemm_glds_occ3_kernel<8, true, false, false>", "gemm_glds_kernel<8, 2, 3, 32, true, false, false>",
              "gemm_glds_kernel<7, 2, 3, 32, true, false, false>", "gemm_glds_kernel<8, 2, 3, 32, false, false, true>",
              "gemm_glds_kernel<7, 2, 3, 32, false, false, true>"):
        assert k in kernels, k
    assert {c["dist"] for c in CASES if c["prec"] == "split"} == {"normal", "common", "small", "bigw"}
    for p in ("fp32", "fp16"):
        assert {c["dist"] for c in CASES if c["prec"] == p} == {"normal", "common", "small"}


# ------------------------------------------------------------------------------------------------------------------- GPU
class _Mini:
    """just enough of DenoiserEngine to emit one GEMM op"""

    def __new__(cls, B, prec, device):
        from slide_amd import engine as E

        class M(E.DenoiserEngine):
            def __init__(self):
                self._plan_state(B, device, prec)
        return M()


def _launch(c, device):
    """emits and runs the case's GEMM; returns (status, got [rows][N] logical, padded output columns, stats or None,
    published scale / shift or None)"""
    import torch
    from slide_amd import engine as E
    from slide_amd._lib import lib
    prec, B, K, N, npxl = c["prec"], c["B"], c["K"], c["N"], c["npxl"]
    rows = B << npxl
    m = _Mini(B, prec, device)
    d = make_data(c)
    ld = ru(K)
    Xp = np.full((rows, ld), 1e30 if prec == "fp32" else 3e4, np.float32)
    Xp[:, ld - 1::-2] *= -1
    Xp[:, :K] = d["X"]
    X = m.A.put(Xp, m.adt)
    lay = E.gn_layout(N) if c["mode"] == EPI_NORM else None
    oidx = lay[0] if lay is not None else np.arange(N)
    Np = ru(lay[1]) if lay is not None else ru(N)

    def phys(a, dtype=None):
        ap = np.zeros(a.shape[:-1] + (Np,), np.float32)
        ap[..., oidx] = a
        return m.A.put(ap, dtype)
    odt = torch.float32 if (prec != "fp16" or c["out_f32"]) else torch.float16
    out = torch.full((rows, Np), 7.0, dtype=odt, device=device)
    m.A.keep.append(out)
    seg = dict(w=d["W"], bias=d["bias"], mode=c["mode"], out=out,
               flags=(E.F_PRE_RELU if c["pre_relu"] else 0) | (E.F_POST_RELU if c["post_relu"] else 0))
    if lay is not None:
        n_norm = gn_params(N)[1]
        seg.update(layout=lay, gn=(d["gamma"][:n_norm], d["beta"][:n_norm]))
    if c["addvec"] == "plain":
        seg["addvec"] = (phys(d["addvec"]), 0, Np, None, 0)
    elif c["addvec"] == "idx":
        seg["addvec"] = (phys(d["addvec_tab"]), 0, Np, m.A.put(np.array([d["addvec_t"]], np.int32)), B * Np)
    if c["resid"]:
        seg["residual"] = phys(d["resid"], m.adt)
    kw = {}
    if c["pre_add"] == "gather":
        seg["pre_add"] = (phys(d["pre"], m.adt), 4 - npxl)
        kw["pre_gather"] = m.A.put(d["nbr"])
    elif c["pre_add"] is not None:
        seg["pre_add"] = (phys(d["pre"], m.adt), c["pre_add"])
    if c["pair"] is not None:
        rvv = None
        if c["pair"] == "nbr":
            rvv = phys(np.stack([d["vd"], d["vw"]]))
            kw["pair_tabs"] = (m.A.put(d["nbr"]), m.A.put(d["d2"]), m.A.put(d["w"]))
        seg["res_pair"] = (phys(d["ta"], m.adt), phys(d["tb"], m.adt), 0, rvv)
    ssum = ssq = None
    if c["mode"] == EPI_STATS:
        ssum, ssq = m.A.zeros(B, Np), m.A.zeros(B, Np)
        seg["stats"] = (ssum, ssq, 0, c["stats_scale"])
    scale = shift = None
    if c["aff"]:
        if c["gn_fin"]:
            G, n_norm, gs = gn_params(K)
            gid = np.full(ld, -1, np.int32); gid[:n_norm] = np.arange(n_norm) // gs
            gam, bet = np.zeros(ld, np.float32), np.zeros(ld, np.float32)
            gam[:K], bet[:K] = d["fin_gamma"], d["fin_beta"]
            sums = [np.zeros((B, ld), np.float32) for _ in range(2)]
            sums[0][:, :K], sums[1][:, :K] = d["sum"], d["sq"]
            scale, shift = m.A.zeros(B, ld), m.A.zeros(B, ld)
            tabs = [m.A.put(a) for a in (sums[0], sums[1], gid, np.arange(G, dtype=np.int32) * gs,
                                          np.arange(1, G + 1, dtype=np.int32) * gs, gam, bet)]
            fin = E.SlideGnFin()
            for n_, t_ in zip(("sum", "sq", "gid", "gstart", "gend", "gamma", "beta", "scale", "shift"), tabs + [scale, shift]):
                setattr(fin, n_, t_.data_ptr())
            fin.inv_count, fin.C, fin.bs, fin.G = 1.0 / (gs << npxl), ld, ld, G
            kw["gn_fin"] = m.A.put(np.frombuffer(bytes(fin), dtype=np.uint8).copy())
            kw["in_affine"] = (scale, shift, 0, ld)
        else:
            sc, sh = np.ones((B, ld), np.float32), np.zeros((B, ld), np.float32)
            sc[:, :K], sh[:, :K] = d["scale"], d["shift"]
            kw["in_affine"] = (m.A.put(sc), m.A.put(sh), 0, ld)
    m._gemm(X, npxl, [seg], **kw)
    from slide_amd.engine import SlideOp
    ops = (SlideOp * 1)(*m.ops)
    st = lib().slide_run_ops(ops, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.float().cpu().numpy()
    pad = np.delete(got, oidx, axis=1)
    stats = None if ssum is None else (ssum.cpu().numpy()[:, oidx], ssq.cpu().numpy()[:, oidx])
    fin = None if scale is None else (scale.cpu().numpy()[:, :K].astype(np.float64), shift.cpu().numpy()[:, :K].astype(np.float64))
    return st, got[:, oidx], pad, stats, fin


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_gemm_op_matches_float64(gpu_device, name):
    c = CASE_BY_NAME[name]
    st, got, pad, stats, fin = _launch(c, gpu_device)
    if c["status"] != 0:
        assert st == c["status"] * 1000, (name, st)  # (slide_run_ops: status * 1000 - index of the failing op)
        print("%s: status %d as expected" % (name, st))
        return
    assert st == 0, (name, st)
    d = make_data(c)
    if c["gn_fin"]:  # the scale / shift the launch published, against the float64 finalisation of the same sums
        sc, sh, dsc, dsh = fin_scale_shift(c, d)
        r_sc = float((np.abs(fin[0] - sc) / np.maximum(dsc, 1e-300)).max())
        r_sh = float((np.abs(fin[1] - sh) / np.maximum(dsh, 1e-300)).max())
        print("%s: published scale / shift worst err/tol %.3g / %.3g" % (name, r_sc, r_sh))
        assert r_sc <= 1 and r_sh <= 1, (r_sc, r_sh)
    ref = forward(c, d, fin=fin)
    assert np.isfinite(got).all()
    err = np.abs(got - ref["y"])
    ratio = err / ref["b"]
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s [%s, %s]: worst err/tol %.3g (err %.3g, |ref| %.3g at %s), worst err %.3g" %
          (name, c["prec"], c["kernel"], ratio[i], err[i], abs(ref["y"][i]), i, err.max()))
    assert ratio.max() <= 1, (name, float(ratio.max()), i)
    assert (pad == 0).all(), "padded output columns must be zero"
    if stats is not None:
        for k in range(2):
            rs = float((np.abs(stats[k] - ref["stats"][k]) / ref["stats_b"][k]).max())
            print("%s: statistics %s worst err/tol %.3g" % (name, ("sum", "sq")[k], rs))
            assert rs <= 1, (name, k, rs)


# ------------------------------------------------------------------------------------------------------------ module path
def _module_case(prec, S, relu, addvec, stats, device, pre_add=False, out_f32=False):
    """from_ncx -> norm_act(defer=True) -> conv(stats=..., pre_add=...) against float64; returns the worst err/tol"""
    import torch
    from pointnet2_ops import pointnet2_modules as PM
    from slide_amd import rows as R
    from gemm_cases import C_ACC
    half = prec == "fp16"
    gen = torch.Generator().manual_seed(S + 2 * relu + 4 * (addvec is not None) + 8 * pre_add)
    B, C, O = 3, 64, 96
    x = (torch.randn(B, C, S, generator=gen) + (30.0 if S == 512 else 0.0)).to(device)
    gn = PM.HipGroupNorm(8, C).to(device)
    conv = PM.HipConv1x1(C, O, bias=True).to(device)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 2.0); gn.bias.uniform_(-1, 1)
    av = None if addvec is None else (torch.randn(B, C, generator=gen) * addvec).to(device)
    r = R.from_ncx(x, half=half)
    r = R.norm_act(r, gn=gn, relu=relu, addvec=av, defer=True)
    sm = np.arange(B * S) // S
    if r.pending is not None:  # deferred: X' = fp16(fp16(x * sc + sh) [-> max(., 0) + fp16(add)]) in the GEMM's loader
        ss = r.pending[0].view(B, 2, r.ld).cpu().double().numpy()[:, :, :C]
        xr = r16(r.data.float().cpu().numpy()[:, :C])
        # the published scale / shift against float64 GroupNorm of the stored input
        xs = xr.reshape(B, S, 8, C // 8)
        mean = xs.mean((1, 3)); var = xs.var((1, 3))
        g64 = gn.weight.detach().double().cpu().numpy().reshape(8, C // 8)
        sc64 = (g64[None] / np.sqrt(var + 1e-5)[:, :, None]).reshape(B, C)
        sh64 = gn.bias.detach().double().cpu().numpy()[None] - np.repeat(mean, C // 8, 1) * sc64
        ex2 = (xs * xs).mean((1, 3))
        tol = 64 * U * (1 + ex2 / (var + 1e-5))
        assert (np.abs(ss[:, 0] - sc64) <= np.repeat(tol, C // 8, 1) * np.abs(sc64)).all()
        Xa = r16(xr * r16(ss[:, 0])[sm] + r16(ss[:, 1])[sm])
        if relu:
            Xa = np.maximum(Xa, 0)
        if av is not None:
            Xa = r16(Xa + r16(av.cpu().double().numpy())[sm])
        Xabs = np.abs(Xa)
    else:
        R.materialise(r)
        Xa = r.data.float().cpu().double().numpy()[:, :C]
        if half:
            Xa = r16(Xa)
        Xabs = np.abs(Xa)
    W = conv.weight.detach().reshape(O, C).double().cpu().numpy()
    bias = conv.bias.detach().double().cpu().numpy()
    if half:
        W = r16(W)
    y = Xa @ W.T + bias
    A = Xabs @ np.abs(W).T + np.abs(bias)
    pa = None
    if pre_add:
        pr = R.from_ncx(torch.randn(B, O, S // 4, generator=gen).to(device), half=half)
        pa = (pr, 4)
        p64 = pr.data.float().cpu().double().numpy()[:, :O]
        y = y + np.repeat(p64, 4, 0)
        A = A + np.abs(np.repeat(p64, 4, 0))
    b = C_ACC * A
    if stats == "relu":
        y = np.maximum(y, 0)
    if out_f32:
        plan = R._ConvPlan(conv.weight, conv.bias, half, device)
        rr = plan.run(r, stats=stats, pre_add=pa, out_f32=True)
    else:
        rr = R.conv(r, conv, stats=stats, pre_add=pa)
    got = rr.data.float().cpu().double().numpy()
    b_out = b * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(y) + 2.0 ** -25 if (half and not out_f32) else b + U * np.abs(y)
    ratio = float((np.abs(got[:, :O] - y) / b_out).max())
    assert (got[:, O:] == 0).all()
    if stats is not None:
        assert rr.stats is not None
        n = 256
        yt, bt = y.reshape(-1, n, O), b.reshape(-1, n, O)
        s_ref, q_ref = yt.sum(1), (yt * yt).sum(1)
        dd = np.log2(n) + 2
        s_b = bt.sum(1) + dd * U * np.abs(yt).sum(1)
        q_b = (2 * np.abs(yt) * bt + bt * bt).sum(1) + dd * U * (yt * yt).sum(1)
        s_got = rr.stats[0].cpu().double().numpy()[:, :O]
        q_got = rr.stats[1].cpu().double().numpy()[:, :O]
        ratio = max(ratio, float((np.abs(s_got - s_ref) / s_b).max()), float((np.abs(q_got - q_ref) / q_b).max()))
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("S", [256, 512, 1024])
def test_module_conv_matches_float64(gpu_device, monkeypatch, prec, S):
    """the module path's GEMM (256-row tiles, aff_tps = S / 256 with the deferred normalisation of fp16 rows) with and without
    the embedding add and the ReLU; published per-tile statistics against float64 column sums"""
    monkeypatch.setenv("SLIDE_MODULE_PREC", prec)
    for relu, addvec, stats in ((True, 5.0, "relu"), (False, None, "raw"), (True, None, None), (False, 5.0, "raw")):
        r = _module_case(prec, S, relu, addvec, stats, gpu_device, pre_add=(S == 512))
        print("module %s S=%d relu=%s addvec=%s stats=%s: worst err/tol %.3g" % (prec, S, relu, addvec is not None, stats, r))
        assert r <= 1, (relu, addvec, stats, r)
    if prec == "fp16":
        r = _module_case(prec, S, True, 5.0, None, gpu_device, out_f32=True)
        print("module fp16 S=%d out_f32: worst err/tol %.3g" % (S, r))
        assert r <= 1, r
