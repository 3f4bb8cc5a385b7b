"""Every training backward kernel of csrc/train_ops.hip against float64, elementwise, at bounds derived from the arithmetic
(tests/train_cases.py: the case matrix, the references, the derivation of the bounds and the mutants they must see).  The
companion of tests/test_hip_rows_arith.py for the backward half of the module path.

  entry point            | kernels                                   | what the cases reach
  slide_gn_rows_bwd      | gn_bwd_sums / finalize / apply_kernel     | ld 32 ... 1024 (rt 32 ... 1, idle threads), S 1 ... 4100 (nchunk clamped, a
                         |                                           | short last chunk), G 0 / 1 / 32 / 64, the four ReLU forms, a seam inside a
                         |                                           | thread's four channels, every -3 clause
  slide_col_sums         | col_sums_kernel (one or two launches)     | 0 ... 140001 rows, the 127 / 128 scratch boundary, the 1024-chunk clamp
  slide_group_rows_bwd   | group_rows_bwd_kernel                     | C % 4, N != np, ldf != ldg, N K-fold accumulation, empty balls
  slide_concat_qk_bwd    | concat_qk_bwd_kernel                      | C1 3 ... 256, K 1 ... 16, three strides, bit-equal repeats
  slide_attn_rows_bwd    | attn_rows_bwd_kernel                      | K 1 ... 48, counts 0 / 1 / K / > K, scores of +-60 and +-100
  ConvRows (Function)    | the split GEMM, hipBLASLt, col_sums       | 16 ... 65536 rows: 1 / 2 / 64 row slabs, 64- and 256-row tiles
Each case is called at the C-ABI through slide_amd._lib.lib() with explicit buffers, every output prefilled; the cases marked
`wrap` also run through the autograd Function of slide_amd.train.functions under torch.autograd.grad."""
import ctypes

import numpy as np
import pytest

import train_cases as TC
from train_cases import CASES, CASE_BY_NAME, EXEMPT, PREFILL, backward, make_data, mutants, ratio, reach

ABI_CASES = [c["name"] for c in CASES if c["op"] != "conv" and c.get("stats", "input") == "input"]
WRAP_CASES = [c["name"] for c in CASES if c["wrap"]]

WANT = {"gn_bwd": ["count_rpc_nchunk", "drop_last_row", "neighbour_sample", "no_m2_term", "post_mask_from_x", "no_pre_mask",
                   "tail_normalised", "tail_no_mask", "dgamma_dbeta_swapped", "dn_without_gamma"],
        "col_sums": ["drop_last_row", "drop_last_chunk", "second_stage_first_32", "rpc_floor"],
        "group_bwd": ["zero_count_receives", "batch_stride_np", "tail_channels_dropped", "strides_swapped"],
        "concat_bwd": ["mask_from_dout", "q_sum_K_minus_1", "seam_off_by_one", "q_row_mod"],
        "attn_bwd": ["slot_past_count", "zero_count_empty", "no_out_term", "no_max_shift"],
        "conv": ["dw_drop_last_slab", "db_drop_last_row"]}


# ------------------------------------------------------------------------------------------------------------------- CPU
def _seen():
    seen = {}
    for c in CASES:
        if c["status"] != 0:
            continue
        d = make_data(c)
        ref = backward(c, d)
        for k, o in ref.items():
            assert np.isfinite(o["b"]).all() and (o["b"] >= 0).all() and np.isfinite(o["y"]).all(), (c["name"], k)
            assert ratio(o, o["stored"]).max() <= 1, (c["name"], k)  # the reference itself, stored to fp32, is inside its own bound
        for m in mutants(c):
            mut = backward(c, d, mutant=m)
            seen[(c["name"], m)] = max(float(ratio(ref[k], mut[k]["stored"]).max()) for k in ref)
    return seen


def test_bounds_see_the_mutants():
    """every case's bound is tighter than the deviation of each of its mutants in at least one element (or the exemption names a
    case of the same op where that mutant is visible); every mutant of the list is shown by some case"""
    seen = _seen()
    for (name, m), r in seen.items():
        if (name, m) in EXEMPT:
            other = CASE_BY_NAME[EXEMPT[(name, m)]]
            assert other["op"] == CASE_BY_NAME[name]["op"], (name, other["name"])
            assert seen[(other["name"], m)] > 1, (name, m, other["name"], seen[(other["name"], m)])
        else:
            assert r > 1, "case %s: the bound does not see mutant %s (max deviation / bound %.3g)" % (name, m, r)
    for key in EXEMPT:
        assert key in seen, key
    shown = {(CASE_BY_NAME[n]["op"], m) for (n, m), r in seen.items() if r > 1}
    for op, ms in WANT.items():
        for m in ms:
            assert (op, m) in shown, (op, m)


def test_relu_masks_are_decidable():
    """no element of any GroupNorm case has its float64 g within the forward bound of 0 (planted exact zeros aside): the cap on
    elements the comparison would have to exclude is zero"""
    for c in CASES:
        if c["op"] == "gn_bwd" and c["status"] == 0:
            d = make_data(c)
            assert TC.ambiguous(c, d) == 0, c["name"]
            x, S = d["x"], c["S"]   # the planted exact zeros survive the redraw
            assert (x[::7, 1] == 0).all() and (x[3::5, c["C"] - 1] == 0).all(), c["name"]
            if c["dist"] == "zero_sample":
                assert (x[S:2 * S] == 0).all(), c["name"]
            if c["gzero"]:
                assert TC._gn_planted(c, d).any() and ((d["gamma"] == 0) & (d["beta"] != 0)).any(), c["name"]


def test_case_matrix_reaches_every_branch():
    """the branch values the issue lists, computed from the case parameters with the launchers' own formulas, all occur"""
    R = [reach(c) for c in CASES]

    def vals(op, key, **where):
        return {r[key] for r in R if r["op"] == op and key in r and all(r.get(k) == v for k, v in where.items())}
    ok = dict(status=0)
    assert vals("gn_bwd", "ld", **ok) == {32, 96, 128, 544, 1024} and vals("gn_bwd", "rt", **ok) == {32, 10, 8, 1}
    assert vals("gn_bwd", "idle", ld=96, **ok) == {16} and vals("gn_bwd", "idle", ld=544, **ok) == {120}
    assert vals("gn_bwd", "S", **ok) >= {1, 16, 40, 255, 256, 257, 4096}
    assert True in vals("gn_bwd", "last_short", clamped=True, nchunk=64, **ok) and 1 in vals("gn_bwd", "nchunk", **ok)
    assert True in vals("gn_bwd", "last_short", clamped=True, rt=1, **ok)
    assert 33 in vals("gn_bwd", "B", **ok) and vals("gn_bwd", "G", **ok) >= {0, 1, 32, 64}
    assert vals("gn_bwd", "flags", **ok) == {0, 1, 2, 3} and vals("gn_bwd", "flags", G=0, **ok) == {0, 1, 2, 3}
    assert vals("gn_bwd", "gs", **ok) >= {1, 2, 3, 16}
    for key in ("tail", "straddle", "full", "gzero"):
        assert True in vals("gn_bwd", key, **ok), key
    assert any(r["op"] == "gn_bwd" and r["straddle"] and r["tail"] and r["ld"] == 32 for r in R)
    assert vals("gn_bwd", "dist", **ok) == {"normal", "common", "zero_sample"}
    assert vals("gn_bwd", "flags", stats="forward", wrap=True) == {0, 1, 2, 3}
    assert vals("gn_bwd", "null", status=-3) == {None, "mr", "scratch", "gamma", "beta", "dgamma", "dbeta"}
    assert len([r for r in R if r["op"] == "gn_bwd" and r["status"] == -3 and r["null"] is None]) == 9  # one per clause of the check
    assert vals("col_sums", "rows", **ok) >= {0, 1, 5, 63, 64, 127, 128, 129, 4096, 65536, 70001} and max(vals("col_sums", "rows")) > 2 * 65536
    assert vals("col_sums", "ld", **ok) == {32, 128, 544, 1024} and vals("col_sums", "stages", rows=127) == {1}
    assert vals("col_sums", "stages", rows=128, **ok) == {2} and vals("col_sums", "scratch", rows=127) == {False}
    assert vals("col_sums", "scratch", status=-3, rows=128) == {False} and vals("col_sums", "ld", status=-3) >= {0, 48, 1056} and vals("gn_bwd", "ld", status=-3) >= {0, 48, 1056}
    assert True in vals("col_sums", "ragged", clamped=True) and False in vals("col_sums", "ragged", clamped=False, stages=2)
    assert vals("col_sums", "dist", **ok) == {"normal", "common"} and vals("col_sums", "rt", stages=2) >= {32, 8, 1}
    assert vals("group_bwd", "C") == {1, 5, 8, 13, 64} and vals("group_bwd", "K") == {1, 5, 16}
    assert vals("group_bwd", "n_ne_np") == {True} and vals("group_bwd", "ld_differ") == {False, True} and min(vals("group_bwd", "B")) > 1
    assert vals("group_bwd", "counts") == {False, True} and True in vals("group_bwd", "onepoint") and vals("group_bwd", "tail_channels") >= {0, 1}
    assert vals("concat_bwd", "C1") == {3, 4, 8, 51, 256} and vals("concat_bwd", "C2") == {12, 60, 139}
    assert vals("concat_bwd", "K") == {1, 8, 16} and True in vals("concat_bwd", "strides_differ")
    assert vals("attn_bwd", "K") == {1, 4, 16, 48} and vals("attn_bwd", "counts") == {False, True} and vals("attn_bwd", "counts", K=1) == {False, True}
    assert vals("attn_bwd", "dist") == {"normal", "pm60", "pm100"} and True in vals("attn_bwd", "strides_differ") and True in vals("attn_bwd", "pad")
    assert vals("conv", "slabs") == {1, 2, 64} and vals("conv", "npx_fwd") == {4, 8} and vals("conv", "npx_bwd") == {4, 8}
    assert vals("conv", "rows") >= {16, 510, 512, 65536} and any(r % 2 for r in vals("conv", "rows")) and vals("conv", "bias") == {False, True}
    assert vals("conv", "I") == {3, 45, 131, 515} and vals("conv", "O") == {51, 70, 128, 256}
    for op in TC.OPS:
        assert any(c["wrap"] for c in CASES if c["op"] == op) or op == "col_sums", op   # (col_sums: inside the GN and ConvRows wrap cases)
    for c in CASES:  # the counts of the count cases hold 0, 1, partial, K and > K
        if c["op"] == "attn_bwd" and c["counts"] and c["K"] > 4:
            cnt, K = make_data(c)["counts"], c["K"]
            assert {0, 1, K} <= set(cnt.tolist()) and (cnt > K).any() and ((cnt > 1) & (cnt < K)).any(), c["name"]
        if c["op"] == "group_bwd" and c["counts"]:
            assert (make_data(c)["counts"] == 0).any()


# ------------------------------------------------------------------------------------------------------------------- GPU
def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Dev:
    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def fill(self, *shape, value=PREFILL):
        return self.torch.full(shape, value, dtype=self.torch.float32, device=self.device)

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _launch(c, d, device):
    """one call of the case's entry point on explicit buffers -> (status, {output name: tensor})"""
    from slide_amd._lib import lib
    D = _Dev(device)
    L, op, st = lib(), c["op"], D.stream()
    # every operand stays referenced until the synchronize below: a tensor freed before its kernel ran would hand its block to the
    # next upload, and the kernel would read another operand's bytes as its index table
    dev = {k: D.put(v) for k, v in d.items() if isinstance(v, np.ndarray)} if op in ("group_bwd", "concat_bwd", "attn_bwd") else {}
    if op == "gn_bwd":
        B, S, G = c["B"], c["S"], c["G"]
        ld = d["x"].shape[1]   # (a refused ld % 32 never launches; its buffers hold the next multiple of 32 all the same)
        x, dy = D.put(d["x"]), D.put(d["dy"])
        dx = D.fill(B * S, ld)
        null = c.get("null")
        need = G > 0 or c["status"] != 0
        t = dict(gamma=D.put(d["gamma"]), beta=D.put(d["beta"]), mr=D.put(d["mr"]), dgamma=D.fill(B, ld), dbeta=D.fill(B, ld),
                 scratch=D.fill(B * (64 * ld * 2 + 128))) if need else {}
        g = lambda k: None if (k == null or not need) else t[k]
        s = L.slide_gn_rows_bwd(B, S, c["ld"], G, c["n_norm"], c["flags"], _P(x), _P(g("gamma")), _P(g("beta")), _P(g("mr")), _P(dy), _P(dx),
                                _P(g("dgamma")), _P(g("dbeta")), _P(g("scratch")), st)
        outs = dict(dx=dx)
        if need:
            outs.update(dgamma=t["dgamma"], dbeta=t["dbeta"])
    elif op == "col_sums":
        ld = d["x"].shape[1]   # (a refused ld <= 0 never launches; its buffers are 32 wide all the same)
        x = D.put(d["x"])
        out = D.fill(ld)
        scratch = D.fill(1024 * ld) if c["scratch"] else None
        s = L.slide_col_sums(ctypes.c_longlong(c["rows"]), c["ld"], _P(x), _P(out), _P(scratch), st)
        outs = dict(out=out)
    elif op == "group_bwd":
        dfeat = D.fill(c["B"] * c["N"], c["ldf"], value=c["init"])
        s = L.slide_group_rows_bwd(c["B"], c["N"], c["np"], c["K"], c["C"], c["ldf"], c["ldg"], _P(dev["idx"]),
                                   _P(dev["counts"]) if c["counts"] else None, _P(dev["dout"]), _P(dfeat), st)
        outs = dict(dfeat=dfeat)
    elif op == "concat_bwd":
        dq, dk = D.fill(c["pts"], c["ldq"]), D.fill(c["pts"] * c["K"], c["ldk"])
        s = L.slide_concat_qk_bwd(ctypes.c_longlong(c["pts"]), c["K"], c["C1"], c["ldq"], c["C2"], c["ldk"], c["ldo"], _P(dev["out"]),
                                  _P(dev["dout"]), _P(dq), _P(dk), st)
        outs = dict(dq=dq, dk=dk)
    elif op == "attn_bwd":
        ds, dv = D.fill(c["pts"] * c["K"], c["lds"]), D.fill(c["pts"] * c["K"], c["ldv"])
        s = L.slide_attn_rows_bwd(ctypes.c_longlong(c["pts"]), c["K"], c["C"], c["lds"], c["ldv"], c["ldo"], _P(dev["S"]), _P(dev["V"]),
                                  _P(dev["counts"]) if c["counts"] else None, _P(dev["dout"]), _P(ds), _P(dv), st)
        outs = dict(ds=ds, dv=dv)
    else:
        raise KeyError(op)
    D.torch.cuda.synchronize()
    del dev
    return s, outs


def _check(name, ref, got, what=""):
    """every element of every output against the reference under the case's bound; returns the worst err / bound"""
    worst = 0.0
    assert set(ref) == set(got), (sorted(ref), sorted(got))
    for k, o in ref.items():
        r = ratio(o, got[k])
        i = np.unravel_index(np.argmax(r), r.shape) if r.size else ()
        exact = bool((o["b"] == 0).all())
        if r.size:
            print("%s%s [%s]: %s, worst err/bound %.3g at %s (got %.9g, ref %.9g), %d elements, %d exact" %
                  (name, what, k, "exact" if exact else "bounded", r[i], i, np.asarray(got[k])[i], o["y"][i], r.size, int((o["b"] == 0).sum())))
            assert r.max() <= 1, (name, k, float(r.max()), i)
            worst = max(worst, float(r.max()))
        if exact:
            assert np.array_equal(np.asarray(got[k], np.float64), o["stored"]), (name, k)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", ABI_CASES)
def test_backward_kernel_matches_float64(gpu_device, name):
    c = CASE_BY_NAME[name]
    d = make_data(c)
    st, outs = _launch(c, d, gpu_device)
    if c["status"] != 0:
        assert st == c["status"], (name, st)
        for k, t in outs.items():
            assert bool((t == PREFILL).all()), "a refused call must not write (%s)" % k
        print("%s: status %d as expected, nothing written" % (name, st))
        return
    assert st == 0, (name, st)
    got = {k: _np(t) for k, t in outs.items()}
    ref = backward(c, d)
    if c["op"] == "gn_bwd" and c["G"] == 0:
        got = dict(dx=got["dx"])
    worst = _check(name, ref, got)
    if c["op"] == "concat_bwd":  # deterministic: a second launch gives the same bits
        _, again = _launch(c, d, gpu_device)
        for k in outs:
            assert bool((again[k] == outs[k]).all()), (name, k)
    print("WORST %s %s %.4g" % (c["op"], name, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("name", WRAP_CASES)
def test_function_matches_float64(gpu_device, name):
    """the autograd Functions of slide_amd.train.functions under torch.autograd.grad: slot packing, zeroed gradient buffers,
    col_sums of the per-sample partials -- inside the same bounds around the same references"""
    import torch
    from slide_amd.train import functions as F
    c = CASE_BY_NAME[name]
    d = make_data(c)
    D = _Dev(gpu_device)
    ref = backward(dict(c, fill=0.0), d)   # (a Function allocates its gradients zeroed: what a C-ABI case leaves at PREFILL is 0 there)
    op = c["op"]
    leaf = lambda a: D.put(a).requires_grad_(True)
    if op == "gn_bwd":
        x, gam, bet = leaf(d["x"]), leaf(d["gamma"][:c["n_norm"]]), leaf(d["beta"][:c["n_norm"]])
        y = F.gn_rows(x, gam, bet, c["B"], c["S"], c["G"], bool(c["flags"] & 1), bool(c["flags"] & 2))
        dx, dg, db = torch.autograd.grad(y, (x, gam, bet), grad_outputs=D.put(d["dy"]))
        got = dict(dx=_np(dx), dgamma=_np(dg), dbeta=_np(db))
    elif op == "group_bwd":
        feat = leaf(d["feat"])
        y = F.group_rows(feat, D.put(d["xyz"]), D.put(d["new_xyz"]), D.put(d["idx"]), None, 0, c["C"])
        assert tuple(y.shape) == d["dout"].shape
        got = dict(dfeat=_np(torch.autograd.grad(y, feat, grad_outputs=D.put(d["dout"]))[0]))
    elif op == "concat_bwd":
        q, k = leaf(d["q"]), leaf(d["k"])
        y = F.concat_qk(q, k, c["K"], c["C1"], c["C2"])
        assert np.array_equal(_np(y), d["out"].astype(np.float64)), "the forward output the reference took as the mask"
        dq, dk = torch.autograd.grad(y, (q, k), grad_outputs=D.put(d["dout"]))
        got = dict(dq=_np(dq), dk=_np(dk))
    elif op == "attn_bwd":
        s, v = leaf(d["S"]), leaf(d["V"])
        y = F.attend_rows(s, v, c["K"], c["C"])
        ds, dv = torch.autograd.grad(y, (s, v), grad_outputs=D.put(d["dout"]))
        got = dict(ds=_np(ds), dv=_np(dv))
    elif op == "conv":
        x, W = leaf(d["x"]), leaf(d["W"])
        b = leaf(d["bias"]) if c["bias"] else None
        y = F.conv_rows(x, W, b)
        g = torch.autograd.grad(y, (x, W) + ((b,) if c["bias"] else ()), grad_outputs=D.put(d["dy"]))
        got = dict(y=_np(y), dx=_np(g[0]), dw=_np(g[1]))
        if c["bias"]:
            got["db"] = _np(g[2])
    worst = _check(name, ref, got, what=" (Function)")
    print("WORST %s %s %.4g" % (op if op == "conv" else op + "_fn", name, worst))


@pytest.mark.gpu
def test_functions_take_zero_rows(gpu_device):
    """zero-row inputs: every Function returns empty activations' gradients and zero parameter gradients, without a fault"""
    import torch
    from slide_amd.train import functions as F
    dev = gpu_device
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)
    x, gam, bet = z(0, 96), torch.ones(64, device=dev, requires_grad=True), z(64)
    y = F.gn_rows(x, gam, bet, 0, 40, 32, True, True)
    dx, dg, db = torch.autograd.grad(y, (x, gam, bet), grad_outputs=torch.zeros_like(y))
    assert dx.shape == (0, 96) and bool((dg == 0).all()) and bool((db == 0).all()) and dg.shape == (64,)
    feat = z(0, 32)
    xyz, new_xyz, idx = torch.zeros(0, 37, 3, device=dev), torch.zeros(0, 11, 3, device=dev), torch.zeros(0, 11, 5, dtype=torch.int64, device=dev)
    y = F.group_rows(feat, xyz, new_xyz, idx, None, 0, 13)
    (dfeat,) = torch.autograd.grad(y, feat, grad_outputs=torch.zeros_like(y))
    assert y.shape == (0, 32) and dfeat.shape == (0, 32)
    q, k = z(0, 64), z(0, 64)
    y = F.concat_qk(q, k, 8, 51, 60)
    dq, dk = torch.autograd.grad(y, (q, k), grad_outputs=torch.zeros_like(y))
    assert dq.shape == (0, 64) and dk.shape == (0, 64)
    s, v = z(0, 64), z(0, 64)
    y = F.attend_rows(s, v, 16, 51)
    ds, dv = torch.autograd.grad(y, (s, v), grad_outputs=torch.zeros_like(y))
    assert ds.shape == (0, 64) and dv.shape == (0, 64)
    x, W, b = z(0, 64), torch.ones(70, 45, device=dev, requires_grad=True), z(70)
    y = F.conv_rows(x, W, b)
    dx, dw, db = torch.autograd.grad(y, (x, W, b), grad_outputs=torch.zeros_like(y))
    assert dx.shape == (0, 64) and bool((dw == 0).all()) and bool((db == 0).all()) and dw.shape == (70, 45)
