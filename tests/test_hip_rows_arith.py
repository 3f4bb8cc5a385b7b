"""Every SLIDE_OP_ROWS_* op of csrc/rows_ops.hip, in fp32 rows and in fp16 rows, against float64, elementwise, at bounds
derived from the arithmetic (tests/rows_cases.py: the case matrix, the references, the derivation of the bounds and the mutants
they must see).  The companion of tests/test_hip_gemm_arith.py for the other half of the module-level path.

  op                     | kernels                                              | what the cases reach
  ROWS_FROM_NCX / TO_NCX | rows_from_ncx_kernel<T>, rows_to_ncx_kernel<T>       | C in 1 ... 515, P in 1 ... 1000, pad columns, round trip
  ROWS_GROUP             | rows_group_kernel<T>                                 | six layouts x int64 / int32 indices, C = 0 ... 64, empty balls
  ROWS_GN                | rows_gn_stats / apply_kernel<T>, rows_gn_finalize    | ld 32 ... 1024 (rt 32 ... 1 / 64 ... 2), S 1 ... 8500, split paths
  ROWS_GN_JOINT          | rows_gn_joint_kernel                                 | groups across the q | k seam, both tq forms, -3 checks
  ROWS_CONCAT_QK         | rows_concat_qk_kernel<T>                             | the seam inside / on a 16-byte piece, three strides
  ROWS_ATTN              | rows_attn_kernel<T>                                  | K 1 ... 48, counts 0 / 1 / K / > K, +-60 and +-100, deferred values
  ROWS_POOL              | rows_pool_kernel<T>                                  | max / mean / [max | mean] with the split inside a piece, counts
  ROWS_PAIR_EXPAND       | rows_pair_expand_kernel<_Float16, 4 / 8>             | XCD tile map with B 1 / 7 / 8 / 9, ragged linear map, tile sums
Each op is launched alone through slide_amd.rows._rop / make_op with explicit slots; the cases marked `wrap` run through the
public wrapper of slide_amd.rows as well (the slot packing).  Every element of every output is compared, pad columns included."""
import ctypes
import types

import numpy as np
import pytest

import rows_cases as RC
from rows_cases import CASES, CASE_BY_NAME, EXEMPT, PREFILL, forward, make_data, mutants, ratio, reach, ru

RUN_CASES = [c["name"] for c in CASES]


# ------------------------------------------------------------------------------------------------------------------- CPU
def _seen():
    seen = {}
    for c in CASES:
        if c["status"] != 0:
            continue
        d = make_data(c)
        ref = forward(c, d)
        for o in ref.values():
            assert np.isfinite(o["b"]).all() and (o["b"] >= 0).all() and np.isfinite(o["y"]).all(), c["name"]
            assert ratio(o, o["stored"]).max() <= 1, c["name"]  # the reference itself, stored, is inside its own bound
        for m in mutants(c):
            mut = forward(c, d, mutant=m)
            seen[(c["name"], m)] = max(float(ratio(ref[k], mut[k]["stored"]).max()) for k in ref)
    return seen


def test_bounds_see_the_mutants():
    """every case's bound is tighter than the deviation of each of its mutants in at least one element (or the exemption names
    a case of the same op and row type where that mutant is visible); every mutant of the list is shown by some case"""
    seen = _seen()
    for (name, m), r in seen.items():
        if (name, m) in EXEMPT:
            other = CASE_BY_NAME[EXEMPT[(name, m)]]
            assert (other["op"], other["half"]) == (CASE_BY_NAME[name]["op"], CASE_BY_NAME[name]["half"]), (name, other["name"])
            assert seen[(other["name"], m)] > 1, (name, m, other["name"], seen[(other["name"], m)])
        else:
            assert r > 1, "case %s: the bound does not see mutant %s (max deviation / bound %.3g)" % (name, m, r)
    for key in EXEMPT:
        assert key in seen, key
    shown = {(CASE_BY_NAME[n]["op"], CASE_BY_NAME[n]["half"], m) for (n, m), r in seen.items() if r > 1}
    want = {"gn": ["unbiased_var", "count_rpc_nchunk", "drop_last_row", "neighbour_sample", "tail_normalised", "stats_no_relu"],
            "attn": ["slot_past_count", "zero_count_empty", "no_max_shift"],
            "pool": ["slot_past_count", "zero_count_empty", "max_first_n"],
            "group": ["rel_sign", "w_k_minus_1", "idx32_as_64"], "concat_qk": ["seam_other_source", "q_row_mod"],
            "from_ncx": ["pad_not_cleared"]}
    for op, ms in want.items():
        for m in ms:
            for h in (False, True):
                assert (op, h, m) in shown, (op, h, m)
    for m in ("cc_without_wrel", "sums_of_rounded"):
        assert ("pair_expand", True, m) in shown, m
    assert any(k[0] == "gn_joint" and k[2] == "q_once" for k in shown)


def test_case_matrix_reaches_every_branch():
    """the branch values the issue lists, computed from the case parameters with the launcher's own formulas, all occur --
    in fp32 rows and in fp16 rows"""
    R = [reach(c) for c in CASES]

    def vals(op, key, half, **where):
        return {r[key] for r in R if r["op"] == op and r["half"] == half and all(r[k] == v for k, v in where.items())}
    for h in (False, True):
        for op in ("from_ncx", "to_ncx"):
            assert vals(op, "C", h) >= {1, 3, 31, 32, 33, 515} and vals(op, "P", h) >= {1, 31, 32, 33, 1000}
            assert 0 in vals(op, "pad", h)
        for i32 in (False, True):
            assert vals("group", "flags", h, idx32=i32, status=0) == {0, 2, 4, 6, 1, 8}
        assert vals("group", "C", h, status=0) == {0, 5, 8, 13, 64} and vals("group", "K", h) == {1, 5, 48}
        assert vals("group", "coord_start", h) == {"none", "boundary", "inside"} and vals("group", "coord_span", h) == {False, True}
        assert True in vals("group", "ld_differ", h) and vals("group", "counts", h, flags=1) == {False, True}
        assert vals("group", "status", h) == {0, -3}
        assert vals("gn", "ld", h) == {32, 96, 128, 544, 1024}
        assert vals("gn", "rt", h) == ({64, 21, 16, 3, 2} if h else {32, 10, 8, 1})
        assert vals("gn", "idle", h, ld=96) == {4 if h else 16} and vals("gn", "idle", h, ld=544) == {52 if h else 120}
        assert vals("gn", "S", h) >= {1, 16, 40, 255, 256, 257, 4096} and True in vals("gn", "clamped", h)
        assert True in vals("gn", "last_short", h, clamped=True) and 64 in vals("gn", "nchunk", h) and 1 in vals("gn", "nchunk", h)
        assert vals("gn", "G", h) == {0, 1, 32, 64} and vals("gn", "relu", h) == {0, 1, 2, 3} and vals("gn", "relu", h, G=0) >= {1, 2}
        for key in ("tail", "addvec", "res", "inplace", "mr", "split"):
            assert vals("gn", key, h) == {False, True}, key
        assert vals("gn", "dist", h) == {"normal", "common", "zero_sample"} and 33 in vals("gn", "B", h)
        assert vals("gn", "tps", h) >= {0, 1, 2} and vals("gn", "tps", h, split=True) >= {0, 2}
        assert vals("concat_qk", "C1", h) == {3, 4, 8, 51, 256} and vals("concat_qk", "C2", h) == {12, 60, 139}
        assert vals("concat_qk", "K", h) == {1, 8, 16} and vals("concat_qk", "seam_aligned", h) == {False, True}
        assert vals("concat_qk", "seam_aligned", h, C1=4) == {not h} and True in vals("concat_qk", "strides_differ", h)
        assert vals("attn", "K", h) == {1, 4, 16, 48} and vals("attn", "counts", h) == {False, True}
        assert vals("attn", "dist", h) == {"normal", "pm60", "pm100"} and True in vals("attn", "pad", h)
        assert vals("attn", "v_relu", h, vss=True) == {0, 1} and True in vals("attn", "strides_differ", h)
        assert any(r["op"] == "attn" and r["half"] == h and r["vss"] and r["pps"] < 24 for r in R)
        for mode in (0, 1, 2):
            assert vals("pool", "counts", h, mode=mode) == {False, True} or mode == 0
            assert True in vals("pool", "strides_differ", h, mode=mode)
        assert True in vals("pool", "split_inside", h, mode=2)
    assert vals("gn_joint", "tq", True, status=0) | vals("gn_joint", "tq", False, status=0) == {1, 2}
    for key in ("one_row", "straddle", "tail"):
        assert True in vals("gn_joint", key, True) | vals("gn_joint", key, False), key
    assert -3 in vals("gn_joint", "status", True)
    assert vals("pair_expand", "CH", True) == {4, 8} and vals("pair_expand", "status", False) == {-3}
    assert vals("pair_expand", "B", True, ragged=False) >= {1, 7, 8, 9} and 0 in vals("pair_expand", "tps", True, ragged=True)
    for key in ("fp", "relu", "stats", "idx32"):
        assert vals("pair_expand", key, True, status=0) == {False, True}, key
    for op in ("group", "gn", "gn_joint", "concat_qk", "attn", "pool", "from_ncx", "to_ncx"):
        assert any(c["wrap"] for c in CASES if c["op"] == op), op


# ------------------------------------------------------------------------------------------------------------------- GPU
KIND = dict(from_ncx=20, to_ncx=21, group=22, gn=23, concat_qk=24, attn=25, pool=26, gn_joint=27, pair_expand=39)
EMPTY_SLOTS = dict(from_ncx=(0, 2), to_ncx=(0, 2), group=(0, 2), gn=(0, 1), gn_joint=(0,), concat_qk=(0,), attn=(0,), pool=(0,),
                   pair_expand=(0, 2))


def _status(kind, half, i, p, f=()):
    import torch
    from slide_amd import rows as R
    from slide_amd._lib import lib
    from slide_amd.engine import SlideOp
    op = R._rop(kind, half, i, p)
    for k, v in enumerate(f):
        op.f[k] = float(v)
    st = lib().slide_run_ops((SlideOp * 1)(op), 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


class _Dev:
    """the case's operands on the device: rows in the row type, everything else as passed"""

    def __init__(self, c, d, device):
        import torch
        self.c, self.d, self.device, self.torch = c, d, device, torch
        self.rdt = torch.float16 if c["half"] else torch.float32

    def rows(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device).to(self.rdt).contiguous()

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def fill(self, shape, rows=True):
        return self.torch.full(tuple(shape), PREFILL, dtype=self.rdt if rows else self.torch.float32, device=self.device)

    def opt(self, key, rows=False):
        if key not in self.d:
            return None
        return self.rows(self.d[key]) if rows else self.put(self.d[key])


def _build(c, d, device):
    """-> (i slots, p slots, f slots, {output name: tensor}, [tensors that must stay as they are])"""
    D = _Dev(c, d, device)
    op = c["op"]
    f = ()
    if op == "from_ncx":
        out = D.fill((c["B"] * c["P"], ru(c["C"])))
        return (c["B"], c["C"], c["P"], ru(c["C"])), (D.put(d["x"]), out), f, dict(out=out)
    if op == "to_ncx":
        out = D.fill((c["B"], c["C"], c["P"]), rows=False)
        return (c["B"], c["C"], c["P"], ru(c["C"])), (D.rows(d["rows"]), out), f, dict(out=out)
    if op == "group":
        out = D.fill((c["B"] * c["np"] * c["K"], c["ldg"]))
        i = (c["B"], c["N"], c["np"], c["K"], c["C"], c["ldf"], c["ldg"], c["flags"])
        p = (D.put(d["xyz"]), D.put(d["new_xyz"]), D.rows(d["feat"]) if c["C"] else None, D.put(d["idx"]), D.put(d["d2"]), out,
             D.opt("counts"))
        return i, p, f, dict(out=out)
    if op == "gn":
        B, S, ld, G = c["B"], c["S"], c["ld"], c["G"]
        x = D.rows(d["x"])
        y = x if c["inplace"] else D.fill((B * S, ld))
        part = D.torch.empty(B * 64 * ld * 2 + B * 2 * ld, device=device) if G else None
        mr = D.fill((B, 64, 2), rows=False) if c["mr"] else None
        i = (B, S, ld, G, c["n_norm"], c["flags"], c["addvec_ld"], c["res_ld"], S // 256 if c["tiles"] else 0)
        p = (x, D.put(d["gamma"]) if G else None, D.put(d["beta"]) if G else None, D.opt("addvec"), D.opt("res", rows=True), part, y,
             D.opt("tsum"), D.opt("tsq"), None, mr)
        outs = dict(out=y)
        if mr is not None:
            outs["mr"] = mr
        return i, p, f, outs
    if op == "gn_joint":
        B, npt, K = c["B"], c["np_"], c["K"]
        ldq, ldk = d["q"].shape[1], d["k"].shape[1]
        tq, tk = (npt // 256 if npt % 256 == 0 else 1), npt * K // 256
        ssq, ssk = D.fill((B, 2, ldq), rows=False), D.fill((B, 2, ldk), rows=False)
        i = (B, c["C1"], ldq, tq, K, c["C2"], ldk, tk, c["G"])
        p = (D.put(d["qsum"]), D.put(d["qsq"]), D.put(d["ksum"]), D.put(d["ksq"]), D.put(d["gamma"]),
             None if c.get("null") else D.put(d["beta"]), ssq, ssk)
        return i, p, (1.0 / (npt * K), float(c["n_norm"])), dict(ssq=ssq, ssk=ssk)
    if op == "concat_qk":
        rows = c["pts"] * c["K"]
        out = D.fill((rows, c["ldo"]))
        return (rows, c["K"], c["C1"], c["ldq"], c["C2"], c["ldk"], c["ldo"]), (D.rows(d["q"]), D.rows(d["k"]), out), f, dict(out=out)
    if op == "attn":
        out = D.fill((c["pts"], c["ldo"]))
        i = (c["pts"], c["K"], c["C"], c["lds"], c["ldv"], c["ldo"], c["pps"], c["v_relu"])
        return i, (D.rows(d["S"]), D.rows(d["V"]), out, D.opt("counts"), D.opt("vss")), f, dict(out=out)
    if op == "pool":
        out = D.fill((c["pts"], c["ldo"]))
        return (c["pts"], c["K"], c["C"], c["ldx"], c["ldo"], c["mode"]), (D.rows(d["x"]), out, D.opt("counts")), f, dict(out=out)
    if op == "pair_expand":
        B, npt, K, ld = c["B"], c["np_"], c["K"], c["ld"]
        rows = B * npt * K
        out = D.fill((rows, ld))
        outs = dict(out=out)
        st = (None, None)
        if c["stats"]:
            st = (D.fill(((rows + 255) // 256, ld), rows=False), D.fill(((rows + 255) // 256, ld), rows=False))
            outs.update(sum=st[0], sq=st[1])
        i = (B, c["N"], npt, K, ld, d["A"].shape[1], (1 if c["relu"] else 0) | (2 if c["fp"] else 0) | (16 if c["idx32"] else 0))
        p = (D.put(d["A"]), D.put(d["bias"]), D.put(d["coef"]), D.put(d["xyz"]), D.put(d["new_xyz"]), D.put(d["idx"]), D.put(d["d2"]),
             out, st[0], st[1])
        return i, p, f, outs
    raise KeyError(op)


def _np(t):
    return t.float().cpu().numpy().astype(np.float64) if t.dtype.is_floating_point else t.cpu().numpy()


def _check(name, ref, got, what=""):
    """every element of every output against the reference under the case's bound; returns the worst err / tol"""
    worst = 0.0
    for k, o in ref.items():
        if k not in got:
            continue
        r = ratio(o, got[k])
        i = np.unravel_index(np.argmax(r), r.shape)
        exact = bool((o["b"] == 0).all())
        print("%s%s [%s]: %s, worst err/tol %.3g at %s (got %.9g, ref %.9g), %d elements" %
              (name, what, k, "exact" if exact else "bounded", r[i], i, np.asarray(got[k])[i], o["y"][i], r.size))
        if exact:
            assert np.array_equal(np.asarray(got[k], np.float64), o["stored"]), (name, k, i)
        assert r.max() <= 1, (name, k, float(r.max()), i)
        worst = max(worst, float(r.max()))
    return worst


def _run_case(c, d, device):
    """launches the case's op alone; -> {output name: float64 array}"""
    i, p, f, outs = _build(c, d, device)
    st = _status(KIND[c["op"]], c["half"], i, p, f)
    if c["status"] != 0:
        assert st == c["status"] * 1000, (c["name"], st)  # (slide_run_ops: status * 1000 - index of the failing op)
        for t in outs.values():
            assert bool((t == PREFILL).all()), "a refused op must not write"
        return None
    assert st == 0, (c["name"], st)
    got = {k: _np(t) for k, t in outs.items()}
    if c["op"] == "gn":
        if not c["inplace"]:
            assert np.array_equal(_np(p[0]), RC.T(c, d["x"])), "out of place: the input must stay"
        if c["split"]:
            got["table"] = _gn_split(c, d, device, got["out"])
    return got


def _gn_split(c, d, device, one_call):
    """GN_STATS_ONLY publishes the table and leaves the tensor alone; GN_APPLY_ONLY with that table equals the one call bit for bit"""
    import torch
    i, p, f, outs = _build(c, d, device)
    x0 = p[0].clone()
    table = torch.full((c["B"], 2, c["ld"]), PREFILL, device=device)
    i1 = i[:5] + (i[5] | RC.GN_STATS_ONLY,) + i[6:]
    assert _status(KIND["gn"], c["half"], i1, p[:9] + (table,)) == 0
    assert torch.equal(p[0], x0), "GN_STATS_ONLY must not touch the tensor"
    i2 = i[:5] + (i[5] | RC.GN_APPLY_ONLY,) + i[6:]
    assert _status(KIND["gn"], c["half"], i2, p[:7] + (None, None, table)) == 0
    assert np.array_equal(_np(outs["out"]), one_call), "GN_APPLY_ONLY with the published table differs from the one-call result"
    return _np(table)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUN_CASES)
def test_rows_op_matches_float64(gpu_device, name):
    c = CASE_BY_NAME[name]
    d = make_data(c)
    got = _run_case(c, d, gpu_device)
    if got is None:
        print("%s: status %d as expected, nothing written" % (name, c["status"] * 1000))
        return
    ref = forward(c, d)
    if c["op"] == "gn" and c["G"] > 0 and not c["split"]:
        ref.pop("table")
    if c["op"] == "gn" and not c["mr"]:
        ref.pop("mr", None)
    assert set(ref) == set(got), (sorted(ref), sorted(got))
    worst = _check(name, ref, got)
    if c["op"] == "gn_joint":  # end to end: the two tables applied to the stored q, k are GroupNorm of the materialised [q x K | k]
        yq, yk, bq, bk = RC.joint_end_to_end(c, d)
        C1, C2 = c["C1"], c["C2"]
        q, k = RC.T(c, d["q"])[:, :C1], RC.T(c, d["k"])[:, :C2]
        B = c["B"]
        aq = q.reshape(B, -1, C1) * got["ssq"][:, 0:1, :C1] + got["ssq"][:, 1:2, :C1]
        ak = k.reshape(B, -1, C2) * got["ssk"][:, 0:1, :C2] + got["ssk"][:, 1:2, :C2]
        rq = np.abs(aq.reshape(-1, C1) - yq) / np.where(bq > 0, bq, 1)
        rk = np.abs(ak.reshape(-1, C2) - yk) / np.where(bk > 0, bk, 1)
        assert (np.abs(aq.reshape(-1, C1) - yq)[bq == 0] == 0).all() and (np.abs(ak.reshape(-1, C2) - yk)[bk == 0] == 0).all()
        print("%s: tables applied to q / k against GroupNorm of the concatenation: worst err/tol %.3g / %.3g" % (name, rq.max(), rk.max()))
        assert rq.max() <= 1 and rk.max() <= 1, (float(rq.max()), float(rk.max()))
        worst = max(worst, float(rq.max()), float(rk.max()))
    print("WORST %s %s %s %.4g" % (c["op"], "f16" if c["half"] else "f32", name, worst))


@pytest.mark.gpu
def test_ncx_round_trip(gpu_device):
    """to_ncx(from_ncx(x)) is x (fp32 rows) or fp16(x) (fp16 rows), through the public wrappers"""
    import torch
    from slide_amd import rows as R
    for h in (False, True):
        for name in ("c33_p1000", "c515_p33", "c1_p1"):
            c = CASE_BY_NAME["from_ncx_%s_%s" % (name, "f16" if h else "f32")]
            x = make_data(c)["x"]
            r = R.from_ncx(torch.from_numpy(x).to(gpu_device), half=h)
            assert r.data.dtype == (torch.float16 if h else torch.float32) and bool((r.data[:, c["C"]:] == 0).all())
            back = R.to_ncx(r).cpu().numpy()
            assert np.array_equal(back, x.astype(np.float16).astype(np.float32) if h else x), (name, h)


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _wrapped(c, d, device):
    """the same case through the public wrapper of slide_amd.rows -> {output name: float64 array}"""
    import torch
    from slide_amd import rows as R
    D = _Dev(c, d, device)
    op, h = c["op"], c["half"]
    if op == "from_ncx":
        return dict(out=_np(R.from_ncx(D.put(d["x"]), half=h).data))
    if op == "to_ncx":
        return dict(out=_np(R.to_ncx(R.Rows(D.rows(d["rows"]), c["B"], c["P"], c["C"]))))
    if op == "group":
        feat = R.Rows(D.rows(d["feat"]), c["B"], c["N"], c["C"]) if c["C"] else None
        r = R.group(D.put(d["xyz"]), D.put(d["new_xyz"]), feat, D.put(d["idx"]), c["flags"] & 15, d2=D.put(d["d2"]),
                    empty_counts=D.opt("counts"), half=h)
        return dict(out=_np(r.data))
    if op == "gn":
        x = R.Rows(D.rows(d["x"]), c["B"], c["S"], c["C"])
        if c["tiles"]:
            x.stats = (D.put(d["tsum"]), D.put(d["tsq"]), bool(c["flags"] & RC.GN_PRE_RELU))
        gn = _ns(num_groups=c["G"], num_channels=c["n_norm"], weight=D.put(d["gamma"]), bias=D.put(d["beta"]))
        res = R.Rows(D.rows(d["res"]), c["B"], c["S"], c["C"]) if c["res_ld"] else None
        R.norm_act(x, gn=gn, pre_relu=bool(c["flags"] & 1), relu=bool(c["flags"] & 2), addvec=D.opt("addvec"), residual=res)
        return dict(out=_np(x.data))
    if op == "gn_joint":
        B, npt, K = c["B"], c["np_"], c["K"]
        q = R.Rows(D.rows(d["q"]), B, npt, c["C1"], stats=(D.put(d["qsum"]), D.put(d["qsq"]), True))
        k = R.Rows(D.rows(d["k"]), B, npt * K, c["C2"], stats=(D.put(d["ksum"]), D.put(d["ksq"]), True))
        gn = _ns(num_groups=c["G"], num_channels=c["n_norm"], weight=D.put(d["gamma"]), bias=D.put(d["beta"]))
        assert R.joint_norm_qk(q, k, K, gn)
        return dict(ssq=_np(q.pending[0]).reshape(B, 2, -1), ssk=_np(k.pending[0]).reshape(B, 2, -1))
    if op == "concat_qk":
        q, k = R.Rows(D.rows(d["q"]), 1, c["pts"], c["C1"]), R.Rows(D.rows(d["k"]), 1, c["pts"] * c["K"], c["C2"])
        return dict(out=_np(R.concat_qk(q, k, c["K"]).data))
    if op == "attn":
        nsmp = c["pts"] // c["pps"]
        s = R.Rows(D.rows(d["S"]), nsmp, c["pps"] * c["K"], c["C"])
        v = R.Rows(D.rows(d["V"]), nsmp, c["pps"] * c["K"], c["C"])
        if c["vss"]:
            v.pending = (D.put(d["vss"]), bool(c["v_relu"]), None)
        return dict(out=_np(R.attend(s, v, c["K"], counts=D.opt("counts")).data))
    if op == "pool":
        x = R.Rows(D.rows(d["x"]), 1, c["pts"] * c["K"], c["C"])
        return dict(out=_np(R.pool(x, c["K"], c["mode"], counts=D.opt("counts")).data))
    raise KeyError(op)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["wrap"]])
def test_public_wrapper_packs_the_same_op(gpu_device, name):
    """norm_act / group / attend / pool / concat_qk / from_ncx / to_ncx / joint_norm_qk pack the slots the op-level case used:
    the wrapper's result is inside the same bound around the same reference"""
    c = CASE_BY_NAME[name]
    d = make_data(c)
    got = _wrapped(c, d, gpu_device)
    ref = {k: v for k, v in forward(c, d).items() if k in got}
    assert set(ref) == set(got)
    _check(name, ref, got, what=" (wrapper)")


@pytest.mark.gpu
def test_pair_coef_matches_the_case_coefficients(gpu_device):
    """rows._pair_coef derives (W_rel + W_abs | W_centre - W_rel | w_d2 | w_w) from a convolution's coordinate columns: the table the
    PAIR_EXPAND cases are launched with"""
    import torch
    from slide_amd import rows as R
    for name, flags in (("pair_expand_ld64_b1_f16", R.GROUP_ABS | R.GROUP_CENTER), ("pair_expand_ld64_b7_fp_f16", R.GROUP_FP)):
        c = CASE_BY_NAME[name]
        d = make_data(c)
        ld = c["ld"]
        if flags & R.GROUP_FP:
            w2 = np.concatenate([d["coef"][:, 6:7], d["coef"][:, 7:8], d["w_abs"], d["w_rel"], d["w_ctr"]], 1)
        else:
            w2 = np.concatenate([d["w_rel"], d["w_abs"], d["w_ctr"]], 1)
        coef = R._pair_coef(torch.from_numpy(w2).to(gpu_device), 0, flags, ld).cpu().numpy()
        assert np.array_equal(coef, d["coef"]), name


@pytest.mark.gpu
@pytest.mark.parametrize("op", RC.OPS)
def test_empty_inputs_launch_nothing(gpu_device, op):
    """B = 0, np / P / S = 0: status 0, no launch, the output untouched"""
    for h in ((True,) if op == "pair_expand" else (False, True)):
        c = next(c for c in CASES if c["op"] == op and c["half"] == h and c["status"] == 0)
        d = make_data(c)
        for slot in EMPTY_SLOTS[op]:
            i, p, f, outs = _build(c, d, gpu_device)
            if op == "gn":
                outs = dict(out=p[6]) if not c["inplace"] else {}
                x0 = p[0].clone()
            i = tuple(0 if k == slot else v for k, v in enumerate(i))
            assert _status(KIND[op], h, i, p, f) == 0, (op, h, slot)
            for t in outs.values():
                assert bool((t == PREFILL).all()), (op, h, slot)
            if op == "gn":
                assert bool((p[0] == x0).all())


@pytest.mark.gpu
def test_fp32_and_fp16_rows_agree_where_exact(gpu_device):
    """movers, MAX pooling and the concatenation are exact in both instantiations: on fp16-representable inputs they give the
    same numbers (the two walk different columns per thread)"""
    n = 0
    for c in CASES:
        exact = c["op"] in ("from_ncx", "to_ncx", "concat_qk") or (c["op"] == "pool" and c["mode"] == RC.POOL_MAX) or \
            (c["op"] == "group" and c["flags"] & RC.GROUP_NO_XYZ)
        if not exact or c["half"] or c["status"] != 0:
            continue
        ch = CASE_BY_NAME[c["name"][:-4] + "_f16"]
        d = {k: (v.astype(np.float16).astype(np.float32) if v.dtype == np.float32 else v) for k, v in make_data(c).items()}
        a, b = _run_case(c, d, gpu_device), _run_case(ch, d, gpu_device)
        for k in a:
            assert np.array_equal(a[k], b[k]), (c["name"], k)
        n += 1
    print("fp32 and fp16 rows agree bit for bit on %d exact cases" % n)
    assert n >= 20
