"""The attention tails one launch at a time against float64, elementwise, at bounds derived from the kernels' rounding steps:
SLIDE_OP_ATTN_TAIL in its five fp16 instantiations (register-X form with fragment-major / chunk-major / row-major u and mo, LDS-ring
form) and in the split arithmetic, and the three-launch form ending in SLIDE_OP_ATTN_COMBINE (tests/tail_cases.py: the case matrix with
its branch -> case table, the reference, the derivations, the CPU kernel model and the mutants the bounds must see).  Every launch is
emitted by the engine's own emitters (_attn_tail, _attn_combine) on a bare plan builder, so the host-side packing -- w5 scattered
through the padded GroupNorm layout, wv zero-padded, the four vectors, chunk-major weights, the f[1] bits -- is under test as well.
Product library only."""
import numpy as np
import pytest

import tail_cases as T
from tail_cases import CASES, CASE_BY_NAME, EXEMPT, KERNELS, NON_MUTANTS, PREFILL, RUN, forward, make_data, model, mutants, ru
from test_hip_pair_arith import _mini, _run

APFX = "att"


# ------------------------------------------------------------------------------------------------------------------- CPU
_REF = {}


def _ref(c):
    """(data, reference) of a case, computed once and shared (nobody writes to either)"""
    if c["name"] not in _REF:
        d = make_data(c)
        _REF[c["name"]] = (d, forward(c, d))
    return _REF[c["name"]]


def _ratio(a, ref):
    return float((np.abs(a - ref["y"]) / ref["b"]).max())


def test_tail_bounds_see_the_mutants():
    """every case's bound is tighter than the deviation of each of its mutants in at least one element of the STORED output (or the
    exemption names a case of the same kernel where that mutant is visible); no mutant is exempt everywhere"""
    seen = {}
    for c in RUN:
        d, ref = _ref(c)
        assert np.isfinite(ref["b"]).all() and (ref["b"] > 0).all(), c["name"]
        assert _ratio(ref["stored"], ref) <= 1, c["name"]  # (the reference's own rounding fits)
        for m in mutants(c):
            assert m in T.MUTANT_DOC, m
            if m == "out2_all_channels":  # the second store is compared for equality: any difference shows
                z = np.arange(4 * ru(c["cout"]), dtype=np.float64).reshape(4, -1)
                seen[(c["name"], m)] = np.inf if (T.second_stores(c, z)[1] != T.second_stores(c, z, m)[1]).any() else 0.0
                continue
            seen[(c["name"], m)] = _ratio(forward(c, d, mutant=m)["stored"], ref)
    for (name, m), r in sorted(seen.items()):
        print("%-20s %-22s %.3g" % (name, m, r))
    for (name, m), r in seen.items():
        if (name, m) in EXEMPT:
            other = EXEMPT[(name, m)]
            assert CASE_BY_NAME[other]["kernel"] == CASE_BY_NAME[name]["kernel"], (name, other)
            assert seen[(other, m)] > 1, (name, m, other, seen[(other, m)])
        else:
            assert r > 1, "case %s: the bound does not see mutant %s (max deviation / bound %.3g)" % (name, m, r)
    for m in T.MUTANT_DOC:
        assert any(k[1] == m for k in seen), m  # every documented mutant applies somewhere
        assert any(k[1] == m and k not in EXEMPT for k in seen), m  # no mutant is exempt everywhere
        for kern in {c["kernel"] for c in RUN if m in mutants(c)}:  # ... nor for a whole kernel
            assert any(seen[(c["name"], m)] > 1 for c in RUN if c["kernel"] == kern and m in mutants(c)), (m, kern)


def test_kernel_model_fits_the_bound():
    """the kernel's steps in float32 (tail_cases.model) lie inside every case's bound, and so do the documented non-mutants"""
    assert NON_MUTANTS == ("drop_score_bias", "ieee_division")
    for c in RUN:
        d, ref = _ref(c)
        r = _ratio(model(c, d), ref)
        nm = {}
        if not c["combine_only"]:  # (there S is an INPUT, rounded to fp16 with its bias: a bias-free S is another input)
            nm["drop_score_bias (reference)"] = _ratio(forward(c, d, mutant="drop_score_bias")["stored"], ref)
        if c["form"] != "three":
            nm["drop_score_bias"] = _ratio(model(c, d, "drop_score_bias"), ref)
            nm["ieee_division"] = _ratio(model(c, d, "ieee_division"), ref)
        print("%-20s [%s] model / bound %.3g; %s" % (c["name"], c["kernel"], r, ", ".join("%s %.3g" % kv for kv in nm.items())))
        assert r <= 1, (c["name"], r)
        for k, v in nm.items():
            assert v <= 1, (c["name"], k, v)


def test_case_matrix_reaches_every_branch():
    """every instantiation the product build's two launchers (and the combine launch) can select has a case, the module docstring's
    table names every case, and the sets of shapes, layouts and distributions the suite promises are all present"""
    kernels = {c["kernel"] for c in RUN}
    for k in KERNELS:
        assert k in kernels, k
        assert k.split("<")[0] in T.__doc__
    for c in CASES:
        assert c["name"] in T.__doc__, c["name"]
    k1 = lambda c: T.layout(c["inter"])[1] // 32
    for form in ("rx_fm", "rx"):
        cs = [c for c in RUN if c["form"] == form]
        assert {c["k2"] // 32 for c in cs} == {4, 8}
        assert {k1(c) for c in cs} == {1, 2, 3, 4, 5} and {(k1(c) - 1) % 4 for c in cs} == {0, 1, 2, 3}
        assert {(c["npxl"], c["B"]) for c in cs} >= {(8, 1), (8, 9), (7, 1), (7, 3)}
    assert {c["xlay"] for c in RUN if c["form"] == "rx_fm"} == {"fm"} and {c["xlay"] for c in RUN if c["form"] == "rx"} == {"cm", "rm"}
    assert {(c["npxl"], c["xlay"]) for c in RUN if c["form"] == "rx" and c["xlay"] == "rm"} == {(8, "rm"), (7, "rm")}
    ring = [c for c in RUN if c["form"] == "ring"]
    assert {c["k2"] // 32 for c in ring} == {1, 2, 3, 5} and {k1(c) for c in ring} == {1, 4}
    assert {(c["npxl"], c["xlay"]) for c in ring} == {(8, "cm"), (8, "rm"), (7, "cm"), (7, "rm")}
    sp = [c for c in RUN if c["form"] == "split"]
    assert {32, 96, 160} <= {c["k2"] for c in sp} | {k1(c) * 32 for c in sp}
    assert {c["wmax"] for c in sp} >= {30.9} and CASE_BY_NAME["three16_w315"]["wmax"] == 31.5
    for group in ([c for c in RUN if c["form"] in ("rx_fm", "rx", "ring")], sp):
        assert {8, 40, 72, 1024} <= {c["cout"] for c in group}
        assert {c["B"] for c in group} == {1, 3, 9} and {c["npxl"] for c in group} == {7, 8}
        assert any(c["out2"] and c["out2"][1] > c["out2"][0] and c["out2"][0] % 32 for c in group)
    assert {c["cout"] for c in RUN} >= {8, 32, 40, 72, 128, 256, 512, 1024}
    assert all(c["B"] == 1 for c in RUN if c["cout"] == 1024)
    for form in ("rx_fm", "rx", "ring"):
        assert any(c["out_cm"] for c in RUN if c["form"] == form) and any(c["out2"] for c in RUN if c["form"] == form)
    assert {c["dist"] for c in RUN} == {"normal", "common", "peaked", "flat", "bias50", "var0"}
    padded = [c for c in RUN if len(T.layout(c["inter"])[0]) and not np.array_equal(T.layout(c["inter"])[0], np.arange(c["inter"]))]
    assert len(padded) >= 2 and any(c["k2l"] < c["k2"] for c in RUN)
    assert {c["kernel"] for c in T.THREE} == {k for k in KERNELS if k.startswith("attn_combine")}
    assert {(c["status"], c["name"]) for c in T.STATUS} == {(-3, "st_fm_rows"), (-3, "st_fm_no_cm"), (-3, "st_k1"), (-4, "st_ring_n6")}


# ------------------------------------------------------------------------------------------------------------------- emission
def _to_layout(x, xlay):
    """[rows][k] -> the same values as the buffer's bytes, viewed [rows][k]: row-major, chunk-major [k / 32][rows][32], or fragment-major
    inside every 32-row group of a chunk (SLIDE_F_OUT_FM, include/slide_engine.h) -- the inverse of test_hip_pair_arith._read_out"""
    rows, k = x.shape
    if xlay == "rm":
        return x
    flat = np.empty((k // 32, rows * 32), x.dtype)
    r, ch = np.arange(rows)[:, None], np.arange(32)[None, :]
    idx = (r & ~31) * 32 + (ch >> 4) * 512 + ((ch >> 3) & 1) * 256 + (r & 31) * 8 + (ch & 7) if xlay == "fm" else r * 32 + ch
    for kc in range(k // 32):
        flat[kc][idx] = x[:, 32 * kc:32 * kc + 32]
    return flat.reshape(rows, k)


def _build(c, d, device):
    """emits the case's launches on a bare plan builder; returns (builder, launch, number of ops, tensors by name)"""
    import torch
    from slide_amd import engine as E
    B, npxl, cout = c["B"], c["npxl"], c["cout"]
    rows, pts, Cp = B << npxl, B * 16, ru(cout)
    m = _mini(B, c["prec"], device)
    m.use_cm = c["prec"] == "fp16" and c["xlay"] != "rm"
    m._tail_of = {}
    m.sd = {APFX + ".weight_conv.5.weight": d["W5"][:, :, None], APFX + ".weight_conv.5.bias": d["b5"],
            APFX + ".feat_out_conv.0.weight": d["Wv"][:, :, None], APFX + ".feat_out_conv.0.bias": d["bv"],
            APFX + ".feat_out_conv.1.group_norm.weight": d["gamma"], APFX + ".feat_out_conv.1.group_norm.bias": d["beta"]}
    lay = E.gn_layout(c["inter"])
    t = {}
    for k, x in zip(("u", "mo"), T.physical(c, d)):
        if c["xlay"] == "rm":
            t[k] = m.A.put(x, m.adt)
        else:
            t[k] = m._buf(rows, x.shape[1], cm=True, fm=c["xlay"] == "fm")
            t[k].copy_(torch.from_numpy(_to_layout(x, c["xlay"])).to(m.adt))
    out_ld = Cp + (32 if B == 3 else 0)
    t["out"] = torch.full((pts + 4, out_ld), PREFILL, dtype=m.adt, device=device)  # (four rows past the last point)
    m.A.keep.append(t["out"])
    if c["form"] == "three":
        S = m._buf(rows, cout)
        m._gemm(t["u"], npxl, [dict(w=d["W5"], bias=d["b5"], mode=E.EPI_RAW, out=S)], in_cols=lay.index)
        L = m._attn_combine(APFX, npxl, S, t["mo"], t["out"])
        assert L.op.i[0] == pts and [e.op.kind for e in m.plan] == [E.OP_GEMM, E.OP_GEMM, E.OP_ATTN_COMBINE]
        t["S"], t["V"] = S, _tensor_at(m, L.op.p[1])
        assert L.op.p[0] == S.data_ptr() and t["V"].shape == S.shape
        return m, L, 3, t
    L = m._attn_tail(APFX, npxl, t["u"], lay, t["mo"], t["out"])
    assert L is m.plan[-1] and len(m.plan) == 1 and L.op.kind == E.OP_ATTN_TAIL and m._tail_of[t["out"].data_ptr()] is L
    ocm = m._cm_copy.get(t["out"].data_ptr())
    assert (ocm is not None) == c["out_cm"]
    if ocm is not None:
        ocm.fill_(PREFILL)
        t["out_cm"] = ocm
    if c["out2"] is not None:  # as _fp_module folds the copy of the skip features into the tail that wrote them
        n2, ld2 = c["out2"]
        t["out2"] = torch.full((pts + 4, ld2), PREFILL, dtype=m.adt, device=device)
        m.A.keep.append(t["out2"])
        L.op.p[7], L.op.f[2], L.op.f[3] = t["out2"].data_ptr(), float(ld2), float(n2)
    if c["patch"] is not None:
        arr, k, v = c["patch"]
        getattr(L.op, arr)[k] = v
    return m, L, 1, t


def _tensor_at(m, ptr):
    return [t for t in m.A.keep if hasattr(t, "data_ptr") and t.data_ptr() == ptr][0]


def test_tail_packing_on_cpu(monkeypatch):
    """each fused case's op, built on the CPU device through _attn_tail and unpacked: weights, vectors, i[], f[] and the pointers"""
    import torch
    from slide_amd import engine as E
    for c in T.FUSED16 + T.SPLIT:
        d = make_data(c)
        monkeypatch.delenv("SLIDE_CM_TABLES", raising=False)
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
        m, L, _, t = _build(c, d, torch.device("cpu"))
        op, h = L.op, c["prec"] == "fp16"
        cout, npxl = c["cout"], c["npxl"]
        Cp, rows = ru(cout), c["B"] << npxl
        idx, k1 = T.layout(c["inter"])
        lay, vlay = E.gn_layout(c["inter"]), E.gn_layout(cout)
        assert vlay.unpermuted and k1 == ru(lay.width) and np.array_equal(idx, lay.index)
        q = T.r16 if h else (lambda a: np.asarray(a, np.float64))

        def logical(ptr, k):
            w = _tensor_at(m, ptr)
            assert w.dtype == (torch.float16 if h else torch.float32)
            w = w.float().numpy().astype(np.float64)
            if m.use_cm:
                assert w.shape == (k // 32, Cp, 32)
                w = w.transpose(1, 0, 2).reshape(Cp, k)
            assert w.shape == (Cp, k)
            return w
        w5 = np.zeros((Cp, k1))
        w5[np.ix_(np.arange(cout), idx)] = q(d["W5"])
        wv = np.zeros((Cp, c["k2"]))
        wv[:cout, :c["k2l"]] = q(d["Wv"])
        assert np.array_equal(logical(op.p[1], k1), w5), c["name"]
        assert np.array_equal(logical(op.p[3], c["k2"]), wv), c["name"]
        assert not w5[:, np.setdiff1d(np.arange(k1), idx)].any()  # (only zero columns meet u's padding)
        vec = _tensor_at(m, op.p[5]).numpy()
        want = np.zeros((4, Cp), np.float32)
        want[0, :cout], want[1, :cout] = d["b5"], d["bv"]
        want[2, :len(d["gamma"])], want[3, :len(d["beta"])] = d["gamma"], d["beta"]
        assert vec.dtype == np.float32 and np.array_equal(vec, want) and np.array_equal(vec, m._tail_vectors(APFX, Cp)), c["name"]
        G, n_norm, gs = T.gn_params(cout)
        ldx = 32 if c["xlay"] != "rm" else None
        assert list(op.i[:10]) == [rows, ldx or k1, k1, ldx or c["k2"], c["k2"], Cp // 32, npxl, gs, n_norm, t["out"].shape[1]], c["name"]
        assert (vlay.gs, vlay.gs_logical, vlay.n_norm) == (gs, gs, n_norm) and m._ldp(t["u"]) == (ldx or k1)
        assert op.f[0] == np.float32(1.0 / (gs * (1 << npxl))), c["name"]
        f1 = int(op.f[1])
        assert op.f[1] == f1 and f1 == (1 if m.use_cm else 0) | (0 if h else 8) | (16 if c["xlay"] == "fm" else 0), (c["name"], f1)
        assert (op.p[0], op.p[2], op.p[4]) == (t["u"].data_ptr(), t["mo"].data_ptr(), t["out"].data_ptr())
        assert op.p[6] == (t["out_cm"].data_ptr() if c["out_cm"] else None)
        if c["out2"]:
            assert (op.p[7], op.f[2], op.f[3]) == (t["out2"].data_ptr(), c["out2"][1], c["out2"][0])
        else:
            assert op.p[7] is None
        assert T.dispatch(list(op.i), op.f[1]) == c["kernel"], c["name"]
        assert L.name == (None if h else c["kernel"])
        assert m._split1_ok(d["W5"], d["Wv"])
    for c in T.STATUS:
        m, L, _, _ = _build(c, make_data(c), torch.device("cpu"))
        assert T.dispatch(list(L.op.i), L.op.f[1]) == c["status"], c["name"]
    c = CASE_BY_NAME["three16_w315"]
    d = make_data(c)
    assert not E.DenoiserEngine._split1_ok(d["W5"], d["Wv"])  # the plan takes the three launches


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_attn_tail_matches_float64(gpu_device, monkeypatch, name):
    c = CASE_BY_NAME[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    d = make_data(c)
    m, L, n_ops, t = _build(c, d, gpu_device)
    if c["status"] != 0:  # host-side refusal before any launch
        assert T.dispatch(list(L.op.i), L.op.f[1]) == c["status"]
        st = _run(m, n_ops)
        assert st == c["status"] * 1000, (name, st)
        assert (t["out"].float().cpu().numpy() == PREFILL).all()
        print("%s: status %d as expected" % (name, st))
        return
    if c["form"] == "three":
        from slide_amd import engine as E
        assert L.op.kind == E.OP_ATTN_COMBINE and (L.op.i[5], L.op.i[6]) == (1 << (c["npxl"] - 4), E.PREC[c["prec"]])
        if c["wmax"] == 31.5:
            assert not m._split1_ok(d["W5"], d["Wv"])
        if c["combine_only"]:
            import torch
            # the product build refuses the fp16 ring GEMM of 128-row samples on stored inputs (SLIDE_ST_EXPERIMENT, csrc/gemm_ring.hip) before
            # any launch; the combine launch then runs alone, on S and V as the reference stores them
            assert _run(m, n_ops) == -20 * 1000
            for k, a in zip(("S", "V"), T._scores_values(c, d)[:2]):
                full = np.full(tuple(t[k].shape), PREFILL)
                full[:, :c["cout"]] = a
                t[k].copy_(torch.from_numpy(full).to(t[k].dtype))
            n_ops = 1
    else:
        assert T.dispatch(list(L.op.i), L.op.f[1]) == c["kernel"] and L.name == (None if c["prec"] == "fp16" else c["kernel"])
    st = _run(m, n_ops)
    assert st == 0, (name, st)
    ref = forward(c, d)
    cout, pts = c["cout"], c["B"] * 16
    Cp = ru(cout)
    raw = t["out"].float().cpu().numpy().astype(np.float64)
    got = raw[:pts, :cout]
    assert np.isfinite(raw).all()
    err = np.abs(got - ref["y"])
    ratio = err / ref["b"]
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s [%s, %s]: worst err/tol %.3g (err %.3g, |ref| %.3g at %s), worst err %.3g" %
          (name, c["prec"], c["kernel"], ratio[i], err[i], abs(ref["y"][i]), i, err.max()))
    assert ratio.max() <= 1, (name, float(ratio.max()), i)
    assert (raw[pts:] == PREFILL).all(), "rows at and past rows >> KLOG keep the prefill"
    if c["form"] == "three":  # (the combine launch writes the logical channels only)
        assert (raw[:pts, cout:] == PREFILL).all()
        return
    assert (raw[:pts, cout:Cp] == 0).all(), "pad channels hold what zero weights give: 0"
    assert (raw[:, Cp:] == PREFILL).all(), "columns past n_cob * 32 keep the prefill"
    ocm, o2 = T.second_stores(c, raw[:pts, :Cp])
    if ocm is not None:
        g = t["out_cm"].float().cpu().numpy().astype(np.float64).reshape(-1)
        assert np.array_equal(g[:ocm.size], ocm.reshape(-1)), "out_cm must be bit-equal to out, chunk-major"
        assert (g[ocm.size:] == PREFILL).all()
    if o2 is not None:
        g = t["out2"].float().cpu().numpy().astype(np.float64)
        assert np.array_equal(g[:pts], o2), "out2: the first out2_n columns bit-equal to out, everything else untouched"
        assert (g[pts:] == PREFILL).all()
