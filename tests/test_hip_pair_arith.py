"""The pair-decomposition ops one launch at a time against float64, elementwise, at bounds derived from the kernels' rounding steps:
SLIDE_OP_PAIR_FIRST, SLIDE_OP_PAIR_NORM version 2 with float tables, SLIDE_OP_GEMM_GX in fp16 and in split arithmetic, SLIDE_OP_SA_CHAIN,
and PAIR_FIRST -> GEMM_GX against the K-expanded float64 evaluation of the layers they decompose (tests/pair_cases.py: the case matrix
with its branch -> case table, the references, the derivations and the mutants the bounds must see).  Every launch is emitted by the
engine's own emitters (_pair_first, _gemm(gx=GxArgs), _chained_layer, _sa_chain) on a bare plan builder, so the host-side packing -- chunk-major weights,
packed epilogue vectors, column offsets, wa = W_rel + W_abs, wb = W_ctr - W_rel -- is under test as well.  Product library only."""
import ctypes

import numpy as np
import pytest

import pair_cases as P
from pair_cases import CASES, CASE_BY_NAME, EXEMPT, KERNELS, NON_MUTANTS, forward, make_data, mutants, ru


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_pair_bounds_see_the_mutants():
    """every case's bound is tighter than the deviation of each of its mutants in at least one element of the STORED output (or the
    exemption names a case of the same kernel where that mutant is visible); the documented non-mutants stay inside the bound"""
    seen = {}
    for c in CASES:
        if c["raises"] or c["status"] != 0 or c["op"] == "comp":
            continue
        if c["op"] in ("pf", "pn"):
            d = P.make_table_data(c)
            ref = P.table_forward(c, d)
            keys = [k for k in ref if k != "_ctx"]
            for k in keys:
                assert np.isfinite(ref[k][2]).all() and (ref[k][2] > 0).all(), (c["name"], k)
                assert float((np.abs(ref[k][1] - ref[k][0]) / ref[k][2]).max()) <= 1, (c["name"], k)
            for m in P.table_mutants(c):
                assert m in P.MUTANT_DOC, m
                mo = P.table_forward(c, d, mutant=m)
                seen[(c["name"], m)] = max(float((np.abs(mo[k][1] - ref[k][0]) / ref[k][2]).max()) for k in keys)
            continue
        d = make_data(c)
        ref = forward(c, d)
        assert np.isfinite(ref["b"]).all() and (ref["b"] > 0).all(), c["name"]
        assert float((np.abs(ref["stored"] - ref["y"]) / ref["b"]).max()) <= 1, c["name"]  # (the reference's own rounding fits)
        for m in mutants(c):
            assert m in P.MUTANT_DOC, m
            dev = np.abs(forward(c, d, mutant=m)["stored"] - ref["y"])
            seen[(c["name"], m)] = float((dev / ref["b"]).max())
        if c["op"] == "sa":
            r = float((np.abs(forward(c, d, mutant="h2_rounded")["stored"] - ref["y"]) / ref["b"]).max())
            print("%s: h2 rounded as the kernel does / kept unrounded: %.3g of the bound" % (c["name"], r))
            assert r <= 1, (c["name"], NON_MUTANTS, r)
    for (name, m), r in sorted(seen.items()):
        print("%-22s %-20s %.3g" % (name, m, r))
    for (name, m), r in seen.items():
        if (name, m) in EXEMPT:
            other = EXEMPT[(name, m)]
            assert CASE_BY_NAME[other]["kernel"] == CASE_BY_NAME[name]["kernel"], (name, other)
            assert seen[(other, m)] > 1, (name, m, other, seen[(other, m)])
        else:
            assert r > 1, "case %s: the bound does not see mutant %s (max deviation / bound %.3g)" % (name, m, r)
    for m in P.MUTANT_DOC:
        if any(k[1] == m for k in seen):
            assert any(k[1] == m and k not in EXEMPT for k in seen), m  # no mutant is exempt everywhere


def test_expanded_and_pair_form_references_agree():
    """the decomposition's algebra and the host's weight folding: the K-expanded float64 evaluation of a block's first layer
    ([feat[q] | rel | abs | centre (| d2 | w)] . W^T, GroupNorm over the K-expanded rows, ReLU, + add) and the pair-form float64
    reference (a[q] + b[p] + d2 vd + w vw from the normalised tables) agree to 1e-12 relative"""
    for c in P.COMP:
        d = P.make_table_data(c)
        a, b = P.comp_first_layer(c, d, True), P.comp_first_layer(c, d, False)
        r = float(np.abs(a - b).max() / np.abs(a).max())
        print("%s: K-expanded vs pair form %.3g" % (c["name"], r))
        assert r <= 1e-12, (c["name"], r)
        f = P.comp_forward(c, d)
        assert np.isfinite(f["b"]).all() and (f["b"] > 0).all()


def test_case_matrix_reaches_every_branch():
    """every instantiation the product build's launchers can select has a case, and the module docstring's table names it"""
    kernels = {c["kernel"] for c in CASES}
    for k in KERNELS:
        assert k in kernels, k
    for c in CASES:
        assert c["name"] in P.__doc__, c["name"]
    kernels_doc = P.__doc__
    for k in ("pair_first_kernel<false / true>", "pair_norm2_kernel<false / true, float, 512>"):
        assert k in kernels_doc
    gx = [c for c in CASES if c["op"] in ("gx", "gxs")]
    assert {c["B"] for c in gx} == {1, 3, 9}
    assert {32, 64, 96, 544} <= {c["k_pad"] for c in gx} and max(c["k_pad"] for c in gx) > 4096
    assert {(c["K"], c["k_pad"]) for c in gx} >= {(35, 64), (543, 544)}
    from slide_amd.engine import gn_layout
    assert {ru(gn_layout(c["N"])[1] if c["epi"] == P.EPI_NORM else c["N"]) // 32 for c in gx} >= {1, 2, 3, 5}  # n_cob
    assert {c["add"] for c in gx if c["gxmode"] == 0} == {None, "plain", "idx"}
    assert {c["nbr"] for c in gx if c["npxl"] == 7} == {"knn", "same", "q15"}
    assert {c["out"] for c in P.GX + P.SA} == {"rm", "cm", "fm"}
    assert any(c["coff"] > 0 and c["t_extra"] > 0 for c in gx)
    pf = [c for c in CASES if c["op"] == "pf"]
    assert {c["K"] for c in pf} == {8, 16} and {bool(c["lead"]) for c in pf} == {False, True}
    assert {s_[1:] for c in pf for s_ in c["segs"]} >= {(P.R, False), (P.NM, False), (P.ST, False), (P.ST, True)}
    assert {s_[0] for c in pf for s_ in c["segs"]} >= {51, 111, 64, 128} and {c["nbr"] for c in pf if c["K"] == 8} == {"knn", "same", "q15"}
    assert any(c["dist"] == "cluster" for c in pf) and any(c["dist"] == "cluster" for c in CASES if c["op"] == "pn")
    pn = [c for c in CASES if c["op"] == "pn"]
    assert {(c["K"], bool(c["fin"])) for c in pn if c["status"] == 0} == {(16, False), (16, True), (8, False), (8, True)}
    assert any(c["ld_claim"] == 2080 and c["status"] == -3 for c in pn)
    sa = [c for c in CASES if c["op"] == "sa"]
    assert {(c["K"], c["N"], c["chain"]["N"]) for c in sa} == {(64, 128, 256), (192, 256, 512), (128, 128, 512)}
    assert {c["add"] for c in sa} == {None, "plain", "idx"} and {c["add1"] for c in sa} == {False, True}


# ------------------------------------------------------------------------------------------------------------------- GPU
def _mini(B, prec, device):
    """just enough of DenoiserEngine to emit one launch of the pair decomposition"""
    from slide_amd import engine as E

    class M(E.DenoiserEngine):
        def __init__(self):
            self._plan_state(B, device, prec)
            self.use_cm = self.use_gx = prec == "fp16"
            self.use_gxs = prec == "split"
            self._cm, self._fm, self._cm_copy, self.sd = set(), set(), {}, {}
    return M()


def _alt(shape, v):
    a = np.full(shape, v, np.float32)
    a[..., 1::2] *= -1
    return a


def _window(a, c, big, pad):
    """[n][K] logical -> [n][t_ld]: the window [coff, coff + k_pad) holds a and finite padding (zero weights meet it), every other
    column a LARGE finite value of alternating sign (a read outside the window changes the result)"""
    t = _alt(a.shape[:-1] + (c["coff"] + c["k_pad"] + c["t_extra"],), big)
    t[..., c["coff"]:c["coff"] + c["k_pad"]] = _alt(a.shape[:-1] + (c["k_pad"],), pad)
    t[..., c["coff"]:c["coff"] + a.shape[-1]] = a
    return t


def _read_out(m, out, rows, Np):
    """the output as [rows][Np] floats: row-major, chunk-major [Np / 32][rows][32], or fragment-major inside every 32-row group"""
    g = out.float().cpu().numpy()
    if not m._is_cm(out):
        return g
    flat = g.reshape(Np // 32, rows * 32)
    r, ch = np.arange(rows)[:, None], np.arange(32)[None, :]
    if m._is_fm(out):
        idx = (r & ~31) * 32 + (ch >> 4) * 512 + ((ch >> 3) & 1) * 256 + (r & 31) * 8 + (ch & 7)
    else:
        idx = r * 32 + ch
    return np.concatenate([flat[k][idx] for k in range(Np // 32)], axis=1)


def _run(m, n_ops):
    import torch
    from slide_amd._lib import lib
    from slide_amd.engine import SlideOp
    ops = (SlideOp * n_ops)(*m.ops[-n_ops:])
    st = lib().slide_run_ops(ops, n_ops, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


def _add_tuple(m, c, d, width):
    """(tensor, offset, per-sample stride, idx tensor or None, idx stride) of the mode-0 add vector, rows padded to `width`"""
    def padded(a):
        t = _alt(a.shape[:-1] + (width,), 0.5)
        t[..., :a.shape[-1]] = a
        return m.A.put(t)
    if c["add"] == "plain":
        return (padded(d["add"]), 0, width, None, 0)
    if c["add"] == "idx":
        return (padded(d["add_tab"]), 0, width, m.A.put(np.array([d["add_t"]], np.int32)), c["B"] * width)
    return None


def _emit_gx(c, d, device):
    """emits a generated-X GEMM case on a plan builder of its own; returns what reading its outputs needs"""
    import torch
    from slide_amd import engine as E
    prec, B, K, k_pad, N, npxl = c["prec"], c["B"], c["K"], c["k_pad"], c["N"], c["npxl"]
    rows, h = B << npxl, prec == "fp16"
    m = _mini(B, prec, device)
    tdt = torch.float16 if h else torch.float32
    big = 3e4 if h else 1e30
    ta, tb = m.A.put(_window(d["ta"], c, big, 8.0), tdt), m.A.put(_window(d["tb"], c, big, 8.0), tdt)

    def seg_of(W, bias, gamma, beta, Nl, epi, flags, norm_layout):
        lay = E.gn_layout(Nl) if norm_layout else None
        oidx = lay[0] if lay is not None else np.arange(Nl)
        Np = ru(lay[1]) if lay is not None else ru(Nl)
        sg = dict(w=W, bias=bias, mode=epi, flags=flags)
        if lay is not None:
            n_norm = P.gn_params(Nl)[1]
            sg.update(layout=lay, gn=(gamma[:n_norm], beta[:n_norm]))
        return sg, oidx, Np

    def phys(a, oidx, Np, dtype=None):
        ap = np.zeros(a.shape[:-1] + (Np,), np.float32)
        ap[..., oidx] = a
        return m.A.put(ap, dtype)
    flags = (E.F_PRE_RELU if c["pre_relu"] else 0) | (E.F_POST_RELU if c["post_relu"] else 0)
    seg, oidx, Np = seg_of(d["W"], d["bias"], d["gamma"], d["beta"], N, c["epi"], flags, c["epi"] == E.EPI_NORM)
    pair_tabs = None
    if npxl == 7:
        pair_tabs = (m.A.put(d["nbr"].reshape(-1, 16)), m.A.put(d["d2"]), m.A.put(d["w"]))
    gx = E.GxArgs(ta, tb, c["coff"], k_pad, rows, c["gxmode"], _add_tuple(m, c, d, k_pad),
                  None if npxl == 8 else m.A.put(_window(np.stack([d["vd"], d["vw"]], 1), c, 3e4, 0.25)))
    kw = {}
    if c["gxmode"] == 1:
        pad1 = lambda a, v: np.concatenate([a, np.full((B, k_pad - K), v, np.float32)], 1)
        kw["in_affine"] = (m.A.put(pad1(d["scale"], 1.0)), m.A.put(pad1(d["shift"], 0.0)), 0, k_pad)

    def res_pair(Nl, oidx_, Np_):
        rvv = None if npxl == 8 else phys(np.stack([d["rvd"], d["rvw"]]), oidx_, Np_)
        return (phys(d["rta"], oidx_, Np_, tdt), phys(d["rtb"], oidx_, Np_, tdt), 0, rvv)
    ssum = ssq = None
    if c["chain"] is None:
        if c["out"] == "rm":
            out = torch.full((rows, Np), 7.0, dtype=tdt, device=device)
            m.A.keep.append(out)
        else:
            out = m._buf(rows, Np, cm=True, fm=c["out"] == "fm")
        seg["out"] = out
        if c["pair"]:
            seg["res_pair"] = res_pair(N, oidx, Np)
        if c["epi"] == E.EPI_STATS:
            ssum, ssq = m.A.zeros(B, Np), m.A.zeros(B, Np)
            seg["stats"] = (ssum, ssq, 0, c["stats_scale"])
        L = m._gemm(None, npxl, [seg], gx=gx, pair_tabs=pair_tabs, **kw)
    else:
        N2 = c["chain"]["N"]
        seg3, oidx, Np3 = seg_of(d["W2"], d["bias2"], d["gamma2"], d["beta2"], N2, E.EPI_NORM, E.F_POST_RELU, True)
        out = torch.full((rows, Np3), 7.0, dtype=tdt, device=device)
        m.A.keep.append(out)
        seg3.update(out=out, res_pair=res_pair(N2, oidx, Np3))
        if c["add1"]:
            seg["addvec"] = (m.A.put(d["add1"]), 0, N, None, 0)
        layer2 = m._chained_layer(seg3, npxl, rows, ru(N))
        seg["out"] = None
        L = m._gemm(None, npxl, [seg], gx=gx, pair_tabs=pair_tabs, chain=layer2, **kw)
        Np = Np3
    assert L.name == c["kernel"], (L.name, c["kernel"])
    return dict(m=m, out=out, rows=rows, Np=Np, oidx=oidx, ssum=ssum, ssq=ssq)


def _read_gx(e):
    """(got [rows][N], padded output columns, stats or None) of an emitted generated-X case after its launch"""
    got = _read_out(e["m"], e["out"], e["rows"], e["Np"])
    oidx = e["oidx"]
    stats = None if e["ssum"] is None else (e["ssum"].cpu().numpy()[:, oidx], e["ssq"].cpu().numpy()[:, oidx])
    return got[:, oidx], np.delete(got, oidx, axis=1), stats


def _launch_gx(c, d, device):
    """emits and runs a generated-X GEMM case; returns (status, got [rows][N], padded output columns, stats or None)"""
    e = _emit_gx(c, d, device)
    st = _run(e["m"], 1)
    return (st,) + _read_gx(e)


def _emit_sa(c, d, device):
    """emits an SA-chain case through _sa_chain; returns (plan builder, output buffer)"""
    import torch
    from slide_amd import engine as E
    B, k1, n1, n2 = c["B"], c["K"], c["N"], c["chain"]["N"]
    m = _mini(B, "fp16", device)
    if E.gn_layout(k1)[3] != E.gn_layout(k1)[4]:
        # (a first layer whose GroupNorm groups are padded -- 192 channels: groups of 6 in 8 -- is outside what the PLAN chains; the
        #  kernel takes any k1 % 64 == 0, which is what this case drives: the plan's eligibility test alone is set aside)
        m._sa_chain_shapes = lambda pfx, npx_log2: True
    pfx = "m"
    m.sd = {pfx + ".first_mlp.0.weight": np.zeros((k1, 1), np.float32), pfx + ".second_mlp.0.weight": d["W"],
            pfx + ".second_mlp.0.bias": d["bias"], pfx + ".rest_mlp.0.weight": d["W2"], pfx + ".rest_mlp.0.bias": d["bias2"],
            pfx + ".rest_mlp.1.group_norm.weight": d["gamma2"], pfx + ".rest_mlp.1.group_norm.bias": d["beta2"]}
    off1, offr, t_ld = 8 if c["t_extra"] else 0, (8 if c["t_extra"] else 0) + k1, k1 + n2 + 2 * c["t_extra"]
    tabs = []
    for a1, ar in ((d["ta"], d["rta"]), (d["tb"], d["rtb"])):
        t = _alt((B * 16, t_ld), 3e4)
        t[:, off1:off1 + k1], t[:, offr:offr + n2] = a1, ar
        tabs.append(m.A.put(t, torch.float16))
    add0 = _add_tuple(m, c, d, k1)
    pair = E.BlockPair(E.PairTables(tabs[0], tabs[1], t_ld, [off1, offr], B * 256, None, None, None), off1, offr, None,
                       E.GnLayout(np.arange(k1), k1, k1, 1, 1), None if add0 is None else E.AddVec(*add0), None)
    seg = dict(gn=(d["gamma"], d["beta"]))
    if c["add1"]:
        seg["addvec"] = (m.A.put(d["add1"]), 0, n1, None, 0)
    out = m._buf(B * 256, n2, cm=True, fm=c["out"] == "fm")
    assert m._sa_chain(pfx, 8, pair, seg, out, 0)
    assert m.plan[-1].name == c["kernel"], (m.plan[-1].name, c["kernel"])
    return m, out


def _launch_sa(c, d, device):
    """emits and runs an SA-chain case; returns (status, got [rows][n2], no padded columns, None)"""
    m, out = _emit_sa(c, d, device)
    st = _run(m, 1)
    return st, _read_out(m, out, c["B"] * 256, c["chain"]["N"]), np.zeros((1, 0)), None


def _launch_table(c, d, device):
    """emits a table pass through _pair_first (composition cases: and the consuming generated-X GEMM) and runs it; returns (status,
    {output name: array in logical channels}, every padded table / vv column, the consumer's output or None)"""
    import torch
    from slide_amd import engine as E
    B, C, K, npxl = c["B"], c["C"], c["K"], c["npxl"]
    nt = B * 16
    m = _mini(B, c["prec"], device)
    m.xyz = m.A.put(d["xyz"])
    if K == 8:
        m.kidx, m.kd2, m.kw = m.A.put(d["nbr"].reshape(nt, 16)), m.A.put(d["d2"]), m.A.put(d["w"])
    segs, lays, stats_t = [], [], {}
    fin = fin_t = None
    if c["fin"]:
        Cq, Ck = c["fin"], c["segs"][-1][0]
        Cf, gsf = Cq + Ck, (Cq + Ck) // 32
        fs, fq = np.zeros((B, Cf), np.float32), np.zeros((B, Cf), np.float32)
        fs[:, :Cq], fq[:, :Cq] = d["qsum"], d["qsq"]
        fin_t = dict(sum=m.A.put(fs), sq=m.A.put(fq), gid=m.A.put((np.arange(Cf) // gsf).astype(np.int32)),
                     gstart=m.A.put(np.arange(32, dtype=np.int32) * gsf), gend=m.A.put(np.arange(1, 33, dtype=np.int32) * gsf),
                     gamma=m.A.put(d["fin_gamma"]), beta=m.A.put(d["fin_beta"]), scale=m.A.zeros(B, Cf), shift=m.A.zeros(B, Cf))
        f_ = E.SlideGnFin()
        for k_, t_ in fin_t.items():
            setattr(f_, k_, t_.data_ptr())
        f_.inv_count, f_.C, f_.bs, f_.G = 1.0 / (gsf * 16 * K), Cf, Cf, 32
        fin = m.A.put(np.frombuffer(bytes(f_), dtype=np.uint8).copy())
    for i, ((N, mode, pre), sg) in enumerate(zip(c["segs"], d["segs"])):
        wf = sg["wf"] if C else np.zeros((N, 0), np.float32)
        s_ = dict(w=np.concatenate([wf, sg["wc"]], 1), bias=sg.get("bias"), mode=mode, flags=E.F_PRE_RELU if pre else 0, out=None)
        lay = E.gn_layout(N) if mode == E.EPI_NORM else None
        if lay is not None:
            n_norm = P.gn_params(N)[1]
            s_.update(layout=lay, gn=(sg["gamma"][:n_norm], sg["beta"][:n_norm]))
        if mode == E.EPI_STATS:
            if c["fin"] and i == len(c["segs"]) - 1:
                s_["stats"] = (fin_t["sum"], fin_t["sq"], c["fin"], 1.0)
            else:
                stats_t[i] = (m.A.zeros(B, ru(N)), m.A.zeros(B, ru(N)))
                s_["stats"] = stats_t[i] + (0, 1.0)
        segs.append(s_)
        lays.append((lay[0] if lay is not None else np.arange(N), ru(lay[1] if lay is not None else N)))
    coords = dict(rel=C, abs=C + 3, ctr=C + 6, d2=C + 9 if K == 8 else None, w=C + 10 if K == 8 else None)
    if C:
        Xp = _alt((nt, ru(C)), 3e4)
        Xp[:, :C] = d["feat"]
        feat = m.A.put(Xp, m.adt)
    else:
        feat = m.A.zeros(nt, 32, dtype=m.adt)
    lead, lead_t = [], None
    if c["lead"]:
        Nl = c["lead"]
        lead_t = (m.A.zeros(nt, ru(Nl), dtype=m.adt), m.A.zeros(B, ru(Nl)), m.A.zeros(B, ru(Nl)))
        lead = [dict(w=d["lead_w"], bias=d["lead_bias"], mode=E.EPI_STATS, flags=E.F_PRE_RELU, out=lead_t[0],
                     stats=(lead_t[1], lead_t[2], 0, float(K)))]
    ctx = m._pair_first(npxl, K, feat, C, segs, coords, fin=fin, lead_segs=lead)
    L = m.plan[-1]
    kern = c["kernel"] if c["op"] != "comp" else "pair_first_kernel<%s>" % ("true" if K == 8 else "false")
    assert L.name == kern, (L.name, kern)
    n_ops = 1
    if c["op"] == "pn":  # the float pass reads y: the case's own, in place of what the per-point GEMM before it would write
        Y = [t for t in m.A.keep if t.data_ptr() == L.op.p[0]][0]
        Yp = np.zeros(tuple(Y.shape), np.float32)
        for (oidx, _), o_, sg in zip(lays, ctx.offs, d["segs"]):
            Yp[:, o_ + oidx] = sg["y"]
        Y.copy_(torch.from_numpy(Yp))
        if c["ld_claim"]:
            L.op.i[1] = c["ld_claim"]  # (the emitter itself asserts ld <= 2048: the launcher's own check is reached with a patched op)
    out2 = None
    if c["op"] == "comp":
        c1, N2 = c["segs"][0][0], c["N2"]
        lay1, k_pad = E.gn_layout(c1), ru(E.gn_layout(c1)[1])
        addp = np.zeros((B, k_pad), np.float32)
        addp[:, lay1[0]] = d["add"]
        lay2 = E.gn_layout(N2) if c["epi2"] == E.EPI_NORM else None
        Np2 = ru(lay2[1] if lay2 is not None else N2)
        out2 = torch.full((B * 16 * K, Np2), 7.0, dtype=torch.float16, device=device)
        m.A.keep.append(out2)
        seg2 = dict(w=d["W2"], bias=d["bias2"], mode=c["epi2"], out=out2, flags=E.F_POST_RELU if lay2 is not None else 0)
        if lay2 is not None:
            seg2.update(layout=lay2, gn=(d["gamma2"][:P.gn_params(N2)[1]], d["beta2"][:P.gn_params(N2)[1]]))
        L2 = m._gemm(None, npxl, [seg2], in_cols=lay1[0],
                     gx=E.GxArgs(ctx.ta, ctx.tb, ctx.offs[0], k_pad, ctx.rows, 0, (m.A.put(addp), 0, k_pad, None, 0), ctx.vv),
                     pair_tabs=ctx.tabs)
        assert L2.name == c["kernel"], (L2.name, c["kernel"])
        n_ops = 2
    st = _run(m, n_ops)
    got, used = {}, np.zeros(ctx.ldy, bool)
    ta, tb = ctx.ta.float().cpu().numpy(), ctx.tb.float().cpu().numpy()
    vv = None if ctx.vv is None else ctx.vv.cpu().numpy()
    for i, ((oidx, _), o_) in enumerate(zip(lays, ctx.offs)):
        used[o_ + oidx] = True
        got["ta%d" % i], got["tb%d" % i] = ta[:, o_ + oidx], tb[:, o_ + oidx]
        if vv is not None:
            got["vv%d" % i] = vv[:, :, o_ + oidx]
        if i in stats_t:
            got["sum%d" % i], got["sq%d" % i] = (t.cpu().numpy()[:, oidx] for t in stats_t[i])
    if lead_t is not None:
        got["lead"], got["lead_sum"], got["lead_sq"] = (t.float().cpu().numpy()[:, :c["lead"]] for t in lead_t)
    if fin_t is not None:
        got["fin_scale"], got["fin_shift"] = fin_t["scale"].cpu().numpy(), fin_t["shift"].cpu().numpy()
    pad = [ta[:, ~used], tb[:, ~used]] + ([] if vv is None else [vv[:, :, ~used]])
    if out2 is not None:
        o2 = out2.float().cpu().numpy()
        oi2 = lay2[0] if lay2 is not None else np.arange(c["N2"])
        pad.append(np.delete(o2, oi2, axis=1))
        out2 = o2[:, oi2]
    return st, got, pad, out2


def _check_table(c, d, got, pad):
    ref = P.table_forward(c, d)
    worst = 0.0
    for k in [k_ for k_ in ref if k_ != "_ctx"]:
        g_ = got[k].astype(np.float64)
        assert np.isfinite(g_).all(), (c["name"], k)
        ratio = np.abs(g_ - ref[k][0]) / ref[k][2]
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        print("%s [%s, %s] %s: worst err/tol %.3g (err %.3g, |ref| %.3g at %s)" %
              (c["name"], c["prec"], c["kernel"], k, ratio[i], abs(g_[i] - ref[k][0][i]), abs(ref[k][0][i]), i))
        worst = max(worst, float(ratio.max()))
    for i, t in enumerate(ref["_ctx"]):
        if t["noab"] is not None and ("sq%d" % i) in got:
            r0 = float((np.abs(got["sq%d" % i] - t["ss"]) / (t["noab"] + P.U * t["ss"])).max())
            print("%s sq%d: against the bound WITHOUT the |A| |B| terms: %.3g" % (c["name"], i, r0))
    for p_ in pad:
        assert (p_ == 0).all(), "padded columns must be exactly zero"
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in P.PF + P.PN + P.COMP])
def test_pair_table_op_matches_float64(gpu_device, name):
    """the table passes (and, composition cases, the generated-X GEMM that consumes their tables, against the K-EXPANDED float64
    evaluation) -- every output: tables, vv, statistics, the leading segment's rows, the finalised joint GroupNorm's scale / shift"""
    c = CASE_BY_NAME[name]
    d = P.make_table_data(c)
    st, got, pad, out2 = _launch_table(c, d, gpu_device)
    if c["status"] != 0:
        assert st == c["status"] * 1000, (name, st)
        print("%s: status %d as expected" % (name, st))
        return
    assert st == 0, (name, st)
    worst = _check_table(c, d, got, pad)
    assert worst <= 1, (name, worst)
    if c["op"] == "comp":
        ref = P.comp_forward(c, d)
        assert np.isfinite(out2).all()
        ratio = np.abs(out2 - ref["y"]) / ref["b"]
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        print("%s [fp16, %s]: worst err/tol %.3g (err %.3g, |ref| %.3g at %s)" %
              (name, c["kernel"], ratio[i], abs(out2[i] - ref["y"][i]), abs(ref["y"][i]), i))
        assert ratio.max() <= 1, (name, float(ratio.max()), i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in P.GX + P.GXS + P.SA])
def test_pair_op_matches_float64(gpu_device, monkeypatch, name):
    from slide_amd._lib import SlideHipError
    c = CASE_BY_NAME[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    d = make_data(c)
    if c["raises"]:
        with pytest.raises(SlideHipError):
            _launch_gx(c, d, gpu_device)
        print("%s: the plan refuses the weight as expected" % name)
        return
    st, got, pad, stats = (_launch_sa if c["op"] == "sa" else _launch_gx)(c, d, gpu_device)
    if c["status"] != 0:
        assert st == c["status"] * 1000, (name, st)
        print("%s: status %d as expected" % (name, st))
        return
    assert st == 0, (name, st)
    ref = forward(c, d)
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


# ------------------------------------------------------------------------------------------------------------ host-pointer pairs
def _run_pair(kind, rows_or_b, op_a, op_b):
    """one launch of a host-pointer pair op (SLIDE_OP_GEMM_GX_DUAL / SLIDE_OP_SA_CHAIN_P): p[0] -> two SlideOps in host memory"""
    import torch
    from slide_amd import abi
    from slide_amd._lib import lib
    pair = (abi.SlideOp * 2)(abi.SlideOp.from_buffer_copy(bytes(op_a)), abi.SlideOp.from_buffer_copy(bytes(op_b)))
    ops = (abi.SlideOp * 1)(abi.make_op(kind, i=(rows_or_b,), p=(ctypes.addressof(pair),)))
    st = lib().slide_run_ops(ops, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


def _hold(name, kernel, got, ref, pad, stats=None):
    assert np.isfinite(got).all()
    ratio = np.abs(got - ref["y"]) / ref["b"]
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s [%s]: worst err/tol %.3g (|ref| %.3g at %s)" % (name, kernel, ratio[i], abs(ref["y"][i]), i))
    assert ratio.max() <= 1, (name, float(ratio.max()), i)
    assert (pad == 0).all(), "padded output columns must be zero"
    if stats is not None:
        for k in range(2):
            rs = float((np.abs(stats[k] - ref["stats"][k]) / ref["stats_b"][k]).max())
            print("%s: statistics %s worst err/tol %.3g" % (name, ("sum", "sq")[k], rs))
            assert rs <= 1, (name, k, rs)


def test_dual_rows_fit_and_do_not_fit():
    """the LDS of the dual form (pair_cases.dual_lds): the first row runs as ONE launch, the second takes the launcher's fallback"""
    from slide_amd import abi
    epi_dw = ctypes.sizeof(abi.SlideEpi) // 4
    for row in P.DUAL:
        c1, c0 = CASE_BY_NAME[row["m1"]], CASE_BY_NAME[row["m0"]]
        assert c1["gxmode"] == 1 and c0["gxmode"] == 0 and c1["B"] == c0["B"] and c1["npxl"] == c0["npxl"] and c1["prec"] == c0["prec"] == "fp16"
        need = max(P.dual_lds(c, epi_dw)[0] for c in (c1, c0))
        assert (need <= P.dual_lds(c1, epi_dw)[1]) == row["fits"], (row["name"], need)
        assert row["name"] in P.__doc__
    assert [r["fits"] for r in P.DUAL] == [True, False]
    for row in P.CHAIN_P:
        assert CASE_BY_NAME[row["sa"]]["B"] == row["q"]["B"] and row["q"]["npxl"] == 4 and row["q"]["aff"] and row["name"] in P.__doc__


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r["name"] for r in P.DUAL])
def test_gx_dual_matches_its_single_launch_references(gpu_device, monkeypatch, name):
    from slide_amd import abi
    row = [r for r in P.DUAL if r["name"] == name][0]
    es = []
    for cn in (row["m1"], row["m0"]):
        c = CASE_BY_NAME[cn]
        with monkeypatch.context() as mp:
            for k, v in c["env"].items():
                mp.setenv(k, v)
            d = make_data(c)
            es.append((c, d, _emit_gx(c, d, gpu_device)))
    st = _run_pair(abi.OP_GEMM_GX_DUAL, es[0][2]["rows"], es[0][2]["m"].ops[-1], es[1][2]["m"].ops[-1])
    assert st == 0, (name, st)
    for c, d, e in es:
        got, pad, stats = _read_gx(e)
        _hold("%s / %s" % (name, c["name"]), "gemm_gx_dual_kernel<7>" if row["fits"] else c["kernel"], got, forward(c, d), pad, stats)


def _emit_query(c, d, device):
    """a 16-row fp16 GEMM of gemm_cases with an input affine, as the SA blocks' per-point query GEMM is emitted"""
    import torch
    import gemm_cases as G
    from slide_amd import engine as E
    B, K, N = c["B"], c["K"], c["N"]
    assert c["prec"] == "fp16" and c["npxl"] == 4 and c["aff"] and not c["gn_fin"] and c["mode"] == G.EPI_NORM
    assert c["addvec"] is None and not c["resid"] and c["pre_add"] is None and c["pair"] is None
    m = _mini(B, "fp16", device)
    m.use_cm = False  # (a per-point GEMM reads row-major weights)
    rows, ld = B * 16, ru(K)
    Xp = _alt((rows, ld), 3e4)
    Xp[:, :K] = d["X"]
    lay = E.gn_layout(N)
    oidx, Np = lay[0], ru(lay[1])
    out = torch.full((rows, Np), 7.0, dtype=torch.float16, device=device)
    m.A.keep.append(out)
    n_norm = G.gn_params(N)[1]
    seg = dict(w=d["W"], bias=d["bias"], mode=c["mode"], out=out, layout=lay, gn=(d["gamma"][:n_norm], d["beta"][:n_norm]),
               flags=(E.F_PRE_RELU if c["pre_relu"] else 0) | (E.F_POST_RELU if c["post_relu"] else 0))
    sc, sh = np.ones((B, ld), np.float32), np.zeros((B, ld), np.float32)
    sc[:, :K], sh[:, :K] = d["scale"], d["shift"]
    m._gemm(m.A.put(Xp, m.adt), 4, [seg], in_affine=(m.A.put(sc), m.A.put(sh), 0, ld))
    return m, out, oidx


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r["name"] for r in P.CHAIN_P])
def test_sa_chain_p_matches_its_single_launch_references(gpu_device, name):
    import gemm_cases as G
    from slide_amd import abi
    row = [r for r in P.CHAIN_P if r["name"] == name][0]
    c, q = CASE_BY_NAME[row["sa"]], row["q"]
    d, dq = make_data(c), G.make_data(q)
    m, out = _emit_sa(c, d, gpu_device)
    mq, outq, oidx = _emit_query(q, dq, gpu_device)
    st = _run_pair(abi.OP_SA_CHAIN_P, c["B"], m.ops[-1], mq.ops[-1])
    assert st == 0, (name, st)
    _hold(name + " / " + c["name"], row["kernel"], _read_out(m, out, c["B"] * 256, c["chain"]["N"]), forward(c, d), np.zeros((1, 0)))
    gq = outq.float().cpu().numpy()
    _hold(name + " / " + q["name"], row["kernel"], gq[:, oidx], G.forward(q, dq), np.delete(gq, oidx, axis=1))
