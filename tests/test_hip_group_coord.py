"""GPU: the grouping layer's coordinate gradient -- csrc/group_coord_bwd.hip at the C-ABI (slide_group_rows_coord_bwd), through
train.functions.GroupRows, and through the public operators train.grouping.query_and_group_rows / group_knn_rows.

Every gradient is held, element by element, to torch's float64 autograd over a restatement of the reference's two operators on the
same fp32 inputs and the same neighbour indices, within |err| <= gamma(n + c) S (tests/group_coord_cases.py: n the element's term
count, c the kernel's rounding steps per term, S the sum of the magnitudes of the element's terms; derived from the kernel's
operations, not from its results).  dnew_xyz is additionally required to be bit-reproducible.  Every comparison prints its worst
err / tol.

Measured on an MI355X (worst err / tol): kernel cases 0.926 (dxyz, SA form with abs + centre, in-degree 1), FP form 0.056; public
operators 0.895 (gradients), 1.000 of one rounding for the forward's rel column; the chain 0.014; one leaf as both inputs 0.084."""
import ctypes

import numpy as np
import pytest
import torch

import group_coord_cases as G

pytestmark = pytest.mark.gpu


def _t(a, d):
    return None if a is None else torch.from_numpy(np.array(a)).to(d)  # (a copy: the cases' arrays are read-only)


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bounds(d, Sx, Sc, indeg, extra=0):
    K = d["K"]
    return G.tolerance(Sx, indeg, d["flags"], K, extra), G.tolerance(Sc, np.full(Sc.shape[:2], K), d["flags"], K, extra)


@pytest.fixture(scope="module")
def reference():
    """case name -> (float64 dxyz, dnew_xyz, their bounds), computed once and shared"""
    cache = {}

    def get(name):
        if name not in cache:
            d = G.make_data(name)
            ox, oc = G.oracle_grads(d)
            _, _, Sx, Sc, indeg = G.closed_form(d)
            for a in (ox, oc):
                a.setflags(write=False)
            cache[name] = (ox, oc) + _bounds(d, Sx, Sc, indeg)
        return cache[name]
    return get


def _device_inputs(d, dev, perm=None):
    sel = (lambda a: a) if perm is None else (lambda a: a[perm])
    rows = d["np"] * d["K"]
    return dict(xyz=_t(sel(d["xyz"]), dev), new_xyz=_t(sel(d["new_xyz"]), dev), idx=_t(sel(d["idx"]), dev), d2=_t(None if d["d2"] is None else sel(d["d2"]), dev),
                counts=_t(None if d["counts"] is None else sel(d["counts"]), dev),
                dout=_t(sel(d["dout"].reshape(G.B, rows, -1)).reshape(G.B * rows, -1), dev))


def _abi(d, t, want_dxyz=True, want_dnew=True):
    """one call at the C-ABI with explicit buffers: dxyz zeroed (the contract), dnew_xyz prefilled with NaN (it is written in full)"""
    from slide_amd._lib import lib
    dev = t["xyz"].device
    dxyz = torch.zeros(G.B, d["N"], 3, device=dev) if want_dxyz else None
    dnew = torch.full((G.B, d["np"], 3), float("nan"), device=dev) if want_dnew else None
    s = lib().slide_group_rows_coord_bwd(G.B, d["N"], d["np"], d["K"], d["C"], d["ldg"], d["flags"], _P(t["xyz"]), _P(t["new_xyz"]), _P(t["idx"]),
                                         _P(t["d2"]), _P(t["counts"]), _P(t["dout"]), _P(dxyz), _P(dnew),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert s == 0, s
    torch.cuda.synchronize()
    return dxyz, dnew


@pytest.mark.parametrize("name", [c["name"] for c in G.CASES])
def test_kernel_matches_the_float64_oracle(gpu_device, reference, name):
    d = G.make_data(name)
    ox, oc, tx, tc = reference(name)
    dxyz, dnew = _abi(d, _device_inputs(d, gpu_device))
    gx, gc = dxyz.cpu().numpy(), dnew.cpu().numpy()
    assert np.isfinite(gx).all() and np.isfinite(gc).all()
    wx, wc = G.worst(gx, ox, tx), G.worst(gc, oc, tc)
    print("%-22s worst err / tol: dxyz %.3f dnew_xyz %.3f" % (name, wx, wc))
    assert wx <= 1 and wc <= 1, (name, wx, wc)


@pytest.mark.parametrize("name", ["fp-base8-C29", "sa_abs_ctr-base16-C5", "sa_abs_ctr-ball-C5", "fp-fan300-C5"])
def test_dnew_is_bit_reproducible_and_independent_of_the_batch_position(gpu_device, reference, name):
    d = G.make_data(name)
    ox, oc, tx, tc = reference(name)
    t = _device_inputs(d, gpu_device)
    x1, c1 = _abi(d, t)
    x2, c2 = _abi(d, t)
    assert torch.equal(c1, c2)
    assert G.worst(x2.cpu().numpy(), ox, tx) <= 1
    perm = [1, 0]
    xs, cs = _abi(d, _device_inputs(d, gpu_device, perm))
    assert torch.equal(cs, c1[perm])
    assert G.worst(xs.cpu().numpy(), ox[perm], tx[perm]) <= 1


@pytest.mark.parametrize("name", ["fp-base8-C5", "sa_abs_ctr-ball-C5"])
def test_a_null_output_leaves_the_other_unchanged(gpu_device, reference, name):
    d = G.make_data(name)
    ox, oc, tx, tc = reference(name)
    t = _device_inputs(d, gpu_device)
    _, both = _abi(d, t)
    only_x, none = _abi(d, t, want_dnew=False)
    assert none is None and G.worst(only_x.cpu().numpy(), ox, tx) <= 1
    none, only_c = _abi(d, t, want_dxyz=False)
    assert none is None and torch.equal(only_c, both)


def _same_leaf_case(form):
    d = G.make_data("fp-coincident-C5")
    if form == "fp":
        return d
    flags = G.FORMS[form]
    assert G.ru(d["C"] + G.ncoord(flags)) == d["ldg"]
    return dict(d, flags=flags, d2=None)


@pytest.mark.parametrize("form", ["fp", "sa_abs_ctr"])
def test_one_leaf_as_sources_and_centres(gpu_device, form):
    """xyz is new_xyz: autograd adds the two results -- one more rounding, relative to the sum of both magnitudes"""
    from slide_amd.train import functions as F
    d = _same_leaf_case(form)
    ox, oc = G.oracle_grads(d, same=True)
    assert np.array_equal(ox, oc)
    _, _, Sx, Sc, indeg = G.closed_form(d)
    tx, tc = _bounds(d, Sx, Sc, indeg)
    tol = tx + tc + G.U / (1 - G.U) * (Sx + Sc)
    t = _device_inputs(d, gpu_device)
    pts = t["xyz"].clone().requires_grad_(True)
    rows = F.group_rows(_t(d["feat"], gpu_device), pts, pts, t["idx"], t["d2"], d["flags"], d["C"])
    (g,) = torch.autograd.grad(rows, pts, t["dout"])
    w = G.worst(g.cpu().numpy(), ox, tol)
    print("one leaf, %s: worst err / tol %.3f" % (form, w))
    assert g.shape == pts.shape and w <= 1, w


@pytest.mark.parametrize("name", ["fp-base8-C29", "sa_abs_ctr-base16-C5"])
def test_features_only_call_is_bit_equal_to_the_layer_before(gpu_device, name):
    """coordinates that do not require grad: rows and dfeat equal, bit for bit, the forward op and the slide_group_rows_bwd call that
    were all of GroupRows before the coordinate gradient (dout holds small integers: its sums are exact in every order, so the
    atomics cannot blur the comparison)"""
    from slide_amd._lib import check, lib
    from slide_amd.rows import OP_ROWS_GROUP, _rop, _run
    from slide_amd.train import functions as F
    d = G.make_data(name)
    t = _device_inputs(d, gpu_device)
    dout = _t(np.random.RandomState(5).randint(-8, 9, d["dout"].shape).astype(np.float32), gpu_device)
    feat = _t(d["feat"], gpu_device).requires_grad_(True)
    rows = F.group_rows(feat, t["xyz"], t["new_xyz"], t["idx"], t["d2"], d["flags"], d["C"])
    assert rows.grad_fn is not None and len(rows.grad_fn.saved_tensors) == 3  # idx and two absent tensors: no coordinates kept
    (dfeat,) = torch.autograd.grad(rows, feat, dout)
    N, P, K, C = d["N"], d["np"], d["K"], d["C"]
    old = torch.empty(G.B * P * K, d["ldg"], device=gpu_device)
    _run(_rop(OP_ROWS_GROUP, False, (G.B, N, P, K, C, feat.shape[1], d["ldg"], d["flags"]),
              (t["xyz"], t["new_xyz"], feat.detach(), t["idx"], t["d2"], old, None)))
    old_dfeat = torch.zeros(G.B * N, feat.shape[1], device=gpu_device)
    check(lib().slide_group_rows_bwd(G.B, N, P, K, C, feat.shape[1], d["ldg"], _P(t["idx"]), None, _P(dout), _P(old_dfeat),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "slide_group_rows_bwd")
    torch.cuda.synchronize()
    assert torch.equal(rows, old) and torch.equal(dfeat, old_dfeat)
    assert old_dfeat.abs().max().item() > 0


def _operator_case(gpu_device, kind, rs):
    """-> (d: a case dictionary on the library's own neighbours, rows, leaves xyz / new_xyz / feat)"""
    from slide_amd.train import group_knn_rows, query_and_group_rows
    C = 5
    N, P, ns = {"nn": (40, 24, 8), "nn_clamp": (5, 7, 8), "radius_open": (24, 12, 6), "radius_subset": (24, 12, 6), "knn": (40, 24, 8)}[kind]
    xyz = rs.uniform(-1, 1, (G.B, N, 3)).astype(np.float32)
    new_xyz = rs.uniform(-1, 1, (G.B, P, 3)).astype(np.float32)
    if kind.startswith("radius"):
        new_xyz[:, 0] = 9.0
        new_xyz[:, 1] = xyz[:, 3] + 0.01
    feat = np.zeros((G.B * N, 32), np.float32)
    feat[:, :C] = rs.standard_normal((G.B * N, C))
    tx, tc, tf = (_t(a, gpu_device).requires_grad_(True) for a in (xyz, new_xyz, feat))
    d2 = counts = None
    if kind == "knn":
        from slide_amd import _ext
        rows = group_knn_rows(tc, tx, tf, C, ns)
        d2t, idx = _ext.knn_points(tc.detach(), tx.detach(), ns)   # the search the operator ran
        flags, d2 = G.FP, d2t.cpu().numpy()
    else:
        flags = G.ABS | G.CENTER
        rows, idx, cnt = query_and_group_rows(tx, tc, tf, C, ns, neighbor_def="radius" if kind.startswith("radius") else "nn", radius=0.6,
                                              include_abs_coordinate=True, include_center_coordinate=True, subset=kind != "radius_open")
        assert cnt.dtype == torch.int32 and cnt.shape == (G.B, P)
        if kind.startswith("radius"):
            assert idx.dtype == torch.int32 and (cnt == 0).any() and ((cnt > 0) & (cnt < ns)).any()
            flags |= G.IDX32
            counts = cnt.cpu().numpy() if kind == "radius_open" else None
        else:
            assert idx.dtype == torch.int64 and (cnt == min(ns, N)).all()
    idx = idx.cpu().numpy()
    K = idx.shape[2]
    assert K == min(ns, N) and rows.shape == (G.B * P * K, G.ru(C + G.ncoord(flags)))
    dout = rs.standard_normal(tuple(rows.shape)).astype(np.float32)
    d = dict(flags=flags, C=C, N=N, np=P, K=K, ldg=rows.shape[1], xyz=xyz, new_xyz=new_xyz, idx=idx, d2=d2, counts=counts, dout=dout, feat=feat)
    return d, rows, (tx, tc, tf)


@pytest.mark.parametrize("kind", ["nn", "nn_clamp", "radius_open", "radius_subset", "knn"])
def test_public_operators_against_the_oracle(gpu_device, kind):
    """rows and gradients of query_and_group_rows / group_knn_rows on the indices of the library's own search"""
    rs = np.random.RandomState(len(kind) * 97 + 3)
    d, rows, (tx, tc, tf) = _operator_case(gpu_device, kind, rs)
    C, K, flags = d["C"], d["K"], d["flags"]
    want = G.oracle_rows(torch.from_numpy(d["xyz"].astype(np.float64)), torch.from_numpy(d["new_xyz"].astype(np.float64)),
                         torch.from_numpy(d["idx"].astype(np.int64)), flags, None if d["d2"] is None else torch.from_numpy(d["d2"].astype(np.float64)),
                         None if d["counts"] is None else torch.from_numpy(d["counts"].astype(np.int64)),
                         torch.from_numpy(d["feat"][:, :C].astype(np.float64)).reshape(G.B, d["N"], C)).numpy()
    got = rows.detach().cpu().numpy().reshape(G.B, d["np"], K, -1)
    nc = C + G.ncoord(flags)
    assert (got[..., nc:] == 0).all()  # pad columns
    wf = G.worst(got[..., :nc], want, G.forward_tolerance(want, flags, C, K))
    gx, gc, gf = torch.autograd.grad(rows, (tx, tc, tf), _t(d["dout"], gpu_device))
    ox, oc = G.oracle_grads(d)
    _, _, Sx, Sc, indeg = G.closed_form(d)
    bx, bc = _bounds(d, Sx, Sc, indeg)
    wx, wc = G.worst(gx.cpu().numpy(), ox, bx), G.worst(gc.cpu().numpy(), oc, bc)
    # the features' gradient: a source point's row is the sum of the dout rows that gathered it (n - 1 additions)
    g4 = d["dout"].reshape(G.B, d["np"], K, -1)[..., :C].astype(np.float64)
    of, Sf, nf = np.zeros((G.B, d["N"], C)), np.zeros((G.B, d["N"], C)), np.zeros((G.B, d["N"]))
    for b in range(G.B):
        live = np.ones(d["np"], bool) if d["counts"] is None else d["counts"][b] > 0
        np.add.at(of[b], d["idx"][b][live].reshape(-1), g4[b][live].reshape(-1, C))
        np.add.at(Sf[b], d["idx"][b][live].reshape(-1), np.abs(g4[b][live]).reshape(-1, C))
        np.add.at(nf[b], d["idx"][b][live].reshape(-1), 1)
    m = nf[..., None] * G.U
    wfe = G.worst(gf.cpu().numpy().reshape(G.B, d["N"], -1)[..., :C], of, m / (1 - m) * Sf)
    print("%-14s worst err / tol: rows %.3f dxyz %.3f dnew_xyz %.3f dfeat %.3f" % (kind, wf, wx, wc, wfe))
    assert max(wf, wx, wc, wfe) <= 1


def test_chain_through_a_displacement_and_a_linear_map(gpu_device):
    """points = parent + 0.01 disp -> group_knn_rows -> fixed linear map (torch) -> sum: the gradient of disp against the oracle.  dout is
    the map's row sums, O terms each added in fp32 (O more roundings per term, magnitudes: the ABSOLUTE row sums); the scale 0.01 rounds
    once more.  The oracle differentiates at the fp32 points the forward produced."""
    from slide_amd import _ext
    from slide_amd.train import group_knn_rows
    rs = np.random.RandomState(21)
    N1, N2, K, C, O = 48, 20, 8, 5, 6
    parent = _t(rs.standard_normal((G.B, N1, 3)).astype(np.float32), gpu_device)
    disp = _t(rs.standard_normal((G.B, N1, 3)).astype(np.float32), gpu_device).requires_grad_(True)
    y = _t(rs.standard_normal((G.B, N2, 3)).astype(np.float32), gpu_device).requires_grad_(True)
    feat = np.zeros((G.B * N2, 32), np.float32)
    feat[:, :C] = rs.standard_normal((G.B * N2, C))
    W = rs.standard_normal((32, O)).astype(np.float32)
    scale = np.float32(0.01)
    points = parent + float(scale) * disp
    rows = group_knn_rows(points, y, _t(feat, gpu_device), C, K)
    loss = (rows @ _t(W, gpu_device)).sum()
    g_disp, g_y = torch.autograd.grad(loss, (disp, y))
    d2, idx = _ext.knn_points(points.detach(), y.detach(), K)
    rowsum = W.astype(np.float64).sum(1)
    dout = np.broadcast_to(rowsum, (G.B * N1 * K, 32))
    d = dict(flags=G.FP, C=C, N=N2, np=N1, K=K, ldg=32, xyz=y.detach().cpu().numpy(), new_xyz=points.detach().cpu().numpy(),
             idx=idx.cpu().numpy(), d2=d2.cpu().numpy(), counts=None, dout=dout)
    oy, op = G.oracle_grads(d)
    gmag = np.broadcast_to(np.abs(W.astype(np.float64)).sum(1)[C:C + 11], (G.B, N1, K, 11))
    _, _, Sy, Sp, indeg = G.closed_form(d, gmag=gmag)
    by, bp = _bounds(d, Sy, Sp, indeg, extra=O + 1)
    wy = G.worst(g_y.cpu().numpy(), oy, by)
    wd = G.worst(g_disp.cpu().numpy(), float(scale) * op, float(scale) * bp)
    print("chain: worst err / tol: d disp %.3f d y %.3f" % (wd, wy))
    assert wd <= 1 and wy <= 1 and np.abs(op).max() > 0


def test_backward_captures_into_a_graph(gpu_device, reference):
    """forward + backward captured once on one stream, replayed twice: dnew_xyz bit-equal to the eager result, dxyz within the bound"""
    from slide_amd.train import functions as F
    name = "fp-base8-C29"
    d = G.make_data(name)
    ox, oc, tx, tc = reference(name)
    t = _device_inputs(d, gpu_device)
    xyz, new = t["xyz"].requires_grad_(True), t["new_xyz"].requires_grad_(True)
    feat = _t(d["feat"], gpu_device)

    def step():
        rows = F.group_rows(feat, xyz, new, t["idx"], t["d2"], d["flags"], d["C"])
        return torch.autograd.grad(rows, (xyz, new), t["dout"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ex, ec = step()
        ex, ec = ex.clone(), ec.clone()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gx, gc = step()
    for _ in range(2):
        gx.fill_(7.0)
        gc.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gc, ec)
        assert G.worst(gx.cpu().numpy(), ox, tx) <= 1
    assert G.worst(ex.cpu().numpy(), ox, tx) <= 1 and G.worst(ec.cpu().numpy(), oc, tc) <= 1


def test_scope_errors(gpu_device):
    from slide_amd.train import group_knn_rows, query_and_group_rows
    x = torch.rand(2, 6, 3)
    with pytest.raises(RuntimeError):
        group_knn_rows(x, x, None, 0, 2)  # no CPU fallback
    with pytest.raises(RuntimeError):
        query_and_group_rows(x, x, None, 0, 2)
    xd = x.to(gpu_device)
    with pytest.raises(ValueError):
        group_knn_rows(xd, xd, None, 0, 7)
    with pytest.raises(ValueError):
        query_and_group_rows(xd, xd, None, 0, 2, neighbor_def="other")
