"""GPU: every row of tests/point_ops_cases.py through slide_amd._ext against its reference -- exact equality for indices, counts,
distances, gathers and three_interpolate (the oracle), the derived scatter-add bound for the three atomic backward ops (float64).
One launch per op and row; tests/test_point_ops_host.py shows that the rows reach every kernel variant of csrc/point_ops.hip."""
import numpy as np
import pytest
import torch

import point_ops_cases as PC

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.cpu().numpy()


def _where(r):
    return "%s [%s: %s]" % (r.id, r.get("variant", r.op), r.get("target", ""))


def _assert_within(got, ref, bound, r, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("WORST %s %s err / bound %.3f" % (what, r.id, worst))
    assert (err <= bound).all(), "%s %s: err / bound %.3f, %d elements outside" % (what, _where(r), worst, int((err > bound).sum()))


# ------------------------------------------------------------------------------------------------ gather / group (+ backward)
@pytest.mark.parametrize("r", PC.GATHER_ROWS + PC.GROUP_ROWS, ids=PC.ids(PC.GATHER_ROWS + PC.GROUP_ROWS))
def test_gather_group(gpu_device, r):
    from slide_amd import _ext
    pts, idx, g = PC.gather_inputs(r)
    fwd, bwd = (_ext.gather_points, _ext.gather_points_grad) if r.op == "gather" else (_ext.group_points, _ext.group_points_grad)
    ti = T(idx, gpu_device)
    assert np.array_equal(N(fwd(T(pts, gpu_device), ti)), PC.gather_ref(pts, idx)), _where(r)
    ref, bound = PC.gather_grad_ref(g, idx, r.n)
    _assert_within(N(bwd(T(g, gpu_device), ti, r.n)), ref, bound, r, r.op + "_grad")


@pytest.mark.parametrize("r", PC.GATHER_ROWS_ROWS, ids=PC.ids(PC.GATHER_ROWS_ROWS))
def test_gather_rows(gpu_device, r):
    from slide_amd import _ext
    pts, idx = PC.gather_rows_inputs(r)
    got = N(_ext.gather_rows(T(pts, gpu_device), T(idx, gpu_device)))
    assert np.array_equal(got, np.take_along_axis(pts, idx[:, :, None].astype(np.int64), axis=1)), _where(r)


# ------------------------------------------------------------------------------------------------ three_interpolate (+ backward)
@pytest.mark.parametrize("r", PC.INTERP_ROWS, ids=PC.ids(PC.INTERP_ROWS))
def test_three_interpolate(gpu_device, r):
    from slide_amd import _ext
    pts, idx, w, g = PC.interp_inputs(r)
    ti, tw = T(idx, gpu_device), T(w, gpu_device)
    got = N(_ext.three_interpolate(T(pts, gpu_device), ti, tw))
    assert np.array_equal(got, PC.reference(r)[0]), _where(r)
    ref, bound = PC.interp_ref(pts, idx, w)
    _assert_within(got, ref, bound, r, "three_interpolate")
    ref, bound = PC.interp_grad_ref(g, idx, w, r.m)
    _assert_within(N(_ext.three_interpolate_grad(T(g, gpu_device), ti, tw, r.m)), ref, bound, r, "three_interpolate_grad")


# ------------------------------------------------------------------------------------------------ misaligned operands
@pytest.mark.parametrize("r", PC.MISALIGNED_ROWS, ids=PC.ids(PC.MISALIGNED_ROWS))
def test_misaligned_operand_falls_back(gpu_device, r):
    """one operand 4 bytes off a 16-byte boundary: the wrapper must take the fallback kernel the mirror names, and the result must
    equal the aligned run (and the reference) bit for bit"""
    from slide_amd import _ext
    if r.op == "three_interpolate":
        pts, idx, w, _ = PC.interp_inputs(r)
        args = dict(points=T(pts, gpu_device), idx=T(idx, gpu_device), weight=T(w, gpu_device))
        run = lambda a: _ext.three_interpolate(a["points"], a["idx"], a["weight"])
        want = PC.reference(r)[0]
    elif r.op == "gather_rows":
        pts, idx = PC.gather_rows_inputs(r)
        args = dict(points=T(pts, gpu_device), idx=T(idx, gpu_device))
        run = lambda a: _ext.gather_rows(a["points"], a["idx"])
        want = np.take_along_axis(pts, idx[:, :, None].astype(np.int64), axis=1)
    else:
        pts, idx, _ = PC.gather_inputs(r)
        args = dict(points=T(pts, gpu_device), idx=T(idx, gpu_device))
        fwd = _ext.gather_points if r.op == "gather" else _ext.group_points
        run = lambda a: fwd(a["points"], a["idx"])
        want = PC.gather_ref(pts, idx)
    assert all(t.data_ptr() % 16 == 0 for t in args.values())
    aligned = run(args)
    off = dict(args)
    off[r.misaligned] = PC.misaligned(args[r.misaligned])
    assert off[r.misaligned].data_ptr() % 16 == 4 and off[r.misaligned].is_contiguous()
    got = run(off)
    assert torch.equal(got, aligned) and np.array_equal(N(got), want), "%s -> %s" % (_where(r), r.variant)


# ------------------------------------------------------------------------------------------------ ball query
@pytest.mark.parametrize("r", PC.BALL_ROWS, ids=PC.ids(PC.BALL_ROWS))
def test_ball_query(gpu_device, r):
    from slide_amd import _ext
    q, xyz = PC.ball_inputs(r)
    idx, cnt = _ext.ball_query(T(q, gpu_device), T(xyz, gpu_device), r.r, r.ns)
    ri, rc = PC.reference(r)
    assert np.array_equal(N(cnt), rc), _where(r)
    assert np.array_equal(N(idx), ri), _where(r)


# ------------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize("r", PC.KNN_ROWS, ids=PC.ids(PC.KNN_ROWS))
def test_knn(gpu_device, r):
    from slide_amd import _ext
    p1, p2, l2 = PC.knn_inputs(r)
    d, i = _ext.knn_points(T(p1, gpu_device), T(p2, gpu_device), r.K, None if l2 is None else torch.from_numpy(l2))
    rd, ri = PC.reference(r)
    assert i.dtype == torch.int64 and np.array_equal(N(i), ri), _where(r)
    assert np.array_equal(N(d), rd), _where(r)


@pytest.mark.parametrize("u", PC.KNN_GATHER_U)
def test_knn_gather(gpu_device, u):
    from slide_amd import _ext
    r = PC.KNN_GATHER_ROW
    ri = PC.reference(r)[1].copy()   # (the shared reference is read-only; torch wants a writable array)
    x = PC.rng("knn_gather%d" % u).standard_normal((r.B, r.n2, u)).astype(np.float32)
    got = N(_ext.knn_gather(T(x, gpu_device), T(ri, gpu_device)))
    assert got.shape == (r.B, r.n1, r.K, u) and np.array_equal(got, x[np.arange(r.B)[:, None, None], ri]), (_where(r), u)


def test_knn_more_than_64_neighbours_is_an_error(gpu_device):
    from slide_amd import _ext
    p = T(PC.lattice(PC.rng("k65"), 1, 70), gpu_device)
    with pytest.raises(RuntimeError):
        _ext.knn_points(p[:, :5].contiguous(), p, 65)


# ------------------------------------------------------------------------------------------------ three_nn
@pytest.mark.parametrize("r", PC.THREE_NN_ROWS, ids=PC.ids(PC.THREE_NN_ROWS))
def test_three_nn(gpu_device, r):
    from slide_amd import _ext
    u, k = PC.three_nn_inputs(r)
    d, i = _ext.three_nn(T(u, gpu_device), T(k, gpu_device))
    rd, ri = PC.reference(r)
    assert np.array_equal(N(i), ri) and np.array_equal(N(d), rd), _where(r)


# ------------------------------------------------------------------------------------------------ FPS
@pytest.mark.parametrize("r", PC.FPS_ROWS, ids=PC.ids(PC.FPS_ROWS))
def test_furthest_point_sampling(gpu_device, r):
    from slide_amd import _ext
    p, _ = PC.fps_inputs(r)
    got = N(_ext.furthest_point_sampling(T(p, gpu_device), r.m))
    assert np.array_equal(got, PC.reference(r)[0]), _where(r)


@pytest.mark.parametrize("r", PC.SFP_ROWS, ids=PC.ids(PC.SFP_ROWS))
def test_sample_farthest_points(gpu_device, r):
    from slide_amd import _ext
    p, start = PC.fps_inputs(r)
    sel, idx = _ext.sample_farthest_points(T(p, gpu_device), K=r.m, start_idx=T(start, gpu_device))
    ref = PC.reference(r)[0]
    assert idx.dtype == torch.int64 and np.array_equal(N(idx), ref), _where(r)
    assert np.array_equal(N(sel), np.take_along_axis(p, ref[:, :, None], axis=1)), _where(r)
