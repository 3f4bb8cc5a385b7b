"""GPU: the Chamfer / F1 metric (slide_amd/csrc/chamfer.hip through metrics_point_cloud.chamfer_and_f1) -- the bidirectional K = 1
kernel bit-equal to slide_knn_points(K=1) and the oracle, distances against a float64 brute force, every case of the reference
module's fixture (tests/golden/golden_chamfer.npz), batch independence of the fused calc_cd, and the scope errors."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

sys.path.insert(0, os.path.join(REPO, "pointnet2"))
pytestmark = pytest.mark.gpu

REDUCTIONS = [(None, None), ("mean", None), ("mean", "mean"), ("mean", "sum"), ("sum", None), ("sum", "mean"), ("sum", "sum")]


def _cloud(rs, B, P, grid=False):
    if grid:  # a 0.25 grid: duplicate points and exactly equidistant neighbours
        return (rs.randint(0, 4, (B, P, 3)) * 0.25).astype(np.float32)
    return rs.standard_normal((B, P, 3)).astype(np.float32)


def _valid(lengths, B, P):
    if lengths is None:
        return np.ones((B, P), bool)
    return np.arange(P)[None] < np.asarray(lengths)[:, None]


@pytest.mark.parametrize("B,P1,P2,grid,het", [
    (1, 1, 1, False, False), (3, 17, 1, False, False), (2, 2047, 2048, False, False), (2, 2048, 2049, True, False),
    (1, 8192, 2048, False, False), (256, 64, 96, False, True), (5, 2049, 17, True, True), (9, 300, 300, True, True)])
def test_chamfer_nn_bit_equal_to_knn_k1_and_oracle(gpu_device, B, P1, P2, grid, het):
    from oracle import ops as O
    from slide_amd import _ext
    rs = np.random.RandomState(B * 7919 + P1 * 31 + P2)
    x, y = _cloud(rs, B, P1, grid), _cloud(rs, B, P2, grid)
    if grid:
        y[:, P2 // 2:P2 // 2 + min(P2 // 4, 64)] = y[:, :min(P2 // 4, 64)]  # exact duplicates at higher indices
    lx = ly = None
    if het:
        lx = rs.randint(1, P1 + 1, B).astype(np.int64)
        ly = rs.randint(1, P2 + 1, B).astype(np.int64)
        lx[0], ly[-1] = P1, 1
    d = gpu_device
    tl = (lambda a: None if a is None else torch.from_numpy(a).to(d))
    xt, yt = torch.from_numpy(x).to(d), torch.from_numpy(y).to(d)
    d1, i1, d2, i2 = [t.cpu().numpy() for t in _ext.chamfer_nn(xt, yt, tl(lx), tl(ly))]
    k1d, k1i = [t.cpu().numpy()[..., 0] for t in _ext.knn_points(xt, yt, 1, tl(ly))]
    k2d, k2i = [t.cpu().numpy()[..., 0] for t in _ext.knn_points(yt, xt, 1, tl(lx))]
    o1d, o1i = [a[..., 0] for a in O.knn_points(x, y, 1, ly)]
    o2d, o2i = [a[..., 0] for a in O.knn_points(y, x, 1, lx)]
    vx, vy = _valid(lx, B, P1), _valid(ly, B, P2)
    for got_d, got_i, refs, v in ((d1, i1, ((k1d, k1i), (o1d, o1i)), vx), (d2, i2, ((k2d, k2i), (o2d, o2i)), vy)):
        for rd, ri in refs:
            assert np.array_equal(got_d[v].view(np.int32), rd[v].view(np.int32))
            assert np.array_equal(got_i[v], ri[v])
        assert not got_d[~v].any() and not got_i[~v].any()  # slots beyond a length: (0, 0)
    # float64 brute force: the fp32 distances agree within fp32 rounding, the selected neighbour is a float64 nearest one
    for b in range(min(B, 3)):
        n1 = P1 if lx is None else lx[b]
        n2 = P2 if ly is None else ly[b]
        D = ((x[b, :n1, None].astype(np.float64) - y[b, None, :n2].astype(np.float64)) ** 2).sum(-1)
        m1 = D.min(1)
        assert np.all(np.abs(d1[b, :n1] - m1) <= 4 * np.finfo(np.float32).eps * np.maximum(m1, 1e-30) + 1e-30)
        assert np.all(np.abs(D[np.arange(n1), i1[b, :n1]] - m1) <= 8 * np.finfo(np.float32).eps * np.maximum(m1, 1e-30) + 1e-30)
        m2 = D.min(0)
        assert np.all(np.abs(d2[b, :n2] - m2) <= 4 * np.finfo(np.float32).eps * np.maximum(m2, 1e-30) + 1e-30)


def test_chamfer_ties_go_to_the_lower_index(gpu_device):
    """a query exactly between two points, and a duplicated point: the lower index wins in both directions"""
    from slide_amd import _ext
    d = gpu_device
    x = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]], device=d)
    y = torch.tensor([[[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]], device=d)
    d1, i1, d2, i2 = _ext.chamfer_nn(x, y)
    assert i1.tolist() == [[0, 2]] and d1.tolist() == [[1.0, 0.0]]
    assert i2.tolist() == [[0, 0, 1, 1]]


def _t(a, d):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(d)


def _close(got, want, tol=1e-6):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.all(np.abs(got - want) <= tol * np.maximum(np.abs(want), 1e-30) + 1e-12)


def test_chamfer_distance_matches_reference_golden(gpu_device):
    import metrics_point_cloud.chamfer_and_f1 as C
    from slide_amd import _ext
    g = load_golden("golden_chamfer.npz")
    d = gpu_device
    for name in ("grid", "rand"):
        x, y, nx, ny, w = (g[name + k] for k in ("_x", "_y", "_nx", "_ny", "_w"))
        lx = g[name + "_lx"] if name + "_lx" in g.files else None
        ly = g[name + "_ly"] if name + "_ly" in g.files else None
        B, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
        # per-point neighbours exactly
        d1, i1, d2, i2 = [t.cpu().numpy() for t in _ext.chamfer_nn(_t(x, d), _t(y, d), _t(lx, d), _t(ly, d))]
        vx, vy = _valid(lx, B, P1), _valid(ly, B, P2)
        assert np.array_equal(d1[vx], g[name + "_knn_d1"][vx]) and np.array_equal(i1[vx], g[name + "_knn_i1"][vx])
        assert np.array_equal(d2[vy], g[name + "_knn_d2"][vy]) and np.array_equal(i2[vy], g[name + "_knn_i2"][vy])
        for nt in ("none", "cos", "mse"):
            for wt in ("none", "w", "zero"):
                for pr, br in REDUCTIONS:
                    key = "%s_cd_%s_%s_%s_%s" % (name, nt, wt, pr, br)
                    r = C.chamfer_distance(_t(x, d), _t(y, d), x_lengths=_t(lx, d), y_lengths=_t(ly, d),
                                           x_normals=None if nt == "none" else _t(nx, d),
                                           y_normals=None if nt == "none" else _t(ny, d),
                                           normal_loss_type="cos" if nt == "none" else nt,
                                           weights=None if wt == "none" else (_t(w, d) if wt == "w" else _t(np.zeros_like(w), d)),
                                           batch_reduction=br, point_reduction=pr)
                    n_ref = sum(1 for k in g.files if k.startswith(key + "_"))
                    assert len(r) == n_ref, key
                    for k, v in enumerate(r):
                        want = g["%s_%d" % (key, k)]
                        got = v.cpu().numpy()
                        if pr is None and k < 2:  # per-point squared distances: exact
                            assert np.array_equal(got, want), key
                        elif pr is None:  # per-point normal terms (torch's GPU ops vs its CPU ops): a few ulp, and an absolute
                            # bound where 1 - |cos| cancels near |cos| = 1
                            assert got.shape == want.shape, key
                            assert np.all(np.abs(got - want) <= 4 * np.finfo(np.float32).eps * np.abs(want) + 1e-6), (key, k)
                        else:
                            assert _close(got, want), (key, k, got, want)


def test_calc_cd_and_fscore_match_reference_golden(gpu_device):
    import metrics_point_cloud.chamfer_and_f1 as C
    g = load_golden("golden_chamfer.npz")
    d = gpu_device
    for tag in ("feat", "xyz"):
        o, gt = _t(g["calc_%s_out" % tag], d), _t(g["calc_%s_gt" % tag], d)
        for nt in ("cos", "mse"):
            r = C.calc_cd(o, gt, calc_f1=True, f1_threshold=1e-3, normal_loss_type=nt)
            keys = sorted(k[len("calc_%s_%s_" % (tag, nt)):] for k in g.files if k.startswith("calc_%s_%s_" % (tag, nt)))
            assert sorted(r) == keys
            for k in keys:
                want = g["calc_%s_%s_%s" % (tag, nt, k)]
                got = r[k].cpu().numpy()
                assert _close(got, want), (tag, nt, k, got, want)
            assert r["f1"][2].item() == 0.0
            # the precision / recall counts exactly: the reduction kernel's counts against the (bit-exact) per-point distances
            red, n_gt, n_out = C.calc_cd_reduced(o, gt, f1_threshold=1e-3, normal_loss_type=nt)
            d1, _, d2, _ = C._hip.chamfer_nn(gt.contiguous(), o.contiguous())
            assert torch.equal(red[:, 0, 2], (d1 < 1e-3).sum(1).float()) and torch.equal(red[:, 1, 2], (d2 < 1e-3).sum(1).float())
            assert red[0, 0, 2].item() > 0
    f, p1, p2 = C.fscore(_t(g["fscore_d1"], d), _t(g["fscore_d2"], d), threshold=0.005)
    for k, v in (("f", f), ("p1", p1), ("p2", p2)):
        assert _close(v.cpu().numpy(), g["fscore_" + k]), k  # (torch's GPU mean vs its CPU mean: last-bit differences)
    assert f[3].item() == 0.0 and f[:3].min().item() > 0
    m = C.Chamfer_F1(f1_threshold=1e-3)
    cd_p, cd_t, f1 = m(_t(g["calc_xyz_out"], d), _t(g["calc_xyz_gt"], d))
    assert _close(cd_p.cpu().numpy(), g["calc_xyz_cos_cd_p"]) and _close(f1.cpu().numpy(), g["calc_xyz_cos_f1"])


def test_calc_cd_of_a_pair_does_not_depend_on_its_batch(gpu_device):
    """one pair scored alone and at positions 0 and 6 of a batch of 7: bit-identical metrics (the per-cloud sums run in a fixed order)"""
    import metrics_point_cloud.chamfer_and_f1 as C
    d = gpu_device
    rs = np.random.RandomState(5)
    gt = torch.from_numpy(rs.standard_normal((7, 2048, 6)).astype(np.float32)).to(d)
    out = torch.from_numpy(rs.standard_normal((7, 2048, 6)).astype(np.float32) * 0.5).to(d)
    for nt in ("mse", "cos"):
        alone = C.calc_cd(out[3:4], gt[3:4], calc_f1=True, f1_threshold=0.05, normal_loss_type=nt)
        for pos in (0, 6):
            o, g_ = out.clone(), gt.clone()
            o[[pos, 3]] = o[[3, pos]]
            g_[[pos, 3]] = g_[[3, pos]]
            r = C.calc_cd(o, g_, calc_f1=True, f1_threshold=0.05, normal_loss_type=nt)
            for k in ("cd_p", "cd_t", "f1", "cd_feature_p", "cd_feature_t"):
                assert torch.equal(r[k][pos:pos + 1], alone[k]), (nt, pos, k)
            assert alone["f1"].item() > 0


def test_chamfer_scope_errors(gpu_device):
    import metrics_point_cloud.chamfer_and_f1 as C
    d = gpu_device
    x = torch.rand(2, 10, 3, device=d)
    y = torch.rand(2, 12, 3, device=d)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        C.chamfer_distance(xg, y)
    with pytest.raises(NotImplementedError):
        C.calc_cd(xg, y)
    with torch.no_grad():  # under no_grad a leaf that requires grad is fine
        C.calc_cd(xg, y)
    with pytest.raises(ValueError):
        C.chamfer_distance(x, y, x_lengths=torch.tensor([0, 10], device=d))
    with pytest.raises(ValueError):
        C.chamfer_distance(x, y, y_lengths=torch.tensor([13, 3], device=d))
    with pytest.raises(ValueError):
        C.chamfer_distance(x, torch.rand(3, 12, 3, device=d))
    with pytest.raises(ValueError):
        C.calc_cd(x, torch.rand(2, 12, 4, device=d))
    with pytest.raises(ValueError):
        C.chamfer_distance(x, y, weights=torch.tensor([1.0, -1.0], device=d))
    with pytest.raises(ValueError):
        C.chamfer_distance(x, y, point_reduction=None, batch_reduction="mean")
    with pytest.raises(ValueError):
        C.chamfer_distance(object(), y)  # a pytorch3d Pointclouds (or anything but a tensor)
    with pytest.raises(RuntimeError):
        C.calc_cd(x.cpu(), y.cpu())  # no CPU fallback
