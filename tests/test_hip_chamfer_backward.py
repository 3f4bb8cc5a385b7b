"""GPU: the differentiable Chamfer loss -- slide_amd/csrc/chamfer_bwd.hip through _ext.chamfer_cd_bwd, train.functions.ChamferCD and
train.losses.calc_cd_loss / autoencoder_losses.

The gradient kernel is held to a float64 restatement of include/slide_train.h's formula on the same fp32 inputs and the same
neighbour indices, element by element, within |err| <= gamma(R + m) S: R = 10 rounding steps of one term, m the point's in-degree, S
the sum of the magnitudes of the element's terms -- derived in tests/chamfer_grad_cases.py from the kernel's operations, not from its
results.  The same bound holds the gradients of calc_cd_loss to the reference's own autograd (tests/golden/golden_chamfer_grad.npz).
Every comparison prints its worst err / tol.

Measured on an MI355X (worst err / tol): kernel against the restatement 0.31 (B 8 x 2048 x 2048, C 6; fixture cases 0.26), calc_cd_loss
against the recorded reference gradients 0.35 (fan-in case, cd_p, w = 0.1), autoencoder_losses levels 0.35; the fit test's loss goes
0.655 -> 0.0098."""
import os
import sys

import numpy as np
import pytest
import torch

from chamfer_grad_cases import dred_of_loss, restate, tolerance
from conftest import REPO, load_golden

sys.path.insert(0, os.path.join(REPO, "pointnet2"))
pytestmark = pytest.mark.gpu

CASES = ("xyz", "feat", "fan")


def _t(a, d):
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


def _worst(got, want, S, m, F):
    """largest err / tol over the elements (an element whose terms are all zero must be exactly zero)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    tol = tolerance(S, m, F)
    assert np.all(err[tol == 0] == 0)
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def _kernel_vs_restatement(x, y, dred, d):
    """x, y, dred numpy fp32 -> worst err / tol of (dx, dy) against the float64 restatement on the kernel's own neighbour indices"""
    from slide_amd import _ext
    xt, yt = _t(x, d), _t(y, d)
    d1, i1, d2, i2 = _ext.chamfer_nn(xt, yt)
    dx, dy = _ext.chamfer_cd_bwd(xt, yt, d1, i1, d2, i2, _t(dred, d))
    assert dx.shape == xt.shape and dy.shape == yt.shape
    rx, ry, Sx, Sy, mx, my = restate(x, y, i1.cpu().numpy(), i2.cpu().numpy(), dred)
    F = x.shape[2] - 3
    gx, gy = dx.cpu().numpy(), dy.cpu().numpy()
    assert np.isfinite(gx).all() and np.isfinite(gy).all()
    return max(_worst(gx, rx, Sx, mx, F), _worst(gy, ry, Sy, my, F))


def test_kernel_matches_float64_restatement_on_the_fixture(gpu_device):
    g = load_golden("golden_chamfer_grad.npz")
    rs = np.random.RandomState(11)
    for name in CASES:
        out, gt = g[name + "_out"], g[name + "_gt"]
        dred = rs.standard_normal((gt.shape[0], 2, 5)).astype(np.float32)
        w = _kernel_vs_restatement(gt, out, dred, gpu_device)
        print("fixture %-4s worst err / tol %.3f" % (name, w))
        assert w <= 1.0, (name, w)


@pytest.mark.parametrize("B,P1,P2,C", [(1, 1, 1, 3), (3, 17, 5, 6), (2, 513, 1025, 6), (2, 2049, 700, 3), (2, 300, 257, 4),
                                       (2, 130, 600, 8), (1, 64, 64, 19), (8, 2048, 2048, 3), (8, 2048, 2048, 6)])
def test_kernel_matches_float64_restatement(gpu_device, B, P1, P2, C):
    rs = np.random.RandomState(B * 7919 + P1 * 31 + P2 + C)
    x = rs.standard_normal((B, P1, C)).astype(np.float32)
    y = (rs.standard_normal((B, P2, C)) * 0.7).astype(np.float32)
    dred = rs.standard_normal((B, 2, 5)).astype(np.float32)
    w = _kernel_vs_restatement(x, y, dred, gpu_device)
    print("B %d P1 %d P2 %d C %d: worst err / tol %.3f" % (B, P1, P2, C, w))
    assert w <= 1.0, w


def _close(got, want, tol=1e-6):  # the tolerance of tests/test_hip_chamfer.py for these quantities against its golden
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.all(np.abs(got - want) <= tol * np.maximum(np.abs(want), 1e-30) + 1e-12)


@pytest.mark.parametrize("name", CASES)
def test_calc_cd_loss_matches_the_reference_autograd(gpu_device, name):
    from slide_amd.train.losses import calc_cd_loss
    g = load_golden("golden_chamfer_grad.npz")
    d = gpu_device
    out, gt, i1, i2 = g[name + "_out"], g[name + "_gt"], g[name + "_i1"], g[name + "_i2"]
    B, n_gt, n_out, F = gt.shape[0], gt.shape[1], out.shape[1], gt.shape[2] - 3
    for k, w in enumerate(g["weights"][:2 if F else 1]):
        for tag in ("p", "t"):
            o, t = _t(out, d).requires_grad_(True), _t(gt, d).requires_grad_(True)
            r = calc_cd_loss(o, t)
            for key in ("cd_p", "cd_t") + (("cd_feature_p", "cd_feature_t") if F else ()):
                assert _close(r[key].detach().cpu().numpy(), g["%s_%s" % (name, key)]), (name, key)
            loss = r["cd_" + tag] + (float(w) * r["cd_feature_" + tag] if F else 0.0)
            go, gg = torch.autograd.grad(loss.mean(), (o, t))
            _, _, Sgt, Sout, mgt, mout = restate(gt, out, i1, i2, dred_of_loss(B, n_gt, n_out, tag, float(w)))
            wo = _worst(go.cpu().numpy(), g["%s_gout_%s_w%d" % (name, tag, k)], Sout, mout, F)
            wg = _worst(gg.cpu().numpy(), g["%s_ggt_%s_w%d" % (name, tag, k)], Sgt, mgt, F)
            print("%s cd_%s w %.1f: worst err / tol output %.3f gt %.3f" % (name, tag, w, wo, wg))
            assert wo <= 1.0 and wg <= 1.0, (name, tag, k, wo, wg)


def test_forward_values_are_bit_equal_to_calc_cd(gpu_device):
    import metrics_point_cloud.chamfer_and_f1 as C
    from slide_amd.train.losses import calc_cd_loss
    d = gpu_device
    rs = np.random.RandomState(3)
    for c in (3, 6):
        gt = _t(rs.standard_normal((5, 700, c)).astype(np.float32), d)
        out = _t((gt.cpu().numpy()[:, :512] + 0.02 * rs.standard_normal((5, 512, c))).astype(np.float32), d)
        with torch.no_grad():
            want = C.calc_cd(out, gt, calc_f1=True, f1_threshold=1e-3, normal_loss_type='mse')
            got = calc_cd_loss(out, gt, calc_f1=True, f1_threshold=1e-3)
        live = calc_cd_loss(out.clone().requires_grad_(True), gt, calc_f1=True, f1_threshold=1e-3)
        assert sorted(got) == sorted(want) == sorted(live)
        for k in want:
            assert torch.equal(got[k], want[k]) and torch.equal(live[k].detach(), want[k]), (c, k)
        assert want["f1"].max().item() > 0
        assert live["cd_p"].requires_grad and not live["f1"].requires_grad


def _grads(out, gt, w=0.1, gt_grad=True):
    from slide_amd.train.losses import calc_cd_loss
    o = out.clone().requires_grad_(True)
    t = gt.clone().requires_grad_(gt_grad)
    r = calc_cd_loss(o, t)
    (r["cd_p"] + w * r["cd_feature_p"] + 0.5 * r["cd_t"] + 0.3 * r["cd_feature_t"]).sum().backward()
    return o.grad, t.grad


def test_gradients_are_deterministic_and_batch_independent(gpu_device):
    d = gpu_device
    rs = np.random.RandomState(5)
    gt = _t(rs.standard_normal((8, 2048, 6)).astype(np.float32), d)
    out = _t((rs.standard_normal((8, 1500, 6)) * 0.5).astype(np.float32), d)
    a, b = _grads(out, gt), _grads(out, gt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    alone = _grads(out[3:4], gt[3:4])  # position 0 of 1
    o, g_ = out.clone(), gt.clone()
    o[[5, 3]] = o[[3, 5]]
    g_[[5, 3]] = g_[[3, 5]]
    moved = _grads(o, g_)  # the same pair at position 5 of 8
    assert torch.equal(moved[0][5:6], alone[0]) and torch.equal(moved[1][5:6], alone[1])
    assert alone[0].abs().max().item() > 0


def test_coincident_points_have_finite_gradients_and_a_zero_square_root_part(gpu_device):
    """output == gt on the first 40 points (d = 0 and t = 0 for those twins) and one shared feature vector everywhere else (t = 0 for
    every pair among those): gradients are finite, agree with the restatement (whose convention is the subgradient 0), and with a
    dred that only has the square-root columns the twins that nobody else selects get exactly 0, and so does every feature whose
    terms all have t = 0"""
    from slide_amd import _ext
    d = gpu_device
    rs = np.random.RandomState(9)
    gt = rs.standard_normal((2, 300, 6)).astype(np.float32)
    out = rs.standard_normal((2, 260, 6)).astype(np.float32)
    out[:, :40] = gt[:, :40]
    gt[:, 40:, 3:] = np.float32([0.5, -0.25, 2.0])
    out[:, 40:, 3:] = np.float32([0.5, -0.25, 2.0])
    dred = np.zeros((2, 2, 5), np.float32)
    dred[:, :, 1] = rs.uniform(0.5, 1.5, (2, 2))
    dred[:, :, 4] = rs.uniform(0.5, 1.5, (2, 2))
    for full in (False, True):
        if full:
            dred[:, :, 0] = 0.7
            dred[:, :, 3] = -0.4
        xt, yt = _t(gt, d), _t(out, d)
        d1, i1, d2, i2 = _ext.chamfer_nn(xt, yt)
        assert (d1[:, :40] == 0).all() and (d2[:, :40] == 0).all()
        dx, dy = [a.cpu().numpy() for a in _ext.chamfer_cd_bwd(xt, yt, d1, i1, d2, i2, _t(dred, d))]
        assert np.isfinite(dx).all() and np.isfinite(dy).all()
        i1n, i2n = i1.cpu().numpy(), i2.cpu().numpy()
        rx, ry, Sx, Sy, mx, my = restate(gt, out, i1n, i2n, dred)
        assert max(_worst(dx, rx, Sx, mx, 3), _worst(dy, ry, Sy, my, 3)) <= 1.0
        if not full:
            lonely_x, lonely_y = mx[:, :40] == 1, my[:, :40] == 1  # selected by their twin only
            assert lonely_x.any() and lonely_y.any()
            assert not dx[:, :40][lonely_x].any() and not dy[:, :40][lonely_y].any()
            # features: a point of the shared-feature set whose own neighbour and whose sources are all in that set
            own_x = (i1n >= 40) & (np.arange(300)[None] >= 40)
            src_ok = np.ones((2, 300), bool)
            for b in range(2):
                bad = np.unique(i2n[b][np.arange(260) < 40])  # targets of twins
                src_ok[b, bad] = False
            sel = own_x & src_ok
            assert sel.any() and not dx[:, :, 3:][sel].any()


def test_optional_outputs(gpu_device):
    from slide_amd import _ext
    d = gpu_device
    rs = np.random.RandomState(2)
    gt = _t(rs.standard_normal((3, 600, 6)).astype(np.float32), d)
    out = _t(rs.standard_normal((3, 777, 6)).astype(np.float32), d)
    both = _grads(out, gt)
    only = _grads(out, gt, gt_grad=False)
    assert only[1] is None and torch.equal(only[0], both[0])
    d1, i1, d2, i2 = _ext.chamfer_nn(gt, out)
    dred = _t(rs.standard_normal((3, 2, 5)).astype(np.float32), d)
    dx, dy = _ext.chamfer_cd_bwd(gt, out, d1, i1, d2, i2, dred)
    dx1, none = _ext.chamfer_cd_bwd(gt, out, d1, i1, d2, i2, dred, need_dy=False)
    none2, dy1 = _ext.chamfer_cd_bwd(gt, out, d1, i1, d2, i2, dred, need_dx=False)
    assert none is None and none2 is None and torch.equal(dx1, dx) and torch.equal(dy1, dy)


def _ae_arrays(d):
    g = load_golden("golden_ae_forward.npz")
    pc = _t(load_golden("golden_encode.npz")["pointcloud"], d)
    n_lv = int(g["levels"])
    levels = [_t(g["level%d" % i], d) for i in range(n_lv)]
    return g, pc, levels, n_lv


def test_autoencoder_losses_match_the_evaluation_forward(gpu_device):
    """the arrays of golden_ae_forward.npz through autoencoder_losses: the reference's loss_list to the 1e-6 of
    test_hip_ae_forward.py::test_metrics_on_the_reference_levels_match_loss_list"""
    from slide_amd.train.losses import autoencoder_losses
    d = gpu_device
    g, pc, levels, n_lv = _ae_arrays(d)
    start = torch.zeros(pc.shape[0], dtype=torch.int32, device=d)
    kl = _t(g["loss%d_kl_loss" % (n_lv - 2)].astype(np.float32), d)
    ll = autoencoder_losses(levels, pc, [float(v) for v in g["feature_weight"]], loss_type='cd_p', kl_loss=kl,
                            kl_weight=float(g["kl_weight"]), apply_kl_regularization=True, fps_start_idx=start)
    assert len(ll) == n_lv - 1
    for i, dct in enumerate(ll):
        assert sorted(dct) == sorted(("cd_p", "cd_t", "cd_feature_p", "cd_feature_t", "f1", "kl_loss", "training_loss"))
        for k, v in dct.items():
            want = g["loss%d_%s" % (i, k)]
            got = v.cpu().numpy()
            assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (i, k, got, want)


def test_autoencoder_losses_gradients_match_float64_autograd(gpu_device):
    from slide_amd import _ext
    from slide_amd.train.losses import autoencoder_losses
    d = gpu_device
    g, pc, levels, n_lv = _ae_arrays(d)
    B = pc.shape[0]
    fw, klw = [float(v) for v in g["feature_weight"]], float(g["kl_weight"])
    start = torch.zeros(B, dtype=torch.int32, device=d)
    lv = [levels[0]] + [l.clone().requires_grad_(True) for l in levels[1:]]
    kl = _t(g["loss%d_kl_loss" % (n_lv - 2)].astype(np.float32), d).requires_grad_(True)
    ll = autoencoder_losses(lv, pc, fw, loss_type='cd_p', kl_loss=kl, kl_weight=klw, apply_kl_regularization=True, fps_start_idx=start)
    sum(dct["training_loss"].mean() for dct in ll).backward()
    assert np.allclose(kl.grad.cpu().numpy(), klw / B, rtol=1e-6, atol=0)
    for i in range(1, n_lv):
        down, _ = _ext.sample_farthest_points(pc, K=lv[i].shape[1], start_idx=start)
        _, i1, _, i2 = _ext.chamfer_nn(down, lv[i].detach())
        # float64 torch restatement of calc_cd on the same neighbours, differentiated by torch
        o = lv[i].detach().cpu().double().requires_grad_(True)
        t = down.cpu().double()
        near_o = o.gather(1, i1.cpu()[:, :, None].expand(-1, -1, 6))
        near_t = t.gather(1, i2.cpu()[:, :, None].expand(-1, -1, 6))
        e1, e2 = t - near_o, o - near_t
        cd_p = ((e1[..., :3] ** 2).sum(-1).sqrt().mean(1) + (e2[..., :3] ** 2).sum(-1).sqrt().mean(1)) / 2
        cd_f = ((e1[..., 3:] ** 2).sum(-1).sqrt().mean(1) + (e2[..., 3:] ** 2).sum(-1).sqrt().mean(1)) / 2
        (want,) = torch.autograd.grad((cd_p + fw[i - 1] * cd_f).mean(), o)
        _, _, _, Sout, _, mout = restate(t.numpy(), o.detach().numpy(), i1.cpu().numpy(), i2.cpu().numpy(),
                                         dred_of_loss(B, t.shape[1], o.shape[1], "p", fw[i - 1]))
        w = _worst(lv[i].grad.cpu().numpy(), want.numpy(), Sout, mout, 3)
        print("level %d: worst err / tol %.3f" % (i, w))
        assert w <= 1.0, (i, w)


def test_a_free_cloud_fits_its_target(gpu_device):
    """200 Adam steps on a free (4, 512, 6) tensor (standard normal start) against a fixed target -- 512 points of the unit sphere
    with their normals as features, the kind of cloud the autoencoder reconstructs -- with cd_p + 0.1 cd_feature_p: the loss ends
    below a tenth of its start and every step's gradient is finite (checked once, on the device, after the loop)"""
    from slide_amd.train.losses import calc_cd_loss
    d = gpu_device
    gen = torch.Generator(device="cpu").manual_seed(0)
    normal = torch.nn.functional.normalize(torch.randn(4, 512, 3, generator=gen), dim=2)
    target = torch.cat([normal, normal], dim=2).to(d)
    free = torch.randn(4, 512, 6, generator=gen).to(d).requires_grad_(True)
    opt = torch.optim.Adam([free], lr=0.1)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.98)
    finite = torch.ones((), dtype=torch.bool, device=d)
    losses = []
    for _ in range(200):
        opt.zero_grad(set_to_none=True)
        r = calc_cd_loss(free, target)
        loss = (r["cd_p"] + 0.1 * r["cd_feature_p"]).mean()
        loss.backward()
        finite = finite & torch.isfinite(free.grad).all()
        losses.append(loss.detach())
        opt.step()
        sched.step()
    with torch.no_grad():
        r = calc_cd_loss(free, target)
        end = (r["cd_p"] + 0.1 * r["cd_feature_p"]).mean().item()
    print("fit: loss %.4f -> %.4f" % (losses[0].item(), end))
    assert finite.item()
    assert end < 0.1 * losses[0].item(), (losses[0].item(), end)


def test_forward_and_backward_capture_into_one_graph(gpu_device):
    """one capture of forward + backward on one stream, one replay: bit-equal to the eager result"""
    from slide_amd.train.losses import calc_cd_loss
    d = gpu_device
    rs = np.random.RandomState(4)
    gt = _t(rs.standard_normal((4, 1024, 6)).astype(np.float32), d)
    out = _t(rs.standard_normal((4, 900, 6)).astype(np.float32), d).requires_grad_(True)

    def step():
        r = calc_cd_loss(out, gt, calc_f1=True)
        loss = (r["cd_p"] + 0.1 * r["cd_feature_p"]).mean()
        (go,) = torch.autograd.grad(loss, out)
        return loss.detach(), go

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager_loss, eager_grad = step()
        eager_loss, eager_grad = eager_loss.clone(), eager_grad.clone()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_loss, g_grad = step()
    g_grad.zero_()
    g_loss.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_loss, eager_loss) and torch.equal(g_grad, eager_grad)
    assert eager_grad.abs().max().item() > 0


def test_scope_errors(gpu_device):
    from slide_amd.train.functions import chamfer_cd
    from slide_amd.train.losses import calc_cd_loss
    d = gpu_device
    x = torch.rand(2, 10, 6, device=d, requires_grad=True)
    y = torch.rand(2, 12, 6, device=d)
    with pytest.raises(NotImplementedError):
        calc_cd_loss(x, y, normal_loss_type='cos')
    with pytest.raises(RuntimeError):
        calc_cd_loss(x.detach().cpu(), y.cpu())  # no CPU fallback
    with pytest.raises(ValueError):
        calc_cd_loss(x, torch.rand(3, 12, 6, device=d))
    with pytest.raises(ValueError):
        calc_cd_loss(x, torch.rand(2, 12, 3, device=d))
    with pytest.raises(ValueError):
        chamfer_cd(x, torch.rand(2, 12, device=d))
    with pytest.raises(ValueError):
        chamfer_cd(torch.rand(2, 4, 20, device=d), torch.rand(2, 4, 20, device=d))  # more than 16 feature channels
    with pytest.raises(RuntimeError):
        chamfer_cd(x.double(), y.double())
    red = chamfer_cd(x, y)
    (gx,) = torch.autograd.grad(red[:, :, 1].sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):  # once_differentiable: no double backward
        torch.autograd.grad(gx.sum(), x)
