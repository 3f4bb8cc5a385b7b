"""tools/gen_golden_chamfer_grad.py -- AUTHORING ONLY (never imported by tests, bench or smoke): records
tests/golden/golden_chamfer_grad.npz, the gradients of the reference's calc_cd from the reference's own autograd.

The reference's pointnet2/metrics_point_cloud/chamfer_and_f1.py is imported where it lies, through tools/ref_shims.py; nothing of it
is copied.  The shim's knn_points returns non-differentiable numpy results, so the module's `knn_points` is overridden here with one
whose indices come from the oracle and whose `dists` are recomputed in torch from them: sum((p1 - p2[idx])^2), whose gradient
2 (p1 - p2[idx]) into both clouds is pytorch3d's own.  calc_cd runs in float64 on fp32-valued inputs.

Cases (output vs gt, `mse` feature term):
  xyz   B 2, output 200 x gt 256 points, C = 3
  feat  B 2, output 256 x gt 200 points, C = 6
  fan   B 1, output 96 x gt 160 points, C = 6: FAN_IN gt points in a small ball around output point 0 (they all pick it), and
        output point 1 far from every gt point (in-degree 0)
Recorded per case (arrays only): <case>_out, <case>_gt (f32), <case>_i1 (gt -> output), <case>_i2 (output -> gt) (int64), the loss
dict <case>_cd_p, _cd_t[, _cd_feature_p, _cd_feature_t] (f64, (B,)) and, for w in `weights` = [0, 0.1] (C = 3: w = 0 only),
<case>_gout_p_w<k>, <case>_ggt_p_w<k>: the gradients of (cd_p + w cd_feature_p).mean() w.r.t. output and gt, and _gout_t_w<k>,
_ggt_t_w<k> those of (cd_t + w cd_feature_t).mean() (f64).

Fixture condition, checked here and again by tests/test_chamfer_grad_host.py: no zero distance and no zero feature term, and every
nearest neighbour beats its runner-up by a relative gap > 1e-4 (the convention of golden_generation_metrics.npz), so an fp32 search
must pick the recorded indices.  A seed that does not meet it is rejected (take another; do not loosen the test).

usage:  python tools/gen_golden_chamfer_grad.py [--seed 0] [--out tests/golden]
"""
import argparse
import collections
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

GAP = 1e-4
FAN_IN = 80
WEIGHTS = (0.0, 0.1)


def make_cases(seed):
    rs = np.random.RandomState(seed)

    def cloud(B, P, C, scale=1.0):
        return (rs.standard_normal((B, P, C)) * scale).astype(np.float32)

    cases = {"xyz": (cloud(2, 200, 3), cloud(2, 256, 3)), "feat": (cloud(2, 256, 6), cloud(2, 200, 6))}
    out, gt = cloud(1, 96, 6), cloud(1, 160, 6)
    out[0, 48:, :3] += np.float32(6.0) * np.sign(out[0, 48:, :3])  # half of the output points far out: most of them in-degree 0
    out[0, 0, :3] = (0.25, -0.5, 0.125)
    gt[0, :FAN_IN, :3] = out[0, 0, :3] + 0.05 * rs.uniform(-1, 1, (FAN_IN, 3)).astype(np.float32)
    out[0, 1, :3] = (40.0, 40.0, 40.0)  # nobody's nearest neighbour
    cases["fan"] = (out, gt)
    return cases


def min_gap_and_zeros(out, gt, i1, i2):
    """-> (smallest relative gap runner-up vs nearest over both directions, smallest distance, smallest feature term)"""
    o, g = out.astype(np.float64), gt.astype(np.float64)
    gap, dmin, tmin = np.inf, np.inf, np.inf
    for b in range(o.shape[0]):
        D = ((g[b, :, None, :3] - o[b, None, :, :3]) ** 2).sum(-1)
        for M, idx, own, other in ((D, i1[b], g[b], o[b]), (D.T, i2[b], o[b], g[b])):
            srt = np.sort(M, axis=1)
            assert np.array_equal(M.argmin(1), idx)
            gap = min(gap, float(((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min()))
            dmin = min(dmin, float(srt[:, 0].min()))
            if own.shape[1] > 3:
                tmin = min(tmin, float(((own[:, 3:] - other[idx, 3:]) ** 2).sum(-1).min()))
    return gap, dmin, tmin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    import ref_shims
    ref_shims.install()
    from oracle import ops as O
    import metrics_point_cloud.chamfer_and_f1 as R
    assert R.__file__.startswith(ref_shims.REF), R.__file__

    KNN = collections.namedtuple("KNN", "dists idx knn")

    def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, **kw):
        assert K == 1
        _, i = O.knn_points(p1.detach().numpy().astype(np.float32), p2.detach().numpy().astype(np.float32), 1, None)
        idx = torch.from_numpy(i)
        near = p2.gather(1, idx[:, :, 0, None].expand(-1, -1, p2.shape[2]))
        return KNN(((p1 - near) ** 2).sum(-1, keepdim=True), idx, None)

    R.knn_points = knn_points
    res = {"seed": np.int64(a.seed), "weights": np.asarray(WEIGHTS, np.float64), "fan_in": np.int64(FAN_IN)}
    for name, (out, gt) in make_cases(a.seed).items():
        o = torch.from_numpy(out).double().requires_grad_(True)
        g = torch.from_numpy(gt).double().requires_grad_(True)
        r = R.calc_cd(o, g, calc_f1=False, normal_loss_type='mse')
        assert r["cd_p"].dtype == torch.float64
        i1 = O.knn_points(gt[:, :, :3].copy(), out[:, :, :3].copy(), 1, None)[1][..., 0]
        i2 = O.knn_points(out[:, :, :3].copy(), gt[:, :, :3].copy(), 1, None)[1][..., 0]
        gap, dmin, tmin = min_gap_and_zeros(out, gt, i1, i2)
        if not (gap > GAP and dmin > 0 and tmin > 0):
            raise SystemExit("seed %d, case %s: gap %.3e, smallest distance %.3e, smallest feature term %.3e -- take another seed" %
                             (a.seed, name, gap, dmin, tmin))
        res.update({name + "_out": out, name + "_gt": gt, name + "_i1": i1, name + "_i2": i2})
        for k, v in r.items():
            res["%s_%s" % (name, k)] = v.detach().numpy()
        feat = out.shape[2] > 3
        for k, w in enumerate(WEIGHTS if feat else WEIGHTS[:1]):
            for tag in ("p", "t"):
                loss = r["cd_" + tag] + (w * r["cd_feature_" + tag] if feat else 0.0)
                go, gg = torch.autograd.grad(loss.mean(), (o, g), retain_graph=True)
                assert torch.isfinite(go).all() and torch.isfinite(gg).all()
                res["%s_gout_%s_w%d" % (name, tag, k)] = go.numpy()
                res["%s_ggt_%s_w%d" % (name, tag, k)] = gg.numpy()
        indeg = np.bincount(i1[0], minlength=out.shape[1])
        print("%-5s out %s gt %s: min gap %.3e, min d %.3e, min t %.3e, max in-degree %d, output points of in-degree 0: %d" %
              (name, out.shape, gt.shape, gap, dmin, tmin, indeg.max(), int((indeg == 0).sum())))
        if name == "fan":
            assert indeg[0] >= 64 and indeg[1] == 0, indeg[:2]
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "golden_chamfer_grad.npz")
    np.savez_compressed(path, **res)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
