"""GPU: the trainable decode side (slide_amd/train/cloudnet.py, decoder.py, losses.decoder_training_loss) against the reference's own
forward, losses and autograd on a reduced two-level decoder (tests/golden/golden_ae_decoder_train.npz, tools/gen_golden_ae_train.py),
against the recorded full-size decode (golden_decode.npz) and the module path's PointAutoencoder.decode, and replayed as one HIP graph.

Tolerances are the project's own for the denoiser step (tests/test_train_denoiser.py): forward 2e-4 max-norm, loss 1e-5 relative,
gradient norms within 1e-3 of the gradient's scale, sampled gradient entries 2e-3, input gradients 2e-3 of their scale, replayed
against eager gradients 1e-5 of scale.  Every selection the reference recorded -- kNN tables, FPS picks, thinning picks, the loss's
down-sampling, the Chamfer neighbours -- must be reproduced exactly.  Measured worst ratios: profiles/decoder_training.md."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_spec, load_golden
from slide_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


@pytest.fixture(scope="module")
def fx():
    g = load_golden("golden_ae_decoder_train.npz")
    spec = golden_spec(g)
    vals = synth_state_dict([("ae." + n, s) for n, s in spec], seed=int(g["seed"]))
    return g, json.loads(str(g["decoder_configs_json"])), {n: vals["ae." + n] for n, _ in spec}


def _decoder(fx, device):
    from slide_amd.train.decoder import TrainableDecoder
    return TrainableDecoder(fx[1], fx[2]).to(device)


class Selections:
    """records what every selection of the code under test returned, in call order: ('knn', idx) for K > 1, ('fps', idx),
    ('sample', idx), ('chamfer', (i1, i2))"""

    def __init__(self, monkeypatch):
        from slide_amd import _ext
        self.events = []
        knn0, fps0, sfp0, cd0 = _ext.knn_points, _ext.furthest_point_sampling, _ext.sample_farthest_points, _ext.chamfer_nn

        def knn_points(p1, p2, K, *a, **k):
            r = knn0(p1, p2, K, *a, **k)
            if K > 1:
                self.events.append(("knn", r[1]))
            return r

        def furthest_point_sampling(p, m):
            r = fps0(p, m)
            self.events.append(("fps", r))
            return r

        def sample_farthest_points(points, *a, **k):
            r = sfp0(points, *a, **k)
            self.events.append(("sample", r[1]))
            return r

        def chamfer_nn(x, y, *a, **k):
            r = cd0(x, y, *a, **k)
            self.events.append(("chamfer", (r[1], r[3])))
            return r

        monkeypatch.setattr(_ext, "knn_points", knn_points)
        monkeypatch.setattr(_ext, "furthest_point_sampling", furthest_point_sampling)
        monkeypatch.setattr(_ext, "sample_farthest_points", sample_farthest_points)
        monkeypatch.setattr(_ext, "chamfer_nn", chamfer_nn)

    def take(self):
        ev, self.events = self.events, []
        return [(k, tuple(t.cpu().numpy().astype(np.int64) for t in v) if isinstance(v, tuple) else v.cpu().numpy().astype(np.int64)) for k, v in ev]


def _recorded(g, prefix):
    keys = sorted(k for k in g.files if k.startswith(prefix + "_sel"))
    return [(k.split("_")[-1], g[k].astype(np.int64)) for k in keys]


def _same_selections(got, want, what):
    """zero mismatches allowed: the fixture's seed search keeps every recorded selection clear of its runner-up"""
    assert [k for k, _ in got] == [k for k, _ in want], (what, [k for k, _ in got], [k for k, _ in want])
    for j, ((k, a), (_, r)) in enumerate(zip(got, want)):
        assert a.shape == r.shape and int((a != r).sum()) == 0, (what, j, k, int((a != r).sum()))


def _compare_grads(named, names, ref_norms, samples, tol_norm=1e-3, tol_full=2e-3):
    """tests/test_train_denoiser.py _grads_vs_golden: norms within tol_norm of the whole gradient's norm, sampled entries within tol_full
    of max(the parameter's largest entry, 1e-3 of the scale); a parameter without a gradient counts as zero -> the two worst ratios"""
    norms = np.array([0.0 if named[n].grad is None else float(named[n].grad.double().norm()) for n in names])
    scale = np.sqrt((ref_norms ** 2).sum())
    wn = float(np.abs(norms - ref_norms).max() / scale)
    assert wn <= tol_norm, (wn, names[int(np.abs(norms - ref_norms).argmax())])
    worst = 0.0
    for n, (r, stride) in samples.items():
        a = named[n].grad.detach().cpu().numpy().reshape(-1)[::stride]
        worst = max(worst, float(np.abs(a - r).max() / max(np.abs(r).max(), 1e-3 * scale)))
    assert worst <= tol_full, worst
    return wn, worst


@pytest.mark.parametrize("lvl", [0, 1])
def test_level_forward_loss_and_gradients_match_the_reference(fx, lvl, gpu_device, monkeypatch):
    """one decoder level on the reference's own level inputs: final_feature and the output points, every selection, the level's
    training loss, every parameter's gradient and the gradients with respect to `features` and `new_xyz`.

    MEASURED (MI355X, profiles/decoder_training.md): level 0 forward 5.5e-6 / 6.2e-7, norms 2.6e-7 of scale, sampled entries 1.1e-5,
    d features 2.6e-6, d new_xyz 1.3e-6; level 1 forward 6.4e-6 / 2.2e-7, norms 5.6e-7, entries 1.6e-5, 5.2e-6, 9.0e-7.  (The first
    fixture missed the norms at 2.4e-3 through ONE ReLU decision on an input of +5.1e-6; the generator's seed search now also
    requires that the reference's near-zero ReLU decisions do not move its gradients: tests/test_ae_decoder_fixture_host.py.)"""
    from slide_amd.train.losses import autoencoder_losses
    g = fx[0]
    dec = _decoder(fx, gpu_device)
    level = dec.decoder.decoders[lvl]
    T = lambda a: torch.from_numpy(np.asarray(a)).to(gpu_device)
    p = "lvl%d" % lvl
    xyz, lab = T(g[p + "_xyz"]), T(g["label"])
    feats, new_xyz = T(g[p + "_features"]).requires_grad_(True), T(g[p + "_new_xyz"]).requires_grad_(True)
    start = torch.zeros(xyz.shape[0], dtype=torch.int32, device=gpu_device)
    sel = Selections(monkeypatch)
    ff, pts = level(xyz, feats, new_xyz, lab, fps_start_idx=start)
    _same_selections(sel.take(), _recorded(g, p), p)
    e_f, e_p = _rel(ff.detach().cpu().numpy(), g[p + "_final_feature"]), _rel(pts.detach().cpu().numpy(), g[p + "_points"])
    print("MEASURED %s forward: final_feature %.3g, points %.3g (max-norm; absolute on the points %.3g)" % (
        p, e_f, e_p, float(np.abs(pts.detach().cpu().numpy() - g[p + "_points"]).max())))
    assert e_f <= 2e-4 and e_p <= 2e-4, (e_f, e_p)
    w = float(g["feature_weight"][lvl + 1])
    d = autoencoder_losses([xyz, pts], T(g["pointcloud"]), [w], fps_start_idx=start)[0]
    ev = sel.take()
    assert [k for k, _ in ev] == ["sample", "chamfer"]
    _same_selections(ev[:1], [("sample", g["loss_sel%02d_sample" % (lvl + 1)].astype(np.int64))], p + " down-sampling")
    assert np.array_equal(ev[1][1][0], g[p + "_cd_i1"]) and np.array_equal(ev[1][1][1], g[p + "_cd_i2"])
    loss = d["training_loss"].mean()
    e_l = abs(float(loss.detach()) - float(g[p + "_loss"])) / abs(float(g[p + "_loss"]))
    assert _rel(d["training_loss"].detach().cpu().numpy(), g[p + "_training_loss"]) <= 1e-5 and e_l <= 1e-5, e_l
    loss.backward()
    names = [str(n) for n in g[p + "_grad_names"]]
    own = "decoder.decoders.%d." % lvl
    samples = {own + k[len(p + "_grad__"):]: (g[k], int(g[k.replace("_grad__", "_stride__")])) for k in g.files if k.startswith(p + "_grad__")}
    assert len(samples) >= 18
    wn, wf = _compare_grads(dict(dec.named_parameters()), names, g[p + "_grad_norms"], samples)
    e_df = float(np.abs(feats.grad.cpu().numpy() - g[p + "_dfeatures"]).max() / np.abs(g[p + "_dfeatures"]).max())
    e_dx = float(np.abs(new_xyz.grad.cpu().numpy() - g[p + "_dnew_xyz"]).max() / np.abs(g[p + "_dnew_xyz"]).max())
    print("MEASURED %s gradients: loss %.3g, norms %.3g of scale, sampled entries %.3g, d features %.3g, d new_xyz %.3g" % (p, e_l, wn, wf, e_df, e_dx))
    assert e_df <= 2e-3 and e_dx <= 2e-3, (e_df, e_dx)


def test_chained_loss_and_gradients_match_the_reference(fx, gpu_device, monkeypatch):
    """decoder_training_loss on the whole chain: the levels, every selection, the loss, every parameter's gradient norm and the
    gradient with respect to feature_at_keypoint.

    MEASURED (MI355X): levels within 5.9e-8 / 5.6e-7 / 7.1e-7, loss 7.9e-8, norms 6.2e-7 of scale, d feature_at_keypoint 3.1e-6."""
    from slide_amd.train.losses import decoder_training_loss
    g = fx[0]
    dec = _decoder(fx, gpu_device)
    T = lambda a: torch.from_numpy(np.asarray(a)).to(gpu_device)
    feat = T(g["feature"]).requires_grad_(True)
    start = torch.zeros(feat.shape[0], dtype=torch.int32, device=gpu_device)
    sel = Selections(monkeypatch)
    l_xyz = dec.decode(T(g["keypoint"]), feat, T(g["label"]), fps_start_idx=start)
    _same_selections(sel.take(), _recorded(g, "chain"), "chain")
    errs = [_rel(l_xyz[i].detach().cpu().numpy(), g["chain_level%d" % i]) for i in (1, 2, 3)]
    print("MEASURED chain forward: levels", " ".join("%.3g" % e for e in errs))
    assert max(errs) <= 2e-4, errs
    feat.grad = None
    loss, loss_list = decoder_training_loss(dec, T(g["keypoint"]), feat, T(g["label"]), T(g["pointcloud"]), g["feature_weight"].tolist(),
                                            fps_start_idx=start)
    ev = sel.take()
    # the decode's own selections again (the same call), then per level the loss's down-sampling and the Chamfer neighbours
    n_dec = len(_recorded(g, "chain"))
    _same_selections(ev[:n_dec], _recorded(g, "chain"), "chain under the loss")
    assert [k for k, _ in ev[n_dec:]] == ["sample", "chamfer"] * 3
    _same_selections(ev[n_dec::2], [("sample", g["loss_sel%02d_sample" % i].astype(np.int64)) for i in range(3)], "loss down-sampling")
    for i, (i1, i2) in enumerate([a for k, a in ev if k == "chamfer"], start=1):
        assert np.array_equal(i1, g["chain_cd%d_i1" % i]) and np.array_equal(i2, g["chain_cd%d_i2" % i]), i
    for i, d in enumerate(loss_list, start=1):
        assert _rel(d["training_loss"].detach().cpu().numpy(), g["chain_training_loss%d" % i]) <= 1e-5, i
    e_l = abs(float(loss.detach()) - float(g["chain_loss"])) / abs(float(g["chain_loss"]))
    assert e_l <= 1e-5, e_l
    loss.backward()
    names = [str(n) for n in g["spec_names"]]
    wn, _ = _compare_grads(dict(dec.named_parameters()), names, g["chain_grad_norms"], {})
    e_df = float(np.abs(feat.grad.cpu().numpy() - g["chain_dfeature"]).max() / np.abs(g["chain_dfeature"]).max())
    print("MEASURED chain gradients: loss %.3g, norms %.3g of scale, d feature_at_keypoint %.3g" % (e_l, wn, e_df))
    assert e_df <= 2e-3, e_df


def test_full_size_decoder_matches_the_recorded_decode_and_the_module_path(gpu_device):
    """golden_decode.npz (the shipped airplane decoder, 16 -> 256 -> 1024 -> 2048 x 6): the trainable decoder's final level against the
    recorded one as a point set (test_autoencoder_decode_matches_reference's comparison and tolerance), and its state dict in the module
    path's PointAutoencoder(None, decs): same set from its decoder level, same cloud from its decode"""
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.autoencoder import PointAutoencoder
    from oracle import denoiser_np as D
    from slide_amd.train.decoder import TrainableDecoder
    g = load_golden("golden_decode.npz")
    decs = json.loads(str(g["decoder_configs_json"]))
    spec = golden_spec(g)
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])
    dec = TrainableDecoder(decs, {n: vals["ae." + n] for n, _ in spec}).to(gpu_device)
    T = lambda a: torch.from_numpy(np.asarray(a)).to(gpu_device)
    kp, feat, lab = T(g["keypoint"]), T(g["feature"]), T(g["label"])
    B = kp.shape[0]
    start = torch.zeros(B, dtype=torch.int32, device=gpu_device)
    with torch.no_grad():
        f2, l2 = dec.decoder.decoders[0](kp, feat, T(g["level1"]), lab, start)
        f3, l3 = dec.decoder.decoders[1](T(g["level1"])[:, :, :3].contiguous(), f2, T(g["level2"]), lab, start)
        full = dec.decode(kp, feat, lab, fps_start_idx=start)[-1]
    for b in range(B):
        err, bij = D.match_point_sets(l3[b].cpu().numpy(), g["level3"][b])
        assert bij and err <= 1e-4, ("level3", err)
    assert full.shape == (B, 2048, 6)
    # a state dict saved here loads into the module path (strict), and decode there gives the same set
    ae = PointAutoencoder(None, decs, apply_kl_regularization=True)
    ae.load_state_dict({k: v.detach().cpu() for k, v in dec.state_dict().items()})
    ae = ae.to(gpu_device).eval()
    m3 = ae.decoder.decoders[1](T(g["level1"])[:, :, :3].contiguous(), f2, T(g["level2"]), label=lab, fps_start_idx=start)[1]
    mfull = ae.decode(kp, feat, label=lab, fps_start_idx=start)
    for b in range(B):
        err, bij = D.match_point_sets(l3[b].cpu().numpy(), m3[b].cpu().numpy())
        assert bij and err <= 1e-4, ("module path level3", err)
        assert D.chamfer(full[b].cpu().numpy(), mfull[b].cpu().numpy()) <= 1e-5
        assert D.chamfer(full[b].cpu().numpy(), g["level3"][b]) <= 1e-5


def test_graph_replay_equals_eager_and_sgd_lowers_the_loss(fx, gpu_device):
    """decoder_training_loss under GraphedTrainingStep unchanged: with the weights held still (SGD, lr 0) every replayed gradient
    equals the eager one within 1e-5 of scale, replay after replay; a few captured SGD steps lower the loss"""
    from slide_amd.train.graph import GraphedTrainingStep
    from slide_amd.train.losses import decoder_training_loss
    g = fx[0]
    dec = _decoder(fx, gpu_device)
    T = lambda a: torch.from_numpy(np.asarray(a)).to(gpu_device)
    kp, feat, lab, pc = T(g["keypoint"]), T(g["feature"]), T(g["label"]), T(g["pointcloud"])
    fw = g["feature_weight"].tolist()
    start = torch.zeros(kp.shape[0], dtype=torch.int32, device=gpu_device)
    fn = lambda: decoder_training_loss(dec, kp, feat, lab, pc, fw, fps_start_idx=start)[0]
    loss = fn()
    loss.backward()
    l0 = float(loss.detach())
    ref = {k: p.grad.clone() for k, p in dec.named_parameters() if p.grad is not None}
    scale = max(float(v.abs().max()) for v in ref.values())
    del loss  # (a live autograd graph keeps its gradient-accumulation nodes, which are bound to the stream they were made on)
    params = [p for p in dec.parameters()]
    step = GraphedTrainingStep(dec, torch.optim.SGD(params, lr=0.0), fn, warmup=1)
    for _ in range(3):
        l_ = step()
        worst = max(float((p.grad - ref[k]).abs().max()) for k, p in dec.named_parameters() if k in ref)
        assert worst <= 1e-5 * scale, (worst, scale)
        assert abs(float(l_) - l0) <= 1e-6 * abs(l0)
    print("MEASURED replay against eager gradients: %.3g of scale" % (worst / scale))
    step = GraphedTrainingStep(dec, torch.optim.SGD(params, lr=0.05), fn, warmup=1)
    ls = [float(step()) for _ in range(5)]
    assert np.isfinite(ls).all() and ls[-1] < ls[0] and ls[-1] < l0, (l0, ls)
