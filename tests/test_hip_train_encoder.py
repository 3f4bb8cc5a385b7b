"""GPU: the trainable encode side and the whole autoencoder (slide_amd/train/encoder.py, losses.autoencoder_training_loss,
pointnet2/train_autoencoder.py) against the reference's own training step on a reduced autoencoder with KL
(tests/golden/golden_ae_encoder_train.npz, tools/gen_golden_ae_encoder_train.py: the recorded eps of both posteriors, every farthest
point sampling started at index 0), replayed as one HIP graph, at full size against the module path's PointAutoencoder.encode, and
through the CLI.

Tolerances are those tests/test_hip_train_decoder.py holds the decoder to: forward 2e-4 max-norm, losses 1e-5 relative, gradient
norms within 1e-3 of the gradient's scale, sampled gradient entries 2e-3, replayed against eager gradients 1e-5 of scale; every
selection the reference recorded must be reproduced exactly.  Measured values: profiles/encoder_training.md."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_spec, load_golden
from slide_amd.synth import synth_state_dict
from test_hip_train_decoder import Selections, _compare_grads, _recorded, _rel, _same_selections

sys.path.insert(0, os.path.join(REPO, "pointnet2"))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    g = load_golden("golden_ae_encoder_train.npz")
    spec = golden_spec(g)
    vals = synth_state_dict([("ae." + n, s) for n, s in spec], seed=int(g["seed"]))
    return g, json.loads(str(g["encoder_config_json"])), json.loads(str(g["decoder_configs_json"])), {n: vals["ae." + n] for n, _ in spec}


def _autoencoder(fx, device):
    from slide_amd.train.encoder import TrainableAutoencoder
    g = fx[0]
    return TrainableAutoencoder(fx[1], fx[2], apply_kl_regularization=True, kl_weight=float(g["kl_weight"]),
                                feature_weight=g["feature_weight"].tolist(), state_dict=fx[3]).to(device)


def _inputs(g, device):
    T = lambda a: torch.from_numpy(np.asarray(a)).to(device)
    start = torch.zeros(g["label"].shape[0], dtype=torch.int32, device=device)
    return T(g["pointcloud"]), T(g["keypoint"]), T(g["label"]), (T(g["eps0"]), T(g["eps1"])), start


def test_training_step_matches_the_reference(fx, gpu_device, monkeypatch):
    """autoencoder_training_loss with the recorded eps: every selection, the encoder's last level, feature_at_keypoint, kl_loss, the
    levels, every level's training loss and the loss, every parameter's gradient norm and the sampled entries of the new kinds.

    MEASURED (MI355X, profiles/encoder_training.md): encoder's last level 2.65e-6, feature_at_keypoint 2.88e-6, kl_loss 1.58e-7, training
    losses 6.8e-8 / 0 / 0, loss identical, gradient norms 6.27e-7 of scale, sampled entries 3.1e-5."""
    from slide_amd.train.losses import autoencoder_training_loss
    g = fx[0]
    ae = _autoencoder(fx, gpu_device)
    pc, kp, lab, eps, start = _inputs(g, gpu_device)
    sel = Selections(monkeypatch)
    with torch.no_grad():
        feat_rows, last_xyz = ae.encoder(pc, lab)
    n_enc = len(_recorded(g, "enc"))
    _same_selections(sel.take(), _recorded(g, "enc"), "encoder")
    e_enc = _rel(feat_rows[:, :ae.encoder.out_channels].reshape(g["encoder_out"].shape).cpu().numpy(), g["encoder_out"])
    assert np.array_equal(last_xyz.cpu().numpy(), g["encoder_xyz"])
    loss, loss_list = autoencoder_training_loss(ae, pc, kp, lab, eps=eps, fps_start_idx=start)
    ev = sel.take()
    want = _recorded(g, "enc") + _recorded(g, "kp") + _recorded(g, "chain")
    _same_selections(ev[:len(want)], want, "encode + decode")
    assert n_enc and [k for k, _ in ev[len(want):]] == ["sample", "chamfer"] * 3
    _same_selections(ev[len(want)::2], [("sample", g["loss_sel%02d_sample" % i].astype(np.int64)) for i in range(3)], "loss down-sampling")
    for i, (i1, i2) in enumerate([a for k, a in ev if k == "chamfer"], start=1):
        assert np.array_equal(i1, g["cd%d_i1" % i]) and np.array_equal(i2, g["cd%d_i2" % i]), i
    e_f = _rel(loss_list[-1]["feature_at_keypoint"].cpu().numpy(), g["feature_at_keypoint"])
    e_kl = _rel(loss_list[-1]["kl_loss"].detach().cpu().numpy(), g["kl_loss"])
    e_tl = [_rel(d["training_loss"].detach().cpu().numpy(), g["training_loss%d" % i]) for i, d in enumerate(loss_list, start=1)]
    e_l = abs(float(loss.detach()) - float(g["loss"])) / abs(float(g["loss"]))
    print("MEASURED encoder step forward: encoder out %.3g, feature_at_keypoint %.3g, kl_loss %.3g, training losses %s, loss %.3g" % (
        e_enc, e_f, e_kl, " ".join("%.3g" % e for e in e_tl), e_l))
    assert e_enc <= 2e-4 and e_f <= 2e-4, (e_enc, e_f)
    assert e_kl <= 1e-5 and max(e_tl) <= 1e-5 and e_l <= 1e-5, (e_kl, e_tl, e_l)
    assert not bool(loss_list[0]["kl_loss"].any()) and not bool(loss_list[1]["kl_loss"].any())   # the KL term enters once, at the last level
    loss.backward()
    names = [str(n) for n in g["grad_names"]]
    samples = {k[len("grad__"):]: (g[k], int(g["stride__" + k[len("grad__"):]])) for k in g.files if k.startswith("grad__")}
    assert len(samples) >= 19
    wn, wf = _compare_grads(dict(ae.named_parameters()), names, g["grad_norms"], samples)
    print("MEASURED encoder step gradients: norms %.3g of scale, sampled entries %.3g" % (wn, wf))
    assert pc.grad is None and all(p.grad is None for n, p in ae.named_parameters() if ".fc_t" in n)


def test_posterior_mode_and_drawn_eps(fx, gpu_device):
    """sample_posterior=False is the posterior's mean (eps is not read); eps=None draws on the device: two calls differ, the KL term
    does not depend on the draw"""
    g = fx[0]
    ae = _autoencoder(fx, gpu_device)
    pc, kp, lab, eps, _ = _inputs(g, gpu_device)
    with torch.no_grad():
        m1, k1 = ae.encode(pc, kp, lab, eps=None, sample_posterior=False)
        m2, k2 = ae.encode(pc, kp, lab, eps=eps, sample_posterior=False)
        s1, k3 = ae.encode(pc, kp, lab)
        s2, _ = ae.encode(pc, kp, lab)
    assert torch.equal(m1, m2) and torch.equal(k1, k2) and m1.shape == (2, 16, 48)
    assert not torch.equal(s1, s2) and not torch.equal(s1, m1) and bool(torch.isfinite(s1).all())
    assert torch.equal(k1[:1], ae.encode(pc[:1], kp[:1], lab[:1], sample_posterior=False)[1])   # a sample alone: the same bits


def test_graph_replay_equals_eager(fx, gpu_device):
    """autoencoder_training_loss under GraphedTrainingStep with static eps tensors: with the weights held still (SGD, lr 0) every
    replayed gradient equals the eager one within 1e-5 of scale (measured 3.5e-7); refilling eps between replays changes the loss"""
    from slide_amd.train.graph import GraphedTrainingStep
    from slide_amd.train.losses import autoencoder_training_loss
    g = fx[0]
    ae = _autoencoder(fx, gpu_device)
    pc, kp, lab, eps, start = _inputs(g, gpu_device)
    fn = lambda: autoencoder_training_loss(ae, pc, kp, lab, eps=eps, fps_start_idx=start)[0]
    loss = fn()
    loss.backward()
    l0 = float(loss.detach())
    ref = {k: p.grad.clone() for k, p in ae.named_parameters() if p.grad is not None}
    scale = max(float(v.abs().max()) for v in ref.values())
    del loss
    step = GraphedTrainingStep(ae, torch.optim.SGD(list(ae.parameters()), lr=0.0), fn, warmup=1)
    for _ in range(2):
        l_ = step()
        worst = max(float((p.grad - ref[k]).abs().max()) for k, p in ae.named_parameters() if k in ref)
        assert worst <= 1e-5 * scale, (worst, scale)
        assert abs(float(l_) - l0) <= 1e-6 * abs(l0)
    print("MEASURED encoder step replay against eager gradients: %.3g of scale" % (worst / scale))
    for e in eps:
        e.normal_()
    l2 = float(step())
    assert np.isfinite(l2) and l2 != l0


def test_full_size_encode_matches_the_module_path_and_backward_is_finite(gpu_device):
    """the shipped encoder and level-1 configs (golden_encode.npz) at B = 2, N = 2048 -- the SA levels at their real row count (32768
    grouped rows per sample at the first level): feature_at_keypoint with sample_posterior=False against the module path's
    PointAutoencoder.encode on the same state dict (fp32 module mode), and one backward of the whole training loss

    TOLERANCE: measured once against that path: 2.1e-6 (profiles/encoder_training.md); the bound is the project's forward tolerance 2e-4
    (max-norm over the largest entry), the one the decoder test holds its levels to."""
    from models.autoencoder import PointAutoencoder
    from slide_amd.train.encoder import TrainableAutoencoder
    from slide_amd.train.losses import autoencoder_training_loss
    ge = load_golden("golden_encode.npz")
    enc, decs = json.loads(str(ge["encoder_config_json"])), json.loads(str(ge["decoder_configs_json"]))
    ref = PointAutoencoder(copy.deepcopy(enc), copy.deepcopy(decs), apply_kl_regularization=True, kl_weight=1e-5, feature_weight=[0, 0, 0.1])
    spec = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])
    sd = {n: torch.from_numpy(vals["ae." + n]) for n, _ in spec}
    ref.load_state_dict(sd)
    ref = ref.to(gpu_device).eval()
    ae = TrainableAutoencoder(enc, decs, apply_kl_regularization=True, kl_weight=1e-5, feature_weight=[0, 0, 0.1], state_dict=sd).to(gpu_device)
    T = lambda a: torch.from_numpy(np.asarray(a)).to(gpu_device)
    pc, kp, lab = T(ge["pointcloud"][:2]), T(ge["keypoint"][:2, :, :3]).contiguous(), T(ge["label"][:2])
    assert pc.shape == (2, 2048, 6)
    with torch.no_grad():
        want = ref.encode(pc, kp, ts=None, label=lab, sample_posterior=False)
        got, kl = ae.encode(pc, kp, lab, sample_posterior=False)
    err = _rel(got.cpu().numpy(), want.cpu().numpy())
    print("MEASURED full-size feature_at_keypoint against the module path: %.3g (max-norm), kl %s" % (err, kl.cpu().numpy()))
    assert got.shape == (2, 16, 48) and err <= 2e-4, err
    start = torch.zeros(2, dtype=torch.int32, device=gpu_device)
    loss, _ = autoencoder_training_loss(ae, pc, kp, lab, fps_start_idx=start)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for n, p in ae.named_parameters():
        if ".fc_t" in n:
            assert p.grad is None, n
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


def test_training_cli_checkpoints_and_resume(fx, gpu_device, tmp_path):
    """three iterations on a synthetic npz with the reduced configs: a checkpoint with the reference's keys that the module path's
    PointAutoencoder loads strictly, and a resume that continues at the next iteration"""
    from models.autoencoder import PointAutoencoder
    from test_ae_encoder_fixture_host import _write_configs
    cfg, enc, decs = _write_configs(tmp_path)
    rs = np.random.RandomState(0)
    u = rs.standard_normal((8, 400, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    np.savez(tmp_path / "clouds.npz", points=(u * rs.uniform(0.3, 0.8, (8, 1, 3))).astype(np.float32), normals=(2 * u).astype(np.float32),
             label=(np.arange(8) % 5).astype(np.int64))
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, os.path.join(REPO, "pointnet2", "train_autoencoder.py"), "-c", cfg, "--dataset_npz", str(tmp_path / "clouds.npz"),
           "--root_directory", str(tmp_path / "exp"), "--iters_per_ckpt", "3"]
    r = subprocess.run(cmd + ["--n_iters", "3"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    ckdir = tmp_path / "exp" / "ae_test" / "checkpoint"
    assert sorted(os.listdir(ckdir)) == ["pointnet_ckpt_2.pkl"], os.listdir(ckdir)
    losses = [float(l.split("loss: ")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("iteration:")]
    assert len(losses) == 3 and np.isfinite(losses).all()
    ck = torch.load(ckdir / "pointnet_ckpt_2.pkl", map_location="cpu")
    assert set(ck) == {"iter", "model_state_dict", "optimizer_state_dict", "training_time_seconds"} and ck["iter"] == 2
    ref = PointAutoencoder(enc, decs, apply_kl_regularization=True)
    ref.load_state_dict(ck["model_state_dict"], strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in ck["model_state_dict"].values())
    r2 = subprocess.run(cmd + ["--n_iters", "6"], env=env, capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr[-3000:]
    its = [int(l.split()[1]) for l in r2.stdout.splitlines() if l.startswith("iteration:")]
    assert "checkpoint of iteration 2 loaded" in r2.stdout and its == [3, 4, 5] and (ckdir / "pointnet_ckpt_5.pkl").exists()
    st = next(iter(torch.load(ckdir / "pointnet_ckpt_5.pkl", map_location="cpu")["optimizer_state_dict"]["state"].values()))
    assert int(st["step"]) == 6
