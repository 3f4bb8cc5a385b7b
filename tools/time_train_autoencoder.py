"""Times the whole autoencoder's training step and the two encode-side kernel pairs on the GPU (numbers: profiles/encoder_training.md).

  1. eager and graphed (slide_amd.train.graph.GraphedTrainingStep, static eps tensors refilled between replays) step time of
     autoencoder_training_loss + backward + Adam at batch 32 on the shipped airplane configs (the configs
     tests/golden/golden_encode.npz records: 2048 x 6 -> 1024 -> 256 -> 64 -> 32 -> 16 key points x 48 -> 256 -> 1024 -> 2048 x 6),
     synthetic weights and clouds;
  2. slide_col_max_seg (+ backward) against torch's amax / argmax + scatter, and slide_gauss_posterior_fwd / _bwd against the
     elementwise torch expression of DiagonalGaussianDistribution with autograd, at the product's shapes.  These tensors are small:
     the table shows launch-bound microseconds, not throughput.

usage:  python tools/time_train_autoencoder.py [--batch 32] [--steps 5] [--skip-step] [--out FILE]
Every timing is the median over `--repeats` windows of device time between two events, after warm-up launches."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.time_train_decoder import _median_ms  # noqa: E402


def time_kernels(B, repeats):
    from slide_amd.train import functions as F
    dev = torch.device("cuda:0")
    rows = []
    for S, C in ((16, 32), (16, 64), (2048, 64)):     # Pnet2Stage's maxima at the key-point level; a whole input cloud for scale
        ld = F.ru(C)
        x = torch.randn(B * S, ld, device=dev).requires_grad_(True)
        w = torch.randn(B, ld, device=dev)

        def ours():
            x.grad = None
            (F.col_max_seg(x, B, S, C)[0] * w).sum().backward()

        def ref():
            x.grad = None
            (x.view(B, S, ld).amax(dim=1) * w).sum().backward()

        rows.append(dict(op="col_max_seg fwd+bwd", B=B, S=S, C=C, ours_us=round(_median_ms(ours, 50, repeats) * 1e3, 2),
                         torch_us=round(_median_ms(ref, 50, repeats) * 1e3, 2)))
        print(json.dumps(rows[-1]), flush=True)
    for S, C in ((16, 16), (16, 32)):                  # the two posteriors of the key-point level
        p = torch.randn(B * S, F.ru(2 * C), device=dev).requires_grad_(True)
        eps = torch.randn(B * S, F.ru(C), device=dev)

        def ours():
            p.grad = None
            z, kl = F.gauss_posterior(p, eps, B, S, C)
            (z.sum() + kl.sum()).backward()

        def ref():
            p.grad = None
            mean, logvar = p[:, :C], torch.clamp(p[:, C:2 * C], -30.0, 20.0)
            z = mean + torch.exp(0.5 * logvar) * eps[:, :C]
            kl = 0.5 * torch.sum((mean.pow(2) + torch.exp(logvar) - 1.0 - logvar).reshape(B, S * C), dim=1)
            (z.sum() + kl.sum()).backward()

        rows.append(dict(op="gauss_posterior fwd+bwd", B=B, S=S, C=C, ours_us=round(_median_ms(ours, 50, repeats) * 1e3, 2),
                         torch_us=round(_median_ms(ref, 50, repeats) * 1e3, 2)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def time_step(B, steps, repeats):
    from slide_amd.synth import synth_keypoints, synth_state_dict
    from slide_amd.train.encoder import TrainableAutoencoder
    from slide_amd.train.graph import GraphedTrainingStep
    from slide_amd.train.losses import autoencoder_training_loss
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "golden_encode.npz"))
    enc, decs = json.loads(str(g["encoder_config_json"])), json.loads(str(g["decoder_configs_json"]))
    ae = TrainableAutoencoder(enc, decs, apply_kl_regularization=True, kl_weight=1e-5, feature_weight=[0, 0, 0.1])
    vals = synth_state_dict([("ae." + k, tuple(v.shape)) for k, v in ae.state_dict().items()])
    ae.load_state_dict({k: torch.from_numpy(vals["ae." + k]) for k in ae.state_dict()})
    ae = ae.to(dev)
    rs = np.random.RandomState(0)
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
    kp = T(synth_keypoints(B, 16, seed=3)[:, :, :3].astype(np.float32)).contiguous()
    label = torch.zeros(B, dtype=torch.int64, device=dev)
    u = rs.standard_normal((B, 2048, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    pc = T(np.concatenate([u * np.array([0.9, 0.35, 0.6]), u], axis=2).astype(np.float32))
    eps = tuple(torch.randn(s, device=dev) for s in ae.posterior_shapes(B, 16))
    fn = lambda: autoencoder_training_loss(ae, pc, kp, label, eps=eps)[0]
    opt = torch.optim.Adam(ae.parameters(), lr=1e-5, capturable=True)

    def eager():
        opt.zero_grad(set_to_none=True)
        fn().backward()
        opt.step()

    res = dict(batch=B, eager_ms=round(_median_ms(eager, steps, repeats, warmup=2), 2))
    print(json.dumps(res), flush=True)
    step = GraphedTrainingStep(ae, opt, fn, warmup=1)

    def replay():
        for e in eps:
            e.normal_()
        step()

    res["graph_ms"] = round(_median_ms(replay, steps, repeats, warmup=2), 2)
    res["loss_finite"] = bool(torch.isfinite(step()))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", type=str, default=None, help="also write the results as JSON to this file")
    a = ap.parse_args()
    out = {"kernels": time_kernels(a.batch, a.repeats)}
    if not a.skip_step:
        out["step"] = time_step(a.batch, a.steps, a.repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
