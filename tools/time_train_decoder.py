"""Times the decode-side training step and the per-sample column-sum kernel on the GPU (numbers: profiles/decoder_training.md).

  1. eager and graphed (slide_amd.train.graph.GraphedTrainingStep) step time of decoder_training_loss + backward + SGD at batch 32 for
     the shipped airplane decoder configs (16 -> 256 -> 1024 -> 2048 x 6; the configs tests/golden/golden_decode.npz records),
     synthetic weights, synthetic key points / latents / target clouds;
  2. slide_col_sums_seg (functions.col_sums_seg) against torch's x.view(B, S, ld).sum(1) at the (S, ld) pairs that decoder's Mlps
     reach at batch 32 (S = centres x neighbours of a set-abstraction level, or the points of an FP level's second Mlp).

usage:  python tools/time_train_decoder.py [--batch 32] [--steps 10] [--skip-step]
Every timing is the median over `--repeats` windows of device time between two events, after warm-up launches."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PAIRS = ((8192, 32), (4096, 32), (2048, 64), (512, 128), (1024, 64), (256, 64), (256, 128), (128, 128), (64, 256), (16, 256))


def _median_ms(fn, iters, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out))


def time_kernel(B, repeats):
    from slide_amd.train.functions import col_sums_seg
    dev = torch.device("cuda:0")
    rows = []
    for S, ld in PAIRS:
        x = torch.randn(B * S, ld, device=dev)
        ours = _median_ms(lambda: col_sums_seg(x, B, S), 50, repeats)
        ref = _median_ms(lambda: x.view(B, S, ld).sum(1), 50, repeats)
        err = float((col_sums_seg(x, B, S) - x.double().view(B, S, ld).sum(1)).abs().max())
        gbs = B * S * ld * 4 / (ours * 1e-3) / 1e9
        rows.append(dict(S=S, ld=ld, B=B, col_sums_seg_us=round(ours * 1e3, 2), torch_sum_us=round(ref * 1e3, 2), read_GBps=round(gbs, 1),
                         max_abs_err_vs_f64=err))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def time_step(B, steps, repeats):
    from slide_amd.synth import synth_keypoints, synth_state_dict
    from slide_amd.train.decoder import TrainableDecoder
    from slide_amd.train.graph import GraphedTrainingStep
    from slide_amd.train.losses import decoder_training_loss
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "golden_decode.npz"))
    decs = json.loads(str(g["decoder_configs_json"]))
    spec = [(str(n), tuple(int(x) for x in str(s).split(","))) for n, s in zip(g["spec_names"], g["spec_shapes"])]
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])
    dec = TrainableDecoder(decs, {n: vals["ae." + n] for n, _ in spec}).to(dev)
    rs = np.random.RandomState(0)
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
    kp = T(synth_keypoints(B, 16, seed=3))
    feat = T((0.5 * rs.standard_normal((B, 16, 48))).astype(np.float32))
    label = torch.zeros(B, dtype=torch.int64, device=dev)
    u = rs.standard_normal((B, 2048, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    pc = T(np.concatenate([u * np.array([0.9, 0.35, 0.6]), u], axis=2).astype(np.float32))
    fn = lambda: decoder_training_loss(dec, kp, feat, label, pc, [0.0, 0.0, 0.1])[0]
    opt = torch.optim.SGD(dec.parameters(), lr=1e-4)

    def eager():
        opt.zero_grad(set_to_none=True)
        fn().backward()
        opt.step()

    e = _median_ms(eager, steps, repeats, warmup=2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    step = GraphedTrainingStep(dec, opt, fn, warmup=1)
    gms = _median_ms(step, steps, repeats, warmup=2)
    row = dict(batch=B, eager_step_ms=round(e, 2), graphed_step_ms=round(gms, 2), peak_GiB=round(peak, 2), loss=float(step.loss))
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    time_kernel(a.batch, a.repeats)
    if not a.skip_step:
        time_step(a.batch, a.steps, a.repeats)
