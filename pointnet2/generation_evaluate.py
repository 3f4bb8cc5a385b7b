"""Scores a set of generated point clouds against a reference set on the GPU: MMD-CD, COV-CD and 1-NNA-CD
(metrics_point_cloud.generation_metrics.compute_all_metrics; reference: pointnet2/models/pvd/metrics/evaluation_metrics.py, CD half).

Both sets are npz files with the clouds under one key ((S, N, C >= 3), xyz first) -- the layout the generation CLIs write and
load_evaluate.py reads.  With --normalize both sets are normalised by load_evaluate.normalize_point_cloud (per shape, one standard
deviation per axis by default) before scoring.  Prints the six numbers and the wall time; --save writes them as JSON.
With --jsd the result also carries JSD, the Jensen-Shannon divergence between the two sets' occupancy distributions on a
--jsd_resolution^3 grid clipped to the unit sphere (generation_metrics.jsd_between_point_cloud_sets), computed after --normalize.
With --emd it also carries the six EMD keys (MMD-EMD, COV-EMD, 1-NNA-EMD: compute_all_metrics(emd=True)), which cost far more
than the Chamfer ones.

usage:  python pointnet2/generation_evaluate.py --samples generated.npz --ref reference.npz [--key points] [--normalize]
            [--normalize_std_per_axis 0|1] [--normalize_per_shape 0|1] [--jsd [--jsd_resolution 28]] [--emd] [--device cuda:0]
            [--save metrics.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

KEYS = ("lgan_mmd-CD", "lgan_cov-CD", "lgan_mmd_smp-CD", "1-NN-CD-acc_t", "1-NN-CD-acc_f", "1-NN-CD-acc")
EMD_KEYS = tuple(k.replace("-CD", "-EMD") for k in KEYS)


def build_parser():
    p = argparse.ArgumentParser(description="MMD-CD / COV-CD / 1-NNA-CD of a generated set against a reference set, on the GPU")
    p.add_argument('--samples', type=str, required=True, help="npz file of the generated clouds")
    p.add_argument('--ref', type=str, required=True, help="npz file of the reference clouds")
    p.add_argument('--key', type=str, default='points', help="array name in both files")
    p.add_argument('--normalize', action='store_true', help="normalise both sets (load_evaluate.normalize_point_cloud)")
    p.add_argument('--normalize_std_per_axis', type=int, default=1, choices=(0, 1), help="one std per axis (1) or one scale (0)")
    p.add_argument('--normalize_per_shape', type=int, default=1, choices=(0, 1),
                   help="statistics per shape (1) or over the whole set (0)")
    p.add_argument('--jsd', action='store_true', help="also report JSD (occupancy grid clipped to the unit sphere)")
    p.add_argument('--jsd_resolution', type=int, default=28, help="grid resolution of --jsd (2 to 32)")
    p.add_argument('--emd', action='store_true', help="also report MMD-EMD / COV-EMD / 1-NNA-EMD (approximate Earth Mover's Distance)")
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--save', type=str, default=None, help="write the metrics to this JSON file")
    return p


def evaluate(samples, refs, device='cuda:0', jsd_resolution=None, emd=False):
    """the six metrics (python floats) of the clouds samples (S, N, C) against refs (R, N', C), numpy arrays; with jsd_resolution
    also 'JSD' on a grid of that resolution; with emd also the six EMD keys"""
    import torch
    from metrics_point_cloud.generation_metrics import compute_all_metrics, jsd_between_point_cloud_sets
    dev = torch.device(device)
    s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).to(dev)
    r = torch.from_numpy(np.ascontiguousarray(refs, dtype=np.float32)).to(dev)
    res = compute_all_metrics(s, r, emd=True) if emd else compute_all_metrics(s, r)
    out = {k: float(res[k]) for k in KEYS + (EMD_KEYS if emd else ())}
    if jsd_resolution is not None:
        out["JSD"] = float(jsd_between_point_cloud_sets(s, r, jsd_resolution))
    return out


def main(argv=None):
    from load_evaluate import normalize_point_cloud
    args = build_parser().parse_args(argv)
    samples = np.load(args.samples)[args.key]
    refs = np.load(args.ref)[args.key]
    if args.normalize:
        samples = normalize_point_cloud(samples, bool(args.normalize_std_per_axis), bool(args.normalize_per_shape),
                                        input_dim=samples.shape[2])
        refs = normalize_point_cloud(refs, bool(args.normalize_std_per_axis), bool(args.normalize_per_shape),
                                     input_dim=refs.shape[2])
    t0 = time.perf_counter()
    res = evaluate(samples, refs, args.device, args.jsd_resolution if args.jsd else None, args.emd)
    dt = time.perf_counter() - t0
    print('%d samples x %d references' % (samples.shape[0], refs.shape[0]))
    for k in KEYS + (EMD_KEYS if args.emd else ()) + (("JSD",) if args.jsd else ()):
        print('%-16s %.9e' % (k, res[k]))
    print('wall time %.3f s' % dt)
    if args.save:
        with open(args.save, 'w') as f:
            json.dump(res, f, indent=1)
        print('saved', args.save)
    return res


if __name__ == "__main__":
    main()
