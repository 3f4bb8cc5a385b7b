"""Chamfer distance / F-score between two sets of point clouds stored as npz files (reference: pointnet2/load_evaluate.py), on the
GPU.  Pair i is ( dir1's points[i], dir2's points[i] ); both sets are normalised as the reference does, scored in batches by
metrics_point_cloud.chamfer_and_f1.calc_cd (fused HIP Chamfer kernels), and the means and per-pair arrays are printed.

The reference script does not run as written (it unpacks three values from pytorch3d 0.7's chamfer_distance, which returns two, and
hands numpy arrays to torch code); this is a working port with the same flags.  Flags parsed with `type=bool` keep the reference's
behaviour: argparse's bool() of a non-empty string is True, so `--normalize False` still normalises; pass an EMPTY string
(`--normalize ''`) to switch one off.

usage:  python pointnet2/load_evaluate.py --dir1 a.npz --dir2 b.npz [--threshold 1e-4] [--batch 256] [--save metrics.npz]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

BOOL_QUIRK = " (type=bool as in the reference: any non-empty value, 'False' included, is True; pass '' for False)"


def normalize_point_cloud(all_points, normalize_std_per_axis=True, normalize_per_shape=True, all_points_mean=None,
                          all_points_std=None, input_dim=3, box_per_shape=False):
    """zero mean, unit standard deviation (reference load_evaluate.py:42-75): per shape or over the whole set, per axis or one
    scale; box_per_shape: min corner to 0, extent to 1; given mean and std are used as they are.  numpy in, numpy out."""
    p = all_points
    if all_points_mean is not None and all_points_std is not None:
        return (p - all_points_mean) / all_points_std
    B = p.shape[0]
    if normalize_per_shape:  # statistics of every shape: over its points
        shift = p.mean(axis=1, keepdims=True)
        scale = p.std(axis=1, keepdims=True) if normalize_std_per_axis else p.reshape(B, -1).std(axis=1)[:, None, None]
    elif box_per_shape:  # bounding box of every shape: min corner -> 0, extent -> 1
        shift = p.min(axis=1, keepdims=True)
        scale = p.max(axis=1, keepdims=True) - shift
    else:  # statistics of the whole set
        rows = p.reshape(-1, input_dim)
        shift = rows.mean(axis=0)[None, None]
        scale = rows.std(axis=0)[None, None] if normalize_std_per_axis else p.reshape(-1).std()[None, None, None]
    return (p - shift) / scale


def build_parser():
    p = argparse.ArgumentParser(description="Chamfer distance (cd_p, cd_t) and F-score between the i-th clouds of two npz files "
                                            "(key 'points', (S, N, 3)), on the GPU")
    p.add_argument('--dir1', type=str, default='data/pointflow_1.npz', help="first npz file (key 'points')")
    p.add_argument('--dir2', type=str, default='data/pointflow_2.npz', help="second npz file (key 'points')")
    p.add_argument('--threshold', type=float, default=0.0001, help="F-score threshold on the SQUARED distance")
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--normalize', type=bool, default=True, help="normalise both sets" + BOOL_QUIRK)
    p.add_argument('--normalize_std_per_axis', type=bool, default=True, help="one std per axis" + BOOL_QUIRK)
    p.add_argument('--normalize_per_shape', type=bool, default=True, help="statistics per shape, not over the set" + BOOL_QUIRK)
    p.add_argument('--batch', type=int, default=256, help="pairs scored per launch")
    p.add_argument('--save', type=str, default=None, help="write cd_p / cd_t / f1 per pair to this npz file")
    return p


def evaluate(p1, p2, threshold=0.0001, device='cuda:0', batch=256):
    """per-pair cd_p, cd_t, f1 (numpy float32, (S,)) of the clouds p1 (S,N1,3) and p2 (S,N2,3) -- Chamfer_F1()(p1, p2) in batches"""
    import torch
    from metrics_point_cloud.chamfer_and_f1 import calc_cd
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("the two sets hold %d and %d clouds" % (p1.shape[0], p2.shape[0]))
    dev = torch.device(device)
    out = {"cd_p": [], "cd_t": [], "f1": []}
    with torch.no_grad():
        for s in range(0, p1.shape[0], batch):
            a = torch.from_numpy(np.ascontiguousarray(p1[s:s + batch], dtype=np.float32)).to(dev)
            b = torch.from_numpy(np.ascontiguousarray(p2[s:s + batch], dtype=np.float32)).to(dev)
            r = calc_cd(a, b, calc_f1=True, f1_threshold=threshold)
            for k in out:
                out[k].append(r[k])
        return {k: torch.cat(v).cpu().numpy() for k, v in out.items()}


def main(argv=None):
    args = build_parser().parse_args(argv)
    p1 = np.load(args.dir1)['points']
    p2 = np.load(args.dir2)['points']
    if args.normalize:
        p1 = normalize_point_cloud(p1, args.normalize_std_per_axis, args.normalize_per_shape)
        p2 = normalize_point_cloud(p2, args.normalize_std_per_axis, args.normalize_per_shape)
    r = evaluate(p1, p2, args.threshold, args.device, args.batch)
    np.set_printoptions(threshold=20)
    for k in ("cd_p", "cd_t", "f1"):
        print('%s: mean %.6e' % (k, float(r[k].mean())))
        print('%s per pair: %s' % (k, r[k]))
    if args.save:
        np.savez(args.save, **r)
        print('saved', args.save)
    return r


if __name__ == "__main__":
    main()
