#!/usr/bin/env python
"""Generated point clouds -> Poisson indicator grids, on the HIP DPSR (dpsr_utils/dpsr.py): the step between the generation /
decode CLIs and the meshes (--save_mesh_dir: marching cubes on the GPU, slide_amd/mesh.py).

  --points x.npz               npz with `points` (n, N, 3) and `normals` (n, N, 3) -- what autoencoder_decode_keypoint.py writes
                               (reconstructed_pcd.npz) -- or with --split_points_to_normals `points` (n, N, 6): xyz + normals
  --explicit_normalize         normalise every cloud to the ShapeNet PSR scale (bounding box centred, longest edge 0.99) ...
  --scale S                    ... or divide by 2 S (the dataset scale the clouds were generated at; default 1)
  --grid_res 128 --psr_sigma 2 the DPSR grid and its Gaussian smoothing
  --batch_size B               clouds per DPSR call
  --save out.npz               receives `psr_grid` (n, r, r, r), `points` (n, N, 3) as DPSR saw them (in [0, 0.99]) and `normals`
  --save_mesh_dir DIR          also one triangle mesh per shape, DIR/<prefix>_<index:05d>.ply (vertices in [0, 1), with normals)
  --mesh_prefix P              ... the prefix (default mesh)
  --sample_points_from_mesh    (with --save_mesh_dir) also DIR/points_sampled_from_mesh.npz: `points`, `normals` (n, 2048, 3), 2048
                               area-weighted samples of every mesh with unit face normals, and
                               DIR/uniform_points_sampled_from_mesh.npz: 20480 samples reduced to 2048 by farthest point sampling.
                               Shape i draws under the id i, so the files do not depend on --batch_size; score them with
                               generation_evaluate.py --samples DIR/uniform_points_sampled_from_mesh.npz --ref <reference set>
  --sample_seed N              ... the seed of the draw (default 0)
  --largest_component          (with --save_mesh_dir) keep only every mesh's connected component with the most vertices (on the GPU,
                               slide_amd/mesh.py filter_components) before it is written and sampled: small blobs away from the
                               shape are dropped.  Without the flag every file is what it was
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=str, required=True, help="npz with points (+ normals)")
    ap.add_argument("--split_points_to_normals", action="store_true", help="`points` holds 6 channels: xyz + normals")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--explicit_normalize", action="store_true")
    g.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--grid_res", type=int, default=128)
    ap.add_argument("--psr_sigma", type=float, default=2)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--save", type=str, required=True)
    ap.add_argument("--save_mesh_dir", type=str, default=None, help="also write one PLY mesh per shape into this directory")
    ap.add_argument("--mesh_prefix", type=str, default="mesh")
    ap.add_argument("--sample_points_from_mesh", action="store_true", help="also sample point sets from the meshes (needs --save_mesh_dir)")
    ap.add_argument("--sample_seed", type=int, default=0)
    ap.add_argument("--largest_component", action="store_true", help="keep only every mesh's largest connected component (needs --save_mesh_dir)")
    a = ap.parse_args()
    if a.sample_points_from_mesh and not a.save_mesh_dir:
        ap.error("--sample_points_from_mesh requires --save_mesh_dir")
    if a.largest_component and not a.save_mesh_dir:
        ap.error("--largest_component requires --save_mesh_dir")

    import torch
    from dpsr_evaluation import batch_mc_from_psr, points_to_dpsr_grid
    from dpsr_utils.dpsr import DPSR

    src = np.load(a.points, allow_pickle=True)
    points = src["points"].astype(np.float32)
    if a.split_points_to_normals:
        if points.shape[2] != 6:
            raise SystemExit("--split_points_to_normals needs `points` of 6 channels, got %d" % points.shape[2])
        points, normals = points[:, :, 0:3], points[:, :, 3:6]
    elif "normals" in src.files:
        normals = src["normals"].astype(np.float32)
    else:
        raise SystemExit("%s has no `normals` (pass --split_points_to_normals for 6-channel `points`)" % a.points)
    if points.shape != normals.shape or points.shape[2] != 3:
        raise SystemExit("points %s and normals %s must both be (n, N, 3)" % (points.shape, normals.shape))
    if not torch.cuda.is_available():
        raise SystemExit("psr_grid.py needs a GPU")
    dev = torch.device("cuda:0")
    dpsr = DPSR((a.grid_res,) * 3, sig=a.psr_sigma).to(dev)
    grids, pts, sampled = [], [], []
    if a.save_mesh_dir:
        os.makedirs(a.save_mesh_dir, exist_ok=True)
    for s in range(0, points.shape[0], a.batch_size):
        grid, p, _ = points_to_dpsr_grid(torch.from_numpy(np.ascontiguousarray(points[s:s + a.batch_size])).to(dev),
                                         torch.from_numpy(np.ascontiguousarray(normals[s:s + a.batch_size])).to(dev), dpsr,
                                         scale=a.scale, explicit_normalize=a.explicit_normalize)
        grids.append(grid.cpu().numpy())
        pts.append(p.cpu().numpy())
        if a.save_mesh_dir:
            out = batch_mc_from_psr(grid, a.save_mesh_dir, a.mesh_prefix, start_idx=s, sample_points_from_mesh=a.sample_points_from_mesh,
                                    seed=a.sample_seed, largest_component=a.largest_component)
            if a.sample_points_from_mesh:
                sampled.append(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.save)), exist_ok=True)
    np.savez(a.save, psr_grid=np.concatenate(grids), points=np.concatenate(pts), normals=normals)
    print("psr_grid %s has been saved to %s" % (np.concatenate(grids).shape, a.save))
    if a.save_mesh_dir:
        print("%d meshes have been saved to %s" % (points.shape[0], a.save_mesh_dir))
    if a.sample_points_from_mesh:
        p, n, up, un = (np.concatenate([o[k] for o in sampled]) for k in range(4))
        np.savez(os.path.join(a.save_mesh_dir, "points_sampled_from_mesh.npz"), points=p, normals=n)
        np.savez(os.path.join(a.save_mesh_dir, "uniform_points_sampled_from_mesh.npz"), points=up, normals=un)
        print("point sets %s sampled from the meshes have been saved to %s" % (p.shape, a.save_mesh_dir))


if __name__ == "__main__":
    main()
