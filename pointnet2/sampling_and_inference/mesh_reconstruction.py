#!/usr/bin/env python
"""Generated point clouds -> refined, up-sampled clouds -> DPSR grids -> meshes and the point sets sampled from them: the reference's
sampling_and_inference/mesh_reconstruction.py (main + dpsr_evaluation.visualize_per_rank) on the HIP kernels.  Per batch:

  compute_center_and_max_length of the input cloud (the mesh is mapped back to it), normals normalised (or zeroed when the
  configuration's include_normals is false), mirror_and_concat when dpsr_config.mirror_before_upsampling is set, the refinement
  network (PointNet2CloudCondition with the up-sampling head, no timestep), network_output_to_dpsr_grid(explicit_normalize=True),
  batch_mc_from_psr(sample_points_from_mesh=True, return_original_scale=True).

  -c / --config                the reference's JSON (refine_and_upsample_configs/...)
  --ckpt                       checkpoint with `model_state_dict`
  --dataset_path x.npz         `points` (n, N, 3) and `normals` (n, N, 3) (or, with --split_points_to_normals, `points` (n, N, 6)),
                               optionally `label` (n,); without it every cloud gets --label_number
  --save_dir DIR               output goes to DIR/<npz stem>/visualization_results_at_iteration_00000000_epoch_0000/:
                                 reconstructed_mesh/reconstructed_mesh_<index:05d>.ply
                                 points_sampled_from_mesh.npz, uniform_points_sampled_from_mesh.npz   points, normals, label
                                 noisy_pcd.npz, refined_pcd.npz   points, normals (the network's input and the refined cloud as
                                 DPSR saw it; the reference writes one PLY per shape instead)
  --batch_size B               clouds per batch (default: the configuration's eval_batch_size)
  --seed N                     seeds the input noise, the permutation of the mirrored cloud and the samples drawn from the meshes
  --noise_magnitude S          noise added to points and normals, as the reference's dataset does (default: the configuration's
                               augmentation.noise_magnitude); shape i draws from numpy RandomState([seed, i])
  --largest_component          keep only every mesh's largest connected component
  --prec fp32|mixed            arithmetic of the network's module path, as in the other CLIs

Every output of a shape is a function of (cloud, seed, shape index) alone: the files do not depend on --batch_size.  (The reference
permutes with torch's global generator and draws its noise from per-worker numpy generators.)  Score the result with
generation_evaluate.py --samples DIR/.../uniform_points_sampled_from_mesh.npz --ref <reference set>."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VIS_DIR = "visualization_results_at_iteration_%s_epoch_%s" % (str(0).zfill(8), str(0).zfill(4))


def load_dataset(path, scale, noise_magnitude, seed, split_points_to_normals):
    """the reference's GeneralNpzDataset: `points` scaled by the dataset scale, noise on `points` and `normals`; shape i draws its noise
    from RandomState([seed, i]), points first"""
    src = np.load(path, allow_pickle=True)
    data = {k: src[k] for k in src.files}
    if split_points_to_normals:
        pts = data["points"]
        if pts.shape[-1] < 6:
            raise SystemExit("--split_points_to_normals needs `points` of 6 channels, got %d" % pts.shape[-1])
        data["points"], data["normals"] = pts[..., 0:3], pts[..., 3:6]
    data["points"] = data["points"] * scale
    if noise_magnitude > 0:
        for key in ("points", "normals"):
            if key in data:
                data[key] = np.array(data[key])
        for i in range(data["points"].shape[0]):
            rs = np.random.RandomState([int(seed), i])
            for key in ("points", "normals"):
                if key in data:
                    data[key][i] = data[key][i] + noise_magnitude * rs.randn(*data[key][i].shape).astype(data[key].dtype)
    return data


def refuse_unsupported(config):
    if "autoencoder_config" in config or config.get("dpsr_config", {}).get("use_autoencoder", False):
        raise NotImplementedError("mesh_reconstruction.py: the autoencoder branch (use_autoencoder) is not part of this build")
    if config.get("dpsr_config", {}).get("split_before_refine", False):
        raise NotImplementedError("mesh_reconstruction.py: dpsr_config.split_before_refine is not part of this build")


def network_input(points, normals, trainset_config, dpsr_config, seed):
    """points, normals (B, N, 3) CUDA -> the refinement network's input X and whether its last channel is the original / mirrored tag"""
    import torch
    from data_utils.mirror_partial import mirror_and_concat
    if trainset_config.get("include_normals", True):
        normals = normals / torch.norm(normals, p=2, dim=2, keepdim=True)
        X = torch.cat([points, normals], dim=2)
    else:
        X = torch.cat([points, torch.zeros_like(points)], dim=2)  # the network estimates the normals
    mirrored = dpsr_config.get("mirror_before_upsampling", False)
    if mirrored:
        X = mirror_and_concat(X, axis=2, num_points=[], attach_label=True, permute=not dpsr_config.get("only_original_points_split", False),
                              seed=seed)[0]
    return X.contiguous(), mirrored


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", type=str, required=True, help="JSON file for configuration")
    ap.add_argument("--ckpt", type=str, required=True, help="the checkpoint to use")
    ap.add_argument("--dataset_path", type=str, required=True, help="npz with the point clouds to reconstruct meshes for")
    ap.add_argument("--save_dir", type=str, default="dpsr_reconstruct_mesh", help="the directory to save meshes")
    ap.add_argument("--split_points_to_normals", action="store_true", help="split `points` of the npz file into points and normals")
    ap.add_argument("--label_number", type=int, default=-1, help="the label of the clouds when the npz file has no `label`")
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise_magnitude", type=float, default=None)
    ap.add_argument("--largest_component", action="store_true")
    ap.add_argument("--prec", default="mixed", choices=["mixed", "fp32"], help="module-path arithmetic, as in the generation CLIs")
    a = ap.parse_args()
    from slide_amd.generation import module_prec_of
    os.environ["SLIDE_MODULE_PREC"] = module_prec_of(a.prec)  # (read when the layers are built and when they run)

    import torch
    from dpsr_evaluation import batch_mc_from_psr, compute_center_and_max_length, network_output_to_dpsr_grid
    from dpsr_utils.dpsr import DPSR
    from models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from slide_amd.checkpoint import load_model_state_dict
    from slide_amd.json_reader import read_json_file

    config = read_json_file(a.config)
    refuse_unsupported(config)
    train_config, pointnet_config, dpsr_config = config["train_config"], config["pointnet_config"], config["dpsr_config"]
    if train_config["dataset"] != "shapenet_psr_dataset":
        raise SystemExit("%s dataset is not supported" % train_config["dataset"])
    trainset_config = config["shapenet_psr_dataset_config"]
    scale = trainset_config["scale"]
    noise = trainset_config["augmentation"]["noise_magnitude"] if a.noise_magnitude is None else a.noise_magnitude
    batch_size = int(trainset_config["eval_batch_size"]) if a.batch_size is None else a.batch_size
    if batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    if not torch.cuda.is_available():
        raise SystemExit("mesh_reconstruction.py needs a GPU")
    dev = torch.device("cuda:0")

    data = load_dataset(a.dataset_path, scale, noise, a.seed, a.split_points_to_normals)
    points = np.ascontiguousarray(data["points"], dtype=np.float32)
    n = points.shape[0]
    include_normals = trainset_config.get("include_normals", True)
    if include_normals and "normals" not in data:
        raise SystemExit("%s has no `normals` (pass --split_points_to_normals for 6-channel `points`)" % a.dataset_path)
    normals = np.ascontiguousarray(data["normals"], dtype=np.float32) if include_normals else np.zeros_like(points)
    if "label" in data:
        label = np.asarray(data["label"]).astype(np.int64)
    elif a.label_number >= 0:
        label = np.full(n, a.label_number, np.int64)
    else:
        raise SystemExit("%s has no `label`: pass --label_number" % a.dataset_path)

    net = PointNet2CloudCondition(pointnet_config)
    net.load_state_dict(load_model_state_dict(a.ckpt))
    net = net.to(dev).eval()
    r = dpsr_config["grid_res"]
    dpsr = DPSR((r, r, r), sig=dpsr_config["psr_sigma"]).to(dev)

    stem = os.path.splitext(os.path.split(a.dataset_path)[1])[0]
    out_dir = os.path.join(a.save_dir, stem, VIS_DIR)
    mesh_dir = os.path.join(out_dir, "reconstructed_mesh")
    os.makedirs(mesh_dir, exist_ok=True)
    print("visualization results will be saved to the folder", out_dir)
    only_orig = dpsr_config.get("only_original_points_split", False)
    kept = {k: [] for k in ("noisy_p", "noisy_n", "refined_p", "refined_n", "p", "n", "up", "un")}
    with torch.no_grad():
        for s in range(0, n, batch_size):
            P = torch.from_numpy(points[s:s + batch_size]).to(dev)
            center, max_length = compute_center_and_max_length(P)
            X, mirrored = network_input(P, torch.from_numpy(normals[s:s + batch_size]).to(dev), trainset_config, dpsr_config, a.seed)
            displacement = net(X, None, ts=None, label=torch.from_numpy(label[s:s + batch_size]).to(dev))
            psr_grid, refined_points, refined_normals = network_output_to_dpsr_grid(
                X, displacement.contiguous(), dpsr, scale, pointnet_config, last_dim_as_indicator=mirrored,
                only_original_points_split=only_orig, explicit_normalize=True)
            sampled = batch_mc_from_psr(psr_grid, mesh_dir, "reconstructed_mesh", start_idx=s, sample_points_from_mesh=True,
                                        return_original_scale=True, original_center=center, original_max_length=max_length,
                                        seed=a.seed, largest_component=a.largest_component)
            for k, v in zip(("noisy_p", "noisy_n", "refined_p", "refined_n"), (X[:, :, 0:3], X[:, :, 3:6], refined_points, refined_normals)):
                kept[k].append(v.cpu().numpy())
            for k, v in zip(("p", "n", "up", "un"), sampled):
                kept[k].append(v)
    cat = {k: np.concatenate(v) for k, v in kept.items()}
    np.savez(os.path.join(out_dir, "noisy_pcd.npz"), points=cat["noisy_p"], normals=cat["noisy_n"])
    np.savez(os.path.join(out_dir, "refined_pcd.npz"), points=cat["refined_p"], normals=cat["refined_n"])
    np.savez(os.path.join(out_dir, "points_sampled_from_mesh.npz"), points=cat["p"], normals=cat["n"], label=label)
    np.savez(os.path.join(out_dir, "uniform_points_sampled_from_mesh.npz"), points=cat["up"], normals=cat["un"], label=label)
    print("%d meshes and the point sets %s sampled from them have been saved to %s" % (n, cat["p"].shape, out_dir))


if __name__ == "__main__":
    main()
