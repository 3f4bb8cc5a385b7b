"""Point clouds -> DPSR indicator grids: the coordinate transformations of the reference's pointnet2/dpsr_evaluation.py
(shapenet_psr_normalize lines 22-32, compute_center_and_max_length 34-43, the tail of network_output_to_dpsr_grid 77-86), the
refinement network's output -> DPSR grids (network_output_to_dpsr_grid 46-86: point_upsample, normalise, clamp in two launches of
slide_amd/refine.py, bit-equal to the reference's torch expressions), and DPSR grids -> meshes on disk, optionally reduced to their
largest connected component, and the point sets sampled from them (batch_mc_from_psr 291-340).  The loop that drives them over a file
of generated clouds (visualize_per_rank 176-289) is sampling_and_inference/mesh_reconstruction.py; the training-time evaluation
(evaluate_per_rank) and the autoencoder branch are not part of this build."""
import os

import numpy as np
import torch


def compute_center_and_max_length(x):
    """x (B, N, 3) -> centre of the bounding box (B, 1, 3) and its longest edge (B, 1, 1)"""
    assert x.shape[2] == 3
    minn = x.min(dim=1, keepdim=True)[0]
    maxx = x.max(dim=1, keepdim=True)[0]
    return (maxx + minn) / 2, (maxx - minn).max(dim=2, keepdim=True)[0]


def shapenet_psr_normalize(x):
    """x (B, N, 3) -> the ShapeNet PSR dataset's scale: bounding box centred, longest edge 0.99"""
    center, max_length = compute_center_and_max_length(x)
    return (x - center) / max_length * 0.99


@torch.no_grad()
def points_to_dpsr_grid(points, normals, dpsr, scale=1, explicit_normalize=False):
    """points / normals (B, N, 3) CUDA float, points roughly in [-scale, scale] -> (psr_grid (B, r, r, r), the points as DPSR saw them,
    normals).  explicit_normalize: shapenet_psr_normalize instead of the division by the dataset scale."""
    if explicit_normalize:
        points = shapenet_psr_normalize(points)
    else:
        points = points / scale / 2
    points = torch.clamp(points / 1.2 + 0.5, min=0, max=0.99).contiguous()
    return dpsr(points, normals.contiguous()), points, normals


def network_output_to_dpsr_grid(X, displacement, dpsr, scale, pointnet_config, last_dim_as_indicator=False,
                                only_original_points_split=False, explicit_normalize=False):
    """X (B, npoints, 6) CUDA float, xyz + normals (7 with last_dim_as_indicator: +1 / -1 marks original / mirrored points, and with
    only_original_points_split only the first half, the original points, is split); displacement (B, npoints, 6 k), the refinement
    network's output; pointnet_config gives point_upsample_factor, first_refine_coarse_points,
    include_displacement_center_to_final_output and output_scale_factor.  -> the reference's triple (psr_grid = dpsr(points, normals),
    the refined points in [0, 0.99] as DPSR saw them, the refined normals).  ValueError for a non-finite refined point or, with
    explicit_normalize, a sample whose refined points coincide (the reference returns NaN grids)."""
    from slide_amd.refine import refine_to_dpsr_points
    points, normals, _ = refine_to_dpsr_points(
        X, displacement, pointnet_config["point_upsample_factor"],
        first_refine_coarse_points=pointnet_config.get("first_refine_coarse_points", False),
        include_displacement_center_to_final_output=pointnet_config.get("include_displacement_center_to_final_output", False),
        output_scale_factor=pointnet_config.get("output_scale_factor", 0.001), scale=scale, explicit_normalize=explicit_normalize,
        last_dim_as_indicator=last_dim_as_indicator, only_original_points_split=only_original_points_split)
    return dpsr(points, normals), points, normals


def batch_mc_from_psr(psr_grid, save_dir, save_prefix, batch_info=None, start_idx=0, sample_points_from_mesh=False,
                      return_original_scale=False, original_center=None, original_max_length=None, seed=0, num_samples=2048,
                      num_dense=20480, largest_component=False):
    """marching cubes of psr_grid (B, res, res, res) and one PLY per shape: <save_prefix>_<start_idx + i:05d>.ply under save_dir (or
    <batch_info[i]>_<...>.ply).  The vertices are in [0, 1) (divided by res); with return_original_scale the mesh's bounding box is
    mapped to original_center (B, 1, 3) and original_max_length (B, 1, 1).  Returns the reference's four results; they are empty
    lists unless sample_points_from_mesh is set (CUDA grids only), and then numpy arrays (B, num_samples, 3) float32:

      points, normals                  num_samples area-weighted samples of every mesh as written to disk, with unit face normals
                                       (slide_amd.mesh.sample_points_from_meshes, noise stream 0)
      uniform points, uniform normals  num_dense samples (noise stream 1) reduced to num_samples by farthest point sampling from
                                       sample 0 -- the samples are i.i.d., so that is a random point -- and their normals

    One sampling call serves the batch.  Mesh i draws with the id start_idx + i under `seed`: a shape's samples do not depend on
    how the shapes are split into batches.  (The reference samples with torch's global generator, one mesh at a time, and starts
    the farthest point sampling at a random index.)

    largest_component: every mesh is reduced to its connected component with the most vertices (slide_amd.mesh.filter_components, one
    call for the batch; the reference's verts_on_largest_mesh) directly after extraction: the bounding box of return_original_scale,
    the PLY and the samples are the kept component's.  Mesh ids and seeds are unchanged."""
    from dpsr_utils.io_utils import save_mesh
    from dpsr_utils.utils import mc_from_psr
    if sample_points_from_mesh and not psr_grid.is_cuda:
        raise NotImplementedError("batch_mc_from_psr: sampling points from the meshes runs on the GPU only (no CPU path)")
    vs, fs, ns = mc_from_psr(psr_grid, zero_level=0)  # (one launch sequence for the batch; a grid's mesh does not depend on it)
    dev = psr_grid.device

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev).reshape(-1, 3)

    if largest_component:
        from slide_amd import mesh
        kept = mesh.filter_components([(up(v, np.float32), up(f, np.int32), up(n, np.float32)) for v, f, n in zip(vs, fs, ns)],
                                      keep="largest", by="verts")
        vs, fs, ns = ([k[j].cpu().numpy() for k in kept] for j in range(3))
    scaled = []
    for i, (v, f, n) in enumerate(zip(vs, fs, ns)):
        if return_original_scale:
            box = torch.from_numpy(np.ascontiguousarray(v)).to(psr_grid.device)[None]
            center, max_length = compute_center_and_max_length(box)
            box = (box - center) / max_length * original_max_length[i:i + 1] + original_center[i:i + 1]
            v = box[0].cpu().numpy()
        stem = save_prefix if batch_info is None else batch_info[i]
        save_mesh(os.path.join(save_dir, "%s_%05d.ply" % (stem, start_idx + i)), v, f, normals=n)
        scaled.append(v)
    if not sample_points_from_mesh:
        return [], [], [], []
    from slide_amd import _ext, mesh
    meshes = [(up(v, np.float32), up(f, np.int32), up(n, np.float32)) for v, f, n in zip(scaled, fs, ns)]
    ids = [start_idx + i for i in range(len(meshes))]
    points, normals = mesh.sample_points_from_meshes(meshes, num_samples, return_normals=True, seed=seed, mesh_ids=ids, stream_id=0)
    dense, dense_n = mesh.sample_points_from_meshes(meshes, num_dense, return_normals=True, seed=seed, mesh_ids=ids, stream_id=1)
    uniform, sel = _ext.sample_farthest_points(dense, K=num_samples, start_idx=torch.zeros(len(meshes), dtype=torch.int64, device=dev))
    uniform_n = torch.gather(dense_n, 1, sel.unsqueeze(-1).expand(-1, -1, 3))
    return tuple(t.cpu().numpy() for t in (points, normals, uniform, uniform_n))
