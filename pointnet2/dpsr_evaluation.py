"""Point clouds -> DPSR indicator grids: the coordinate transformations of the reference's pointnet2/dpsr_evaluation.py
(shapenet_psr_normalize lines 22-32, compute_center_and_max_length 34-43, the tail of network_output_to_dpsr_grid 77-86).  The
refine-and-upsample network in front of them and the evaluation loop behind them are not part of this build."""
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
