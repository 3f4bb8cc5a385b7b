"""The reference's pointnet2/data_utils/mirror_partial.py on the HIP kernels of slide_amd/refine.py: mirror a cloud across the plane
through its centroid, tag and concatenate the two halves, down-sample the result by farthest point sampling.

Differences from the reference, none in what is computed: the centroid is summed in double and rounded once (the reference's float32
torch.mean is within rounding of it), and the permutation is the one of `seed` (slide_amd.refine.refine_permutation: a CPU
torch.Generator, so a run's clouds do not depend on torch's global generator or on how they are batched) instead of a global
torch.randperm per call."""
import torch
from pointnet2_ops import pointnet2_utils

from slide_amd import refine


def mirror(partial, axis=1):
    """partial (B, N, F) CUDA float, xyz first and normals in channels 3..5 when F >= 6 -> the cloud mirrored across the plane through
    its centroid normal to `axis`"""
    out, _ = refine.mirror_and_concat(partial, axis=axis, attach_label=False, perm=None)
    return out[:, partial.shape[1]:, :].contiguous()


def down_sample_points(xyz, npoints):
    """xyz (B, N, F), xyz in the first three channels -> (B, npoints, F) by farthest point sampling from point 0"""
    xyz_flipped = xyz.transpose(1, 2).contiguous()
    idx = pointnet2_utils.furthest_point_sample(xyz[:, :, 0:3].contiguous(), npoints)
    return pointnet2_utils.gather_operation(xyz_flipped, idx).transpose(1, 2).contiguous()


def mirror_and_concat(partial, axis=2, num_points=[2048, 3072], attach_label=False, permute=True, seed=0):
    """-> (concat (B, 2N, F + attach_label), then one down-sampled cloud per entry of num_points): the reference's tuple.  The label is
    +1 on the original points and -1 on the mirrored ones."""
    B, N, _ = partial.size()
    perm = refine.refine_permutation(2 * N, seed) if permute else None
    concat, _ = refine.mirror_and_concat(partial.cuda(), axis=axis, attach_label=attach_label, perm=perm)
    return tuple([concat] + [down_sample_points(concat, n) for n in num_points])
