"""Chamfer distance and F-score (reference: pointnet2/metrics_point_cloud/chamfer_and_f1.py), forward only, on gfx950 HIP kernels.

`chamfer_distance`, `fscore`, `calc_cd` and `Chamfer_F1` keep the reference's signatures, return values, validation errors and
reduction semantics.  The nearest-neighbour search is slide_amd/csrc/chamfer.hip's bidirectional K = 1 kernel (bit-equal to
knn_points(K=1) in each direction: same distances, ties -> lower index).  `calc_cd` takes the fused path -- that kernel, then the
per-cloud reduction kernel (sums in a fixed order: a pair's metrics do not depend on the batch it is scored in), then O(B)
arithmetic -- and never builds a (B, P) torch chain.

Scope: CUDA tensors only (no CPU fallback), no autograd (inputs that require grad raise NotImplementedError), and no pytorch3d
`Pointclouds` inputs (pytorch3d is not a dependency: anything but a tensor raises the reference's ValueError)."""
from typing import Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from slide_amd import _ext as _hip


def _validate_chamfer_reduction_inputs(batch_reduction: Union[str, None], point_reduction: str):
    if batch_reduction is not None and batch_reduction not in ["mean", "sum"]:
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction is not None and point_reduction not in ["mean", "sum"]:
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    if point_reduction is None and batch_reduction is not None:
        raise ValueError('batch_reduction must be set to None if point_reduction is already None')


def _handle_pointcloud_input(points, lengths, normals):
    if torch.is_tensor(points):
        if points.ndim != 3:
            raise ValueError("Expected points to be of shape (N, P, D)")
        X = points
        if lengths is not None and (lengths.ndim != 1 or lengths.shape[0] != X.shape[0]):
            raise ValueError("Expected lengths to be of shape (N,)")
        if lengths is None:
            lengths = torch.full((X.shape[0],), X.shape[1], dtype=torch.int64, device=points.device)
        if normals is not None and normals.ndim != 3:
            raise ValueError("Expected normals to be of shape (N, P, 3")
    else:
        raise ValueError("The input pointclouds should be either Pointclouds objects or torch.Tensor of shape "
                         "(minibatch, num_points, 3).")
    return X, lengths, normals


def _forward_only(*tensors):
    if torch.is_grad_enabled() and any(t is not None and torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError("metrics_point_cloud.chamfer_and_f1 is forward only (no backward kernels): call it under "
                                  "torch.no_grad() or on tensors that do not require grad")


def _check_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("metrics_point_cloud.chamfer_and_f1 runs on the GPU only: got a %s tensor" % t.device)


def _check_lengths(lengths, P, name):
    if bool(((lengths < 1) | (lengths > P)).any()):
        raise ValueError("%s must lie in [1, %d]" % (name, P))


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, normal_loss_type='cos', weights=None,
                     batch_reduction: Union[str, None] = "mean", point_reduction: str = "mean"):
    """Chamfer distance between two batches of point clouds (reference chamfer_and_f1.py:66-221).

    x (N, P1, D), y (N, P2, D) float32 CUDA tensors, optional int64 lengths (N,), normals (N, P, C), weights (N,).  Returns
    (cham_x, cham_y, cham_norm_x, cham_norm_y): squared nearest-neighbour distances x -> y and y -> x and the normal terms
    (`cos`: 1 - |cosine similarity|, `mse`: sum of squared differences), reduced over points (None / "mean" / "sum") and then
    over the batch (None / "mean" / "sum"); the normal terms are 0-dim zeros without normals."""
    _validate_chamfer_reduction_inputs(batch_reduction, point_reduction)
    assert normal_loss_type in ['mse', 'cos']
    x, x_lengths, x_normals = _handle_pointcloud_input(x, x_lengths, x_normals)
    y, y_lengths, y_normals = _handle_pointcloud_input(y, y_lengths, y_normals)
    _forward_only(x, y, x_normals, y_normals, weights)
    return_normals = x_normals is not None and y_normals is not None

    N, P1, D = x.shape
    P2 = y.shape[1]
    if y.shape[0] != N or y.shape[2] != D:
        raise ValueError("y does not have the correct shape.")
    _check_device(x, y, x_normals, y_normals)
    x_lengths = x_lengths.to(device=x.device, dtype=torch.int64)
    y_lengths = y_lengths.to(device=x.device, dtype=torch.int64)
    _check_lengths(x_lengths, P1, "x_lengths")
    _check_lengths(y_lengths, P2, "y_lengths")
    if weights is not None:
        if weights.size(0) != N:
            raise ValueError("weights must be of shape (N,).")
        if not (weights >= 0).all():
            raise ValueError("weights cannot be negative.")
        if weights.sum() == 0.0:
            weights = weights.view(N, 1)
            if batch_reduction in ["mean", "sum"]:
                return ((x.sum((1, 2)) * weights).sum() * 0.0, (x.sum((1, 2)) * weights).sum() * 0.0)
            return ((x.sum((1, 2)) * weights) * 0.0, (x.sum((1, 2)) * weights) * 0.0)

    x32 = x.float()
    y32 = y.float()
    is_x_het = bool((x_lengths != P1).any())
    is_y_het = bool((y_lengths != P2).any())
    lx = x_lengths if is_x_het else None
    ly = y_lengths if is_y_het else None
    d1, i1, d2, i2 = _hip.chamfer_nn(x32, y32, lx, ly)  # slots beyond a length are 0 already

    cham_norm_x = x.new_zeros(())
    cham_norm_y = x.new_zeros(())
    if point_reduction is None:
        cham_x, cham_y = d1, d2
        if weights is not None:
            cham_x = cham_x * weights.view(N, 1)
            cham_y = cham_y * weights.view(N, 1)
        if return_normals:
            x_normals_near = torch.gather(y_normals, 1, i1[:, :, None].expand(-1, -1, y_normals.shape[2]))
            y_normals_near = torch.gather(x_normals, 1, i2[:, :, None].expand(-1, -1, x_normals.shape[2]))
            if normal_loss_type == 'cos':
                cham_norm_x = 1 - torch.abs(F.cosine_similarity(x_normals, x_normals_near, dim=2, eps=1e-6))
                cham_norm_y = 1 - torch.abs(F.cosine_similarity(y_normals, y_normals_near, dim=2, eps=1e-6))
            else:
                cham_norm_x = torch.sum((x_normals - x_normals_near) ** 2, dim=2)
                cham_norm_y = torch.sum((y_normals - y_normals_near) ** 2, dim=2)
            if is_x_het:
                cham_norm_x = cham_norm_x.masked_fill(torch.arange(P1, device=x.device)[None] >= x_lengths[:, None], 0.0)
            if is_y_het:
                cham_norm_y = cham_norm_y.masked_fill(torch.arange(P2, device=y.device)[None] >= y_lengths[:, None], 0.0)
            if weights is not None:
                cham_norm_x = cham_norm_x * weights.view(N, 1)
                cham_norm_y = cham_norm_y * weights.view(N, 1)
        return cham_x, cham_y, cham_norm_x, cham_norm_y

    # point reduction on the device: per-cloud sums of the fused reduction kernel
    if return_normals:
        red = _hip.chamfer_reduce(d1, i1, d2, i2, lx, ly, fx=x_normals.float(), fy=y_normals.float(), term=normal_loss_type)
    else:
        red = _hip.chamfer_reduce(d1, i1, d2, i2, lx, ly)
    cham_x, cham_y = red[:, 0, 0], red[:, 1, 0]
    if return_normals:
        cham_norm_x, cham_norm_y = red[:, 0, 3], red[:, 1, 3]
    if weights is not None:
        w = weights.to(cham_x.dtype)
        cham_x, cham_y = cham_x * w, cham_y * w
        if return_normals:
            cham_norm_x, cham_norm_y = cham_norm_x * w, cham_norm_y * w
    if point_reduction == "mean":
        cham_x = cham_x / x_lengths
        cham_y = cham_y / y_lengths
        if return_normals:
            cham_norm_x = cham_norm_x / x_lengths
            cham_norm_y = cham_norm_y / y_lengths
    if batch_reduction is not None:
        cham_x, cham_y = cham_x.sum(), cham_y.sum()
        if return_normals:
            cham_norm_x, cham_norm_y = cham_norm_x.sum(), cham_norm_y.sum()
        if batch_reduction == "mean":
            div = weights.sum() if weights is not None else N
            cham_x, cham_y = cham_x / div, cham_y / div
            if return_normals:
                cham_norm_x, cham_norm_y = cham_norm_x / div, cham_norm_y / div
    return cham_x, cham_y, cham_norm_x, cham_norm_y


def fscore(dist1, dist2, threshold=0.0001):
    """F-score of two batches of squared nearest-neighbour distances (B, P1), (B, P2) at `threshold` (a SQUARED distance)
    -> (fscore, precision_1, precision_2), each (B,); 0 where both precisions are 0 (reference chamfer_and_f1.py:223-238)."""
    precision_1 = torch.mean((dist1 < threshold).float(), dim=1)
    precision_2 = torch.mean((dist2 < threshold).float(), dim=1)
    f = 2 * precision_1 * precision_2 / (precision_1 + precision_2)
    f[torch.isnan(f)] = 0
    return f, precision_1, precision_2


def calc_cd_reduced(output, gt, f1_threshold=0.0001, normal_loss_type='cos'):
    """the fused path of calc_cd: -> (red (B, 2, 5) f32 per-cloud sums of chamfer_reduce, direction 0 = gt -> output), P_gt, P_out"""
    _forward_only(output, gt)
    if not (torch.is_tensor(output) and torch.is_tensor(gt)) or output.ndim != 3 or gt.ndim != 3:
        raise ValueError("Expected points to be of shape (N, P, D)")
    if output.shape[0] != gt.shape[0] or output.shape[2] != gt.shape[2]:
        raise ValueError("y does not have the correct shape.")
    if gt.shape[1] < 1 or output.shape[1] < 1:
        raise ValueError("point clouds must hold at least one point")
    assert normal_loss_type in ['mse', 'cos']
    _check_device(output, gt)
    gt = gt.float().contiguous()
    output = output.float().contiguous()
    d1, i1, d2, i2 = _hip.chamfer_nn(gt, output)
    if gt.shape[2] > 3:
        red = _hip.chamfer_reduce(d1, i1, d2, i2, threshold=f1_threshold, fx=gt[:, :, 3:], fy=output[:, :, 3:],
                                  term=normal_loss_type)
    else:
        red = _hip.chamfer_reduce(d1, None, d2, None, threshold=f1_threshold)
    return red, gt.shape[1], output.shape[1]


def calc_cd(output, gt, calc_f1=False, f1_threshold=0.0001, normal_loss_type='cos'):
    """per-pair metrics of output vs gt (B, N, C >= 3; xyz = channels 0:3, features behind them) (reference chamfer_and_f1.py:240-262):
    cd_p = mean of the two directions' mean Euclidean distance, cd_t = sum of the two mean squared distances, with features
    cd_feature_p / cd_feature_t of the normal term the same way, with calc_f1 the F-score at f1_threshold -- each (B,)."""
    red, n_gt, n_out = calc_cd_reduced(output, gt, f1_threshold, normal_loss_type)
    result = {}
    result['cd_p'] = (red[:, 0, 1] / n_gt + red[:, 1, 1] / n_out) / 2
    result['cd_t'] = red[:, 0, 0] / n_gt + red[:, 1, 0] / n_out
    if gt.shape[2] > 3:
        result['cd_feature_p'] = (red[:, 0, 4] / n_gt + red[:, 1, 4] / n_out) / 2
        result['cd_feature_t'] = red[:, 0, 3] / n_gt + red[:, 1, 3] / n_out
    if calc_f1:
        p1 = red[:, 0, 2] / n_gt
        p2 = red[:, 1, 2] / n_out
        f = 2 * p1 * p2 / (p1 + p2)
        result['f1'] = torch.where(torch.isnan(f), torch.zeros_like(f), f)
    return result


class Chamfer_F1(nn.Module):
    def __init__(self, f1_threshold=0.0001):
        super().__init__()
        self.f1_threshold = f1_threshold

    def forward(self, xyz1, xyz2):
        """xyz1, xyz2 (B, N, 3) -> cd_p, cd_t, f1, each (B,)"""
        r = calc_cd(xyz1, xyz2, calc_f1=True, f1_threshold=self.f1_threshold)
        return r['cd_p'], r['cd_t'], r['f1']
