"""Differentiable row-major counterparts of the reference's two grouping operators (pointnet2_ops/pointnet2_utils.py:307-448
QueryAndGroup, :497-524 group_knn).  The neighbour search runs without gradients on the existing kernels (knn_points / ball_query);
for the neighbours it finds, the rows are differentiable in the features and in BOTH coordinate tensors (functions.GroupRows:
csrc/train_ops.hip for the features, csrc/group_coord_bwd.hip for the coordinates) -- the decoder's points are outputs of the level
before, and the Chamfer gradient reaches that level through these terms.  No gradient flows through the neighbour selection."""
import torch

from .. import _ext
from ..abi import GROUP_ABS, GROUP_CENTER, GROUP_FP
from .functions import group_rows


def _chk_points(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("CPU not supported: the grouping layers launch HIP kernels")
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.float32:
            raise ValueError("expected float32 points of shape (B, N, 3)")


def query_and_group_rows(xyz, new_xyz, feat_rows, C, nsample, neighbor_def="nn", radius=None, include_abs_coordinate=False,
                         include_center_coordinate=False, subset=True):
    """QueryAndGroup(use_xyz=True) on rows: xyz (B, N, 3) source points, new_xyz (B, np, 3) centres, feat_rows [B*N, ld] with C valid
    channels (or None, C = 0) -> (rows [B*np*K, ru(C + 3 | 6 | 9)] = [feat | rel | abs? | centre?], idx (B, np, K), counts (B, np) int32).
    'nn': the K = min(nsample, N) nearest source points, idx int64, counts = K.  'radius': ball_query, K = nsample, idx int32; with
    subset=False a centre with an empty ball is its own neighbour with zero features (subset=True: source point 0, as the reference)."""
    _chk_points(xyz, new_xyz)
    flags = (GROUP_ABS if include_abs_coordinate else 0) | (GROUP_CENTER if include_center_coordinate else 0)
    with torch.no_grad():
        if neighbor_def == "nn":
            _, idx = _ext.knn_points(new_xyz.detach(), xyz.detach(), min(int(nsample), xyz.shape[1]))
            counts = torch.full(idx.shape[:2], idx.shape[2], device=idx.device, dtype=torch.int32)
        elif neighbor_def == "radius":
            if radius is None:
                raise ValueError("neighbor_def 'radius' needs a radius")
            idx, counts = _ext.ball_query(new_xyz.detach().contiguous(), xyz.detach().contiguous(), float(radius), int(nsample))
        else:
            raise ValueError("Neighbor definition %s is not supported" % neighbor_def)
    empty_rule = neighbor_def == "radius" and not subset
    return group_rows(feat_rows, xyz, new_xyz, idx, None, flags, C, counts if empty_rule else None), idx, counts


def group_knn_rows(x, y, feat_y_rows, C, K):
    """group_knn(x, y, features_at_y, K) on rows: x (B, N1, 3) centres, y (B, N2, 3) source points, feat_y_rows [B*N2, ld] with C valid
    channels (or None) -> rows [B*N1*K, ru(C + 11)] = [feat | d2 | w | abs | rel | centre] over the K nearest points of y"""
    _chk_points(x, y)
    if not 1 <= K <= y.shape[1]:
        raise ValueError("K must be between 1 and the number of source points")
    with torch.no_grad():
        d2, idx = _ext.knn_points(x.detach(), y.detach(), int(K))
    return group_rows(feat_y_rows, y, x, idx, d2, GROUP_FP, C)
