"""Approximate Earth Mover's Distance (reference: pointnet2/metrics_point_cloud/emd.py on the `emd_cuda` extension), forward only,
on the gfx950 HIP kernel slide_amd/csrc/emd_pairwise.hip.

`earth_mover_distance` and `EMD_distance` keep the reference's names, argument lists and result: for xyz1 (b, n, 3) and xyz2
(b, m, 3) the (b,) costs sum_kl d(k, l) match(k, l) of the auction's approximate match (d the squared distance), divided by
max(n, m) as the reference module does.  The undivided cost is `slide_amd._ext.emd_pairwise(xyz1, xyz2, paired=True)`; the PVD
metric (metrics_point_cloud.generation_metrics.pairwise_emd) divides it by n instead.  The function is not symmetric in its
arguments.  2-D inputs are one cloud each.

Scope: CUDA tensors only (a CPU tensor raises RuntimeError: no CPU fallback); no autograd -- inputs that require grad raise
NotImplementedError, as the backward kernels (matchcostgrad) are not implemented; `return_match=True` raises NotImplementedError:
the kernel adds d * w into the cost in the sweep that would store the match and never builds the (b, m, n) matrix."""
import torch
import torch.nn as nn

from slide_amd import _ext as _hip


def _emd(xyz1, xyz2, transpose, return_match):
    if return_match:
        raise NotImplementedError("metrics_point_cloud.emd never builds the match matrix: return_match=True is not supported")
    for t, name in ((xyz1, "xyz1"), (xyz2, "xyz2")):
        if not torch.is_tensor(t) or t.dim() not in (2, 3):
            raise ValueError("Expected %s to be a tensor of shape (b, n, 3) or (n, 3)" % name)
        if torch.is_grad_enabled() and t.requires_grad:
            raise NotImplementedError("metrics_point_cloud.emd is forward only (no backward kernels): call it under torch.no_grad() "
                                      "or on tensors that do not require grad")
        if not t.is_cuda:
            raise RuntimeError("metrics_point_cloud.emd runs on the GPU only: got a %s tensor" % t.device)
    if xyz1.dim() == 2:
        xyz1 = xyz1.unsqueeze(0)
    if xyz2.dim() == 2:
        xyz2 = xyz2.unsqueeze(0)
    if transpose:
        xyz1 = xyz1.transpose(1, 2)
        xyz2 = xyz2.transpose(1, 2)
    if xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError("xyz1 and xyz2 must hold the same number of clouds")
    if xyz1.shape[2] < 3 or xyz2.shape[2] < 3 or xyz1.shape[1] < 1 or xyz2.shape[1] < 1:
        raise ValueError("clouds must hold at least one point of at least 3 channels (xyz first)")
    cost = _hip.emd_pairwise(xyz1.detach().float(), xyz2.detach().float(), paired=True)
    return cost / max(xyz1.shape[1], xyz2.shape[1])


def earth_mover_distance(xyz1, xyz2, transpose=False, return_match=False):
    """Earth Mover Distance (Approx)

    Args:
        xyz1 (torch.Tensor): (b, n, 3)
        xyz2 (torch.Tensor): (b, m, 3)
        transpose (bool): whether to transpose inputs as it might be BCN format.

    Returns:
        cost (torch.Tensor): (b), divided by max(n, m)
    """
    return _emd(xyz1, xyz2, transpose, return_match)


class EMD_distance(nn.Module):
    def forward(self, xyz1, xyz2, transpose=False, return_match=False):
        return _emd(xyz1, xyz2, transpose, return_match)
