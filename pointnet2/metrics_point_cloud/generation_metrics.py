"""Set-level generation metrics, Chamfer half (reference: pointnet2/models/pvd/metrics/evaluation_metrics.py): MMD-CD, COV-CD and
1-NNA-CD of a generated set against a reference set, from three all-pairs Chamfer matrices on the GPU.

`pairwise_cd`, `lgan_mmd_cov`, `knn` and `compute_all_metrics` keep the reference's names, argument orders, result keys and
reductions.  A matrix is ONE launch of slide_amd/csrc/chamfer_pairwise.hip (both directions of every pair searched and reduced
inside a workgroup; the symmetric matrices compute their upper triangle and mirror it); every entry is bit-equal to what
chamfer_and_f1.calc_cd gives for that pair (`cd_t`), wherever the pair sits in the matrix.

Scope: CUDA tensors only for `pairwise_cd` / `compute_all_metrics` (no CPU fallback), no autograd (inputs that require grad raise
NotImplementedError), fixed-size clouds (a set is a dense (M, P, C) tensor).  `lgan_mmd_cov` and `knn` are plain torch and run on
any device.  The reference's EMD keys are absent: Earth Mover's Distance is not implemented in this project."""
import torch

from slide_amd import _ext as _hip


def _check_set(t, name):
    if not torch.is_tensor(t) or t.ndim != 3:
        raise ValueError("Expected %s to be a tensor of shape (M, P, C)" % name)
    if t.shape[2] < 3:
        raise ValueError("%s must hold at least 3 channels (xyz first)" % name)
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must hold at least one cloud of at least one point" % name)


def pairwise_cd(sample_pcs, ref_pcs=None, batch_size=None):
    """(N_sample, N_ref) float32 matrix of mean_p d(x -> y) + mean_q d(y -> x) over squared nearest-neighbour distances (the
    reference's `dl.mean(1) + dr.mean(1)` of `_pairwise_EMD_CD_`, this project's `cd_t`), one launch.

    sample_pcs (M, P, C >= 3), ref_pcs (N, Q, C >= 3) float CUDA tensors, xyz = the first three channels (read in place).
    ref_pcs=None scores the set against itself: the upper triangle is computed and mirrored, the result is bitwise symmetric.
    batch_size is accepted and ignored (the reference needs it to bound its memory; one launch here holds only the matrix)."""
    _check_set(sample_pcs, "sample_pcs")
    if ref_pcs is not None:
        _check_set(ref_pcs, "ref_pcs")
    for t in (sample_pcs, ref_pcs):
        if t is not None and torch.is_grad_enabled() and t.requires_grad:
            raise NotImplementedError("metrics_point_cloud.generation_metrics is forward only (no backward kernels): call it under "
                                      "torch.no_grad() or on tensors that do not require grad")
        if t is not None and not t.is_cuda:
            raise RuntimeError("metrics_point_cloud.generation_metrics runs on the GPU only: got a %s tensor" % t.device)
    x = sample_pcs.detach().float()
    y = None if ref_pcs is None else ref_pcs.detach().float()
    s = _hip.chamfer_pairwise(x, y)
    P, Q = x.shape[1], (x if y is None else y).shape[1]
    return s[:, :, 0, 0] / P + s[:, :, 1, 0] / Q


def lgan_mmd_cov(all_dist):
    """all_dist (N_sample, N_ref) -> {'lgan_mmd': mean over references of the distance to the nearest sample, 'lgan_cov': fraction
    of references that are some sample's nearest reference, 'lgan_mmd_smp': mean over samples of the distance to the nearest
    reference}, 0-dim tensors of all_dist's dtype and device.  A sample equidistant from several references votes for the one
    with the lowest index (the reference leaves that to torch.min)."""
    N_sample, N_ref = all_dist.size(0), all_dist.size(1)
    min_val_fromsmp = all_dist.min(dim=1)[0]
    # the first column that attains the row minimum: ties -> lowest index, on every device
    cols = torch.arange(N_ref, device=all_dist.device).expand(N_sample, N_ref)
    min_idx = torch.where(all_dist == min_val_fromsmp[:, None], cols, cols.new_full((), N_ref)).min(dim=1)[0]
    min_val = all_dist.min(dim=0)[0]
    cov = float(min_idx.unique().numel()) / float(N_ref)
    return {
        'lgan_mmd': min_val.mean(),
        'lgan_cov': torch.tensor(cov).to(all_dist),
        'lgan_mmd_smp': min_val_fromsmp.mean(),
    }


def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """k-nearest-neighbour two-sample test on the (n0 + n1)^2 distance matrix [[Mxx, Mxy], [Mxy^T, Myy]] with the diagonal
    excluded: every element is classified by the majority label of its k nearest others (label 1 = the x set) -> the reference's
    dictionary: tp / fp / fn / tn, precision, recall, acc_t, acc_f, acc (0-dim tensors on Mxx's device).  Equal distances rank by
    index: the lowest index wins (the reference leaves that to torch.topk)."""
    n0, n1 = Mxx.size(0), Myy.size(0)
    label = torch.cat((torch.ones(n0), torch.zeros(n1))).to(Mxx)
    M = torch.cat((torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.transpose(0, 1), Myy), 1)), 0)
    if sqrt:
        M = M.abs().sqrt()
    M = M + torch.diag(float('inf') * torch.ones(n0 + n1).to(Mxx))
    idx = torch.sort(M, dim=0, stable=True)[1][:k]  # stable: ties -> lowest index, on every device
    count = torch.zeros(n0 + n1).to(Mxx)
    for i in range(0, k):
        count = count + label.index_select(0, idx[i])
    pred = torch.ge(count, (float(k) / 2) * torch.ones(n0 + n1).to(Mxx)).float()
    s = {
        'tp': (pred * label).sum(),
        'fp': (pred * (1 - label)).sum(),
        'fn': ((1 - pred) * label).sum(),
        'tn': ((1 - pred) * (1 - label)).sum(),
    }
    s.update({
        'precision': s['tp'] / (s['tp'] + s['fp'] + 1e-10),
        'recall': s['tp'] / (s['tp'] + s['fn'] + 1e-10),
        'acc_t': s['tp'] / (s['tp'] + s['fn'] + 1e-10),
        'acc_f': s['tn'] / (s['tn'] + s['fp'] + 1e-10),
        'acc': torch.eq(label, pred).float().mean(),
    })
    return s


def all_pairs_matrices(sample_pcs, ref_pcs):
    """the three matrices of compute_all_metrics: (M_rs (N_ref, N_sample), M_rr, M_ss), float32 on the device"""
    return pairwise_cd(ref_pcs, sample_pcs), pairwise_cd(ref_pcs), pairwise_cd(sample_pcs)


def compute_all_metrics(sample_pcs, ref_pcs, batch_size=None):
    """MMD-CD, COV-CD and 1-NNA-CD of sample_pcs (N_s, P, C >= 3) against ref_pcs (N_r, Q, C >= 3), CUDA tensors -> dict of 0-dim
    device tensors with the reference's CD keys: lgan_mmd-CD, lgan_cov-CD, lgan_mmd_smp-CD, 1-NN-CD-acc_t, 1-NN-CD-acc_f,
    1-NN-CD-acc.  Three launches (references x samples, references x references and samples x samples in the symmetric form);
    the (N_r + N_s)^2 matrix of the 1-NN test stays on the device.  batch_size is accepted and ignored.

    The reference's EMD keys (lgan_*-EMD, 1-NN-EMD-*) are absent: this project has no Earth Mover's Distance."""
    with torch.no_grad():
        M_rs_cd, M_rr_cd, M_ss_cd = all_pairs_matrices(sample_pcs, ref_pcs)
        results = {"%s-CD" % k: v for k, v in lgan_mmd_cov(M_rs_cd.t()).items()}
        one_nn_cd_res = knn(M_rr_cd, M_rs_cd, M_ss_cd, 1, sqrt=False)
        results.update({"1-NN-CD-%s" % k: v for k, v in one_nn_cd_res.items() if 'acc' in k})
    return results
