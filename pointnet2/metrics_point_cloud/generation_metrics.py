"""Set-level generation metrics (reference: pointnet2/models/pvd/metrics/evaluation_metrics.py): MMD, COV and 1-NNA of a generated
set against a reference set under the Chamfer distance and, on request, the approximate Earth Mover's Distance, from three
all-pairs matrices per distance on the GPU.

`pairwise_cd`, `lgan_mmd_cov`, `knn` and `compute_all_metrics` keep the reference's names, argument orders, result keys and
reductions.  A matrix is ONE launch of slide_amd/csrc/chamfer_pairwise.hip (both directions of every pair searched and reduced
inside a workgroup; the symmetric matrices compute their upper triangle and mirror it); every entry is bit-equal to what
chamfer_and_f1.calc_cd gives for that pair (`cd_t`), wherever the pair sits in the matrix.

Scope: CUDA tensors only for `pairwise_cd` / `compute_all_metrics` (no CPU fallback), no autograd (inputs that require grad raise
NotImplementedError), fixed-size clouds (a set is a dense (M, P, C) tensor).  `lgan_mmd_cov` and `knn` are plain torch and run on
any device.

EMD (`pairwise_emd`, `all_pairs_matrices_emd`, `compute_all_metrics(..., emd=True)`): the second output of the reference's
`_pairwise_EMD_CD_`, cost / P of its approximate match, on slide_amd/csrc/emd_pairwise.hip -- one workgroup per ORDERED pair (the
function is not symmetric in its arguments, so a set against itself is computed in full), the match matrix never stored.  It
costs 30 exponentials per pair of points where Chamfer costs two distance evaluations, so the six EMD keys are opt-in, as JSD is;
a large matrix runs as several bounded launches.

JSD block (`unit_cube_grid_point_cloud`, `entropy_of_occupancy_grid`, `jensen_shannon_divergence`, `jsd_between_point_cloud_sets`;
the reference's names, argument lists, defaults and return types): the Jensen-Shannon divergence between the occupancy distributions
of two sets on a resolution^3 grid clipped to the unit sphere.  The per-cloud nearest-cell query and the two counting loops of the
reference are ONE launch of slide_amd/csrc/occupancy_grid.hip; the grid and its sphere mask are built here in numpy with the
reference's expressions and uploaded, so the boundary cells are the reference's.  The entropy / JSD arithmetic runs over at most
32 768 numbers on the host in float64 (no scipy).  Resolutions 2 to 32."""
import functools
import warnings

import numpy as np
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


def pairwise_emd(sample_pcs, ref_pcs=None, batch_size=None):
    """(N_sample, N_ref) float32 matrix of the approximate Earth Mover's Distance with sample_pcs[i] as xyz1 and ref_pcs[j] as xyz2,
    divided by the points per sample cloud (the reference's `EMD(sample_batch_exp, ref_batch, transpose=False)` of
    `_pairwise_EMD_CD_`).  Same inputs and scope as pairwise_cd.  ref_pcs=None scores the set against itself, in full: the
    distance is not symmetric in its arguments.  batch_size is accepted and ignored (launches are bounded by work, not by memory)."""
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
    return _hip.emd_pairwise(x, y) / x.shape[1]


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


def all_pairs_matrices_emd(sample_pcs, ref_pcs):
    """the three EMD matrices of compute_all_metrics(emd=True): (M_rs (N_ref, N_sample), M_rr, M_ss), float32 on the device, every
    one computed in full"""
    return pairwise_emd(ref_pcs, sample_pcs), pairwise_emd(ref_pcs), pairwise_emd(sample_pcs)


def compute_all_metrics(sample_pcs, ref_pcs, batch_size=None, emd=False):
    """MMD-CD, COV-CD and 1-NNA-CD of sample_pcs (N_s, P, C >= 3) against ref_pcs (N_r, Q, C >= 3), CUDA tensors -> dict of 0-dim
    device tensors with the reference's CD keys: lgan_mmd-CD, lgan_cov-CD, lgan_mmd_smp-CD, 1-NN-CD-acc_t, 1-NN-CD-acc_f,
    1-NN-CD-acc.  Three launches (references x samples, references x references and samples x samples in the symmetric form);
    the (N_r + N_s)^2 matrix of the 1-NN test stays on the device.  batch_size is accepted and ignored.

    emd=True adds the reference's six EMD keys (lgan_mmd-EMD, lgan_cov-EMD, lgan_mmd_smp-EMD, 1-NN-EMD-acc_t, 1-NN-EMD-acc_f,
    1-NN-EMD-acc) from three more matrices (all_pairs_matrices_emd) through the same lgan_mmd_cov and knn; the CD values do not
    change.  Off by default: the EMD matrices cost far more than the Chamfer ones."""
    with torch.no_grad():
        M_rs_cd, M_rr_cd, M_ss_cd = all_pairs_matrices(sample_pcs, ref_pcs)
        results = {"%s-CD" % k: v for k, v in lgan_mmd_cov(M_rs_cd.t()).items()}
        if emd:
            M_rs_emd, M_rr_emd, M_ss_emd = all_pairs_matrices_emd(sample_pcs, ref_pcs)
            results.update({"%s-EMD" % k: v for k, v in lgan_mmd_cov(M_rs_emd.t()).items()})
        one_nn_cd_res = knn(M_rr_cd, M_rs_cd, M_ss_cd, 1, sqrt=False)
        results.update({"1-NN-CD-%s" % k: v for k, v in one_nn_cd_res.items() if 'acc' in k})
        if emd:
            one_nn_emd_res = knn(M_rr_emd, M_rs_emd, M_ss_emd, 1, sqrt=False)
            results.update({"1-NN-EMD-%s" % k: v for k, v in one_nn_emd_res.items() if 'acc' in k})
    return results


#######################################################
# JSD : occupancy grids (Achlioptas et al., "Learning Representations and Generative Models for 3D Point Clouds")
#######################################################
@functools.lru_cache(maxsize=8)
def _grid_axis_and_mask(resolution, clip_sphere):
    """(axis (R,) float32, grid (R^3, 3) float32, mask (R^3,) bool): a cell-centre coordinate is `i * spacing - 0.5` evaluated in
    double and rounded once to float32; the sphere mask is numpy's float32 norm of the float32 grid against 0.5"""
    resolution = int(resolution)
    spacing = 1.0 / float(resolution - 1)
    axis = (np.arange(resolution, dtype=np.float64) * spacing - 0.5).astype(np.float32)
    gi, gj, gk = np.meshgrid(axis, axis, axis, indexing="ij")
    grid = np.stack((gi, gj, gk), axis=-1).reshape(-1, 3)
    mask = (np.linalg.norm(grid, axis=1) <= 0.5) if clip_sphere else np.ones(len(grid), bool)
    for a in (axis, grid, mask):
        a.setflags(write=False)
    return axis, grid, mask


def unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """Returns the center coordinates of each cell of a 3D grid with resolution^3 cells, that is placed in the unit-cube:
    (grid, spacing), grid float32 (resolution, resolution, resolution, 3), or with clip_sphere the (n, 3) cells that lie inside the
    unit sphere (norm <= 0.5) in flattened order."""
    _, grid, mask = _grid_axis_and_mask(int(resolution), bool(clip_sphere))
    spacing = 1.0 / float(resolution - 1)
    if clip_sphere:
        return grid[mask], spacing
    return grid.reshape(resolution, resolution, resolution, 3).copy(), spacing


def _bernoulli_entropy_sum(rvars, n):
    """sum over the cells with g > 0 of the entropy (natural log) of a Bernoulli variable with p = g / n:
    -(p ln p + (1 - p) ln(1 - p)), the second term 0 at p = 1"""
    g = np.asarray(rvars, np.float64)
    p = g[g > 0] / float(n)
    q = 1.0 - p
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -(p * np.log(p)) - np.where(q > 0, q * np.log(q), 0.0)
    return float(np.sum(h))


def occupancy_counters(pclouds, grid_resolution, in_sphere=False):
    """(grid_counters, grid_bernoulli_rvars) of the reference's entropy_of_occupancy_grid: float64 arrays over the admissible
    cells in flattened order -- points per cell over all clouds, and clouds with at least one point in the cell.  One launch."""
    if not 2 <= int(grid_resolution) <= 32:
        raise ValueError("grid_resolution must be in [2, 32], got %r" % (grid_resolution,))
    pts = _as_device_clouds(pclouds)
    axis, _, mask = _grid_axis_and_mask(int(grid_resolution), bool(in_sphere))
    counts, clouds = _hip.occupancy_grid(pts, torch.tensor(axis), torch.tensor(mask))  # (copies: the cached arrays are read-only)
    both = torch.stack((counts, clouds)).cpu().numpy()
    return both[0][mask].astype(np.float64), both[1][mask].astype(np.float64)


def _as_device_clouds(pclouds):
    if torch.is_tensor(pclouds):
        if not pclouds.is_cuda:
            raise RuntimeError("metrics_point_cloud.generation_metrics runs on the GPU only: got a %s tensor" % pclouds.device)
        t = pclouds.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(pclouds)).to(torch.device("cuda", torch.cuda.current_device()))
    if t.ndim != 3 or t.shape[2] < 3:
        raise ValueError("Expected pclouds of shape (#point-clouds, points per point-cloud, 3)")
    return t.float()


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False, verbose=False):
    """Given a collection of point-clouds, estimate the entropy of the random variables corresponding to occupancy-grid activation
    patterns.  pclouds: #point-clouds x points per point-cloud x 3, a CUDA tensor or a numpy array (moved to the current device).
    -> (mean Bernoulli entropy per cell (float), grid_counters: numpy float64, one per admissible cell in flattened order)."""
    pts = _as_device_clouds(pclouds)
    epsilon = 10e-4
    bound = 0.5 + epsilon
    if verbose and pts.numel():
        xyz = pts[:, :, :3]
        if abs(float(xyz.max())) > bound or abs(float(xyz.min())) > bound:
            warnings.warn('Point-clouds are not in unit cube.')
        if in_sphere and float(xyz.pow(2).sum(2).sqrt().max()) > bound:
            warnings.warn('Point-clouds are not in unit sphere.')
    grid_counters, grid_bernoulli_rvars = occupancy_counters(pts, grid_resolution, in_sphere)
    acc_entropy = _bernoulli_entropy_sum(grid_bernoulli_rvars, len(pts)) if len(pts) else 0.0
    return acc_entropy / len(grid_counters), grid_counters


def _entropy_base2(p):
    """-sum p log2 p of a float64 vector that sums to one (zero entries contribute 0)"""
    p = p[p > 0]
    return float(-np.sum(p * np.log(p)) / np.log(2.0))


def jensen_shannon_divergence(P, Q):
    P, Q = np.asarray(P), np.asarray(Q)
    if np.any(P < 0) or np.any(Q < 0):
        raise ValueError('Negative values.')
    if len(P) != len(Q):
        raise ValueError('Non equal size.')

    P_ = P / np.sum(P)  # Ensure probabilities.
    Q_ = Q / np.sum(Q)

    e1 = _entropy_base2(P_)
    e2 = _entropy_base2(Q_)
    e_sum = _entropy_base2((P_ + Q_) / 2.0)
    res = e_sum - ((e1 + e2) / 2.0)

    res2 = _jsdiv(P_, Q_)

    if not np.allclose(res, res2, atol=10e-5, rtol=0):
        warnings.warn('Numerical values of two JSD methods don\'t agree.')

    return res


def _jsdiv(P, Q):
    """another way of computing JSD: the mean of the two Kullback-Leibler divergences (base 2) to the mixture"""

    def _kldiv(A, B):
        idx = np.logical_and(A > 0, B > 0)
        a, b = A[idx], B[idx]
        return float(np.sum(a * np.log2(a / b)))

    P_ = P / np.sum(P)
    Q_ = Q / np.sum(Q)
    M = 0.5 * (P_ + Q_)
    return 0.5 * (_kldiv(P_, M) + _kldiv(Q_, M))


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """Computes the JSD between two sets of point-clouds, as introduced in the paper ```Learning Representations And Generative
    Models For 3D Point Clouds```.  sample_pcs (S1, R1, 3), ref_pcs (S2, R2, 3): CUDA tensors or numpy arrays; resolution: the
    grid resolution (2 to 32).  The grid is clipped to the unit sphere; a point goes to its nearest cell inside it."""
    in_unit_sphere = True
    sample_grid_var = entropy_of_occupancy_grid(sample_pcs, resolution, in_unit_sphere)[1]
    ref_grid_var = entropy_of_occupancy_grid(ref_pcs, resolution, in_unit_sphere)[1]
    return jensen_shannon_divergence(sample_grid_var, ref_grid_var)
