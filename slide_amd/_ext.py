"""Drop-in counterpart of the reference's native module `pointnet2_ops._ext`
(_ext-src/src/bindings.cpp:6-19): the same nine functions, argument order, dtypes, output
allocation (zeros where an op leaves elements unwritten -- ball_query, the grads, three_nn, FPS -- and the FPS scratch
1e10; the three forward gathers write every element, so their outputs are allocated uninitialised) and error behaviour (RuntimeError on non-contiguous /
wrong dtype / CPU tensors: _ext-src/include/utils.h:5-25, sampling.cpp:21-34), implemented on
hand-written gfx950 HIP kernels through the C-ABI in include/slide_hip.h.

Asynchronous on torch's current stream, no host sync, inputs borrowed and never mutated.
"""

import ctypes

import torch

from ._lib import check, lib
from .abi import CHAMFER_TERM, ptr, stream_of


def _chk_contig(x, name):
    if not x.is_contiguous():
        raise RuntimeError("%s must be a contiguous tensor" % name)


def _chk_float(x, name):
    if x.dtype != torch.float32:
        raise RuntimeError("%s must be a float tensor" % name)


def _chk_int(x, name):
    if x.dtype != torch.int32:
        raise RuntimeError("%s must be an int tensor" % name)


def _chk_cuda(x, name):
    if not x.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)


def _need_gpu(x):
    if not x.is_cuda:
        raise RuntimeError("CPU not supported")  # sampling.cpp:34 et al.


def gather_points(points, idx):
    """sampling.cpp:15-38  points (B,C,N) f32, idx (B,M) i32 -> (B,C,M)"""
    _chk_contig(points, "points"); _chk_contig(idx, "idx"); _chk_float(points, "points"); _chk_int(idx, "idx")
    if points.is_cuda:
        _chk_cuda(idx, "idx")
    # the kernel writes every element: the reference's zero fill would only add a second pass over the output
    out = torch.empty((points.size(0), points.size(1), idx.size(1)), device=points.device, dtype=torch.float32)
    _need_gpu(points)
    check(lib().gather_points_kernel_wrapper(points.size(0), points.size(1), points.size(2), idx.size(1),
                                             ptr(points), ptr(idx), ptr(out), stream_of()), "gather_points")
    return out


def gather_points_grad(grad_out, idx, n):
    """sampling.cpp:40-65"""
    _chk_contig(grad_out, "grad_out"); _chk_contig(idx, "idx"); _chk_float(grad_out, "grad_out"); _chk_int(idx, "idx")
    if grad_out.is_cuda:
        _chk_cuda(idx, "idx")
    out = torch.zeros((grad_out.size(0), grad_out.size(1), n), device=grad_out.device, dtype=torch.float32)
    _need_gpu(grad_out)
    check(lib().gather_points_grad_kernel_wrapper(grad_out.size(0), grad_out.size(1), int(n), idx.size(1),
                                                  ptr(grad_out), ptr(idx), ptr(out), stream_of()),
          "gather_points_grad")
    return out


def furthest_point_sampling(points, nsamples):
    """sampling.cpp:66-87  points (B,N,3) -> (B,nsamples) i32"""
    _chk_contig(points, "points"); _chk_float(points, "points")
    out = torch.zeros((points.size(0), nsamples), device=points.device, dtype=torch.int32)
    tmp = torch.full((points.size(0), points.size(1)), 1e10, device=points.device, dtype=torch.float32)
    _need_gpu(points)
    check(lib().furthest_point_sampling_kernel_wrapper(points.size(0), points.size(1), int(nsamples), ptr(points),
                                                       ptr(tmp), ptr(out), stream_of()), "furthest_point_sampling")
    return out


def three_nn(unknown, known):
    """interpolate.cpp:14-40 -> [dist2 (B,n,3) f32, idx (B,n,3) i32]"""
    _chk_contig(unknown, "unknowns"); _chk_contig(known, "knows"); _chk_float(unknown, "unknowns")
    _chk_float(known, "knows")
    if unknown.is_cuda:
        _chk_cuda(known, "knows")
    idx = torch.zeros((unknown.size(0), unknown.size(1), 3), device=unknown.device, dtype=torch.int32)
    dist2 = torch.zeros((unknown.size(0), unknown.size(1), 3), device=unknown.device, dtype=torch.float32)
    _need_gpu(unknown)
    check(lib().three_nn_kernel_wrapper(unknown.size(0), unknown.size(1), known.size(1), ptr(unknown), ptr(known),
                                        ptr(dist2), ptr(idx), stream_of()), "three_nn")
    return [dist2, idx]


def three_interpolate(points, idx, weight):
    """interpolate.cpp:42-70  points (B,c,m), idx (B,n,3), weight (B,n,3) -> (B,c,n)"""
    for t, n in ((points, "points"), (idx, "idx"), (weight, "weight")):
        _chk_contig(t, n)
    _chk_float(points, "points"); _chk_int(idx, "idx"); _chk_float(weight, "weight")
    if points.is_cuda:
        _chk_cuda(idx, "idx"); _chk_cuda(weight, "weight")
    out = torch.empty((points.size(0), points.size(1), idx.size(1)), device=points.device, dtype=torch.float32)
    _need_gpu(points)
    check(lib().three_interpolate_kernel_wrapper(points.size(0), points.size(1), points.size(2), idx.size(1),
                                                 ptr(points), ptr(idx), ptr(weight), ptr(out), stream_of()),
          "three_interpolate")
    return out


def three_interpolate_grad(grad_out, idx, weight, m):
    """interpolate.cpp:71-99"""
    for t, n in ((grad_out, "grad_out"), (idx, "idx"), (weight, "weight")):
        _chk_contig(t, n)
    _chk_float(grad_out, "grad_out"); _chk_int(idx, "idx"); _chk_float(weight, "weight")
    if grad_out.is_cuda:
        _chk_cuda(idx, "idx"); _chk_cuda(weight, "weight")
    out = torch.zeros((grad_out.size(0), grad_out.size(1), m), device=grad_out.device, dtype=torch.float32)
    _need_gpu(grad_out)
    check(lib().three_interpolate_grad_kernel_wrapper(grad_out.size(0), grad_out.size(1), grad_out.size(2), int(m),
                                                      ptr(grad_out), ptr(idx), ptr(weight), ptr(out), stream_of()),
          "three_interpolate_grad")
    return out


def ball_query(new_xyz, xyz, radius, nsample):
    """ball_query.cpp:10-38 -> (idx (B,m,nsample) i32, counts (B,m) i32)"""
    _chk_contig(new_xyz, "new_xyz"); _chk_contig(xyz, "xyz"); _chk_float(new_xyz, "new_xyz"); _chk_float(xyz, "xyz")
    if new_xyz.is_cuda:
        _chk_cuda(xyz, "xyz")
    idx = torch.zeros((new_xyz.size(0), new_xyz.size(1), nsample), device=new_xyz.device, dtype=torch.int32)
    counts = torch.zeros((new_xyz.size(0), new_xyz.size(1)), device=new_xyz.device, dtype=torch.int32)
    _need_gpu(new_xyz)
    check(lib().query_ball_point_kernel_wrapper(xyz.size(0), xyz.size(1), new_xyz.size(1), radius,
                                                int(nsample), ptr(new_xyz), ptr(xyz), ptr(idx), ptr(counts),
                                                stream_of()), "ball_query")
    return idx, counts


def group_points(points, idx):
    """group_points.cpp:12-36  points (B,C,N), idx (B,np,ns) -> (B,C,np,ns)"""
    _chk_contig(points, "points"); _chk_contig(idx, "idx"); _chk_float(points, "points"); _chk_int(idx, "idx")
    if points.is_cuda:
        _chk_cuda(idx, "idx")
    out = torch.empty((points.size(0), points.size(1), idx.size(1), idx.size(2)), device=points.device,
                      dtype=torch.float32)
    _need_gpu(points)
    check(lib().group_points_kernel_wrapper(points.size(0), points.size(1), points.size(2), idx.size(1), idx.size(2),
                                            ptr(points), ptr(idx), ptr(out), stream_of()), "group_points")
    return out


def group_points_grad(grad_out, idx, n):
    """group_points.cpp:38-62"""
    _chk_contig(grad_out, "grad_out"); _chk_contig(idx, "idx"); _chk_float(grad_out, "grad_out"); _chk_int(idx, "idx")
    if grad_out.is_cuda:
        _chk_cuda(idx, "idx")
    out = torch.zeros((grad_out.size(0), grad_out.size(1), n), device=grad_out.device, dtype=torch.float32)
    _need_gpu(grad_out)
    check(lib().group_points_grad_kernel_wrapper(grad_out.size(0), grad_out.size(1), int(n), idx.size(1), idx.size(2),
                                                 ptr(grad_out), ptr(idx), ptr(out), stream_of()), "group_points_grad")
    return out


# ------------------------------------------------------------------ pytorch3d.ops.knn counterpart
def knn_points(p1, p2, K, lengths2=None):
    """pytorch3d knn_points (call sites pointnet2_ops/pointnet2_utils.py:370,506):
    -> (dists (B,N1,K) f32 ascending squared L2, idx (B,N1,K) int64)"""
    p1 = p1.contiguous(); p2 = p2.contiguous()
    _chk_float(p1, "p1"); _chk_float(p2, "p2"); _need_gpu(p1); _chk_cuda(p2, "p2")
    B, N1, _ = p1.shape
    dists = torch.zeros((B, N1, K), device=p1.device, dtype=torch.float32)
    idx = torch.zeros((B, N1, K), device=p1.device, dtype=torch.int64)
    lp = None
    if lengths2 is not None:
        lengths2 = lengths2.to(device=p1.device, dtype=torch.int64).contiguous()
        lp = ptr(lengths2)
    check(lib().slide_knn_points(B, N1, p2.size(1), int(K), ptr(p1), ptr(p2), lp, ptr(dists), ptr(idx), stream_of()),
          "knn_points")
    return dists, idx


def knn_gather(x, idx):
    """pytorch3d knn_gather: x (B,N2,U), idx (B,N1,K) int64 -> (B,N1,K,U)"""
    x = x.contiguous(); idx = idx.contiguous()
    _chk_float(x, "x"); _need_gpu(x)
    if idx.dtype != torch.int64:
        raise RuntimeError("idx must be an int64 tensor")
    B, N2, U = x.shape
    _, N1, K = idx.shape
    out = torch.empty((B, N1, K, U), device=x.device, dtype=torch.float32)
    check(lib().slide_knn_gather(B, N2, U, N1, K, ptr(x), ptr(idx), ptr(out), stream_of()), "knn_gather")
    return out


def gather_rows(points, idx):
    """row-layout counterpart of gather_points: points (B,N,C) float32, idx (B,M) int32 -> (B,M,C).  Moves only the gathered rows
    (gather_points on the reference's (B,C,N) layout pays a 64-byte sector per gathered element)."""
    points = points.contiguous(); idx = idx.contiguous()
    _chk_float(points, "points"); _need_gpu(points)
    if idx.dtype != torch.int32:
        raise RuntimeError("idx must be an int tensor")
    B, N, C = points.shape
    M = idx.shape[1]
    out = torch.empty((B, M, C), device=points.device, dtype=torch.float32)
    check(lib().slide_gather_rows(B, N, M, C, ptr(points), ptr(idx), ptr(out), stream_of()), "gather_rows")
    return out


def sample_farthest_points(points, lengths=None, K=50, random_start_point=False, start_idx=None):
    """pytorch3d.ops.sample_farthest_points counterpart (call site point_upsample_decoder.py:178-180):
    -> (selected points (B,K,C), idx int64 (B,K)).  FPS on points[..., :3]; `random_start_point` draws the first index
    from torch's device generator (the reference's results are therefore only distributionally reproducible)."""
    assert lengths is None
    _need_gpu(points)
    xyz = points[:, :, 0:3].contiguous().float()
    B, N, _ = xyz.shape
    if start_idx is None and random_start_point:
        start_idx = torch.randint(0, N, (B,), device=points.device)
    sp = None
    if start_idx is not None:
        # any non-negative integer is a valid start: it is taken modulo N (callers hand one per-shape draw to every level of a
        # decoder, whose candidate counts differ -- ADVICE r4); no device sync, never out of bounds
        start_idx = torch.remainder(start_idx.to(device=points.device, dtype=torch.int64), N).to(torch.int32).contiguous()
        sp = ptr(start_idx)
    idx = torch.zeros((B, K), device=points.device, dtype=torch.int32)
    tmp = torch.full((B, N), 1e10, device=points.device, dtype=torch.float32)
    check(lib().slide_sample_farthest_points(B, N, int(K), ptr(xyz), sp, ptr(tmp), ptr(idx), stream_of()),
          "sample_farthest_points")
    idx = idx.long()
    return torch.gather(points, 1, idx.unsqueeze(-1).expand(-1, -1, points.shape[2])), idx


# ------------------------------------------------------------------ Chamfer / F1 metric (include/slide_hip.h Part 4)
def _pts3(t, name):
    """(B,N,C >= 3) float32 CUDA tensor read in place (xyz = the first three channels) -> (contiguous tensor, point stride)"""
    _need_gpu(t)
    _chk_float(t, name)
    if t.dim() != 3 or t.size(2) < 3:
        raise RuntimeError("%s must be a (B, N, C >= 3) tensor" % name)
    t = t.contiguous()
    return t, t.size(2)


def _lengths_ptr(lengths, dev):
    if lengths is None:
        return None, None
    lengths = lengths.to(device=dev, dtype=torch.int64).contiguous()
    return lengths, ptr(lengths)


def chamfer_nn(x, y, x_lengths=None, y_lengths=None):
    """nearest neighbour (K = 1) in both directions: x (B,P1,C>=3), y (B,P2,C>=3) f32 (xyz = channels 0:3), lengths (B,) int64 in
    [1, P] or None -> (d1 (B,P1) f32, i1 (B,P1) int64, d2 (B,P2), i2 (B,P2)): squared L2 distance to the nearest valid point of the
    other cloud and its index; slots beyond a cloud's length (0, 0).  Bit-equal to knn_points(K=1) in each direction."""
    x, sx = _pts3(x, "x")
    y, sy = _pts3(y, "y")
    _chk_cuda(y, "y")
    B, P1, P2 = x.size(0), x.size(1), y.size(1)
    if y.size(0) != B:
        raise RuntimeError("x and y must have the same batch size")
    d1 = torch.empty((B, P1), device=x.device, dtype=torch.float32)
    i1 = torch.empty((B, P1), device=x.device, dtype=torch.int64)
    d2 = torch.empty((B, P2), device=x.device, dtype=torch.float32)
    i2 = torch.empty((B, P2), device=x.device, dtype=torch.int64)
    lx, lxp = _lengths_ptr(x_lengths, x.device)
    ly, lyp = _lengths_ptr(y_lengths, x.device)
    check(lib().slide_chamfer_nn(B, P1, P2, ptr(x), sx, ptr(y), sy, lxp, lyp, ptr(d1), ptr(i1), ptr(d2), ptr(i2), stream_of()),
          "chamfer_nn")
    return d1, i1, d2, i2


def chamfer_reduce(d1, i1, d2, i2, x_lengths=None, y_lengths=None, threshold=1e-4, fx=None, fy=None, term=None):
    """per-cloud sums of chamfer_nn's output over the valid points, in a fixed order -> (B, 2, 5) f32:
    [pair][direction] = (sum d, sum sqrt d, count d < threshold, sum term, sum sqrt term).  fx (B,P1,F) / fy (B,P2,F) per-point
    features (any row stride: a channel slice of a (B,N,C) tensor is read in place) and term in {"mse", "cos"}, or both None."""
    mode = CHAMFER_TERM[term]
    B, P1 = d1.shape
    P2 = d2.shape[1]
    for t, n in ((d1, "d1"), (d2, "d2")):
        _chk_contig(t, n); _chk_float(t, n); _need_gpu(t)
    F = sfx = sfy = 0
    pfx = pfy = pi1 = pi2 = None
    if mode:
        i1 = i1.contiguous(); i2 = i2.contiguous()
        pi1, pi2 = ptr(i1), ptr(i2)
        F = fx.size(2)
        if fy.size(2) != F:
            raise RuntimeError("fx and fy must have the same number of channels")
        for t, n in ((fx, "fx"), (fy, "fy")):
            _chk_float(t, n); _need_gpu(t)
            if t.stride(2) != 1 or t.stride(0) != t.size(1) * t.stride(1):
                raise RuntimeError("%s must be a channel slice of a contiguous (B, N, C) tensor" % n)
        sfx, sfy = fx.stride(1), fy.stride(1)
        pfx, pfy = ptr(fx), ptr(fy)
    lx, lxp = _lengths_ptr(x_lengths, d1.device)
    ly, lyp = _lengths_ptr(y_lengths, d1.device)
    out = torch.empty((B, 2, 5), device=d1.device, dtype=torch.float32)
    check(lib().slide_chamfer_reduce(B, P1, P2, ptr(d1), pi1, ptr(d2), pi2, lxp, lyp, threshold, F, mode,
                                     pfx, sfx, pfy, sfy, ptr(out), stream_of()), "chamfer_reduce")
    return out


def chamfer_cd_bwd(x, y, d1, i1, d2, i2, dred, need_dx=True, need_dy=True):
    """backward of chamfer_reduce(*chamfer_nn(x, y), fx=x[:, :, 3:], fy=y[:, :, 3:], term="mse") (term None when C = 3) in one launch
    (include/slide_train.h slide_chamfer_cd_bwd): x (B,P1,C), y (B,P2,C) f32, C = 3 + F with F <= 16, (d1, i1, d2, i2) chamfer_nn's
    output for them, dred (B,2,5) the gradient of the reduced sums -> (dx (B,P1,C), dy (B,P2,C)); None for one that is not needed.
    Where a distance (or a feature term) is 0 its square root contributes the subgradient 0 (torch's autograd: NaN).  Deterministic:
    no atomics, every element stored once in a fixed summation order."""
    x, sx = _pts3(x, "x")
    y, sy = _pts3(y, "y")
    B, P1, P2, C = x.size(0), x.size(1), y.size(1), x.size(2)
    if y.size(0) != B or y.size(2) != C:
        raise RuntimeError("x and y must have the same batch size and channel count")
    if C - 3 > 16:
        raise RuntimeError("chamfer_cd_bwd supports at most 16 feature channels")
    for t, n, shape, dt in ((d1, "d1", (B, P1), torch.float32), (d2, "d2", (B, P2), torch.float32), (i1, "i1", (B, P1), torch.int64),
                            (i2, "i2", (B, P2), torch.int64), (dred, "dred", (B, 2, 5), torch.float32)):
        _chk_cuda(t, n); _chk_contig(t, n)
        if t.dtype != dt or tuple(t.shape) != shape:
            raise RuntimeError("%s must be a %s tensor of shape %s" % (n, dt, shape))
    dx = torch.empty((B, P1, C), device=x.device, dtype=torch.float32) if need_dx else None
    dy = torch.empty((B, P2, C), device=x.device, dtype=torch.float32) if need_dy else None
    check(lib().slide_chamfer_cd_bwd(B, P1, P2, C - 3, ptr(x), sx, ptr(y), sy, ptr(d1), ptr(i1), ptr(d2), ptr(i2), ptr(dred),
                                     ptr(dx), ptr(dy), stream_of()),
          "chamfer_cd_bwd")
    return dx, dy


def chamfer_pairwise(x, y=None):
    """all-pairs Chamfer sums of two sets of fixed-size clouds in one launch: x (M,P,C>=3), y (N,Q,C>=3) f32 CUDA tensors (xyz =
    channels 0:3, read in place) -> (M,N,2,2) f32, [i][j][direction] = (sum d, sum sqrt d): direction 0 over the points of x[i]
    towards y[j], direction 1 over the points of y[j] towards x[i].  y=None: the symmetric form (y is x; the upper triangle is
    computed and mirrored).  Every entry is bit-equal to chamfer_reduce(*chamfer_nn(x[i:i+1], y[j:j+1]))[0, :, :2]."""
    x, sx = _pts3(x, "x")
    symmetric = y is None
    if symmetric:
        y, sy = x, sx
    else:
        y, sy = _pts3(y, "y")
        if y.device != x.device:
            raise RuntimeError("x and y must be on the same device")
    M, P, N, Q = x.size(0), x.size(1), y.size(0), y.size(1)
    if M and N and not (P and Q):
        raise RuntimeError("chamfer_pairwise: clouds must hold at least one point")
    out = torch.empty((M, N, 2, 2), device=x.device, dtype=torch.float32)
    check(lib().slide_chamfer_pairwise(M, N, P, Q, ptr(x), sx, ptr(y), sy, int(symmetric), ptr(out), stream_of()),
          "chamfer_pairwise")
    return out


# point-pair evaluations (one exponential each: rows * N * P * Q * 3 sweeps * 10 levels) one launch of emd_pairwise may cover; a
# larger matrix is split into row blocks.  The kernel was measured at 3.9e12 evaluations/s on an MI355X (profiles/pairwise_emd.md),
# so a launch stays under a second: other work shares the device.
EMD_EVALS_PER_PAIR_OF_POINTS = 30
EMD_EVALS_PER_LAUNCH = 3.5e12


def emd_pairwise(x, y=None, paired=False, max_evals=None):
    """all-pairs approximate Earth Mover's Distance of two sets of fixed-size clouds (include/slide_hip.h slide_emd_pairwise): x
    (M,P,C>=3), y (N,Q,C>=3) f32 CUDA tensors (xyz = channels 0:3, read in place) -> (M,N) f32, [i][j] = the raw cost with x[i] as
    xyz1 and y[j] as xyz2 (not divided by a point count; not symmetric in its arguments).  y=None: the set against itself,
    computed in full.  paired=True: M == N and only the pairs (i, i) -> (M,).  A large matrix is split into row-block launches of
    at most max_evals (default EMD_EVALS_PER_LAUNCH) exponentials each, at least one row; every entry is bit-equal to what one
    launch gives, and to the paired form's."""
    x, sx = _pts3(x, "x")
    if y is None:
        y, sy = x, sx
    else:
        y, sy = _pts3(y, "y")
        if y.device != x.device:
            raise RuntimeError("x and y must be on the same device")
    M, P, N, Q = x.size(0), x.size(1), y.size(0), y.size(1)
    if paired and M != N:
        raise RuntimeError("emd_pairwise: the paired form needs as many clouds in y as in x")
    if M and N and not (P and Q):
        raise RuntimeError("emd_pairwise: clouds must hold at least one point")
    out = torch.empty((M,) if paired else (M, N), device=x.device, dtype=torch.float32)
    per_row = float(EMD_EVALS_PER_PAIR_OF_POINTS) * (1 if paired else max(N, 1)) * max(P, 1) * max(Q, 1)
    rows = int(max(1.0, min(float(max(M, 1)), (EMD_EVALS_PER_LAUNCH if max_evals is None else max_evals) // per_row)))
    for r0 in range(0, max(M, 1), rows):
        r1 = min(M, r0 + rows)
        yb = y[r0:r1] if paired else y
        check(lib().slide_emd_pairwise(r1 - r0, yb.size(0), P, Q, ptr(x[r0:r1]), sx, ptr(yb), sy, int(bool(paired)), ptr(out[r0:r1]),
                                       stream_of()), "emd_pairwise")
    return out


def occupancy_grid(points, axis, mask, return_cells=False):
    """occupancy counters of a set of clouds on an R^3 lattice in one launch (include/slide_hip.h slide_occupancy_grid): points
    (S,P,C>=3) f32 CUDA tensor (xyz = channels 0:3, read in place), axis (R,) f32 cell-centre coordinates of one axis (strictly
    ascending, 2 <= R <= 32), mask R^3 admissibility flags (bool / uint8, any shape of R^3 elements, flat index (i R + j) R + k)
    -> (counts (R^3,) int32: points whose nearest admissible cell is c, clouds (R^3,) int32: clouds with at least one such point);
    with return_cells also cells (S,P) int32, every point's cell.  axis and mask may be host tensors (they are uploaded).
    ValueError for a non-finite coordinate or a mask without an admissible cell (one host read of a flag word)."""
    points, sp = _pts3(points, "points")
    dev = points.device
    axis = torch.as_tensor(axis)
    if axis.dtype != torch.float32 or axis.dim() != 1:
        raise RuntimeError("axis must be a 1-D float tensor")
    R = axis.numel()
    if not 2 <= R <= 32:
        raise ValueError("the grid resolution must be in [2, 32], got %d" % R)
    mask = torch.as_tensor(mask)
    if mask.numel() != R ** 3 or mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("mask must hold R^3 = %d bool / uint8 flags" % R ** 3)
    S, P = points.size(0), points.size(1)
    if S * P > 2 ** 31 - 1:
        raise ValueError("occupancy_grid counts in 32 bits: at most 2^31 - 1 points per call")
    axis = axis.to(dev).contiguous()
    # a row of cells -> one word, bit k = cell (i, j, k)
    rowmask = ((mask.to(dev).reshape(R * R, R) != 0).long() << torch.arange(R, device=dev)).sum(1).to(torch.int32).contiguous()
    counts = torch.zeros(R ** 3, device=dev, dtype=torch.int32)
    clouds = torch.zeros(R ** 3, device=dev, dtype=torch.int32)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    cells = torch.empty((S, P), device=dev, dtype=torch.int32) if return_cells else None
    check(lib().slide_occupancy_grid(S, P, ptr(points), sp, R, ptr(axis), ptr(rowmask), ptr(counts), ptr(clouds),
                                     ptr(cells), ptr(flag), stream_of()), "occupancy_grid")
    if S and P:
        f = int(flag.item())
        if f & 1:
            raise ValueError("occupancy_grid: points holds a non-finite coordinate")
        if f & 2:
            raise ValueError("occupancy_grid: the mask admits no cell")
    return (counts, clouds, cells) if return_cells else (counts, clouds)


# ---------------------------------------------------------------------------------------------------------------- DPSR
FFT_SIZES = (16, 32, 64, 128, 256)
_DPSR_WORKSPACE_BYTES = 1 << 30  # dpsr_grid's default chunk: as many samples as keep its workspace within this


def _chk_f32_cuda(x, name, dim=None):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    _chk_float(x, name)
    if dim is not None and x.dim() != dim:
        raise RuntimeError("%s must have %d dimensions" % (name, dim))
    return x.contiguous()


def _chk_fft_size(r):
    if r not in FFT_SIZES:
        raise ValueError("the grid resolution must be one of %s, got %r" % (FFT_SIZES, r))


def _raise_dpsr_flag(flag, what):
    if int(flag.item()) & 1:
        raise ValueError("%s: a coordinate is non-finite or outside [0, 1), or a value is non-finite or not below 2^20" % what)


def _pts_vals(pts, vals, what):
    pts = _chk_f32_cuda(pts, "pts", 3)
    vals = _chk_f32_cuda(vals, "vals", 3)
    if pts.size(2) != 3 or pts.shape[:2] != vals.shape[:2]:
        raise ValueError("%s: pts (B,n,3) and vals (B,n,nf) must agree, got %s and %s" % (what, tuple(pts.shape), tuple(vals.shape)))
    return pts, vals


def point_rasterize_fixed(pts, vals, r):
    """the trilinear scatter in 64-bit fixed point (include/slide_hip.h slide_point_rasterize): pts (B,n,3) in [0, 1), vals (B,n,nf),
    nf 1 or 3 -> (B,nf,r,r,r) int64 in units of 2^-32.  Bit-reproducible; ValueError for a point the kernel left out."""
    pts, vals = _pts_vals(pts, vals, "point_rasterize")
    B, n, nf = vals.shape
    if nf not in (1, 3):
        raise ValueError("point_rasterize: 1 or 3 value columns, got %d" % nf)
    grid = torch.zeros((B, nf, r, r, r), device=pts.device, dtype=torch.int64)
    flag = torch.zeros(1, device=pts.device, dtype=torch.int32)
    check(lib().slide_point_rasterize(B, n, nf, r, ptr(pts), ptr(vals), ptr(grid), ptr(flag), stream_of()), "point_rasterize")
    if B and n:
        _raise_dpsr_flag(flag, "point_rasterize")
    return grid


def grid_fixed_to_float(grid):
    out = torch.empty(grid.shape, device=grid.device, dtype=torch.float32)
    check(lib().slide_grid_fixed_to_float(grid.numel(), ptr(grid), ptr(out), stream_of()), "grid_fixed_to_float")
    return out


def point_rasterize(pts, vals, r):
    """point_rasterize_fixed as floats: (B,nf,r,r,r) f32, each cell rounded once from the exact fixed-point sum"""
    return grid_fixed_to_float(point_rasterize_fixed(pts, vals, r))


def grid_interp(grid, pts):
    """trilinear gather (slide_grid_interp): grid (B,r,r,r,C) f32, pts (B,n,3) in [0, 1) -> (B,n,C)"""
    grid = _chk_f32_cuda(grid, "grid", 5)
    pts = _chk_f32_cuda(pts, "pts", 3)
    B, r, C = grid.size(0), grid.size(1), grid.size(4)
    if grid.size(2) != r or grid.size(3) != r or pts.size(0) != B or pts.size(2) != 3 or C < 1:
        raise ValueError("grid_interp: grid (B,r,r,r,C) and pts (B,n,3) expected, got %s and %s" % (tuple(grid.shape), tuple(pts.shape)))
    out = torch.empty((B, pts.size(1), C), device=grid.device, dtype=torch.float32)
    flag = torch.zeros(1, device=grid.device, dtype=torch.int32)
    check(lib().slide_grid_interp(B, pts.size(1), C, r, ptr(grid), ptr(pts), ptr(out), ptr(flag), stream_of()), "grid_interp")
    if B and pts.size(1):
        _raise_dpsr_flag(flag, "grid_interp")
    return out


def fft3_r2c(x):
    """numpy's rfftn over the last three axes: x (..., r, r, r) f32, or the int64 grid of point_rasterize_fixed (read times 2^-32)
    -> (..., r, r, r/2 + 1) complex64"""
    if not x.is_cuda or x.dtype not in (torch.float32, torch.int64) or x.dim() < 3:
        raise RuntimeError("fft3_r2c: a CUDA float or int64 tensor of at least three dimensions is expected")
    r = x.size(-1)
    _chk_fft_size(r)
    if x.size(-2) != r or x.size(-3) != r:
        raise ValueError("fft3_r2c: cubic grids only, got %s" % (tuple(x.shape),))
    x = x.contiguous()
    spec = torch.empty(tuple(x.shape[:-1]) + (r // 2 + 1, 2), device=x.device, dtype=torch.float32)
    check(lib().slide_fft3_r2c(x.numel() // r ** 3, r, ptr(x), int(x.dtype == torch.int64), ptr(spec), stream_of()), "fft3_r2c")
    return torch.view_as_complex(spec)


def fft3_c2r(spec, overwrite=False):
    """numpy's irfftn(s = (r, r, r)) over the last three axes: spec (..., r, r, r/2 + 1) complex64 -> (..., r, r, r) f32.  The
    kernels transform axes 1 and 2 in place: overwrite=False works on a copy."""
    if not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() < 3:
        raise RuntimeError("fft3_c2r: a CUDA complex64 tensor of at least three dimensions is expected")
    r = spec.size(-2)
    _chk_fft_size(r)
    if spec.size(-3) != r or spec.size(-1) != r // 2 + 1:
        raise ValueError("fft3_c2r: (..., r, r, r/2 + 1) expected, got %s" % (tuple(spec.shape),))
    work = torch.view_as_real(spec.contiguous() if overwrite else spec.clone(memory_format=torch.contiguous_format))
    out = torch.empty(tuple(spec.shape[:-1]) + (r,), device=spec.device, dtype=torch.float32)
    check(lib().slide_fft3_c2r(out.numel() // r ** 3, r, ptr(work), ptr(out), stream_of()), "fft3_c2r")
    return out


def dpsr_spectral(spec, G):
    """the spectral Poisson solve (slide_dpsr_spectral): spec (B,3,r,r,h) complex64, G r*r*h f32 -> (B,r,r,h) complex64"""
    if not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() != 5 or spec.size(1) != 3:
        raise RuntimeError("dpsr_spectral: a CUDA complex64 tensor (B,3,r,r,h) is expected")
    B, r = spec.size(0), spec.size(2)
    _chk_fft_size(r)
    G = _chk_f32_cuda(G, "G")
    if G.numel() != r * r * (r // 2 + 1) or tuple(spec.shape[2:]) != (r, r, r // 2 + 1):
        raise ValueError("dpsr_spectral: spec (B,3,r,r,r/2+1) and G of r*r*(r/2+1) values expected")
    s = torch.view_as_real(spec.contiguous())
    out = torch.empty((B, r, r, r // 2 + 1, 2), device=spec.device, dtype=torch.float32)
    check(lib().slide_dpsr_spectral(B, r, ptr(s), ptr(G), ptr(out), stream_of()), "dpsr_spectral")
    return torch.view_as_complex(out)


def dpsr_finish(phi, fv, shift=True, scale=True):
    """shift and scale IN PLACE (slide_dpsr_finish): phi (B,r,r,r) f32, fv (B,n) f32 -> phi"""
    phi = _chk_f32_cuda(phi, "phi", 4)
    fv = _chk_f32_cuda(fv, "fv", 2)
    B, r = phi.size(0), phi.size(1)
    coef = torch.empty((B, 2), device=phi.device, dtype=torch.float32)
    check(lib().slide_dpsr_finish(B, fv.size(1), r, ptr(fv), int(shift), int(scale), ptr(coef), ptr(phi), stream_of()), "dpsr_finish")
    return phi


def dpsr_chunk(r, n, chunk=None):
    """samples per slide_dpsr_grid call: the workspace (int64 grid + half spectra, about 84 MB per sample at r 128) stays bounded"""
    if chunk is not None:
        if int(chunk) < 1:
            raise ValueError("chunk must be positive")
        return int(chunk)
    h = r // 2 + 1
    per = 3 * r ** 3 * 8 + 4 * r * r * h * 8 + 4 * n + 8
    return max(1, _DPSR_WORKSPACE_BYTES // per)


def _dpsr_args(pts, normals, G, what):
    pts, normals = _pts_vals(pts, normals, what)
    if normals.size(2) != 3 or pts.size(1) < 1:
        raise ValueError("%s: normals (B,n,3) with n >= 1 expected, got %s" % (what, tuple(normals.shape)))
    G = _chk_f32_cuda(G, "G")
    r = G.size(0)
    _chk_fft_size(r)
    if G.numel() != r * r * (r // 2 + 1):
        raise ValueError("%s: G must hold r*r*(r/2+1) values" % what)
    return pts, normals, G, r


def dpsr_grid(pts, normals, G, shift=True, scale=True, chunk=None, return_coef=False):
    """DPSR.forward on the composed entry point (slide_dpsr_grid): pts / normals (B,n,3) f32, G the filter of r*r*(r/2+1) floats of
    shape (r,r,r/2+1,...) -> phi (B,r,r,r) f32.  Samples run `chunk` at a time (default: dpsr_chunk); a sample's grid does not depend
    on the chunk or the batch.  One host read of a flag word at the end: ValueError for a point the kernels rejected.
    return_coef: -> (phi, coef (B,2) f32), coef = (offset, |phi[0,0,0] - offset|) per sample as slide_dpsr_finish computes them
    (zeros without shift and scale) -- what dpsr_grid_backward needs; the launches and phi's bits are the same."""
    pts, normals, G, r = _dpsr_args(pts, normals, G, "dpsr_grid")
    h = r // 2 + 1
    B, n = pts.size(0), pts.size(1)
    dev = pts.device
    phi = torch.empty((B, r, r, r), device=dev, dtype=torch.float32)
    coef = torch.zeros((B, 2), device=dev, dtype=torch.float32) if return_coef else None
    if B == 0:
        return (phi, coef) if return_coef else phi
    cb = min(dpsr_chunk(r, n, chunk), B)
    ws_grid = torch.empty((cb, 3, r, r, r), device=dev, dtype=torch.int64)
    ws_spec = torch.empty((cb, 3, r, r, h, 2), device=dev, dtype=torch.float32)
    ws_phis = torch.empty((cb, r, r, h, 2), device=dev, dtype=torch.float32)
    ws_fv = torch.empty((cb, n), device=dev, dtype=torch.float32)
    ws_coef = None if return_coef else torch.empty((cb, 2), device=dev, dtype=torch.float32)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    for s in range(0, B, cb):
        e = min(s + cb, B)
        check(lib().slide_dpsr_grid(e - s, n, r, ptr(pts[s:e]), ptr(normals[s:e]), ptr(G), int(shift), int(scale), ptr(ws_grid),
                                    ptr(ws_spec), ptr(ws_phis), ptr(ws_fv), ptr(coef[s:e] if return_coef else ws_coef), ptr(phi[s:e]),
                                    ptr(flag), stream_of()),
              "dpsr_grid")
    _raise_dpsr_flag(flag, "dpsr_grid")
    return (phi, coef) if return_coef else phi


def dpsr_bwd_sum_blocks(r):
    """workgroups per sample of the first stage of slide_dpsr_bwd_sums"""
    return (r ** 3 + 4095) // 4096


def dpsr_bwd_sums(g, phi):
    """per-sample (sum g, sum g * phi) in double, fixed order (slide_dpsr_bwd_sums): g, phi (B,r,r,r) f32 -> (B,2) f64"""
    g = _chk_f32_cuda(g, "g", 4)
    phi = _chk_f32_cuda(phi, "phi", 4)
    if g.shape != phi.shape:
        raise ValueError("dpsr_bwd_sums: g and phi must have the same shape")
    B, r = g.size(0), g.size(1)
    part = torch.empty((B, dpsr_bwd_sum_blocks(r), 2), device=g.device, dtype=torch.float64)
    sums = torch.empty((B, 2), device=g.device, dtype=torch.float64)
    check(lib().slide_dpsr_bwd_sums(B, r, ptr(g), ptr(phi), ptr(part), ptr(sums), stream_of()), "dpsr_bwd_sums")
    return sums


def dpsr_bwd_dpre(g, phi, sums, coef, w, n, shift=True, scale=True):
    """the adjoint of the finish and the shift (slide_dpsr_bwd_dpre): g, phi (B,r,r,r) f32, sums (B,2) f64, coef (B,2) f32, w
    (B,r,r,r) int64 = point_rasterize_fixed(pts, ones) or None without shift -> dpre (B,r,r,r) f32"""
    g = _chk_f32_cuda(g, "g", 4)
    phi = _chk_f32_cuda(phi, "phi", 4)
    B, r = g.size(0), g.size(1)
    if shift and (w is None or w.dtype != torch.int64 or w.numel() != g.numel()):
        raise ValueError("dpsr_bwd_dpre: with shift, w must be the int64 density grid of g's size")
    out = torch.empty_like(g)
    check(lib().slide_dpsr_bwd_dpre(B, n, r, ptr(g), ptr(phi), ptr(sums), ptr(coef), ptr(w.contiguous()) if shift else None, int(shift),
                                    int(scale), ptr(out), stream_of()), "dpsr_bwd_dpre")
    return out


def dpsr_spectral_adj(spec, G):
    """the adjoint of dpsr_spectral (slide_dpsr_spectral_adj): spec (B,r,r,h) complex64, G r*r*h f32 -> (B,3,r,r,h) complex64"""
    if not spec.is_cuda or spec.dtype != torch.complex64 or spec.dim() != 4:
        raise RuntimeError("dpsr_spectral_adj: a CUDA complex64 tensor (B,r,r,h) is expected")
    B, r = spec.size(0), spec.size(1)
    _chk_fft_size(r)
    G = _chk_f32_cuda(G, "G")
    if G.numel() != r * r * (r // 2 + 1) or tuple(spec.shape[1:]) != (r, r, r // 2 + 1):
        raise ValueError("dpsr_spectral_adj: spec (B,r,r,r/2+1) and G of r*r*(r/2+1) values expected")
    s = torch.view_as_real(spec.contiguous())
    out = torch.empty((B, 3, r, r, r // 2 + 1, 2), device=spec.device, dtype=torch.float32)
    check(lib().slide_dpsr_spectral_adj(B, r, ptr(s), ptr(G), ptr(out), stream_of()), "dpsr_spectral_adj")
    return torch.view_as_complex(out)


def dpsr_bwd_points(pts, normals, dras, phi=None, sums=None, coef=None, shift=False, scale=False, need_v=True, need_n=True):
    """the per-point gather of the backward (slide_dpsr_bwd_points): pts / normals (B,n,3), dras (B,3,r,r,r) f32 and, with shift,
    phi (B,r,r,r), sums (B,2) f64, coef (B,2) -> (dV, dN), each (B,n,3) or None when not needed"""
    pts, normals = _pts_vals(pts, normals, "dpsr_bwd_points")
    dras = _chk_f32_cuda(dras, "dras", 5)
    B, n, r = pts.size(0), pts.size(1), dras.size(2)
    if normals.size(2) != 3 or tuple(dras.shape) != (B, 3, r, r, r):
        raise ValueError("dpsr_bwd_points: normals (B,n,3) and dras (B,3,r,r,r) expected")
    if shift:
        phi = _chk_f32_cuda(phi, "phi", 4)
        if tuple(phi.shape) != (B, r, r, r):
            raise ValueError("dpsr_bwd_points: phi (B,r,r,r) expected")
    dv = torch.empty_like(pts) if need_v else None
    dn = torch.empty_like(pts) if need_n else None
    flag = torch.zeros(1, device=pts.device, dtype=torch.int32)
    check(lib().slide_dpsr_bwd_points(B, n, r, ptr(pts), ptr(normals), ptr(dras), ptr(phi) if shift else None,
                                      ptr(sums) if shift else None, ptr(coef) if shift else None, int(shift), int(scale),
                                      ptr(dv) if need_v else None, ptr(dn) if need_n else None, ptr(flag), stream_of()), "dpsr_bwd_points")
    if B and n and (need_v or need_n):
        _raise_dpsr_flag(flag, "dpsr_bwd_points")
    return dv, dn


def dpsr_grid_backward(pts, normals, G, phi, coef, g, shift=True, scale=True, need_v=True, need_n=True, chunk=None):
    """the backward of dpsr_grid on the composed entry point (slide_dpsr_grid_bwd): phi, coef = dpsr_grid(..., return_coef=True),
    g = dL/dphi (B,r,r,r) f32 -> (dV, dN), each (B,n,3) f32 or None when not needed.  Samples run `chunk` at a time exactly as in
    dpsr_grid (the workspace per sample is the forward's); a sample's gradients do not depend on the chunk or the batch."""
    pts, normals, G, r = _dpsr_args(pts, normals, G, "dpsr_grid_backward")
    phi = _chk_f32_cuda(phi, "phi", 4)
    g = _chk_f32_cuda(g, "g", 4)
    coef = _chk_f32_cuda(coef, "coef", 2)
    B, n = pts.size(0), pts.size(1)
    if tuple(phi.shape) != (B, r, r, r) or g.shape != phi.shape or tuple(coef.shape) != (B, 2):
        raise ValueError("dpsr_grid_backward: phi and g (B,r,r,r) and coef (B,2) expected, got %s, %s and %s" % (
            tuple(phi.shape), tuple(g.shape), tuple(coef.shape)))
    dev = pts.device
    dv = torch.empty_like(pts) if need_v else None
    dn = torch.empty_like(pts) if need_n else None
    if B == 0 or not (need_v or need_n):
        return dv, dn
    h = r // 2 + 1
    cb = min(dpsr_chunk(r, n, chunk), B)
    ws_w = torch.empty((cb, r, r, r), device=dev, dtype=torch.int64) if shift else None
    ws_ones = torch.empty((cb, n), device=dev, dtype=torch.float32) if shift else None
    ws_dpre = torch.empty((cb, r, r, r), device=dev, dtype=torch.float32)
    ws_spec = torch.empty((cb, r, r, h, 2), device=dev, dtype=torch.float32)
    ws_spec3 = torch.empty((cb, 3, r, r, h, 2), device=dev, dtype=torch.float32)
    ws_dras = torch.empty((cb, 3, r, r, r), device=dev, dtype=torch.float32)
    ws_part = torch.empty((cb, dpsr_bwd_sum_blocks(r), 2), device=dev, dtype=torch.float64)
    ws_sums = torch.empty((cb, 2), device=dev, dtype=torch.float64)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    for s in range(0, B, cb):
        e = min(s + cb, B)
        check(lib().slide_dpsr_grid_bwd(e - s, n, r, ptr(pts[s:e]), ptr(normals[s:e]), ptr(G), ptr(phi[s:e]), ptr(coef[s:e]), ptr(g[s:e]),
                                        int(shift), int(scale), ptr(ws_w) if shift else None, ptr(ws_ones) if shift else None,
                                        ptr(ws_dpre), ptr(ws_spec), ptr(ws_spec3), ptr(ws_dras), ptr(ws_part), ptr(ws_sums),
                                        ptr(dv[s:e]) if need_v else None, ptr(dn[s:e]) if need_n else None, ptr(flag), stream_of()),
              "dpsr_grid_backward")
    _raise_dpsr_flag(flag, "dpsr_grid_backward")
    return dv, dn


# ---------------------------------------------------------------------------------------------------------------- marching cubes
MC_RMAX = 256
_MC_WORKSPACE_BYTES = 1 << 30  # marching_cubes' default chunk: as many grids as keep the per-point id volume within this


def mc_bricks(r):
    """workgroups per grid of slide_mc_count / slide_mc_emit (slide_mc_bricks)"""
    n = lib().slide_mc_bricks(int(r))
    if n < 0:
        raise ValueError("marching_cubes: the grid resolution must be in [2, %d], got %r" % (MC_RMAX, r))
    return n


def marching_cubes(phi, level=0.0, chunk=None):
    """slide_mc_count + slide_mc_emit: phi (B,r,r,r) f32, 2 <= r <= 256 -> a list of B tuples (verts (V,3) f32 in grid-index units,
    faces (F,3) int32 local to the grid, normals (V,3) f32).  Grids run `chunk` at a time (default: the int32 id volume stays within
    1 GiB); a grid's mesh does not depend on the chunk, the batch or its position.  One host read of the per-grid totals per chunk
    sizes the outputs."""
    phi = _chk_f32_cuda(phi, "phi", 4)
    B, r = phi.size(0), phi.size(1)
    if phi.size(2) != r or phi.size(3) != r:
        raise ValueError("marching_cubes: cubic grids (B,r,r,r) only, got %s" % (tuple(phi.shape),))
    nbricks = mc_bricks(r)
    if chunk is not None and int(chunk) < 1:
        raise ValueError("chunk must be positive")
    cb = max(1, min(B, int(chunk) if chunk is not None else _MC_WORKSPACE_BYTES // (4 * r ** 3)))
    dev, out = phi.device, []
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    if B == 0:
        return out
    counts = torch.empty((cb, nbricks, 2), **i32)
    totals = torch.empty((cb, 4), device=dev, dtype=torch.int64)
    ws = torch.empty((cb, r, r, r), **i32)
    for s in range(0, B, cb):
        e = min(s + cb, B)
        check(lib().slide_mc_count(e - s, r, ptr(phi[s:e]), float(level), ptr(counts), ptr(totals), stream_of()), "mc_count")
        tot = totals[:e - s].cpu().tolist()
        nv, nf = sum(t[0] for t in tot), sum(t[1] for t in tot)
        verts, normals, faces = torch.empty((nv, 3), **f32), torch.empty((nv, 3), **f32), torch.empty((nf, 3), **i32)
        if nv:
            check(lib().slide_mc_emit(e - s, r, ptr(phi[s:e]), float(level), ptr(counts), ptr(totals), ptr(verts), ptr(normals),
                                      ptr(faces), ptr(ws), stream_of()), "mc_emit")
        for v, f, v0, f0 in tot:
            out.append((verts[v0:v0 + v], faces[f0:f0 + f], normals[v0:v0 + v]))
    return out


# ---------------------------------------------------------------------------------------------------------------- mesh sampling
MESH_SAMPLE_MAX_BATCH = 65535


def mesh_cdf_span(level):
    """faces per thread (0), wave (1) and workgroup pass (2) of the cdf scan (slide_mesh_cdf_span)"""
    return lib().slide_mesh_cdf_span(int(level))


def _mesh_offsets(off, rows, name, dev):
    """host offsets (b + 1) -> (device int64 tensor, b): checked here, because the kernels trust them"""
    off = [int(x) for x in (off.tolist() if hasattr(off, "tolist") else off)]
    if len(off) < 1 or off[0] != 0 or off[-1] != rows or any(a > b for a, b in zip(off, off[1:])):
        raise ValueError("%s must run from 0 to %d without decreasing, got %s" % (name, rows, off if len(off) <= 8 else off[:8] + ["..."]))
    return torch.tensor(off, device=dev, dtype=torch.int64), len(off) - 1


def _mesh_faces(faces, voff, foff, nv, verts=None):
    """the face and offset checks of every packed-mesh entry point -> (faces, voff, foff as device tensors, b); verts: the caller's
    (sum V, 3) tensor when it has one -- its shape then joins the shape check, and nv = its rows"""
    if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
        raise RuntimeError("faces must be a CUDA tensor")
    _chk_int(faces, "faces")
    faces = faces.contiguous()
    faces_ok = faces.dim() == 2 and faces.size(1) == 3
    if verts is None:
        if not faces_ok:
            raise ValueError("packed faces are (sum F, 3), got %s" % (tuple(faces.shape),))
        if nv > 2 ** 31 - 1 or faces.size(0) > 2 ** 31 - 1:
            raise ValueError("at most 2^31 - 1 vertices and faces per call")
    else:
        if verts.size(1) != 3 or not faces_ok:
            raise ValueError("packed meshes are verts (sum V, 3) and faces (sum F, 3), got %s and %s" % (tuple(verts.shape), tuple(faces.shape)))
        if faces.size(0) > 2 ** 31 - 1:
            raise ValueError("at most 2^31 - 1 faces per call")
    dev = faces.device if verts is None else verts.device
    vo, b = _mesh_offsets(voff, nv, "voff", dev)
    fo, bf = _mesh_offsets(foff, faces.size(0), "foff", dev)
    if b != bf:
        raise ValueError("voff and foff describe %d and %d meshes" % (b, bf))
    return faces, vo, fo, b


def mesh_face_cdf(verts, faces, voff, foff):
    """slide_mesh_face_cdf on packed meshes: verts (sum V, 3) f32 and faces (sum F, 3) int32 CUDA tensors (vertex indices local to the
    mesh), voff / foff (b + 1) HOST offsets -> (areas (sum F,) f32, cdf (sum F,) int64 holding the uint64 sums, voff, foff as device
    tensors).  ValueError after one read of the flag word for a face index out of its mesh's range or a non-finite vertex of a face."""
    verts = _chk_f32_cuda(verts, "verts", 2)
    faces, vo, fo, b = _mesh_faces(faces, voff, foff, verts.size(0), verts)
    nf = faces.size(0)
    areas = torch.empty(nf, device=verts.device, dtype=torch.float32)
    cdf = torch.empty(nf, device=verts.device, dtype=torch.int64)
    if b and nf:
        if not verts.size(0):
            raise ValueError("mesh_face_cdf: faces without vertices")
        flag = torch.zeros(1, device=verts.device, dtype=torch.int32)
        check(lib().slide_mesh_face_cdf(b, nf, ptr(verts), ptr(faces), ptr(vo), ptr(fo), ptr(areas), ptr(cdf), ptr(flag), stream_of()),
              "mesh_face_cdf")
        f = int(flag.item())
        if f & 1:
            raise ValueError("mesh_face_cdf: a face holds a vertex index outside [0, V) of its mesh")
        if f & 2:
            raise ValueError("mesh_face_cdf: a face refers to a vertex with a non-finite coordinate")
    return areas, cdf, vo, fo


def mesh_sample(verts, faces, voff, foff, cdf, num_samples, seed=0, mesh_ids=None, stream_id=0, vnormals=None, normals=None,
                return_face_idx=False, words=None):
    """slide_mesh_sample with cdf, voff, foff as mesh_face_cdf returned them (device tensors): -> (points (b,S,3), normals (b,S,3)
    or None, face_idx (b,S) int32 or None, valid (b,) int32).  normals: None, "face" or "vertex" (interpolated from vnormals
    (sum V, 3)); mesh_ids (b,) integers, default the position; words (b,S,4) integers in [0, 2^32) replace the Philox draw."""
    verts = _chk_f32_cuda(verts, "verts", 2)
    for t, name, dtype in ((faces, "faces", torch.int32), (voff, "voff", torch.int64), (foff, "foff", torch.int64), (cdf, "cdf", torch.int64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError("%s must be a contiguous CUDA %s tensor, as mesh_face_cdf returns it" % (name, dtype))
    if voff.numel() != foff.numel() or voff.numel() < 1 or cdf.numel() != faces.size(0):
        raise ValueError("mesh_sample: voff, foff and cdf do not describe the same meshes")
    dev, b, S = verts.device, voff.numel() - 1, int(num_samples)
    if normals not in (None, "face", "vertex"):
        raise ValueError("normals must be None, 'face' or 'vertex', got %r" % (normals,))
    if S < 0:
        raise ValueError("num_samples must not be negative")
    if b > MESH_SAMPLE_MAX_BATCH:
        raise ValueError("at most %d meshes per call" % MESH_SAMPLE_MAX_BATCH)
    if normals == "vertex":
        if vnormals is None:
            raise ValueError("normals='vertex' needs the meshes' vertex normals")
        vnormals = _chk_f32_cuda(vnormals, "vertex normals", 2)
        if vnormals.shape != verts.shape:
            raise ValueError("vertex normals %s do not match verts %s" % (tuple(vnormals.shape), tuple(verts.shape)))
    seed = int(seed) & (2 ** 64 - 1)
    i32 = lambda w: ((int(w) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000  # noqa: E731  (the C int with that bit pattern)
    ids = None
    if mesh_ids is not None:
        ids = torch.as_tensor([i32(x) for x in (mesh_ids.tolist() if hasattr(mesh_ids, "tolist") else mesh_ids)], dtype=torch.int32).to(dev)
        if ids.numel() != b:
            raise ValueError("mesh_ids must hold one number per mesh (%d), got %d" % (b, ids.numel()))
    if words is not None:
        words = torch.as_tensor(words)
        if tuple(words.shape) != (b, S, 4):
            raise ValueError("words must be (b, S, 4) = %s, got %s" % ((b, S, 4), tuple(words.shape)))
        # uint32 bit patterns in an int32 tensor
        words = ((words.to(torch.int64) & 0xFFFFFFFF) ^ 0x80000000).sub_(0x80000000).to(torch.int32).to(dev).contiguous()
    f32 = dict(device=dev, dtype=torch.float32)
    points = torch.zeros((b, S, 3), **f32)
    out_n = torch.zeros((b, S, 3), **f32) if normals else None
    fidx = torch.full((b, S), -1, device=dev, dtype=torch.int32) if return_face_idx else None
    valid = torch.zeros(b, device=dev, dtype=torch.int32)
    if b and S and faces.size(0) and verts.size(0):
        check(lib().slide_mesh_sample(b, S, ptr(verts), ptr(faces), ptr(vnormals) if normals == "vertex" else None, ptr(voff),
                                      ptr(foff), ptr(cdf), i32(seed), i32(seed >> 32), i32(stream_id), ptr(ids), ptr(words),
                                      1 if normals == "vertex" else 0, ptr(points), ptr(out_n), ptr(fidx), ptr(valid), stream_of()),
              "mesh_sample")
    return points, out_n, fidx, valid


# ---------------------------------------------------------------------------------------------------------------- mesh components
MESH_CC_GROUP = 4  # rounds of labelling per host read of the status words (profiles/mesh_components.md)
_MESH_CC_ROUND_CAP = -5  # slide_mesh_cc_label: more rounds than max_rounds


def mesh_cc_span(level):
    """elements per workgroup of the per-face / per-vertex launches (0), per wave (1) and per workgroup pass (2) of the per-mesh scans
    (slide_mesh_cc_span)"""
    return lib().slide_mesh_cc_span(int(level))


def mesh_cc_label(faces, voff, foff, nv, group=None, max_rounds=None):
    """slide_mesh_cc_label on packed faces (sum F, 3) int32 CUDA (vertex indices local to the mesh) with HOST offsets voff / foff (b + 1)
    and nv = sum V -> (labels (sum V,) int32 = every vertex's root, the smallest index of its component; voff, foff as device tensors;
    info = dict(rounds, reads, issued)).  ValueError for a face index outside [0, V) of its mesh (tested on the device before it is
    used; the status words are read once per `group` rounds); RuntimeError beyond max_rounds (default: the largest V + 1, which
    always suffices)."""
    nv = int(nv)
    faces, vo, fo, b = _mesh_faces(faces, voff, foff, nv)
    nf, dev = faces.size(0), faces.device
    if b > MESH_SAMPLE_MAX_BATCH:
        raise ValueError("at most %d meshes per call" % MESH_SAMPLE_MAX_BATCH)
    if nf and not nv:
        raise ValueError("mesh_components: faces without vertices")
    host_v = [int(x) for x in (voff.tolist() if hasattr(voff, "tolist") else voff)]
    group = MESH_CC_GROUP if group is None else int(group)
    cap = (max(hi - lo for lo, hi in zip(host_v, host_v[1:])) + 1 if b else 1) if max_rounds is None else int(max_rounds)
    if group < 1 or cap < 1:
        raise ValueError("group and max_rounds must be positive")
    labels = torch.empty(nv, device=dev, dtype=torch.int32)
    info = (ctypes.c_int * 4)()
    if b and nv:
        state = torch.empty(2, device=dev, dtype=torch.int32)
        st = lib().slide_mesh_cc_label(b, nv, nf, ptr(faces), ptr(vo), ptr(fo), ptr(labels), ptr(state), group, cap,
                                       ctypes.addressof(info), stream_of())
        if st == _MESH_CC_ROUND_CAP:
            raise RuntimeError("mesh_components: the labels did not settle within %d rounds" % cap)
        check(st, "mesh_cc_label")
        if info[0]:
            raise ValueError("mesh_components: a face holds a vertex index outside [0, V) of its mesh")
    return labels, vo, fo, dict(rounds=int(info[1]), reads=int(info[2]), issued=int(info[3]))


def mesh_cc_stats(faces, voff, foff, labels):
    """slide_mesh_cc_stats with labels, voff, foff as mesh_cc_label returned them -> (cid (sum V,), nverts (sum V,), nfaces (sum V,),
    totals (b, 4), cnt_v, cnt_f): int32 device tensors; nverts / nfaces hold a mesh's C counts from its first row on, totals[:, 2] = C;
    cnt_v / cnt_f hold the counts at every root's row (what mesh_cc_select reads)."""
    nv, nf, b, dev = labels.numel(), faces.size(0), voff.numel() - 1, labels.device
    new = lambda n: torch.empty(n, device=dev, dtype=torch.int32)  # noqa: E731
    cnt_v, cnt_f, rank, cid, nverts, nfaces = (new(nv) for _ in range(6))
    totals = torch.zeros((b, 4), device=dev, dtype=torch.int32)
    if b and nv:
        check(lib().slide_mesh_cc_stats(b, nv, nf, ptr(faces), ptr(voff), ptr(foff), ptr(labels), ptr(cnt_v), ptr(cnt_f), ptr(rank),
                                        ptr(cid), ptr(nverts), ptr(nfaces), ptr(totals), stream_of()), "mesh_cc_stats")
    return cid, nverts, nfaces, totals, cnt_v, cnt_f


def mesh_cc_select(faces, voff, foff, labels, cnt_v, cnt_f, totals, by="verts", min_size=0, keep="largest"):
    """slide_mesh_cc_select -> (vnew (sum V,), fnew (sum F,)) int32: a row's place among its mesh's kept rows, or -1; totals[:, 0],
    [:, 1] and [:, 3] receive V', F' and the selected root"""
    if by not in ("verts", "faces"):
        raise ValueError("by must be 'verts' or 'faces', got %r" % (by,))
    if keep not in ("largest", "all"):
        raise ValueError("keep must be 'largest' or 'all', got %r" % (keep,))
    nv, nf, b, dev = labels.numel(), faces.size(0), voff.numel() - 1, labels.device
    vnew = torch.empty(nv, device=dev, dtype=torch.int32)
    fnew = torch.full((nf,), -1, device=dev, dtype=torch.int32)
    if b and nv:
        check(lib().slide_mesh_cc_select(b, nv, nf, ptr(faces), ptr(voff), ptr(foff), ptr(labels), ptr(cnt_v), ptr(cnt_f),
                                         1 if by == "faces" else 0, max(-2 ** 62, min(2 ** 62, int(min_size))), 1 if keep == "all" else 0,
                                         ptr(vnew), ptr(fnew), ptr(totals), stream_of()), "mesh_cc_select")
    return vnew, fnew


def mesh_cc_compact(verts, normals, faces, voff, foff, vnew, fnew, kept_v, kept_f):
    """slide_mesh_cc_compact with kept_v / kept_f = the HOST lists of V' / F' per mesh -> (verts (sum V', 3), normals or None,
    faces (sum F', 3), vert_idx (sum V',), ovoff, ofoff as host lists)"""
    verts = _chk_f32_cuda(verts, "verts", 2)
    dev, b = verts.device, voff.numel() - 1
    ovoff, ofoff = [0], [0]
    for v, f in zip(kept_v, kept_f):
        ovoff.append(ovoff[-1] + int(v))
        ofoff.append(ofoff[-1] + int(f))
    if normals is not None:
        normals = _chk_f32_cuda(normals, "normals", 2)
        if normals.shape != verts.shape:
            raise ValueError("normals %s do not match verts %s" % (tuple(normals.shape), tuple(verts.shape)))
    out_v = torch.empty((ovoff[-1], 3), device=dev, dtype=torch.float32)
    out_n = torch.empty((ovoff[-1], 3), device=dev, dtype=torch.float32) if normals is not None else None
    out_f = torch.empty((ofoff[-1], 3), device=dev, dtype=torch.int32)
    vidx = torch.empty(ovoff[-1], device=dev, dtype=torch.int32)
    if b and ovoff[-1]:
        ov = torch.tensor(ovoff, device=dev, dtype=torch.int64)
        of = torch.tensor(ofoff, device=dev, dtype=torch.int64)
        check(lib().slide_mesh_cc_compact(b, verts.size(0), faces.size(0), ptr(verts), ptr(normals), ptr(faces), ptr(voff), ptr(foff),
                                          ptr(vnew), ptr(fnew), ptr(ov), ptr(of), ptr(out_v), ptr(out_n), ptr(out_f), ptr(vidx),
                                          stream_of()), "mesh_cc_compact")
    return out_v, out_n, out_f, vidx, ovoff, ofoff
