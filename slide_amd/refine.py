"""The refine-and-upsample front of DPSR on the HIP kernels of csrc/refine_front.hip (include/slide_hip.h Part 9): mirror a cloud
across a plane through its centroid and tag the halves, split every point into its children, normalise and clamp them into DPSR's
cube -- what the reference does with torch ops in data_utils/mirror_partial.py, models/point_upsample_module.py and the tail of
network_output_to_dpsr_grid.  fp32, every operation rounded once in the reference's order: bit-equal to it, for a sample alone, at
any batch position and on every run.  CUDA float32 tensors only; no CPU path."""
import ctypes

import torch

from ._lib import check, lib
from .abi import ptr, stream_of

ST_MESSAGES = {-2: "a count is out of range, an array is missing or misaligned", -3: "X must have 6 channels, or 7 with the indicator",
               -4: "the displacement's width does not match the form", -5: "include_displacement_center_to_final_output needs "
               "first_refine_coarse_points", -6: "point_upsample_factor must be at least 1"}


def _f32(x, name, dim=3):
    """dtype and rank; the device is checked by _cuda AFTER the argument checks, so those are testable without a GPU"""
    if not isinstance(x, torch.Tensor):
        raise RuntimeError("%s must be a tensor" % name)
    if x.dtype != torch.float32:
        raise RuntimeError("%s must be a float tensor" % name)
    if x.dim() != dim:
        raise RuntimeError("%s must have %d dimensions" % (name, dim))
    return x.contiguous()


def _cuda(x, name):
    if not x.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor (there is no CPU path)" % name)


def refine_permutation(n, seed):
    """the permutation of a run's 2N mirrored-and-concatenated rows: torch.randperm(n) of a CPU generator seeded with `seed`, int32.
    One permutation serves every batch of a run, so a shape's result does not depend on how the shapes are batched."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randperm(int(n), generator=g).to(torch.int32)


def _status(st, what):
    if st in ST_MESSAGES and st != 0:
        raise ValueError("%s: %s" % (what, ST_MESSAGES[st]))
    check(st, what)


@torch.no_grad()
def mirror_and_concat(x, axis=2, attach_label=True, perm=None):
    """x (B, N, C) CUDA f32, C >= 3 -> (out (B, 2N, C + attach_label), center (B, 3)).  center = the mean of x[:, :, 0:3] (summed in
    double, rounded once); out = [x, label +1; x mirrored across the plane through center normal to `axis`, label -1], rows taken in
    the order perm (2N,) when given.  With C >= 6 channel axis + 3 (the normal's component) is negated too.  ValueError for a perm
    entry outside [0, 2N)."""
    x = _f32(x, "x")
    B, N, C = x.shape
    if C < 3:
        raise ValueError("mirror_and_concat: x needs at least 3 channels, got %d" % C)
    if axis not in (0, 1, 2):
        raise ValueError("mirror_and_concat: axis must be 0, 1 or 2, got %r" % (axis,))
    if perm is not None:
        if not isinstance(perm, torch.Tensor) or perm.dim() != 1 or perm.numel() != 2 * N or perm.dtype not in (torch.int32, torch.int64):
            raise ValueError("mirror_and_concat: perm must be an integer tensor of %d entries" % (2 * N))
    _cuda(x, "x")
    if perm is not None:
        perm = perm.to(device=x.device, dtype=torch.int32).contiguous()
    label = 1 if attach_label else 0
    out = torch.empty((B, 2 * N, C + label), device=x.device, dtype=torch.float32)
    center = torch.empty((B, 3), device=x.device, dtype=torch.float32)
    if B == 0 or N == 0:
        return out, center
    flag = torch.empty(2, device=x.device, dtype=torch.int32)
    with torch.cuda.device(x.device):
        _status(lib().slide_mirror_concat(B, N, C, ptr(x), int(axis), label, ptr(perm), ptr(out), ptr(center), ptr(flag), stream_of()),
                "mirror_and_concat")
    if perm is not None:
        bits, smp = flag.tolist()
        if bits & 1:
            raise ValueError("mirror_and_concat: perm has an entry outside [0, %d)" % (2 * N))
    return out, center


def refined_rows(rows, factor, first_refine, include_center):
    """output rows per sample of refine_to_dpsr_points"""
    return rows * (factor - 1) + rows if include_center else rows * factor


@torch.no_grad()
def refine_to_dpsr_points(X, displacement, factor, first_refine_coarse_points=False,
                          include_displacement_center_to_final_output=False, output_scale_factor=0.001, scale=1,
                          explicit_normalize=False, last_dim_as_indicator=False, only_original_points_split=False):
    """The reference's point_upsample followed by the normalise / clamp tail of network_output_to_dpsr_grid, in two launches.
    X (B, M, 6) CUDA f32, xyz + normal (B, M, 7 with last_dim_as_indicator: the indicator is dropped); displacement (B, M, 6 k) with
    k = factor, or factor + 1 with first_refine_coarse_points alone.  only_original_points_split (with the indicator): only the
    first M // 2 points, the original ones, are split.
    -> points (B, R, 3) in [0, 0.99] as DPSR takes them, normals (B, R, 3) (the children's, not renormalised), bbox (B, 2, 3): the
    minimum and maximum of the children before the normalisation.  explicit_normalize: the children's bounding box is centred and
    its longest edge scaled to 0.99; otherwise they are divided by 2 `scale`.
    ValueError: an argument the form does not allow, a non-finite child (the sample is named), or -- with explicit_normalize -- a
    sample whose children coincide."""
    X = _f32(X, "X")
    displacement = _f32(displacement, "displacement")
    B, M, ldx = X.shape
    if ldx != (7 if last_dim_as_indicator else 6):
        raise ValueError("refine_to_dpsr_points: X must have %d channels, got %d" % (7 if last_dim_as_indicator else 6, ldx))
    if displacement.shape[:2] != X.shape[:2]:
        raise ValueError("refine_to_dpsr_points: X %s and displacement %s disagree" % (tuple(X.shape), tuple(displacement.shape)))
    if only_original_points_split and not last_dim_as_indicator:
        raise ValueError("refine_to_dpsr_points: only_original_points_split needs last_dim_as_indicator")
    factor = int(factor)
    first, inc = bool(first_refine_coarse_points), bool(include_displacement_center_to_final_output)
    if factor < 1:
        raise ValueError("refine_to_dpsr_points: %s" % ST_MESSAGES[-6])
    if inc and not first:
        raise ValueError("refine_to_dpsr_points: %s" % ST_MESSAGES[-5])
    dw = displacement.shape[2]
    if dw != 6 * (factor + 1 if first and not inc else factor):
        raise ValueError("refine_to_dpsr_points: displacement has %d channels, the form needs %d"
                         % (dw, 6 * (factor + 1 if first and not inc else factor)))
    if not explicit_normalize and not float(scale) > 0:
        raise ValueError("refine_to_dpsr_points: scale must be positive, got %r" % (scale,))
    _cuda(X, "X")
    _cuda(displacement, "displacement")
    rows = M // 2 if only_original_points_split else M
    R = refined_rows(rows, factor, first, inc)
    dev = X.device
    points = torch.empty((B, R, 3), device=dev, dtype=torch.float32)
    normals = torch.empty((B, R, 3), device=dev, dtype=torch.float32)
    bbox = torch.empty((B, 2, 3), device=dev, dtype=torch.float32)
    if B == 0 or R == 0:
        return points, normals, bbox
    L = lib()
    tiles = -(-R // L.slide_refine_span(0))
    partials = torch.empty((B, tiles, 6), device=dev, dtype=torch.float32)
    flag = torch.empty(2, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _status(L.slide_refine_to_dpsr(B, M, ldx, dw, rows, ptr(X), ptr(displacement), factor, int(first), int(inc),
                                       ctypes.c_float(float(output_scale_factor)), 0 if explicit_normalize else 1,
                                       ctypes.c_float(float(scale)), ptr(points), ptr(normals), ptr(bbox), ptr(partials), ptr(flag),
                                       stream_of()), "refine_to_dpsr_points")
    bits, smp = flag.tolist()  # the one host read
    if bits & 1:
        raise ValueError("refine_to_dpsr_points: sample %d has a non-finite refined point" % (smp - 1))
    if bits & 2:
        raise ValueError("refine_to_dpsr_points: the refined points of sample %d coincide (bounding box of length 0)" % (smp - 1))
    return points, normals, bbox
