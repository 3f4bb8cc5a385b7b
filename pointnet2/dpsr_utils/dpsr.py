"""Differentiable Poisson surface reconstruction: oriented points -> the Poisson indicator grid.  Counterpart of the
reference's pointnet2/dpsr_utils/dpsr.py (DPSR, lines 10-78) on the HIP kernels of slide_amd/csrc/dpsr.hip: rasterize the normals,
3-D real FFT, spectral Poisson solve with the Gaussian filter G, inverse FFT, shift by the mean value at the points, scale by the
value at cell (0, 0, 0).  No torch.fft, no float scatter: the grid is bit-reproducible and independent of the batch.  When V or N
requires grad the grid carries a grad_fn (slide_amd.train.functions.DpsrGrid, backward kernels in slide_amd/csrc/dpsr_bwd.hip); its
bits are those of the plain path."""
import torch
import torch.nn as nn

from slide_amd import _ext as _hip

from .utils import cubic_size, spec_gaussian_filter


class DPSR(nn.Module):
    def __init__(self, res, sig=10, scale=True, shift=True):
        """res: (r, r, r) with r in {16, 32, 64, 128, 256}; sig: degree of Gaussian smoothing"""
        super().__init__()
        r = cubic_size(res)
        if r not in _hip.FFT_SIZES:
            raise ValueError("DPSR: the grid resolution must be one of %s, got %d" % (_hip.FFT_SIZES, r))
        self.res = tuple(int(s) for s in res)
        self.sig = sig
        self.dim = 3
        self.scale = scale
        self.shift = shift
        self.register_buffer("G", spec_gaussian_filter(res=self.res, sig=sig).float())  # (r, r, r/2 + 1, 1, 1)

    def forward(self, V, N, chunk=None):
        """V (B, n, 3) coordinates in [0, 1), N (B, n, 3) normals, CUDA float -> phi (B, r, r, r).  `chunk`: samples per launch
        group (default: as many as keep the workspace within 1 GiB); the result does not depend on it."""
        if not (isinstance(V, torch.Tensor) and isinstance(N, torch.Tensor) and V.is_cuda and N.is_cuda):
            raise RuntimeError("DPSR runs on CUDA tensors only")
        if V.shape != N.shape:
            raise ValueError("V and N must have the same shape, got %s and %s" % (tuple(V.shape), tuple(N.shape)))
        if torch.is_grad_enabled() and (V.requires_grad or N.requires_grad):
            from slide_amd.train.functions import dpsr_grid
            return dpsr_grid(V, N, self.G.to(V.device), shift=self.shift, scale=self.scale, chunk=chunk)
        with torch.no_grad():
            return _hip.dpsr_grid(V, N, self.G.to(V.device), shift=self.shift, scale=self.scale, chunk=chunk)
