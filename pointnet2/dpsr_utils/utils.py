"""The DPSR helpers of the reference's pointnet2/dpsr_utils/utils.py (lines 24-196) on the HIP kernels of slide_amd/csrc/dpsr.hip:
same names, arguments and return shapes; 3-D cubic grids, CUDA float tensors, forward only.

  fftfreqs, spec_gaussian_filter   host tensors, the reference's values bit for bit (numpy's fftfreq / rfftfreq; the filter in float64)
  point_rasterize(pts, vals, size) trilinear scatter, (B, nf, r, r, r) float: converted once per cell from the kernel's exact
                                   64-bit fixed-point sums (bit-reproducible, unlike a float scatter_add_)
  grid_interp(grid, pts, batched)  trilinear gather, (B, n, C)

and its mesh helpers (lines 246-287, 498-507) on slide_amd/mesh.py:

  mc_from_psr(psr_grid, ...)       marching cubes of every grid of a batch on the GPU, (verts, faces, normals) lists of length B
  export_mesh(name, v, f)          a binary PLY of one mesh
  verts_on_largest_mesh(v, f)      the connected component with the most vertices (lines 352-375: igl + trimesh on the host there)
"""
import numpy as np
import torch

from slide_amd import _ext as _hip


def fftfreqs(res, dtype=torch.float32, exact=True):
    """frequency tensor (*res[:-1], res[-1] / 2 + 1, len(res)): fftfreq on every axis but the last, rfftfreq on the last (without its
    Nyquist bin when not exact)"""
    freqs = [torch.tensor(np.fft.fftfreq(r, d=1 / r), dtype=dtype) for r in res[:-1]]
    last = np.fft.rfftfreq(res[-1], d=1 / res[-1])
    freqs.append(torch.tensor(last if exact else last[:-1], dtype=dtype))
    return torch.stack(torch.meshgrid(*freqs, indexing="ij"), dim=-1)


def spec_gaussian_filter(res, sig):
    """exp(-0.5 (2 sig |k| / res[0])^2) in float64, (*half spectrum shape, 1, 1)"""
    omega = fftfreqs(res, dtype=torch.float64)
    dis = torch.sqrt(torch.sum(omega ** 2, dim=-1))
    return torch.exp(-0.5 * ((sig * 2 * dis / res[0]) ** 2)).unsqueeze(-1).unsqueeze(-1)


def cubic_size(size):
    """r of a 3-D cubic size tuple (the kernels' scope); ValueError otherwise"""
    size = tuple(int(s) for s in size)
    if len(size) != 3 or size[0] != size[1] or size[0] != size[2]:
        raise ValueError("3-D cubic grids only, got size %s" % (size,))
    return size[0]


def point_rasterize(pts, vals, size):
    """pts (B, n, 3) in [0, 1), vals (B, n, nf) with nf 1 or 3 -> (B, nf, *size)"""
    return _hip.point_rasterize(pts, vals, cubic_size(size))


def grid_interp(grid, pts, batched=True):
    """grid (B, r, r, r, C), pts (B, n, 3) in [0, 1) -> (B, n, C); without `batched` both lack the leading axis"""
    if not batched:
        return _hip.grid_interp(grid.unsqueeze(0), pts.unsqueeze(0)).squeeze(0)
    return _hip.grid_interp(grid, pts)


def mc_from_psr(psr_grid, pytorchify=False, real_scale=False, zero_level=0):
    """psr_grid (B, s, s, s) CUDA float -> three lists of length B: verts (V, 3) divided by s (by s - 1 with real_scale), faces (F, 3)
    int32, normals (V, 3): numpy arrays, or with pytorchify float tensors on the grid's device with the normals NEGATED (the
    reference's torch.Tensor(...) conversion: the faces become floats too).  Like the reference, zero_level is honoured for a batch
    of one only; larger batches are cut at level 0."""
    from slide_amd import mesh
    B, s = psr_grid.shape[0], psr_grid.shape[-1]
    meshes = mesh.marching_cubes(psr_grid.detach(), level=zero_level if B == 1 else 0)
    unit = (s - 1) if real_scale else s  # vertices to [0, 1] or to [0, 1)
    verts = [v.cpu().numpy() / unit for v, _, _ in meshes]
    faces = [f.cpu().numpy() for _, f, _ in meshes]
    normals = [n.cpu().numpy() for _, _, n in meshes]
    if pytorchify:
        def as_float(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(psr_grid.device)
        verts, faces, normals = [as_float(v) for v in verts], [as_float(f) for f in faces], [as_float(-n) for n in normals]
    return verts, faces, normals


def export_mesh(name, v, f):
    """one mesh as a binary PLY; v (V, 3) / f (F, 3) arrays or tensors, or batched with a leading axis (the first one is written)"""
    from slide_amd import mesh
    if len(v.shape) > 2:
        v, f = v[0], f[0]
    mesh.save_ply(name, v, f)


def verts_on_largest_mesh(verts, faces):
    """verts (N, 3) and faces (F, 3), numpy arrays or tensors (squeezed like the reference's) -> (v_large (N', 3) float32, f_large
    (F', 3) int32) as numpy arrays: the connected component with the most vertices (ties: the one holding the smallest vertex index,
    the reference's argmax), vertices and faces in their order, faces renumbered.  Runs on the GPU (slide_amd.mesh.filter_components):
    host inputs are uploaded; there is no CPU path."""
    from slide_amd import mesh

    def dev(a, dtype):
        if torch.is_tensor(a):
            a = a.detach().squeeze()
        else:
            a = torch.from_numpy(np.ascontiguousarray(np.squeeze(np.asarray(a))))
        return a.to(device="cuda", dtype=dtype).reshape(-1, 3).contiguous()

    (v, f, _), = mesh.filter_components([(dev(verts, torch.float32), dev(faces, torch.int32))], keep="largest", by="verts")
    return v.cpu().numpy(), f.cpu().numpy()
