"""Mesh output of the reference's pointnet2/dpsr_utils/io_utils.py (save_mesh, lines 11-20, there on pytorch3d.io.save_ply) on the
numpy PLY writer of slide_amd/mesh.py."""
from slide_amd.mesh import save_ply


def save_mesh(save_file, vertices, faces, normals=None):
    """vertices (N, 3), faces (F, 3), normals (N, 3) or None: tensors or numpy arrays -> a binary little-endian PLY"""
    save_ply(save_file, vertices, faces, normals)
