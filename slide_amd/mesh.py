"""Triangle meshes from indicator grids: marching cubes on the HIP kernels of csrc/marching_cubes.hip, and a PLY reader / writer
in numpy (what the reference does with skimage.measure.marching_cubes and pytorch3d.io.save_ply)."""
import numpy as np

from . import _ext

_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1", "int8": "i1",
              "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}


def marching_cubes(psr_grid, level=0.0):
    """psr_grid (B,r,r,r) CUDA f32, 2 <= r <= 256 -> a list of B tuples (verts (V,3) f32 in grid-index units, faces (F,3) int32,
    normals (V,3) f32 pointing down the gradient, like skimage's).  A corner is inside iff psr_grid < level; one vertex per
    sign-changing grid edge; faces wound so that their right-hand normal points toward increasing values.  Classic marching cubes with
    consistent faces (tools/gen_mc_table.py), not skimage's Lewiner variant: on cells with an ambiguous face the topology may differ."""
    return _ext.marching_cubes(psr_grid, level)


def _host(x, dtype):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def save_ply(path, verts, faces, normals=None):
    """binary little-endian PLY: float32 x y z [nx ny nz] per vertex, `list uchar int vertex_indices` per face.  verts (V,3),
    faces (F,3), normals (V,3) or None: numpy arrays or tensors."""
    v, f = _host(verts, "<f4").reshape(-1, 3), _host(faces, "<i4").reshape(-1, 3)
    props = ["x", "y", "z"]
    if normals is not None:
        n = _host(normals, "<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("save_ply: normals %s do not match verts %s" % (n.shape, v.shape))
        v = np.concatenate([v, n], axis=1)
        props += ["nx", "ny", "nz"]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0]]
    header += ["property float %s" % p for p in props]
    header += ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"], rec["idx"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(np.ascontiguousarray(v).tobytes())
        fh.write(rec.tobytes())


def load_ply(path):
    """reads what save_ply writes (binary little-endian, scalar vertex properties, triangles) -> (verts (V,3) f32, faces (F,3) int32,
    normals (V,3) f32 or None)"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: not a binary little-endian PLY" % path)
    elems = []  # [name, count, [(property, dtype) or (property, count dtype, item dtype)]]
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            elems.append([w[1], int(w[2]), []])
        elif w[:1] == ["property"]:
            elems[-1][2].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]) if w[1] == "list" else (w[2], _PLY_TYPES[w[1]]))
    verts = faces = normals = None
    for name, count, props in elems:
        if any(len(p) == 3 for p in props):
            if len(props) != 1:
                raise ValueError("%s: element %s mixes a list with other properties" % (path, name))
            dt = np.dtype([("n", props[0][1]), ("idx", props[0][2], (3,))])
            block = np.frombuffer(data, dtype=dt, count=count, offset=end)
            if count and not (block["n"] == 3).all():
                raise ValueError("%s: triangles only" % path)
            if name == "face":
                faces = block["idx"].astype(np.int32)
        else:
            dt = np.dtype([(p, t) for p, t in props])
            block = np.frombuffer(data, dtype=dt, count=count, offset=end)
            if name == "vertex":
                verts = np.stack([block[c] for c in "xyz"], axis=1).astype(np.float32)
                if all(c in dt.names for c in ("nx", "ny", "nz")):
                    normals = np.stack([block[c] for c in ("nx", "ny", "nz")], axis=1).astype(np.float32)
        end += dt.itemsize * count
    return verts, faces, normals
