"""Triangle meshes from indicator grids: marching cubes on the HIP kernels of csrc/marching_cubes.hip, area-weighted point samples
from the meshes on those of csrc/mesh_sample.hip, connected components and the keep-largest filter on those of
csrc/mesh_components.hip, and a PLY reader / writer in numpy (what the reference does with skimage.measure.marching_cubes,
pytorch3d.ops.sample_points_from_meshes, igl.connected_components + trimesh split and pytorch3d.io.save_ply)."""
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


def pack_meshes(meshes):
    """a list of (verts (V,3) f32, faces (F,3) int32[, normals (V,3) f32 or None]) CUDA tensors -> (verts (sum V,3), faces (sum F,3),
    normals (sum V,3) or None when a mesh lacks them, voff, foff): one torch.cat per array, the offsets as host lists"""
    import torch
    if len(meshes) == 0:
        raise ValueError("pack_meshes: an empty list of meshes has no device")
    for m in meshes:
        for t, what in zip(m[:3], ("verts", "faces", "normals")):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("sample_points_from_meshes runs on the GPU only: %s must be a CUDA tensor" % what)
            if torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError("sample_points_from_meshes is forward only (no backward kernels): call it under "
                                          "torch.no_grad() or on tensors that do not require grad")
        if m[0].dim() != 2 or m[0].size(1) != 3 or m[1].dim() != 2 or m[1].size(1) != 3:
            raise ValueError("a mesh is verts (V, 3) and faces (F, 3), got %s and %s" % (tuple(m[0].shape), tuple(m[1].shape)))
    voff, foff = [0], [0]
    for m in meshes:
        voff.append(voff[-1] + m[0].size(0))
        foff.append(foff[-1] + m[1].size(0))
    verts = torch.cat([m[0].detach() for m in meshes])
    faces = torch.cat([m[1].detach() for m in meshes])
    normals = None
    if all(len(m) > 2 and m[2] is not None for m in meshes):
        normals = torch.cat([m[2].detach() for m in meshes])
    return verts, faces, normals, voff, foff


def sample_points_from_meshes(meshes, num_samples=10000, return_normals=False, seed=0, mesh_ids=None, stream_id=0, normals="face",
                              return_face_idx=False, words=None):
    """pytorch3d.ops.sample_points_from_meshes on the HIP kernels of csrc/mesh_sample.hip, for the whole batch in three launches.
    meshes: the list of (verts, faces, normals) that marching_cubes returns, or hand-made CUDA tensors (f32, int32, f32 or absent).
    -> points (B, S, 3) [, normals (B, S, 3)] [, face_idx (B, S) int32, the face's row in its mesh].

    A face is drawn with probability proportional to its area, quantised to 32 bits below the mesh's largest area, by ONE
    Philox4x32-10 call per sample keyed with `seed` on the counter (sample, mesh id, stream_id, constant); the point has pytorch3d's
    barycentric weights (1 - sqrt u, sqrt u (1 - v), sqrt u v).  mesh_ids (default: the position in the list) names a mesh's noise: a
    mesh's samples depend on (mesh, seed, mesh id, stream_id) alone, not on the batch or the position; two runs are bit-equal.
    normals: "face" = the unit face normal (v1 - v0) x (v2 - v0), what pytorch3d returns; "vertex" = the vertex normals interpolated
    with the weights and normalised.  A mesh without faces or of zero area yields zeros (pytorch3d's behaviour).  words (B, S, 4)
    integers in [0, 2^32) replace the Philox draw.  ValueError for a face index out of range or a non-finite vertex of a face.
    CUDA only, no autograd."""
    if normals not in ("face", "vertex"):
        raise ValueError("normals must be 'face' or 'vertex', got %r" % (normals,))
    verts, faces, vnormals, voff, foff = pack_meshes(meshes)
    if normals == "vertex" and vnormals is None:
        raise ValueError("normals='vertex' needs vertex normals for every mesh")
    verts, faces = verts.float(), faces.int()  # (no copies of float32 / int32 tensors)
    _, cdf, vo, fo = _ext.mesh_face_cdf(verts, faces, voff, foff)
    points, out_n, fidx, _ = _ext.mesh_sample(verts, faces, vo, fo, cdf, num_samples, seed=seed, mesh_ids=mesh_ids,
                                              stream_id=stream_id, vnormals=vnormals if normals == "vertex" else None,
                                              normals=normals if return_normals else None, return_face_idx=return_face_idx,
                                              words=words)
    out = (points,) + ((out_n,) if return_normals else ()) + ((fidx,) if return_face_idx else ())
    return out[0] if len(out) == 1 else out


def _label(meshes):
    verts, faces, normals, voff, foff = pack_meshes(meshes)
    faces = faces.int()
    labels, vo, fo, info = _ext.mesh_cc_label(faces, voff, foff, verts.size(0))
    return verts, faces, normals, voff, foff, vo, fo, labels, info


def mesh_components(meshes, return_info=False):
    """connected components of every mesh of a batch on the HIP kernels of csrc/mesh_components.hip.  meshes: the list that
    marching_cubes returns, or hand-made CUDA tensors (verts (V,3), faces (F,3) int32[, normals]).  -> per mesh a tuple
    (labels (V,) int32, nverts (C,) int32, nfaces (C,) int32) of CUDA tensors.

    Any two distinct indices of a face are joined; a vertex without a face is a component of its own.  labels[v] is the rank of the
    smallest vertex index of v's component among those of all components (scipy.sparse.csgraph.connected_components' and igl's
    numbering); nfaces counts a face in the component of its FIRST index.  The result is a function of the mesh alone: the same in
    any batch, at any position, on every run.  ValueError for a face index outside [0, V).  CUDA only, no autograd.
    return_info: also a dict with the labelling rounds that changed a label, the host reads and the rounds issued."""
    verts, faces, _, voff, foff, vo, fo, labels, info = _label(meshes)
    cid, nverts, nfaces, totals, _, _ = _ext.mesh_cc_stats(faces, vo, fo, labels)
    ncomp = totals[:, 2].cpu().tolist()
    out = [(cid[voff[m]:voff[m + 1]], nverts[voff[m]:voff[m] + c], nfaces[voff[m]:voff[m] + c]) for m, c in enumerate(ncomp)]
    return (out, info) if return_info else out


def filter_components(meshes, keep="largest", by="verts", min_size=0, return_index=False):
    """keeps whole connected components of every mesh (the reference's verts_on_largest_mesh for a batch, on the GPU): -> a list of
    (verts (V',3), faces (F',3) int32, normals (V',3) or None[, vert_idx (V',) int32]), the structure marching_cubes returns.

    Candidates are the components with at least one face whose size -- by="verts": vertices, "faces": faces -- is >= min_size;
    keep="largest" keeps the largest candidate (ties: the one holding the smallest vertex index), keep="all" every candidate.  No
    candidate: (0,3) verts and (0,3) faces.  Kept vertices and faces keep their order and winding, rows are copied bit for bit and
    face indices renumbered; vert_idx holds the kept rows' original indices, ascending.  Independent of the batch and reproducible,
    like mesh_components.  ValueError for a face index outside [0, V).  CUDA only, no autograd."""
    if keep not in ("largest", "all"):
        raise ValueError("keep must be 'largest' or 'all', got %r" % (keep,))
    if by not in ("verts", "faces"):
        raise ValueError("by must be 'verts' or 'faces', got %r" % (by,))
    verts, faces, normals, voff, foff, vo, fo, labels, _ = _label(meshes)
    verts = verts.float()
    _, _, _, totals, cnt_v, cnt_f = _ext.mesh_cc_stats(faces, vo, fo, labels)
    vnew, fnew = _ext.mesh_cc_select(faces, vo, fo, labels, cnt_v, cnt_f, totals, by=by, min_size=min_size, keep=keep)
    tot = totals.cpu().tolist()  # (the one host read that sizes the outputs)
    out_v, out_n, out_f, vidx, ov, of = _ext.mesh_cc_compact(verts, normals, faces, vo, fo, vnew, fnew, [t[0] for t in tot], [t[1] for t in tot])
    out = []
    for m in range(len(tot)):
        one = (out_v[ov[m]:ov[m + 1]], out_f[of[m]:of[m + 1]], out_n[ov[m]:ov[m + 1]] if out_n is not None else None)
        out.append(one + (vidx[ov[m]:ov[m + 1]],) if return_index else one)
    return out
