#!/usr/bin/env python
"""AUTHORING ONLY: records tests/golden/golden_mc.npz, the reference's marching cubes on the grids of tests/mc_cases.py.

The reference extracts its meshes with scikit-image (pointnet2/dpsr_utils/utils.py:246-287 mc_from_psr):
    verts, faces, normals, values = measure.marching_cubes(psr_grid_numpy[i], level=0)
That module cannot be imported here (it needs trimesh, igl and open3d at import time), so this script makes the same library call.
It needs scikit-image (0.18.3 was used, under a Python 3.9 of its own); the project's interpreter does not have it and the tests
never import it.

Per case: grid_<name> float32, sk_verts_<name> float32, sk_faces_<name> int32, sk_normals_<name> float32, and in `ambiguous` the
number of cell faces whose signs alternate diagonally.  Cases: the six synthetic 16^3 grids, `noise` (8^3) and psr0 / psr1, the two
real indicator grids phi32_r16_s2_sh1_sc1 of golden_dpsr.npz.  `strict` lists the cases the tests compare with skimage: for each
of them this script asserts min |phi| > 1e-7, no ambiguous face, and skimage's V equal to the number of sign-changing grid edges
(Lewiner's variant adds vertices inside ambiguous cells, so the comparison is meaningful only without them).  A psr grid that fails
one of these is dropped from `strict` with a note; `noise` is never strict.

usage:  python3.9 tools/gen_golden_mc.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "golden_mc.npz")
SIZE_CAP = 781323  # the largest committed fixture


def main():
    import skimage
    from skimage import measure

    import mc_cases as C
    grids = C.synthetic_grids()
    psr = np.load(os.path.join(REPO, "tests", "golden", "golden_dpsr.npz"))["phi32_r16_s2_sh1_sc1"]
    grids["psr0"], grids["psr1"] = np.ascontiguousarray(psr[0]), np.ascontiguousarray(psr[1])
    out, strict, names, amb = {}, [], [], []
    for name, grid in grids.items():
        verts, faces, normals, _ = measure.marching_cubes(grid, level=0)
        assert verts.dtype == np.float32 and normals.dtype == np.float32 and faces.dtype == np.int32
        x = C.crossings(grid)
        a = C.ambiguous_faces(grid)
        ok = float(np.abs(grid).min()) > 1e-7 and a == 0 and len(verts) == len(x["keys"])
        print("%-8s r %2d  V %4d  F %4d  sign-changing edges %4d  ambiguous faces %3d  min |phi| %.3e  Euler %d%s" % (
            name, grid.shape[0], len(verts), len(faces), len(x["keys"]), a, np.abs(grid).min(), C.euler(len(verts), faces),
            "" if ok or name == "noise" else "   NOT strict"))
        if name in C.STRICT:
            assert ok, name
        if ok and name != "noise":
            strict.append(name)
            C.vertex_keys(verts, grid.shape[0])  # (every vertex lies strictly inside one grid edge)
            assert (C.orientation(verts, faces, grid) > 0).all(), name
        elif name.startswith("psr"):
            print("  %s is dropped from the strict comparison" % name)
        names.append(name)
        amb.append(a)
        out["grid_" + name] = grid
        out["sk_verts_" + name], out["sk_faces_" + name], out["sk_normals_" + name] = verts, faces, normals
    out["names"], out["strict"], out["ambiguous"] = np.array(names), np.array(strict), np.array(amb, dtype=np.int64)
    out["skimage_version"] = np.array(skimage.__version__)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote %s: %d bytes, strict cases %s" % (os.path.relpath(OUT, REPO), size, strict))
    assert size <= SIZE_CAP


if __name__ == "__main__":
    main()
