"""tools/time_marching_cubes.py -- time of marching cubes on the GPU (slide_amd/csrc/marching_cubes.hip), one process, not a test and
not part of bench.py:

  kernels      slide_mc_count (3 launches) and slide_mc_emit (2 launches) on preallocated buffers, device events
  end to end   slide_amd.mesh.marching_cubes: the two calls, the host read of the totals between them and the output allocation,
               wall clock around a synchronised call

at B grids of r^3 (default 32 x 128^3) holding spheres of differing radii off the lattice; the median over --iters.  GPU times only:
the reference's skimage call runs on a host and is not timed here.

usage:  python tools/time_marching_cubes.py [--batch 32] [--res 128] [--iters 7]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def _event_ms(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def run(B, r, iters):
    import numpy as np
    import torch
    import mc_cases as C
    from slide_amd import _ext, mesh
    from slide_amd._lib import check, lib
    from slide_amd.abi import ptr, stream_of
    assert torch.cuda.is_available(), "time_marching_cubes.py needs a GPU"
    dev = torch.device("cuda:0")
    phi = torch.from_numpy(np.stack([C.sphere_grid(r, 0.2 + 0.2 * b / max(B - 1, 1)) for b in range(B)])).to(dev)
    L, nbricks = lib(), _ext.mc_bricks(r)
    counts = torch.empty((B, nbricks, 2), device=dev, dtype=torch.int32)
    totals = torch.empty((B, 4), device=dev, dtype=torch.int64)
    ws = torch.empty((B, r, r, r), device=dev, dtype=torch.int32)

    def count():
        check(L.slide_mc_count(B, r, ptr(phi), 0.0, ptr(counts), ptr(totals), stream_of()), "mc_count")

    count()
    tot = totals.cpu()
    nv, nf = int(tot[:, 0].sum()), int(tot[:, 1].sum())
    verts = torch.empty((nv, 3), device=dev)
    normals = torch.empty((nv, 3), device=dev)
    faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)

    def emit():
        check(L.slide_mc_emit(B, r, ptr(phi), 0.0, ptr(counts), ptr(totals), ptr(verts), ptr(normals), ptr(faces), ptr(ws), stream_of()), "mc_emit")

    print("%d grids of %d^3 (%d bricks each): %d vertices, %d faces in all; median of %d" % (B, r, nbricks, nv, nf, iters), flush=True)
    t_count, t_emit = _event_ms(count, iters), _event_ms(emit, iters)
    print("%-58s %9.3f ms" % ("slide_mc_count (count, scan, bases: 3 launches)", t_count))
    print("%-58s %9.3f ms" % ("slide_mc_emit (vertices + normals, faces: 2 launches)", t_emit))
    print("%-58s %9.3f ms  (the count pass reads the %.1f MB of grids)" % ("kernels, sum", t_count + t_emit, B * r ** 3 * 4 / 1e6))
    wall = []
    mesh.marching_cubes(phi)
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = mesh.marching_cubes(phi)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    print("%-58s %9.3f ms  (wall clock; chunks of %d grids)" % ("mesh.marching_cubes end to end", sorted(wall)[len(wall) // 2],
                                                                  max(1, min(B, _ext._MC_WORKSPACE_BYTES // (4 * r ** 3)))))
    again = mesh.marching_cubes(phi)
    print("two runs bit-equal: %s" % all(torch.equal(x, y) for a, b in zip(out, again) for x, y in zip(a, b)))
    v0, f0, _ = out[0]
    print("grid 0: V %d F %d, V - E + F = %d" % (len(v0), len(f0), C.euler(len(v0), f0.cpu().numpy())))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    run(a.batch, a.res, a.iters)
