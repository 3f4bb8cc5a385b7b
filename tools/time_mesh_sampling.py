"""tools/time_mesh_sampling.py -- time of sampling points from triangle meshes on the GPU (slide_amd/csrc/mesh_sample.hip), one
process, not a test and not part of bench.py.  B sphere grids of r^3 with differing radii off the lattice -> marching cubes -> per
mesh 2048 samples and 20480 samples, with face normals (what batch_mc_from_psr draws per batch).

  kernels      slide_mesh_face_cdf (2 launches) and slide_mesh_sample (1 launch) at S = 2048 and S = 20480 on preallocated buffers,
               device events around --reps back-to-back calls, the median over --iters windows
  search       the S = 20480 launch again on the same vertices with every mesh cut down to ONE face: no search step and three
               gathers that hit one cache line.  1 - (that time / the full time) bounds the share of the sample kernel that the
               binary search AND the misses of the vertex gathers take together, from above
  end to end   slide_amd.mesh.sample_points_from_meshes on the list of meshes, both sample counts: packing (torch.cat), the three
               launches, the host read of the flag word; wall clock around synchronised calls
  composition  the reference's steps in torch, one mesh at a time as the reference runs them: gathers, cross product, norm,
               torch.multinomial(areas, S, replacement=True), two torch.rand, the weights, gathers; same meshes, same two sample
               counts, wall clock around synchronised calls
  sweep        end to end against the composition at smaller batches and grids

usage:  python tools/time_mesh_sampling.py [--batch 32] [--res 128] [--iters 7] [--reps 20] [--no-sweep]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

S_PLAIN, S_DENSE = 2048, 20480


def _event_ms(fn, iters, reps):
    """median over `iters` windows of the time of one call, each window `reps` calls between two device events"""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return sorted(ts)[len(ts) // 2]


def _wall_ms(fn, iters):
    import torch
    fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def composition(meshes, S):
    """pytorch3d's steps in torch, one mesh at a time -> points, normals (B, S, 3)"""
    import torch
    pts, nrm = [], []
    for v, f, _ in meshes:
        fl = f.long()
        v0, v1, v2 = v[fl[:, 0]], v[fl[:, 1]], v[fl[:, 2]]
        n = torch.cross(v1 - v0, v2 - v0, dim=1)
        ln = n.norm(dim=1)
        idx = torch.multinomial(0.5 * ln, S, replacement=True)
        u, w = torch.rand(S, device=v.device), torch.rand(S, device=v.device)
        su = u.sqrt()
        w0, w1, w2 = 1.0 - su, su * (1.0 - w), su * w
        pts.append(w0[:, None] * v0[idx] + w1[:, None] * v1[idx] + w2[:, None] * v2[idx])
        nrm.append(n[idx] / ln[idx].clamp_min(1.1920929e-07)[:, None])
    return torch.stack(pts), torch.stack(nrm)


def make_meshes(B, r, dev):
    import numpy as np
    import torch
    import mc_cases
    from slide_amd import mesh
    phi = torch.from_numpy(np.stack([mc_cases.sphere_grid(r, 0.2 + 0.2 * b / max(B - 1, 1)) for b in range(B)])).to(dev)
    return mesh.marching_cubes(phi)


def end_to_end(meshes):
    from slide_amd import mesh
    return (mesh.sample_points_from_meshes(meshes, S_PLAIN, return_normals=True, stream_id=0),
            mesh.sample_points_from_meshes(meshes, S_DENSE, return_normals=True, stream_id=1))


def run(B, r, iters, reps, sweep):
    import torch
    from slide_amd import _ext, mesh
    from slide_amd._lib import check, lib
    from slide_amd.abi import ptr, stream_of
    assert torch.cuda.is_available(), "time_mesh_sampling.py needs a GPU"
    dev = torch.device("cuda:0")
    meshes = make_meshes(B, r, dev)
    verts, faces, _, voff, foff = mesh.pack_meshes(meshes)
    nv, nf = verts.size(0), faces.size(0)
    L = lib()
    areas, cdf, vo, fo = _ext.mesh_face_cdf(verts, faces, voff, foff)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    valid = torch.zeros(B, device=dev, dtype=torch.int32)
    bufs = {S: (torch.empty((B, S, 3), device=dev), torch.empty((B, S, 3), device=dev)) for S in (S_PLAIN, S_DENSE)}

    def face_cdf():
        check(L.slide_mesh_face_cdf(B, nf, ptr(verts), ptr(faces), ptr(vo), ptr(fo), ptr(areas), ptr(cdf), ptr(flag), stream_of()), "face_cdf")

    def sampler(S, f_, fo_, cdf_):
        p, n = bufs[S]

        def go():
            check(L.slide_mesh_sample(B, S, ptr(verts), ptr(f_), None, ptr(vo), ptr(fo_), ptr(cdf_), 1, 0, 0, None, None, 0, ptr(p),
                                      ptr(n), None, ptr(valid), stream_of()), "mesh_sample")
        return go

    # every mesh cut down to its first face
    first = torch.stack([faces[foff[b]] for b in range(B)]).contiguous()
    fo1 = torch.arange(B + 1, device=dev, dtype=torch.int64)
    cdf1 = torch.full((B,), 1 << 32, device=dev, dtype=torch.int64)
    print("%d meshes from %d^3 grids: %d vertices, %d faces in all (%d to %d per mesh), cdf table %.1f MB; median of %d windows of %d calls"
          % (B, r, nv, nf, min(b - a for a, b in zip(foff, foff[1:])), max(b - a for a, b in zip(foff, foff[1:])), nf * 8 / 1e6, iters, reps),
          flush=True)
    t_cdf = _event_ms(face_cdf, iters, reps)
    t_s = {S: _event_ms(sampler(S, faces, fo, cdf), iters, reps) for S in (S_PLAIN, S_DENSE)}
    t_one = _event_ms(sampler(S_DENSE, first, fo1, cdf1), iters, reps)
    print("%-66s %9.3f ms" % ("slide_mesh_face_cdf (areas; maximum, quantise, scan: 2 launches)", t_cdf))
    for S in (S_PLAIN, S_DENSE):
        print("%-66s %9.3f ms  (%.2f ns per sample)" % ("slide_mesh_sample S = %d" % S, t_s[S], t_s[S] * 1e6 / (B * S)))
    print("%-66s %9.3f ms" % ("slide_mesh_sample S = %d, one face per mesh (no search)" % S_DENSE, t_one))
    print("%-66s %9.1f %%" % ("search + gather misses, share of the S = %d launch (upper bound)" % S_DENSE, 100.0 * (1.0 - t_one / t_s[S_DENSE])))
    print("%-66s %9.3f ms" % ("kernels for one batch: 2 x face_cdf + both sample launches", 2 * t_cdf + t_s[S_PLAIN] + t_s[S_DENSE]))
    t_e2e = _wall_ms(lambda: end_to_end(meshes), iters)
    t_ref = _wall_ms(lambda: (composition(meshes, S_PLAIN), composition(meshes, S_DENSE)), iters)
    print("%-66s %9.3f ms  (wall clock)" % ("mesh.sample_points_from_meshes, %d + %d samples, end to end" % (S_PLAIN, S_DENSE), t_e2e))
    print("%-66s %9.3f ms  (wall clock)" % ("torch composition, one mesh at a time, %d + %d samples" % (S_PLAIN, S_DENSE), t_ref))
    print("%-66s %9.2f x" % ("composition / end to end", t_ref / t_e2e))
    a, b = end_to_end(meshes), end_to_end(meshes)
    print("two runs bit-equal: %s" % all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q)))
    # the same surface statistic from both: the mean distance of the samples from the sphere's centre over its radius
    pc, _ = composition(meshes[:1], S_DENSE)
    c = meshes[0][0].mean(dim=0)
    rad = (meshes[0][0] - c).norm(dim=1).mean()
    print("mesh 0: mean |p - centre| / radius: kernels %.5f, composition %.5f"
          % (float((a[1][0][0] - c).norm(dim=1).mean() / rad), float((pc[0] - c).norm(dim=1).mean() / rad)))
    if sweep:
        print("sweep: end to end against the composition, ms (wall clock), both sample counts")
        for rr in (32, 128):
            for bb in (1, 8, 32):
                if (bb, rr) == (B, r):
                    continue
                ms = make_meshes(bb, rr, dev)
                te = _wall_ms(lambda: end_to_end(ms), iters)
                tr = _wall_ms(lambda: (composition(ms, S_PLAIN), composition(ms, S_DENSE)), iters)
                print("  B %2d r %3d (%7d faces): end to end %8.3f, composition %8.3f, ratio %6.2f" % (bb, rr, sum(len(m[1]) for m in ms), te, tr, tr / te))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-sweep", action="store_true")
    a = ap.parse_args()
    run(a.batch, a.res, a.iters, a.reps, not a.no_sweep)
