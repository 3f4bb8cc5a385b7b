"""tools/time_mesh_components.py -- time of the mesh clean-up on the GPU (slide_amd/csrc/mesh_components.hip): connected components,
selection of the largest and compaction; one process, not a test and not part of bench.py.  The workload is the one of
tools/time_marching_cubes.py: B sphere grids of r^3 with differing radii off the lattice -> marching cubes; --floaters N adds N small
spheres to every grid, so that there is something to remove.

  labelling    slide_mesh_cc_label at several group sizes (rounds per host read): the call blocks for its reads, so device events and
               the wall clock agree; rounds that lowered a label, rounds issued, host reads
  stages       slide_mesh_cc_stats (2 launches, 2 memsets), slide_mesh_cc_select (1), slide_mesh_cc_compact (1), device events
  end to end   slide_amd.mesh.filter_components on the list of meshes: packing (torch.cat), every stage, the host read of the totals
  host route   what the reference does, per mesh: D2H copy, scipy connected_components, numpy remap, H2D copy
  torch route  per mesh on the GPU: scatter_reduce_(amin) over the edge list + one pointer jump per round until a round changes
               nothing (one host read per round), then bincount, boolean masks and cumsum
  sweep        the same at one mesh and at 32 meshes of 32^3
  pipeline     batch_mc_from_psr with and without largest_component (marching cubes, PLY files, no sampling)

usage:  python tools/time_mesh_components.py [--batch 32] [--res 128] [--iters 7] [--floaters 0] [--no-sweep] [--no-pipeline]
"""
import argparse
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "pointnet2"))

GROUPS = (1, 2, 4, 8, 16)


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


def make_grids(B, r, floaters, dev):
    import numpy as np
    import torch
    import mc_cases
    grids = []
    for b in range(B):
        g = mc_cases.sphere_grid(r, 0.2 + 0.2 * b / max(B - 1, 1))
        small = mc_cases.sphere_grid(r, 0.03)
        for k in range(floaters):  # small spheres toward the corners of the grid
            shift = [int(r * 0.42) * (1 if (k >> a) & 1 else -1) for a in range(3)]
            g = np.minimum(g, np.roll(small, shift, axis=(0, 1, 2)))
        grids.append(g)
    return torch.from_numpy(np.stack(grids)).to(dev)


def host_route(meshes):
    """per mesh: D2H, scipy, numpy remap, H2D"""
    import numpy as np
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    out = []
    for v, f, n in meshes:
        hv, hf, hn = v.cpu().numpy(), f.cpu().numpy().astype(np.int64), n.cpu().numpy()
        i, j = np.concatenate([hf[:, 0], hf[:, 1]]), np.concatenate([hf[:, 1], hf[:, 2]])
        _, lab = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(len(hv), len(hv))), directed=False)
        keep = lab == np.bincount(lab).argmax()
        new = np.cumsum(keep) - 1
        kf = hf[keep[hf[:, 0]]]
        out.append((torch.from_numpy(hv[keep]).to(v.device), torch.from_numpy(new[kf].astype(np.int32)).to(v.device),
                    torch.from_numpy(hn[keep]).to(v.device)))
    return out


def torch_route(meshes):
    """per mesh on the GPU: min-label propagation with scatter_reduce_, then masks and cumsum"""
    import torch
    out, rounds = [], 0
    for v, f, n in meshes:
        fl = f.long()
        e0, e1 = torch.cat([fl[:, 0], fl[:, 1]]), torch.cat([fl[:, 1], fl[:, 2]])
        L = torch.arange(v.size(0), device=v.device)
        while True:
            m = torch.minimum(L[e0], L[e1])
            new = L.clone()
            new.scatter_reduce_(0, e0, m, "amin")
            new.scatter_reduce_(0, e1, m, "amin")
            new = new[new]
            rounds += 1
            if torch.equal(new, L):
                break
            L = new
        keep = L == torch.bincount(L).argmax()
        idx = torch.cumsum(keep, 0) - 1
        kf = fl[keep[fl[:, 0]]]
        out.append((v[keep], idx[kf].int(), n[keep]))
    return out, rounds


def measure(B, r, floaters, iters, dev, groups=GROUPS, baselines=True):
    import torch
    from slide_amd import _ext, mesh
    meshes = mesh.marching_cubes(make_grids(B, r, floaters, dev))
    verts, faces, normals, voff, foff = mesh.pack_meshes(meshes)
    nv, nf = verts.size(0), faces.size(0)
    print("\n%d meshes from %d^3 grids, %d floaters each: %d vertices, %d faces in all; median of %d" % (B, r, floaters, nv, nf, iters), flush=True)
    for g in groups:
        labels, vo, fo, info = _ext.mesh_cc_label(faces, voff, foff, nv, group=g)
        t = _event_ms(lambda: _ext.mesh_cc_label(faces, voff, foff, nv, group=g), iters)
        print("%-62s %9.3f ms  (%d rounds lowered a label, %d issued, %d host reads)"
              % ("slide_mesh_cc_label, %d rounds per host read" % g, t, info["rounds"], info["issued"], info["reads"]))
    labels, vo, fo, info = _ext.mesh_cc_label(faces, voff, foff, nv)
    cid, nverts, nfaces, totals, cnt_v, cnt_f = _ext.mesh_cc_stats(faces, vo, fo, labels)
    t_stats = _event_ms(lambda: _ext.mesh_cc_stats(faces, vo, fo, labels), iters)
    vnew, fnew = _ext.mesh_cc_select(faces, vo, fo, labels, cnt_v, cnt_f, totals)
    t_sel = _event_ms(lambda: _ext.mesh_cc_select(faces, vo, fo, labels, cnt_v, cnt_f, totals), iters)
    tot = totals.cpu().tolist()
    kv, kf = [t[0] for t in tot], [t[1] for t in tot]
    t_cmp = _event_ms(lambda: _ext.mesh_cc_compact(verts, normals, faces, vo, fo, vnew, fnew, kv, kf), iters)
    print("%-62s %9.3f ms" % ("slide_mesh_cc_stats (counts, ranks: 2 launches + 2 memsets)", t_stats))
    print("%-62s %9.3f ms" % ("slide_mesh_cc_select (selection, two scans: 1 launch)", t_sel))
    print("%-62s %9.3f ms  (with the two offset uploads)" % ("slide_mesh_cc_compact (1 launch)", t_cmp))
    print("components per mesh: %d to %d; kept %d of %d vertices, %d of %d faces"
          % (min(t[2] for t in tot), max(t[2] for t in tot), sum(kv), nv, sum(kf), nf))
    t_e2e = _wall_ms(lambda: mesh.filter_components(meshes), iters)
    print("%-62s %9.3f ms  (wall clock, default group %d)" % ("mesh.filter_components end to end", t_e2e, _ext.MESH_CC_GROUP))
    a, b = mesh.filter_components(meshes, return_index=True), mesh.filter_components(meshes, return_index=True)
    print("two runs bit-equal: %s" % all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q)))
    if baselines:
        t_host = _wall_ms(lambda: host_route(meshes), max(3, iters // 2))
        t_torch = _wall_ms(lambda: torch_route(meshes), max(3, iters // 2))
        h, (t, rounds) = host_route(meshes), torch_route(meshes)
        same = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[0], z[0]) and torch.equal(x[1], z[1]) for x, y, z in zip(a, h, t))
        print("%-62s %9.3f ms  (wall clock)" % ("host route: D2H, scipy, numpy, H2D, per mesh", t_host))
        print("%-62s %9.3f ms  (wall clock, %d rounds over the batch)" % ("torch route: scatter_reduce_ rounds, masks, cumsum, per mesh", t_torch, rounds))
        print("host / end to end %.2f x, torch / end to end %.2f x; all three give the same meshes: %s" % (t_host / t_e2e, t_torch / t_e2e, same))
    return meshes


def pipeline(B, r, floaters, iters, dev):
    from dpsr_evaluation import batch_mc_from_psr
    grids = make_grids(B, r, floaters, dev)
    with tempfile.TemporaryDirectory() as d:
        t_off = _wall_ms(lambda: batch_mc_from_psr(grids, d, "m"), iters)
        t_on = _wall_ms(lambda: batch_mc_from_psr(grids, d, "m", largest_component=True), iters)
    print("\nbatch_mc_from_psr, %d grids of %d^3, %d floaters (marching cubes, host copies, PLY files): %.1f ms, with largest_component %.1f ms (%+.1f ms)"
          % (B, r, floaters, t_off, t_on, t_on - t_off))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--floaters", type=int, default=0)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_mesh_components.py needs a GPU"
    dev = torch.device("cuda:0")
    measure(a.batch, a.res, a.floaters, a.iters, dev)
    if a.floaters == 0:
        measure(a.batch, a.res, 4, a.iters, dev, groups=(4,))
    if not a.no_sweep:
        measure(1, a.res, a.floaters, a.iters, dev, groups=(1, 4, 16))
        measure(32, 32, a.floaters, a.iters, dev, groups=(1, 4, 16))
    if not a.no_pipeline:
        pipeline(a.batch, a.res, a.floaters, max(3, a.iters // 2), dev)
