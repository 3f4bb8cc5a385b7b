"""tools/time_refine_front.py -- time of the refine-and-upsample front of DPSR on the GPU (slide_amd/csrc/refine_front.hip): one
process, not a test and not part of bench.py.  At B x N x factor = 32 x 4096 x 5 (the shipped symmetry configuration: 2048 points
mirrored) and 32 x 2048 x 10, medians of --iters runs after a warm-up:

  kernels      slide_mirror_concat (2 launches) on B x N/2 x 6 and slide_refine_to_dpsr (2 launches, explicit_normalize) on its output
               and a displacement, device events; then both through the Python wrappers with their host reads of the flags, wall clock
  torch route  the reference's own steps on the same inputs: mean, clone, slices, cat, index; view, broadcast add, min / max,
               elementwise, clamp -- device events and wall clock; and whether its outputs equal the kernels' bit for bit
  pipeline     the stages of one mesh_reconstruction.py batch with the shipped configuration and synthetic weights: network, front,
               DPSR, marching cubes, components, sampling (wall clock, synchronised around every stage)

usage:  python tools/time_refine_front.py [--batch 32] [--iters 21] [--no-pipeline] [--prec mixed|fp32]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "pointnet2"))


def _event_ms(fn, iters):
    import torch
    for _ in range(3):
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
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def clouds(B, N, dev, seed=0):
    """B ellipsoids of N oriented points (xyz + unit normal)"""
    import numpy as np
    import torch
    rs = np.random.RandomState(seed)
    u = rs.standard_normal((B, N, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    axes = rs.uniform(0.25, 0.45, (B, 1, 3))
    n = u / axes
    x = np.concatenate([u * axes, n / np.linalg.norm(n, axis=2, keepdims=True)], axis=2).astype(np.float32)
    return torch.from_numpy(x).to(dev)


def torch_mirror(x, perm, axis=2):
    import torch
    B, N, _ = x.shape
    center = torch.mean(x[:, :, 0:3], dim=1, keepdim=True)
    m = x.clone()
    m[:, :, 0:3] = m[:, :, 0:3] - center
    m[:, :, axis] = -m[:, :, axis]
    m[:, :, axis + 3] = -m[:, :, axis + 3]
    m[:, :, 0:3] = m[:, :, 0:3] + center
    one = torch.ones(B, N, 1, device=x.device, dtype=x.dtype)
    return torch.cat([torch.cat([x, one], dim=2), torch.cat([m, one * (-1)], dim=2)], dim=1)[:, perm, :]


def torch_refine(X, disp, factor, s):
    import numpy as np
    import torch
    Xr = X[:, :, 0:-1]
    B, N, F = Xr.shape
    up = (Xr.unsqueeze(2) + (disp * (1 / np.sqrt(factor))).view(B, N, factor, F) * s).reshape(B, -1, F).contiguous()
    p, n = up[:, :, 0:3], up[:, :, 3:]
    mn, mx = p.min(dim=1, keepdim=True)[0], p.max(dim=1, keepdim=True)[0]
    p = (p - (mx + mn) / 2) / (mx - mn).max(dim=2, keepdim=True)[0] * 0.99
    return torch.clamp(p / 1.2 + 0.5, min=0, max=0.99), n


def front(B, N, factor, iters, dev):
    import ctypes
    import torch
    from slide_amd import refine
    from slide_amd._lib import lib
    from slide_amd.abi import ptr, stream_of
    x = clouds(B, N // 2, dev)
    perm = refine.refine_permutation(N, 0).to(dev)
    disp = torch.randn(B, N, 6 * factor, device=dev)
    s = 0.001
    L = lib()
    R = N * factor
    out, center = torch.empty(B, N, 7, device=dev), torch.empty(B, 3, device=dev)
    pts, nrm, bbox = torch.empty(B, R, 3, device=dev), torch.empty(B, R, 3, device=dev), torch.empty(B, 2, 3, device=dev)
    partials = torch.empty(B, -(-R // L.slide_refine_span(0)), 6, device=dev)
    flag = torch.empty(2, device=dev, dtype=torch.int32)

    def k_mirror():
        assert L.slide_mirror_concat(B, N // 2, 6, ptr(x), 2, 1, ptr(perm), ptr(out), ptr(center), ptr(flag), stream_of()) == 0

    def k_refine():
        assert L.slide_refine_to_dpsr(B, N, 7, 6 * factor, N, ptr(out), ptr(disp), factor, 0, 0, ctypes.c_float(s), 0, ctypes.c_float(1.0),
                                      ptr(pts), ptr(nrm), ptr(bbox), ptr(partials), ptr(flag), stream_of()) == 0

    def k_both():
        k_mirror()
        k_refine()

    def wrappers():
        X, _ = refine.mirror_and_concat(x, axis=2, attach_label=True, perm=perm)
        return refine.refine_to_dpsr_points(X, disp, factor, output_scale_factor=s, explicit_normalize=True, last_dim_as_indicator=True)

    def t_both():
        return torch_refine(torch_mirror(x, perm), disp, factor, s)

    print("\nB %d x N %d x factor %d: %d refined points per cloud, %.1f MB read + written; median of %d"
          % (B, N, factor, R, (x.numel() + out.numel() * 2 + disp.numel() * 2 + pts.numel() * 2) * 4 / 1e6, iters), flush=True)
    rows = [("slide_mirror_concat (2 launches)", _event_ms(k_mirror, iters), "events"),
            ("slide_refine_to_dpsr (2 launches)", _event_ms(k_refine, iters), "events"),
            ("both kernels (4 launches)", _event_ms(k_both, iters), "events"),
            ("both through slide_amd.refine (2 host reads of the flags)", _wall_ms(wrappers, iters), "wall clock"),
            ("torch: mirror (mean, clone, slices, cat, index)", _event_ms(lambda: torch_mirror(x, perm), iters), "events"),
            ("torch: upsample, normalise, clamp", _event_ms(lambda: torch_refine(out, disp, factor, s), iters), "events"),
            ("torch: both", _event_ms(t_both, iters), "events"),
            ("torch: both", _wall_ms(t_both, iters), "wall clock")]
    for name, t, how in rows:
        print("%-62s %9.1f us  (%s)" % (name, t * 1e3, how))
    k, t = rows[2][1], rows[6][1]
    print("events: torch / kernels %.2f x%s;  wall clock: torch / wrappers %.2f x%s"
          % (t / k, "" if t >= k else "  (THE TORCH COMPOSITION WINS)", rows[7][1] / rows[3][1],
             "" if rows[7][1] >= rows[3][1] else "  (THE TORCH COMPOSITION WINS)"))
    k_both()
    tp, tn = t_both()
    Xt = torch_mirror(x, perm)
    print("bit-equal to the torch composition on this GPU: mirrored rows %s, points %s (%d of %d elements differ), normals %s"
          % (torch.equal(out, Xt), torch.equal(pts, tp), int((pts != tp).sum()), pts.numel(), torch.equal(nrm, tn)))
    a, b = wrappers(), wrappers()
    print("two runs bit-equal: %s" % all(torch.equal(p, q) for p, q in zip(a, b)))


def pipeline(B, iters, dev, prec):
    import tempfile
    import torch
    from slide_amd.generation import module_prec_of
    os.environ["SLIDE_MODULE_PREC"] = module_prec_of(prec)
    from data_utils.mirror_partial import mirror_and_concat
    from dpsr_evaluation import compute_center_and_max_length, network_output_to_dpsr_grid
    from dpsr_utils.dpsr import DPSR
    from models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    from slide_amd import _ext, mesh
    from slide_amd.configs import refine_and_upsample_config
    from slide_amd.synth import synth_state_dict
    cfg = refine_and_upsample_config()
    hp, dc = cfg["pointnet_config"], cfg["dpsr_config"]
    net = PointNet2CloudCondition(hp)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in
                         synth_state_dict([(k, tuple(t.shape)) for k, t in net.state_dict().items()]).items()})
    net = net.to(dev).eval()
    dpsr = DPSR((dc["grid_res"],) * 3, sig=dc["psr_sigma"]).to(dev)
    x = clouds(B, 2048, dev)
    label = torch.zeros(B, dtype=torch.int64, device=dev)
    st = {}

    def stage(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        st.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return r

    def up(a, dtype):
        import numpy as np
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev).reshape(-1, 3)

    with torch.no_grad():
        for it in range(iters + 1):
            if it == 1:
                st.clear()  # (the first pass warms up)
            X = stage("front: mirror_and_concat", lambda: mirror_and_concat(x, axis=2, num_points=[], attach_label=True, permute=True, seed=0)[0])
            disp = stage("network forward (module path, %s)" % prec, lambda: net(X, None, ts=None, label=label).contiguous())
            pts, nrm = stage("front: upsample, normalise, clamp", lambda: network_output_to_dpsr_grid(
                X, disp, lambda p, n: None, 1, hp, last_dim_as_indicator=True, explicit_normalize=True)[1:])
            grid = stage("DPSR %d^3" % dc["grid_res"], lambda: dpsr(pts, nrm))
            meshes = stage("marching cubes", lambda: mesh.marching_cubes(grid))
            kept = stage("components: keep the largest", lambda: mesh.filter_components(meshes, keep="largest", by="verts"))
            ids = list(range(B))
            dense = stage("sampling: 2048 + 20480 samples per mesh", lambda: (
                mesh.sample_points_from_meshes(kept, 2048, return_normals=True, seed=0, mesh_ids=ids, stream_id=0),
                mesh.sample_points_from_meshes(kept, 20480, return_normals=True, seed=0, mesh_ids=ids, stream_id=1))[1])
            stage("sampling: farthest point sampling to 2048", lambda: _ext.sample_farthest_points(
                dense[0], K=2048, start_idx=torch.zeros(B, dtype=torch.int64, device=dev)))
    print("\none mesh_reconstruction.py batch, B %d x 2048 points, shipped symmetry configuration, synthetic weights; median of %d (wall clock)"
          % (B, iters))
    total = 0.0
    for name, ts in st.items():
        t = sorted(ts)[len(ts) // 2]
        total += t
        print("%-62s %9.3f ms" % (name, t))
    print("%-62s %9.3f ms  (without the host copies and the PLY files of batch_mc_from_psr)" % ("sum", total))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--prec", default="mixed", choices=["mixed", "fp32"])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_refine_front.py needs a GPU"
    dev = torch.device("cuda:0")
    front(a.batch, 4096, 5, a.iters, dev)
    front(a.batch, 2048, 10, a.iters, dev)
    if not a.no_pipeline:
        pipeline(a.batch, max(3, a.iters // 4), dev, a.prec)
