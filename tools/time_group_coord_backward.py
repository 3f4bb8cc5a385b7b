"""tools/time_group_coord_backward.py -- cost of the grouping layer's coordinate backward (csrc/group_coord_bwd.hip,
slide_group_rows_coord_bwd: dout -> dxyz, dnew_xyz) on the GPU against a torch composition of the same arithmetic on the same
neighbour indices (slices of dout, elementwise terms, a sum over K for the centres, index_add_ for the source points), alternating in
one process:

  FP form, K 8   (group_knn: [d2 | w | abs | rel | centre])        N = np in 256, 1024, 2048 and the cross-level 256 -> 1024, 1024 -> 2048
  SA form, K 32  (QueryAndGroup 'nn' with abs + centre)            the same shapes

at B 32 and 256, C feature channels in front of the coordinate columns (ldg = C + 11 | 9 rounded up to 32).  Warmed up, median of
device events over --iters calls; the kernel's time includes zeroing dxyz (its contract), the composition's its own allocations.  Also
printed: the bytes the kernel must move -- the coordinate-gradient columns of dout (the 32-byte sectors they touch), indices, d2, both
gradients -- over its time.  Prints markdown table rows.

usage:  python tools/time_group_coord_backward.py [--batches 32,256] [--channels 32] [--iters 20]
"""
import argparse
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(256, 256), (1024, 1024), (2048, 2048), (256, 1024), (1024, 2048)]  # (N source points, np centres)


def _events_ms(fns, iters):
    """device-event time per call of each of fns, the calls alternating so that clocks and caches are shared; medians"""
    import torch
    for f in fns:
        f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for _ in fns]
    for i in range(iters):
        for k, f in enumerate(fns):
            ev[k][i][0].record()
            f()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(b) for a, b in e)[len(e) // 2] for e in ev]


def torch_backward(fp, C, xyz, new_xyz, idx, d2, dout):
    """the gradient of slide_group_rows_coord_bwd from torch ops (no counts)"""
    import torch
    B, N, _ = xyz.shape
    _, P, K = idx.shape
    g = dout.view(B, P, K, -1)
    flat = (idx + (torch.arange(B, device=idx.device) * N)[:, None, None]).reshape(-1)
    if fp:
        g_d2, g_w, g_abs, g_rel, g_ctr = g[..., C], g[..., C + 1], g[..., C + 2:C + 5], g[..., C + 5:C + 8], g[..., C + 8:C + 11]
        r = 1.0 / (d2 + 1e-8)
        S = r.sum(-1, keepdim=True)
        T = (g_w * (r / S)).sum(-1, keepdim=True)
        G = g_d2 - (r * r / S) * (g_w - T)
        q = xyz.reshape(B * N, 3)[flat].view(B, P, K, 3)
        v = (2 * G)[..., None] * (q - new_xyz[:, :, None])
        tq, tc = v + g_abs + g_rel, -v - g_rel + g_ctr
    else:
        g_rel, g_abs, g_ctr = g[..., C:C + 3], g[..., C + 3:C + 6], g[..., C + 6:C + 9]
        tq, tc = g_rel + g_abs, g_ctr - g_rel
    dxyz = torch.zeros(B * N, 3, device=xyz.device).index_add_(0, flat, tq.reshape(-1, 3)).view(B, N, 3)
    return dxyz, tc.sum(2)


def run(batches, C, iters):
    import torch
    from slide_amd import _ext
    from slide_amd._lib import check, lib
    assert torch.cuda.is_available(), "time_group_coord_backward.py needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    print("| form | B | N | np | K | ldg | kernel ms | torch ms | torch / kernel | kernel GB/s | max rel diff |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for fp, K in ((True, 8), (False, 32)):
        flags = 1 if fp else 2 | 4
        ldg = (C + (11 if fp else 9) + 31) // 32 * 32
        for B in batches:
            for N, P in SHAPES:
                xyz = torch.randn(B, N, 3, generator=gen).to(dev)
                new_xyz = xyz if N == P else torch.randn(B, P, 3, generator=gen).to(dev)
                d2, idx = _ext.knn_points(new_xyz, xyz, K)
                dout = torch.randn(B * P * K, ldg, device=dev)
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

                def kernel():
                    dxyz = torch.zeros(B, N, 3, device=dev)
                    dnew = torch.empty(B, P, 3, device=dev)
                    check(lib().slide_group_rows_coord_bwd(B, N, P, K, C, ldg, flags, *(ctypes.c_void_p(t.data_ptr()) for t in
                                                           (xyz, new_xyz, idx, d2)), None, ctypes.c_void_p(dout.data_ptr()),
                                                           ctypes.c_void_p(dxyz.data_ptr()), ctypes.c_void_p(dnew.data_ptr()), stream),
                          "slide_group_rows_coord_bwd")
                    return dxyz, dnew

                def composed():
                    return torch_backward(fp, C, xyz, new_xyz, idx, d2, dout)

                err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(kernel(), composed()))
                assert err <= 1e-4, err
                tk, tt = _events_ms([kernel, composed], iters)
                ncol = 11 if fp else 9
                sectors = ((C * 4 + ncol * 4 - 1) // 32) - (C * 4 // 32) + 1
                nbytes = B * P * K * (sectors * 32 + 8 + (4 if fp else 0) + (12 if fp else 0)) + 2 * (B * N * 12) + 2 * B * P * 12
                print("| %s | %d | %d | %d | %d | %d | %.3f | %.3f | %.2f | %.0f | %.1e |" % ("FP" if fp else "SA", B, N, P, K, ldg, tk, tt, tt / tk,
                                                                                         nbytes / tk / 1e6, err), flush=True)
                del dout


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    run([int(s) for s in a.batches.split(",")], a.channels, a.iters)
