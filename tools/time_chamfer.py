"""tools/time_chamfer.py -- throughput of the Chamfer / F1 metric on the GPU (metrics_point_cloud.chamfer_and_f1), one process:

  (a) calc_cd, the fused path (chamfer_nn_kernel + chamfer_reduce_kernel + O(B) arithmetic), xyz only and with 3 normal channels
  (b) the composition it replaces: two slide_knn_points K = 1 launches (x -> y, y -> x) + torch reductions (sqrt, means, counts)
  (c) pointnet2/load_evaluate.py's evaluate() over 2048 pairs of 2048 points, end to end (host arrays in, per-pair metrics out)

at B 256 x P x P for P in 1024, 2048 (the shape SLIDE emits), 8192.  Rates are DIRECTED pair evaluations per second
(2 B P^2: every (query, point) pair of both directions) over device-event time.  Outputs of (a) and (b) are compared on every shape.

  --stats FILE   instead: read a rocprofv3 --kernel-trace --stats kernel_stats.csv of a run of this script and report each kernel's
                 time per call and the NN kernel's share of its VALU-issue bound (VALU_PAIRS_PER_SIMD_CYCLE below)

usage:  python tools/time_chamfer.py [--sizes 1024,2048,8192] [--batch 256] [--iters 20]
        rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/time_chamfer.py --iters 5 --no-cli
        python tools/time_chamfer.py --stats OUT/.../run_kernel_stats.csv
"""
import argparse
import csv
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "pointnet2"))

# VALU-issue bound of chamfer_nn_kernel: its inner step evaluates 8 search points x 2 queries per lane
# (1024 directed pairs per wave) in 111 VALU instructions (gfx950 ISA of the product build: 63 single-issue -- compares, selects,
# moves -- and 48 packed-f32 v_pk_add / v_pk_mul / v_pk_fma).  A wave64 VALU instruction occupies a SIMD-32 for 2 cycles
# (MI355X_MICROARCH: v_fma_f32 2 cyc); the 157.3 TFLOP/s vector peak is one fp32 FMA per lane per such issue, so a packed
# instruction is counted as two: 63 * 2 + 48 * 4 = 318 SIMD cycles per 1024 pairs.
VALU_PAIRS_PER_SIMD_CYCLE = 1024 / 318.0
SIMDS = 256 * 4
CLOCK_HZ = 2.4e9
VALU_BOUND_PAIRS_PER_S = VALU_PAIRS_PER_SIMD_CYCLE * SIMDS * CLOCK_HZ  # ~7.9e12


def _events_ms(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def composition(o, gt, thr):
    """calc_cd's xyz metrics from two knn_points K = 1 launches and torch reductions (what the fused path replaces)"""
    import torch
    from slide_amd import _ext
    g3, o3 = gt[:, :, :3].contiguous(), o[:, :, :3].contiguous()
    d1 = _ext.knn_points(g3, o3, 1)[0][..., 0]
    d2 = _ext.knn_points(o3, g3, 1)[0][..., 0]
    p1 = (d1 < thr).float().mean(1)
    p2 = (d2 < thr).float().mean(1)
    f = 2 * p1 * p2 / (p1 + p2)
    return {"cd_p": (torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1)) / 2, "cd_t": d1.mean(1) + d2.mean(1),
            "f1": torch.where(torch.isnan(f), torch.zeros_like(f), f)}


def run(sizes, B, iters, cli=True):
    import numpy as np
    import torch
    import load_evaluate as L
    from metrics_point_cloud.chamfer_and_f1 import calc_cd
    assert torch.cuda.is_available(), "time_chamfer.py needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    thr = 1e-3
    print("B %d, rates in directed pair evaluations/s (2 B P^2); VALU-issue bound of the NN kernel %.2e/s" % (B, VALU_BOUND_PAIRS_PER_S))
    with torch.no_grad():
        for P in sizes:
            gt = torch.randn(B, P, 6, generator=gen).to(dev)
            o = (gt + 0.02 * torch.randn(B, P, 6, generator=gen).to(dev)).contiguous()
            o3, g3 = o[:, :, :3].contiguous(), gt[:, :, :3].contiguous()
            pairs = 2.0 * B * P * P
            t_a3 = _events_ms(lambda: calc_cd(o3, g3, calc_f1=True, f1_threshold=thr), iters)
            t_a6 = _events_ms(lambda: calc_cd(o, gt, calc_f1=True, f1_threshold=thr, normal_loss_type='mse'), iters)
            t_b = _events_ms(lambda: composition(o, gt, thr), iters)
            r, c = calc_cd(o3, g3, calc_f1=True, f1_threshold=thr), composition(o, gt, thr)
            err = max(float(((r[k] - c[k]).abs() / c[k].abs().clamp_min(1e-30)).max()) for k in ("cd_p", "cd_t"))
            assert err <= 1e-5 and torch.equal(r["f1"], c["f1"]), err
            print("P %5d  (a) calc_cd xyz %8.3f ms %.3e/s | with normals %8.3f ms %.3e/s | (b) knn K=1 x2 + torch %8.3f ms %.3e/s "
                  "| (b)/(a) %.2fx | max rel diff %.1e" % (P, t_a3, pairs / t_a3 * 1e3, t_a6, pairs / t_a6 * 1e3, t_b,
                                                          pairs / t_b * 1e3, t_b / t_a3, err), flush=True)
        if not cli:
            return
        # (c) load_evaluate end to end: 2048 pairs x 2048 points from npz files (normalisation, host -> device, batches of 256)
        rs = np.random.RandomState(1)
        a = rs.standard_normal((2048, 2048, 3)).astype(np.float32)
        b = (a + 0.02 * rs.standard_normal(a.shape)).astype(np.float32)
        with tempfile.TemporaryDirectory() as tmp:
            pa, pb = os.path.join(tmp, "a.npz"), os.path.join(tmp, "b.npz")
            np.savez(pa, points=a)
            np.savez(pb, points=b)
            import time
            L.evaluate(a[:256], b[:256])  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            import contextlib
            import io
            with contextlib.redirect_stdout(io.StringIO()):
                L.main(["--dir1", pa, "--dir2", pb])
            dt = time.perf_counter() - t0
        print("(c) load_evaluate 2048 pairs x 2048 points end to end (npz load + normalise + GPU metrics): %.3f s, %.0f pairs/s, "
              "%.3e directed pair evaluations/s" % (dt, 2048 / dt, 2.0 * 2048 * 2048 * 2048 / dt), flush=True)


def stats(path, sizes, B, iters):
    """kernel_stats.csv -> time per call of every kernel, and the NN kernel's share of the VALU-issue bound"""
    rows = list(csv.DictReader(open(path)))
    print("%-60s %8s %12s" % ("kernel", "calls", "avg us"))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        print("%-60s %8s %12.1f" % (r["Name"][:60], r["Calls"], float(r["AverageNs"]) / 1e3))
    nn = [r for r in rows if r["Name"].startswith("chamfer_nn_kernel") or "chamfer_nn_kernel" in r["Name"]]
    if nn:
        # every size runs (warm-up + iters) x 2 calc_cd calls + 1 check call
        per = 2 * (iters + 1) + 1
        pairs = sum(per * 2.0 * B * P * P for P in sizes)
        t = float(nn[0]["TotalDurationNs"]) * 1e-9
        assert int(nn[0]["Calls"]) == per * len(sizes), (nn[0]["Calls"], per * len(sizes))
        print("chamfer_nn_kernel: %.3e directed pairs/s over kernel time = %.1f %% of the VALU-issue bound (%.2e/s)" %
              (pairs / t, 100.0 * pairs / t / VALU_BOUND_PAIRS_PER_S, VALU_BOUND_PAIRS_PER_S))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048,8192")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--no-cli", action="store_true", help="skip (c) (the profiled run: --stats counts the NN launches of (a) and (b))")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.stats:
        stats(a.stats, sizes, a.batch, a.iters)
    else:
        run(sizes, a.batch, a.iters, cli=not a.no_cli)
