"""tools/time_pairwise_cd.py -- throughput of the all-pairs Chamfer matrix on the GPU (slide_amd/csrc/chamfer_pairwise.hip), one process:

  (a) _ext.chamfer_pairwise, the general form (x against y) and the symmetric form (x against itself: upper triangle + mirror)
  (b) the composition it replaces: every sample cloud expanded against row blocks of 256 references through
      chamfer_and_f1.calc_cd_reduced (chamfer_nn_kernel + chamfer_reduce_kernel per block)

at M = N in --sizes (default 256, 1024), P = Q = 2048.  Rates are DIRECTED pair evaluations per second over device-event time; the
general form and (b) evaluate 2 M N P Q of them, the symmetric form's rate is quoted for the same 2 M N P Q (the work it stands
for).  (a) and (b) are compared bitwise on every size.  With --all-metrics S, also the wall time of compute_all_metrics on two
sets of S clouds (three matrices + the set statistics).

  --stats FILE   instead: read a rocprofv3 --kernel-trace --stats kernel_stats.csv of a run of this script and print each kernel's
                 calls and time per call

usage:  python tools/time_pairwise_cd.py [--sizes 256,1024] [--points 2048] [--iters 3] [--all-metrics 1000]
        rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/time_pairwise_cd.py --sizes 256 --iters 2
"""
import argparse
import csv
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "pointnet2"))

# VALU-issue bound of chamfer_pairwise_kernel: the inner step of its four-queries-per-thread tile evaluates
# 8 search points x 4 queries per lane (2048 directed pairs per wave) in 209 VALU instructions (gfx950 ISA of the product build:
# 96 v_sub_f32, 32 v_mul_f32, 64 v_fmac_f32, 16 v_min3_f32, 1 move; none packed), 2 SIMD cycles each.
VALU_PAIRS_PER_SIMD_CYCLE = 2048 / (209 * 2.0)
SIMDS = 256 * 4
CLOCK_HZ = 2.4e9
VALU_BOUND_PAIRS_PER_S = VALU_PAIRS_PER_SIMD_CYCLE * SIMDS * CLOCK_HZ  # ~1.2e13
ROW_BLOCK = 256


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


def composition(x, y):
    """the (M, N, 2, 2) sums from the per-pair kernels: x[i] expanded against blocks of 256 clouds of y"""
    import torch
    from metrics_point_cloud.chamfer_and_f1 import calc_cd_reduced
    rows = []
    for i in range(x.shape[0]):
        blocks = []
        for s in range(0, y.shape[0], ROW_BLOCK):
            yb = y[s:s + ROW_BLOCK]
            xe = x[i:i + 1].expand(yb.shape[0], -1, -1).contiguous()
            blocks.append(calc_cd_reduced(yb, xe)[0][:, :, :2])  # calc_cd_reduced(output, gt): direction 0 runs over gt = x[i]
        rows.append(torch.cat(blocks))
    return torch.stack(rows)


def run(sizes, P, iters, all_metrics):
    import torch
    from metrics_point_cloud.generation_metrics import compute_all_metrics
    from slide_amd import _ext
    assert torch.cuda.is_available(), "time_pairwise_cd.py needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    print("P = Q = %d, rates in directed pair evaluations/s (2 M N P Q); VALU-issue bound of the pairwise kernel %.3e/s"
          % (P, VALU_BOUND_PAIRS_PER_S), flush=True)
    with torch.no_grad():
        for M in sizes:
            x = torch.randn(M, P, 3, generator=gen).to(dev)
            y = (0.9 * torch.randn(M, P, 3, generator=gen)).to(dev)
            pairs = 2.0 * M * M * P * P
            t_g = _events_ms(lambda: _ext.chamfer_pairwise(x, y), iters)
            t_s = _events_ms(lambda: _ext.chamfer_pairwise(x), iters)
            t_c = _events_ms(lambda: composition(x, y), max(1, iters // 2))
            same = torch.equal(_ext.chamfer_pairwise(x, y).view(torch.int32), composition(x, y).view(torch.int32))
            print("M = N %5d  (a) general %9.2f ms %.3e/s = %.1f %% of the VALU bound | symmetric %9.2f ms %.3e/s, %.3f x general "
                  "| (b) per-pair kernels by row blocks %9.2f ms %.3e/s | (b)/(a) %.2fx | bitwise equal: %s"
                  % (M, t_g, pairs / t_g * 1e3, 100.0 * pairs / t_g * 1e3 / VALU_BOUND_PAIRS_PER_S, t_s, pairs / t_s * 1e3, t_s / t_g,
                     t_c, pairs / t_c * 1e3, t_c / t_g, same), flush=True)
            assert same
        if all_metrics:
            S = all_metrics
            a = torch.randn(S, P, 3, generator=gen).to(dev)
            b = (0.9 * torch.randn(S, P, 3, generator=gen)).to(dev)
            compute_all_metrics(a[:8], b[:8])  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = compute_all_metrics(a, b)
            vals = {k: float(v) for k, v in r.items()}
            dt = time.perf_counter() - t0
            print("compute_all_metrics, %d x %d clouds of %d points: %.3f s wall  %s" % (S, S, P, dt, vals), flush=True)


def stats(path):
    rows = list(csv.DictReader(open(path)))
    print("%-60s %8s %12s" % ("kernel", "calls", "avg us"))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        print("%-60s %8s %12.1f" % (r["Name"][:60], r["Calls"], float(r["AverageNs"]) / 1e3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--all-metrics", type=int, default=0, help="also time compute_all_metrics on two sets of this many clouds")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    else:
        run([int(s) for s in a.sizes.split(",")], a.points, a.iters, a.all_metrics)
