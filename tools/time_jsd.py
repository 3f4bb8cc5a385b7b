"""tools/time_jsd.py -- time of the JSD metric's occupancy counters on the GPU (slide_amd/csrc/occupancy_grid.hip), one process:

  (a) metrics_point_cloud.generation_metrics.entropy_of_occupancy_grid (one kernel launch + the host's float64 entropy) and the
      launch alone (_ext.occupancy_grid)
  (b) the composition it replaces, from what the library already had: _ext.knn_points K = 1 of all points against the admissible
      cells, torch.bincount for the counters and torch.unique over (cloud, cell) keys for the per-cloud Bernoulli variables

at S x P points (default 1000 x 2048), resolution 28, in_sphere True, on clouds normalised into the unit sphere and on the same
clouds scaled by 1.5 (many points then leave the sphere: their lattice cell is not admissible and the kernel scans for them).
(a) and (b) are compared for equality.  Device-event times, the calls alternating, the median over --iters.

How the kernel's time splits between its two steps: the same points are also timed with in_sphere False (every cell admissible:
the lattice step only); the difference to in_sphere True is the scan step's share.  The fraction of points that take the scan step
is reported with it.

  --stats FILE   instead: read a rocprofv3 --kernel-trace --stats kernel_stats.csv of a run of this script and print each kernel's
                 calls and time per call

usage:  python tools/time_jsd.py [--clouds 1000] [--points 2048] [--resolution 28] [--iters 7]
        rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/time_jsd.py --iters 2
"""
import argparse
import csv
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "pointnet2"))


def _alternating_ms(fns, iters):
    """median device-event time of each function, the calls interleaved (a, b, c, a, b, c, ...) after one warm-up round"""
    import torch
    for f in fns:
        f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            times[i].append(a.elapsed_time(b))
    return [sorted(t)[len(t) // 2] for t in times]


def composition(pts, grid_adm):
    """(counters, Bernoulli variables) over the admissible cells from knn_points + bincount + unique"""
    import torch
    from slide_amd import _ext
    S, P, n = pts.shape[0], pts.shape[1], grid_adm.shape[0]
    idx = _ext.knn_points(pts.reshape(1, S * P, 3), grid_adm[None], 1)[1].reshape(S, P)
    counts = torch.bincount(idx.reshape(-1), minlength=n)
    keys = torch.unique(idx + torch.arange(S, device=pts.device)[:, None] * n)
    return counts, torch.bincount(keys % n, minlength=n)


def run(S, P, R, iters):
    import numpy as np
    import torch
    import metrics_point_cloud.generation_metrics as G
    from slide_amd import _ext
    assert torch.cuda.is_available(), "time_jsd.py needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(S, P, 3, generator=gen) * (0.3 + 0.7 * torch.rand(S, 1, 3, generator=gen))
    x = (x / x.norm(dim=2).amax(dim=1)[:, None, None] * 0.5).to(dev)
    axis, grid, mask = G._grid_axis_and_mask(R, True)
    ones = np.ones_like(mask)
    a_t, m_t, o_t = torch.tensor(axis).to(dev), torch.tensor(mask).to(dev), torch.from_numpy(ones).to(dev)
    grid_adm = torch.tensor(grid[mask]).to(dev)
    print("%d x %d points, resolution %d, %d of %d cells inside the sphere; device-event ms, median of %d alternating calls"
          % (S, P, R, int(mask.sum()), len(mask), iters), flush=True)
    with torch.no_grad():
        for name, pts in (("normalised", x), ("scaled by 1.5", (x * 1.5).contiguous())):
            cells = _ext.occupancy_grid(pts, a_t, o_t, return_cells=True)[2]
            scan_fraction = 1.0 - float(m_t[cells.reshape(-1).long()].float().mean())
            t_fn, t_k, t_lat, t_c = _alternating_ms([lambda: G.entropy_of_occupancy_grid(pts, R, True),
                                                     lambda: _ext.occupancy_grid(pts, a_t, m_t),
                                                     lambda: _ext.occupancy_grid(pts, a_t, o_t),
                                                     lambda: composition(pts, grid_adm)], iters)
            t0 = time.perf_counter()
            G.entropy_of_occupancy_grid(pts, R, True)
            wall = (time.perf_counter() - t0) * 1e3
            counts, clouds = _ext.occupancy_grid(pts, a_t, m_t)
            c_counts, c_clouds = composition(pts, grid_adm)
            same = bool(torch.equal(counts[m_t].long(), c_counts) and torch.equal(clouds[m_t].long(), c_clouds))
            print("%-14s (a) entropy_of_occupancy_grid %8.3f ms (wall %8.3f ms) | launch alone %8.3f ms = %.3e points/s | in_sphere "
                  "False (lattice step only) %8.3f ms -> scan step %8.3f ms for %.1f %% of the points | (b) knn_points + bincount + "
                  "unique %8.3f ms | (b)/(a) %.2fx, against the launch alone %.2fx | equal counters: %s"
                  % (name, t_fn, wall, t_k, S * P / t_k * 1e3, t_lat, t_k - t_lat, 100.0 * scan_fraction, t_c, t_c / t_fn, t_c / t_k,
                     same), flush=True)


def stats(path):
    rows = list(csv.DictReader(open(path)))
    print("%-60s %8s %12s" % ("kernel", "calls", "avg us"))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        print("%-60s %8s %12.1f" % (r["Name"][:60], r["Calls"], float(r["AverageNs"]) / 1e3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=1000)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--resolution", type=int, default=28)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    else:
        run(a.clouds, a.points, a.resolution, a.iters)
