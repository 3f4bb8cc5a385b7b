"""tools/time_pairwise_emd.py -- throughput of the all-pairs approximate Earth Mover's Distance on the GPU
(slide_amd/csrc/emd_pairwise.hip), one process:

  (a) _ext.emd_pairwise, the matrix form (M x M ordered pairs) and the paired form (4096 pairs), in ONE launch each (the wrapper's
      row-block split is switched off for the measurement, and reported separately with the default bound)
  (b) a dense torch composition of the same ten levels on the same device: the (B, n, m) distance, exponential and match tensors
      materialised per level, for a batch of pairs that fits in memory

at M in --sizes (default 64, 256) and P = Q in --points (default 1024, 2048).  Rates are exponential evaluations per second over
device-event time: a pair of clouds costs 3 sweeps x 10 levels x P x Q of them.  (a) and (b) are compared within the tolerance of
tests/emd_cases.py.  With --all-metrics S, also the wall time of compute_all_metrics(emd=True) on two sets of S clouds of the
last --points value, next to its extrapolation from the measured matrix rate.

usage:  python tools/time_pairwise_emd.py [--sizes 64,256] [--points 1024,2048] [--iters 2] [--all-metrics 1000]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "pointnet2"))
sys.path.insert(0, os.path.join(REPO, "tests"))

# VALU-issue bound of emd_pairwise_kernel<double>, from the gfx950 ISA of the product build.  With 8 own
# points per thread one inner step evaluates 4 staged points x 8 own points per lane (2048 point pairs per wave):
#   sweeps A and B: 322 VALU instructions (96 v_sub_f32, 64 v_mul_f32, 64 v_fmac_f32, 2 moves | 32 v_cvt_f64_f32, 32 v_fmac_f64 |
#                   32 v_exp_f32)
#   sweep C:        265 VALU instructions (48 v_pk_add_f32, 32 v_pk_mul_f32, 48 v_pk_fma_f32, 32 v_mul_f32, 4 v_cvt_f32_f64, 5 moves |
#                   32 v_cvt_f64_f32, 32 v_fmac_f64 | 32 v_exp_f32)
# priced at 2 SIMD cycles per plain or packed float instruction (32 lanes per cycle), 4 per double-precision instruction or
# conversion (half rate) and 8 per transcendental (quarter rate).
CYCLES_AB = 226 * 2.0 + 64 * 4.0 + 32 * 8.0
CYCLES_C = 169 * 2.0 + 64 * 4.0 + 32 * 8.0
EVALS_PER_SIMD_CYCLE = 3 * 2048 / (2 * CYCLES_AB + CYCLES_C)
SIMDS = 256 * 4
CLOCK_HZ = 2.4e9
VALU_BOUND_EVALS_PER_S = EVALS_PER_SIMD_CYCLE * SIMDS * CLOCK_HZ  # ~5.4e12
PAIRED = 4096
COMPOSITION_BATCH = 32


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
    """the raw costs (B,) of x (B, n, 3) against y (B, m, 3): ten levels of dense (B, n, m) tensors, the algorithm of
    tests/emd_cases.py::emd_ref in float32 torch"""
    import torch
    from emd_cases import LEVELS
    B, n, m = x.shape[0], x.shape[1], y.shape[1]
    d = (x[:, :, None, :] - y[:, None, :, :]).pow(2).sum(-1)
    multiL, multiR = (1, n // m) if n >= m else (m // n, 1)
    remainL = torch.full((B, n), float(multiL), device=x.device)
    remainR = torch.full((B, m), float(multiR), device=x.device)
    cost = torch.zeros(B, device=x.device)
    for level in LEVELS:
        e = torch.exp(level * d)
        ratioL = remainL / (1e-9 + torch.bmm(e, remainR[:, :, None])[:, :, 0])
        sumr = remainR * torch.bmm(ratioL[:, None, :], e)[:, 0]
        ratioR = torch.clamp(remainR / (sumr + 1e-9), max=1.0) * remainR
        remainR = torch.clamp(remainR - sumr, min=0.0)
        w = e * ratioL[:, :, None] * ratioR[:, None, :]
        cost = cost + (d * w).sum((1, 2))
        remainL = torch.clamp(remainL - w.sum(2), min=0.0)
    return cost


def run(sizes, points, iters, all_metrics):
    import torch
    import emd_cases
    from metrics_point_cloud.generation_metrics import compute_all_metrics
    from slide_amd import _ext
    assert torch.cuda.is_available(), "time_pairwise_emd.py needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    one = float("inf")  # one launch, whatever the size
    print("rates in exponential evaluations/s (30 P Q per ordered pair); VALU-issue bound of the kernel %.3e/s" % VALU_BOUND_EVALS_PER_S,
          flush=True)
    rate = None
    with torch.no_grad():
        for P in points:
            for M in sizes:
                x = torch.randn(M, P, 3, generator=gen).to(dev)
                y = (0.9 * torch.randn(M, P, 3, generator=gen)).to(dev)
                evals = 30.0 * M * M * P * P
                t_m = _events_ms(lambda: _ext.emd_pairwise(x, y, max_evals=one), iters)
                t_d = _events_ms(lambda: _ext.emd_pairwise(x, y), iters)
                ii = torch.arange(PAIRED, device=dev)
                xp, yp = x[ii % M].contiguous(), y[(ii // M) % M].contiguous()
                t_p = _events_ms(lambda: _ext.emd_pairwise(xp, yp, paired=True, max_evals=one), iters)
                ev_p = 30.0 * PAIRED * P * P
                rate = evals / t_m * 1e3
                print("P = Q %5d  M = N %4d  matrix %9.2f ms %.3e/s = %.1f %% of the VALU bound | default row-block split %9.2f ms "
                      "(%d launches) | paired x %d %9.2f ms %.3e/s"
                      % (P, M, t_m, rate, 100.0 * rate / VALU_BOUND_EVALS_PER_S, t_d,
                         -(-M // max(1, int(_ext.EMD_EVALS_PER_LAUNCH // (30.0 * M * P * P)))), PAIRED, t_p, ev_p / t_p * 1e3), flush=True)
            B = COMPOSITION_BATCH
            xb, yb = x[:B].contiguous(), y[:B].contiguous()
            t_c = _events_ms(lambda: composition(xb, yb), iters)
            t_k = _events_ms(lambda: _ext.emd_pairwise(xb, yb, paired=True), iters)
            got, want = _ext.emd_pairwise(xb, yb, paired=True).double().cpu(), composition(xb, yb).double().cpu()
            S = torch.tensor([emd_cases.scale(a, b) for a, b in zip(xb.cpu().numpy(), yb.cpu().numpy())])
            worst = float(((got - want).abs() / (want.abs() + S)).max())
            print("P = Q %5d  %d pairs: dense torch composition %9.2f ms %.3e/s | kernel (paired, %d workgroups) %9.2f ms | "
                  "composition / kernel %.2fx | largest |kernel - composition| / (|composition| + S) %.2e"
                  % (P, B, t_c, 30.0 * B * P * P / t_c * 1e3, B, t_k, t_c / t_k, worst), flush=True)
        if all_metrics:
            S_, P = all_metrics, points[-1]
            a = torch.randn(S_, P, 3, generator=gen).to(dev)
            b = (0.9 * torch.randn(S_, P, 3, generator=gen)).to(dev)
            compute_all_metrics(a[:8], b[:8], emd=True)  # warm-up
            torch.cuda.synchronize()
            predicted = 3 * 30.0 * S_ * S_ * P * P / rate
            print("compute_all_metrics(emd=True), %d x %d clouds of %d points: extrapolated from the last matrix rate %.1f s"
                  % (S_, S_, P, predicted), flush=True)
            t0 = time.perf_counter()
            r = compute_all_metrics(a, b, emd=True)
            vals = {k: float(v) for k, v in r.items()}
            dt = time.perf_counter() - t0
            print("  measured %.1f s wall  %s" % (dt, vals), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--points", default="1024,2048")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--all-metrics", type=int, default=0, help="also time compute_all_metrics(emd=True) on two sets of this many clouds")
    a = ap.parse_args()
    run([int(s) for s in a.sizes.split(",")], [int(s) for s in a.points.split(",")], a.iters, a.all_metrics)
