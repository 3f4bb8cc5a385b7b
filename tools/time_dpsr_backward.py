"""tools/time_dpsr_backward.py -- time of DPSR forward + backward on the GPU (slide_amd/csrc/dpsr.hip + dpsr_bwd.hip through
slide_amd.train.functions.DpsrGrid), one process, not a test and not part of bench.py:

  (a) loss.backward() through dpsr_utils.dpsr.DPSR (V and N require grad; the composed entry points, in chunks), and the forward of it alone
  (b) forward + backward of the torch composition of tools/time_dpsr.py (index arithmetic, scatter_add_, torch.fft.rfftn / irfftn,
      gathers) under torch's autograd, on the same chunks (chunk by chunk, the gradients accumulated by autograd)
  (c) each separately callable step of the backward on one chunk

at B x n points (default 32 x 20480), r 128, sig 2, upstream gradient of a mean-squared error (tests/dpsr_grad_cases.py: its
magnitude).  Device-event times, the calls alternating, the median over --iters.  --only hip runs (a) alone (for a kernel trace).

usage:  python tools/time_dpsr_backward.py [--batch 32] [--points 20480] [--res 128] [--sig 2] [--iters 5] [--only hip]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "pointnet2"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def run(B, n, r, sig, iters, only):
    import torch
    import dpsr_cases as C
    from dpsr_utils.dpsr import DPSR
    from slide_amd import _ext
    from time_dpsr import _alternating_ms, torch_dpsr, torch_multipliers
    assert torch.cuda.is_available(), "time_dpsr_backward.py needs a GPU"
    dev = torch.device("cuda:0")
    Vn, Nn = C.sphere_cloud(0, B, n)
    V, N = torch.from_numpy(Vn).to(dev), torch.from_numpy(Nn).to(dev)
    m = DPSR((r, r, r), sig=sig).to(dev)
    cb = min(_ext.dpsr_chunk(r, n), B)
    print("%d x %d points, r %d, sig %g, chunks of %d samples; device-event ms, median of %d alternating calls" % (B, n, r, sig, cb, iters),
          flush=True)
    with torch.no_grad():
        phi0 = m(V, N)
        target = 0.9 * torch.tanh(phi0) + 0.05 * torch.randn(phi0.shape, device=dev, generator=torch.Generator(dev).manual_seed(0))
    out = {}

    def hip_step():
        Vg, Ng = V.detach().requires_grad_(True), N.detach().requires_grad_(True)
        torch.nn.functional.mse_loss(m(Vg, Ng), target).backward()
        out["hip"] = (Vg.grad, Ng.grad)

    def hip_forward():
        with torch.no_grad():
            m(V, N)

    fns, names = [hip_step, hip_forward], ["DPSR forward + backward (B %d)" % B, "DPSR forward alone (B %d)" % B]
    if only != "hip":
        try:
            mult = torch_multipliers(r, sig, dev)

            def torch_step():
                Vg, Ng = V.detach().requires_grad_(True), N.detach().requires_grad_(True)
                for s in range(0, B, cb):
                    phi = torch_dpsr(Vg[s:s + cb], Ng[s:s + cb], mult, r)
                    (((phi - target[s:s + cb]) ** 2).sum() / target.numel()).backward()
                out["torch"] = (Vg.grad, Ng.grad)

            torch_step()
            torch.cuda.synchronize()
            fns.append(torch_step)
            names.append("torch composition forward + backward (B %d, same chunks)" % B)
        except Exception as e:  # noqa: BLE001 (whatever the FFT library raises)
            print("torch.fft is not usable here (%s: %s): absolute times only" % (type(e).__name__, str(e).split("\n")[0]), flush=True)
    n_tot = len(fns)
    parts = []
    if only != "hip":
        Vc, Nc = V[:cb].contiguous(), N[:cb].contiguous()
        with torch.no_grad():
            phi, coef = _ext.dpsr_grid(Vc, Nc, m.G, return_coef=True)
            g = (2 * (phi - target[:cb]) / target.numel()).contiguous()
            ones = torch.ones(cb, n, 1, device=dev)
            sums = _ext.dpsr_bwd_sums(g, phi)
            w = _ext.point_rasterize_fixed(Vc, ones, r)[:, 0].contiguous()
            dpre = _ext.dpsr_bwd_dpre(g, phi, sums, coef, w, n)
            spec = _ext.fft3_r2c(dpre)
            spec3 = _ext.dpsr_spectral_adj(spec, m.G)
            dras = _ext.fft3_c2r(spec3)
        parts = [("sums (2 launches)", lambda: _ext.dpsr_bwd_sums(g, phi)),
                 ("density W: zero fill + scatter, 1 column", lambda: _ext.point_rasterize_fixed(Vc, ones, r)),
                 ("dpre (elementwise)", lambda: _ext.dpsr_bwd_dpre(g, phi, sums, coef, w, n)),
                 ("fft3_r2c, 1 grid per sample (3 launches)", lambda: _ext.fft3_r2c(dpre)),
                 ("adjoint spectral solve", lambda: _ext.dpsr_spectral_adj(spec, m.G)),
                 ("fft3_c2r, 3 grids per sample (3 launches) + spectrum copy", lambda: _ext.fft3_c2r(spec3)),
                 ("spectrum copy alone", lambda: spec3.clone()),
                 ("per-point gather", lambda: _ext.dpsr_bwd_points(Vc, Nc, dras, phi, sums, coef, shift=True, scale=True))]
    ms = _alternating_ms(fns + [p[1] for p in parts], iters)
    for name, t in zip(names + ["  chunk of %d: %s" % (cb, p[0]) for p in parts], ms):
        print("%-72s %9.3f ms" % (name, t), flush=True)
    print("backward alone (difference): %.3f ms" % (ms[0] - ms[1]))
    if n_tot == 3:
        print("torch composition / DPSR, forward + backward: %.2fx" % (ms[2] / ms[0]))
        for k, what in enumerate(("dV", "dN")):
            a, b = out["hip"][k], out["torch"][k]
            print("max |%s - torch composition's| %.3e (max |%s| %.3e)" % (what, float((a - b).abs().max()), what, float(a.abs().max())))
    first = out["hip"]
    hip_step()
    print("two runs bit-equal: %s" % bool(torch.equal(first[0], out["hip"][0]) and torch.equal(first[1], out["hip"][1])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=20480)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--sig", type=float, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", choices=("all", "hip"), default="all")
    a = ap.parse_args()
    run(a.batch, a.points, a.res, a.sig, a.iters, a.only)
