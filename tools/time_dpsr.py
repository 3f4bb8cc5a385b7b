"""tools/time_dpsr.py -- time of DPSR.forward on the GPU (slide_amd/csrc/dpsr.hip), one process, not a test and not part of bench.py:

  (a) dpsr_utils.dpsr.DPSR.forward (the composed entry point, in chunks) and each of its separately callable entry points on one
      chunk: rasterize (zero fill + scatter), fft3_r2c (3 launches), spectral solve, fft3_c2r (3 launches), grid_interp,
      shift + scale (2 launches)
  (b) the torch composition a user would otherwise write: index arithmetic, scatter_add_, torch.fft.rfftn / irfftn and gathers
      (written here from the formulas; a float scatter: its result differs from run to run)

at B x n points (default 32 x 20480), r 128, sig 2.  Device-event times, the calls alternating, the median over --iters; the two
results are compared.  If torch.fft cannot run on the machine (its library compiles kernels at run time) that is reported and (a)
is timed alone.

usage:  python tools/time_dpsr.py [--batch 32] [--points 20480] [--res 128] [--sig 2] [--iters 5]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "pointnet2"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def _alternating_ms(fns, iters):
    """median device-event time of each function, the calls interleaved after one warm-up round"""
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


def torch_multipliers(r, sig, dev):
    """-i omega_d G / (-|omega|^2 + 1e-6) as (3, r, r, r/2 + 1) complex64"""
    import torch
    k = torch.fft.fftfreq(r, d=1 / r)
    k3 = torch.fft.rfftfreq(r, d=1 / r)
    om = [2 * torch.pi * t for t in torch.meshgrid(k, k, k3, indexing="ij")]
    den = -(om[0] ** 2 + om[1] ** 2 + om[2] ** 2) + 1e-6
    G = torch.exp(-0.5 * (sig * 2 * torch.sqrt(om[0] ** 2 + om[1] ** 2 + om[2] ** 2) / (2 * torch.pi) / r) ** 2)
    return torch.stack([torch.complex(torch.zeros_like(o), -(o * G) / den) for o in om]).to(dev)


def torch_dpsr(V, N, mult, r):
    import torch
    B, n, _ = V.shape
    cs = 1.0 / r
    q = V / cs
    f0 = torch.floor(q)
    i0, i1 = f0.long(), torch.fmod(torch.ceil(q), r).long()
    wa, wb = (V - (f0 + 1) * cs).abs() / cs, (V - f0 * cs).abs() / cs
    ras = torch.zeros(B, 3, r ** 3, device=V.device)
    corners = []
    for c in range(8):
        b = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        idx = ((i1 if b[0] else i0)[..., 0] * r + (i1 if b[1] else i0)[..., 1]) * r + (i1 if b[2] else i0)[..., 2]
        w = (wb if b[0] else wa)[..., 0] * (wb if b[1] else wa)[..., 1] * (wb if b[2] else wa)[..., 2]
        ras.scatter_add_(2, idx[:, None, :].expand(B, 3, n), (w[..., None] * N).transpose(1, 2))
        corners.append((idx, w))
    S = torch.fft.rfftn(ras.view(B, 3, r, r, r), dim=(2, 3, 4))
    Phi = (S * mult).sum(1)
    Phi[:, 0, 0, 0] = 0
    phi = torch.fft.irfftn(Phi, s=(r, r, r), dim=(1, 2, 3))
    flat = phi.reshape(B, -1)
    fv = sum(flat.gather(1, idx) * w for idx, w in corners)
    phi = phi - fv.mean(1)[:, None, None, None]
    return -phi / phi[:, 0, 0, 0].abs()[:, None, None, None] * 0.5


def run(B, n, r, sig, iters):
    import torch
    import dpsr_cases as C
    from dpsr_utils.dpsr import DPSR
    from slide_amd import _ext
    assert torch.cuda.is_available(), "time_dpsr.py needs a GPU"
    dev = torch.device("cuda:0")
    Vn, Nn = C.sphere_cloud(0, B, n)
    V, N = torch.from_numpy(Vn).to(dev), torch.from_numpy(Nn).to(dev)
    m = DPSR((r, r, r), sig=sig).to(dev)
    cb = min(_ext.dpsr_chunk(r, n), B)
    print("%d x %d points, r %d, sig %g, chunks of %d samples; device-event ms, median of %d alternating calls" % (B, n, r, sig, cb, iters),
          flush=True)
    with torch.no_grad():
        fns, names = [lambda: m(V, N)], ["DPSR.forward (B %d)" % B]
        mult = None
        try:
            mult = torch_multipliers(r, sig, dev)
            ref = torch_dpsr(V[:cb], N[:cb], mult, r)
            torch.cuda.synchronize()
            fns.append(lambda: torch.cat([torch_dpsr(V[s:s + cb], N[s:s + cb], mult, r) for s in range(0, B, cb)]))
            names.append("torch composition (B %d, same chunks)" % B)
        except Exception as e:  # noqa: BLE001 (whatever the FFT library raises)
            print("torch.fft is not usable here (%s: %s): absolute times only" % (type(e).__name__, str(e).split("\n")[0]), flush=True)
        # the entry points, on one chunk
        Vc, Nc = V[:cb].contiguous(), N[:cb].contiguous()
        fixed = _ext.point_rasterize_fixed(Vc, Nc, r)
        spec = _ext.fft3_r2c(fixed)
        phis = _ext.dpsr_spectral(spec, m.G)
        work = phis.clone()
        phi = _ext.fft3_c2r(phis)
        fv = _ext.grid_interp(phi.unsqueeze(-1), Vc).squeeze(-1)
        out4 = torch.empty_like(phi)
        flag = torch.zeros(1, device=dev, dtype=torch.int32)
        from slide_amd._lib import check, lib
        from slide_amd.abi import ptr, stream_of
        L = lib()
        spec_r = torch.view_as_real(spec)
        work_r = torch.view_as_real(work)

        def rasterize():
            fixed.zero_()
            check(L.slide_point_rasterize(cb, n, 3, r, ptr(Vc), ptr(Nc), ptr(fixed), ptr(flag), stream_of()), "rasterize")

        def c2r():  # (the copy restores the spectrum the in-place passes overwrite; it is timed separately and subtracted)
            work.copy_(phis)
            check(L.slide_fft3_c2r(cb, r, ptr(work_r), ptr(out4), stream_of()), "c2r")

        parts = [("rasterize (zero fill + scatter)", rasterize),
                 ("fft3_r2c, 3 components (3 launches)", lambda: check(L.slide_fft3_r2c(3 * cb, r, ptr(fixed), 1, ptr(spec_r), stream_of()), "r2c")),
                 ("spectral solve", lambda: _ext.dpsr_spectral(spec, m.G)),
                 ("fft3_c2r (3 launches) + spectrum copy", c2r),
                 ("spectrum copy alone", lambda: work.copy_(phis)),
                 ("grid_interp at the points", lambda: _ext.grid_interp(phi.unsqueeze(-1), Vc)),
                 ("shift + scale (2 launches)", lambda: _ext.dpsr_finish(out4, fv))]
        ms = _alternating_ms(fns + [p[1] for p in parts], iters)
        for name, t in zip(names + ["  chunk of %d: %s" % (cb, p[0]) for p in parts], ms):
            print("%-62s %9.3f ms" % (name, t), flush=True)
        if len(fns) == 2:
            print("torch composition / DPSR.forward: %.2fx" % (ms[1] / ms[0]))
            got = m(V[:cb].contiguous(), N[:cb].contiguous())
            print("max |DPSR.forward - torch composition| on the first chunk: %.3e (max |phi| %.3f)" % (
                float((got - ref).abs().max()), float(got.abs().max())))
        a, b = m(V, N), m(V, N)
        print("two runs bit-equal: %s" % bool(torch.equal(a, b)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=20480)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--sig", type=float, default=2)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    run(a.batch, a.points, a.res, a.sig, a.iters)
