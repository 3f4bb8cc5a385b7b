"""tools/gen_golden_dpsr_grad.py -- AUTHORING ONLY, CPU (never imported by tests, bench or smoke): records
tests/golden/golden_dpsr_grad.npz, the gradients of the reference's DPSR (pointnet2/dpsr_utils/dpsr.py) under its own autograd.  The
reference modules are imported where they lie through tools/gen_golden_dpsr.py's stub-module loader; nothing of the reference is copied.

Inputs: V_r16 / N_r16 / V_r32 / N_r32 of tests/golden/golden_dpsr.npz (the point at 0, lattice-plane points, last-cell points, 40
coincident points).  Cases: the six of tests/dpsr_cases.py.  Upstream gradient: tests/dpsr_grad_cases.upstream (a mean-squared-error
gradient against 0.9 tanh(phi) + 0.05 noise over the element count, float32) of the float64 restatement of phi.
Recorded per case:
  dV64_<case>, dN64_<case>   phi.backward(g) of the reference's float64 evaluation (inputs, G and omega in double), f64
  dV32_<case>, dN32_<case>   of its float32 run, f32
  g_<case>                   the upstream gradient, r 16 only (tests/test_dpsr_grad_host.py pins the recipe to it)
and prints, per case, the reference's float32 error, the distance of every wrong arithmetic of tests/dpsr_grad_cases.py and the
derived bounds -- the table of profiles/dpsr_backward.md.

usage:  python tools/gen_golden_dpsr_grad.py [--reference DIR] [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def run_case(D, U, torch, V, N, r, sig, shift, scale, g, double):
    res = (r, r, r)
    m = D.DPSR(res, sig=sig, scale=scale, shift=shift)
    Vt, Nt, gt = torch.from_numpy(V), torch.from_numpy(N), torch.from_numpy(g)
    if double:
        m.G = U.spec_gaussian_filter(res=res, sig=sig)
        m.omega = U.fftfreqs(res, dtype=torch.float64).unsqueeze(-1) * (2 * np.pi)
        Vt, Nt, gt = Vt.double(), Nt.double(), gt.double()
    Vt.requires_grad_(True)
    Nt.requires_grad_(True)
    phi = m(Vt, Nt)
    phi.backward(gt)
    return phi.detach().numpy(), Vt.grad.numpy(), Nt.grad.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference tree (default: tools/ref_shims.REF)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    import gen_golden_dpsr as F
    if a.reference is None:
        import ref_shims
        a.reference = ref_shims.REF
    D, U = F.load_reference(a.reference)
    import torch
    import dpsr_cases as C
    import dpsr_grad_cases as GC
    golden = np.load(os.path.join(a.out, "golden_dpsr.npz"))
    out = {}
    for index, (name, r, sig, shift, scale) in enumerate(GC.CASES):
        V, N = golden["V_r%d" % r], golden["N_r%d" % r]
        g = GC.upstream(index, C.restate(V, N, r, sig, shift, scale))
        phi64, dV64, dN64 = run_case(D, U, torch, V, N, r, sig, shift, scale, g, True)
        _, dV32, dN32 = run_case(D, U, torch, V, N, r, sig, shift, scale, g, False)
        assert dV64.dtype == np.float64 and dV32.dtype == np.float32
        out["dV64_" + name], out["dN64_" + name], out["dV32_" + name], out["dN32_" + name] = dV64, dN64, dV32, dN32
        if r == 16:
            out["g_" + name] = g
        rV, rN, d = GC.backward(V, N, r, sig, shift, scale, g, detail=True)
        bV, bN = GC.grad_bounds(V, N, r, sig, shift, scale, d, rV, rN)
        nb = len(V)
        mx = lambda x: np.abs(x).reshape(nb, -1).max(1)
        print("%s: max |dV| %s max |dN| %s; restatement against the reference's float64 %.1e / %.1e (relative)" % (
            name, mx(dV64), mx(dN64), (mx(rV - dV64) / mx(dV64)).max(), (mx(rN - dN64) / mx(dN64)).max()))
        print("    bound dV %s dN %s (relative %s %s)" % (bV, bN, bV / mx(dV64), bN / mx(dN64)))
        print("    reference float32: dV %s dN %s bounds (relative %.1e %.1e)" % (
            mx(dV32 - dV64) / bV, mx(dN32 - dN64) / bN, (mx(dV32 - dV64) / mx(dV64)).max(), (mx(dN32 - dN64) / mx(dN64)).max()))
        for w in GC.WRONG:
            wV, wN = GC.backward(V, N, r, sig, shift, scale, g, wrong=w)
            print("    %-12s dV %s dN %s bounds away%s" % (w, mx(wV - dV64) / bV, mx(wN - dN64) / bN, "".join(
                "" if GC.applies(w, what, sig, shift, scale) else " (%s exempt)" % what for what in ("dV", "dN"))))
    path = os.path.join(a.out, "golden_dpsr_grad.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes, cap %d)" % (path, size, C.SIZE_CAP))
    assert size <= C.SIZE_CAP, "the fixture exceeds the cap"


if __name__ == "__main__":
    main()
