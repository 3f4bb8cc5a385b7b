"""tools/gen_golden_emd.py -- AUTHORING ONLY (never imported by tests, bench or smoke): records tests/golden/golden_emd.npz.

The reference's EMD kernels need CUDA and cannot be built here, so the matrices come from the float64 numpy restatement of its
algorithm, tests/emd_cases.py::emd_ref (pinned to the reference by its two-point known answer), evaluated on the `samples`
(24, 256, 3) and `refs` (20, 256, 3) of tests/golden/golden_generation_metrics.npz.  The set statistics are the REFERENCE's own
`lgan_mmd_cov` and `knn` (pointnet2/models/pvd/metrics/evaluation_metrics.py, imported where it lies with the stub modules of
tools/gen_golden_generation_metrics.py; nothing of it is copied) applied to those matrices.

Recorded (arrays only):
  M_rs (20, 24), M_rr (20, 20), M_ss (24, 24) f64   emd_ref(xyz1 = row cloud, xyz2 = column cloud) / 256: the second output of
                                                    _pairwise_EMD_CD_(refs, samples), (refs, refs), (samples, samples)
  mmd_cov_<key>, knn_<key>  f64 scalars             lgan_mmd_cov(M_rs.t()) and knn(M_rr, M_rs, M_ss, 1) on those matrices
  gap_nn, gap_cov                                   the smallest relative gap (runner-up - minimum) / minimum over the columns whose
                                                    arg-min decides a 1-NN vote / coverage (emd_cases.separation)

Fixture condition, checked here and again by tests/test_emd_host.py: both gaps are at least 20 R (emd_cases.R, the kernel's
tolerance), so coverage and the 1-NN confusion counts of the fp32 kernel must equal the recorded ones exactly.

usage:  python tools/gen_golden_emd.py [--reference DIR] [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def matrix(a, b):
    from emd_cases import emd_ref
    return np.array([[emd_ref(x1, x2) / len(x1) for x2 in b] for x1 in a], np.float64)


def main():
    import emd_cases
    from gen_golden_generation_metrics import load_reference
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference tree (default: tools/ref_shims.REF)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    if a.reference is None:
        import ref_shims
        a.reference = ref_shims.REF
    E = load_reference(a.reference)
    g = np.load(os.path.join(REPO, "tests", "golden", "golden_generation_metrics.npz"))
    samples, refs = g["samples"], g["refs"]
    M_rs, M_rr, M_ss = matrix(refs, samples), matrix(refs, refs), matrix(samples, samples)
    gap_nn, gap_cov = emd_cases.separation(M_rs, M_rr, M_ss)
    if not min(gap_nn, gap_cov) >= 20 * emd_cases.R:
        raise SystemExit("the deciding minima are separated by %.3e / %.3e < 20 R = %.3e" % (gap_nn, gap_cov, 20 * emd_cases.R))
    res = {"M_rs": M_rs, "M_rr": M_rr, "M_ss": M_ss, "gap_nn": np.float64(gap_nn), "gap_cov": np.float64(gap_cov)}
    t_rs, t_rr, t_ss = (torch.from_numpy(M) for M in (M_rs, M_rr, M_ss))
    for k, v in E.lgan_mmd_cov(t_rs.t()).items():
        res["mmd_cov_" + k] = np.float64(v.item())
    for k, v in E.knn(t_rr, t_rs, t_ss, 1, sqrt=False).items():
        res["knn_" + k] = np.float64(v.item())
    path = os.path.join(a.out, "golden_emd.npz")
    np.savez_compressed(path, **res)
    print("wrote %s: gaps 1-NN %.3e coverage %.3e; asymmetry of M_rr %.3e" % (path, gap_nn, gap_cov, np.abs(M_rr - M_rr.T).max()))
    for k in sorted(res):
        if k.startswith(("mmd_cov_", "knn_")):
            print("  %-22s %.17g" % (k, float(res[k])))


if __name__ == "__main__":
    main()
