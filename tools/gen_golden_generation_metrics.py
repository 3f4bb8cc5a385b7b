"""tools/gen_golden_generation_metrics.py -- AUTHORING ONLY (never imported by tests, bench or smoke): records
tests/golden/golden_generation_metrics.npz from the reference's pointnet2/models/pvd/metrics/evaluation_metrics.py.

The reference module is imported where it lies (--reference, default tools/ref_shims.REF); nothing of it is copied.  Its CUDA-only
imports (metrics.PyTorchEMD, metrics.ChamferDistancePytorch) are stub modules in sys.modules, as tools/ref_shims.py does it for the
other fixtures; scipy and tqdm are stubbed only where they are not installed.  The Chamfer stub hands the reference's OWN
`distChamfer` (its pure-torch all-pairs formulation) to the reference's `_pairwise_EMD_CD_` loop, evaluated in float64.

Recorded (arrays only):
  samples (24, 256, 3) f32, refs (20, 256, 3) f32   clouds of varied scale and offset; refs[COPY_REF] is samples[COPY_SMP], so the
                                                    cross matrix holds a zero off its diagonal
  M_rs (20, 24), M_rr (20, 20), M_ss (24, 24) f64   _pairwise_EMD_CD_(refs, samples), (refs, refs), (samples, samples)
  mmd_cov_<key>, knn_<key>  f64 scalars             lgan_mmd_cov(M_rs.t()) and knn(M_rr, M_rs, M_ss, 1) on those matrices
  min_gap                                           the smallest relative gap (runner-up - minimum) / minimum over every row /
                                                    column whose arg-min decides coverage or a 1-NN vote

Fixture condition, checked here and again by tests/test_generation_metrics_host.py: min_gap > 1e-4, three orders above the fp32
kernel's error bound (8 eps), so coverage and the 1-NN confusion counts of an fp32 evaluation must equal the recorded ones exactly.
A seed that does not meet it is rejected (take another; do not loosen the test).

usage:  python tools/gen_golden_generation_metrics.py [--reference DIR] [--seed 0] [--out tests/golden]
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

N_SMP, N_REF, POINTS = 24, 20, 256
COPY_SMP, COPY_REF = 3, 7
GAP = 1e-4


def load_reference(ref_root):
    """the reference's evaluation_metrics module with its native / missing imports stubbed"""
    sys.dont_write_bytecode = True
    holder = {}

    class chamfer_3DDist:  # the CUDA op's interface: (dist of x's points, dist of y's points, idx1, idx2)
        def __call__(self, a, b):
            per_y, per_x = holder["m"].distChamfer(a, b)
            return per_x, per_y, None, None

    def stub(name, **attrs):
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
        return mod

    stub("metrics")
    stub("metrics.PyTorchEMD")
    stub("metrics.PyTorchEMD.emd", earth_mover_distance=lambda a, b, transpose=False: a.new_zeros(a.shape[0]))
    stub("metrics.ChamferDistancePytorch")
    stub("metrics.ChamferDistancePytorch.chamfer3D")
    stub("metrics.ChamferDistancePytorch.chamfer3D.dist_chamfer_3D", chamfer_3DDist=chamfer_3DDist)
    stub("metrics.ChamferDistancePytorch.fscore", fscore=None)
    try:
        import scipy.stats  # noqa: F401
    except ImportError:
        stub("scipy")
        stub("scipy.stats", entropy=None)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stub("tqdm", tqdm=lambda it: it)
    torch.Tensor.cuda = lambda self, *a, **k: self  # the reference moves every block to the GPU; this run is on the CPU
    path = os.path.join(ref_root, "pointnet2", "models", "pvd", "metrics", "evaluation_metrics.py")
    spec = importlib.util.spec_from_file_location("reference_evaluation_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    holder["m"] = mod
    return mod


def make_sets(seed):
    """clouds that differ in scale and offset (so that nearest neighbours, coverage and the 1-NN test are not degenerate); the
    samples are drawn a little wider than the references"""
    rs = np.random.RandomState(seed)

    def clouds(n, spread):
        scale = rs.uniform(0.5, 1.5, (n, 1, 3))
        shift = spread * rs.standard_normal((n, 1, 3))
        return (rs.standard_normal((n, POINTS, 3)) * scale + shift).astype(np.float32)

    samples, refs = clouds(N_SMP, 0.4), clouds(N_REF, 0.3)
    # the shared cloud sits apart from all others: CD(c, shared) is the same number in two blocks of the 1-NN matrix (once with a
    # reference's label, once with a sample's), so it must not be any OTHER cloud's nearest neighbour or that vote would be a tie
    samples[COPY_SMP] += np.float32(4.0)
    refs[COPY_REF] = samples[COPY_SMP]
    return samples, refs


def min_relative_gap(M_rs, M_rr, M_ss):
    """smallest (runner-up - minimum) / minimum over the deciding rows and columns: coverage takes each sample's nearest reference
    (columns of M_rs), the 1-NN test each element's nearest other element (columns of the full matrix, diagonal excluded)"""
    def gaps(A):  # per column
        srt = np.sort(A, axis=0)
        lo, up = srt[0], srt[1]
        return (up - lo) / np.maximum(np.abs(lo), 1e-300)

    full = np.block([[M_rr, M_rs], [M_rs.T, M_ss]]).astype(np.float64)
    np.fill_diagonal(full, np.inf)
    return float(min(gaps(M_rs).min(), gaps(full).min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference tree (default: tools/ref_shims.REF)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    if a.reference is None:
        import ref_shims
        a.reference = ref_shims.REF
    E = load_reference(a.reference)
    samples, refs = make_sets(a.seed)
    s64, r64 = torch.from_numpy(samples).double(), torch.from_numpy(refs).double()
    M_rs = E._pairwise_EMD_CD_(r64, s64, 7)[0]  # a block size that does not divide either set
    M_rr = E._pairwise_EMD_CD_(r64, r64, 7)[0]
    M_ss = E._pairwise_EMD_CD_(s64, s64, 7)[0]
    assert M_rs.dtype == torch.float64 and M_rs.shape == (N_REF, N_SMP)
    gap = min_relative_gap(M_rs.numpy(), M_rr.numpy(), M_ss.numpy())
    if not gap > GAP:
        raise SystemExit("seed %d: smallest relative gap %.3e <= %.0e -- take another seed" % (a.seed, gap, GAP))
    res = {"samples": samples, "refs": refs, "M_rs": M_rs.numpy(), "M_rr": M_rr.numpy(), "M_ss": M_ss.numpy(),
           "min_gap": np.float64(gap), "seed": np.int64(a.seed), "copy_smp_ref": np.array([COPY_SMP, COPY_REF], np.int64)}
    for k, v in E.lgan_mmd_cov(M_rs.t()).items():
        res["mmd_cov_" + k] = np.float64(v.item())
    for k, v in E.knn(M_rr, M_rs, M_ss, 1, sqrt=False).items():
        res["knn_" + k] = np.float64(v.item())
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "golden_generation_metrics.npz")
    np.savez_compressed(path, **res)
    print("wrote %s: min gap %.3e, cross zero %.3e" % (path, gap, float(M_rs[COPY_REF, COPY_SMP])))
    for k in sorted(res):
        if k.startswith(("mmd_cov_", "knn_")):
            print("  %-22s %.17g" % (k, float(res[k])))


if __name__ == "__main__":
    main()
