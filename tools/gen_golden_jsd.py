"""tools/gen_golden_jsd.py -- AUTHORING ONLY (never imported by tests, bench or smoke; needs scipy and scikit-learn): records
tests/golden/golden_jsd.npz from the JSD block of the reference's pointnet2/models/pvd/metrics/evaluation_metrics.py
(unit_cube_grid_point_cloud, entropy_of_occupancy_grid, jensen_shannon_divergence, jsd_between_point_cloud_sets).

The reference module is imported where it lies through tools/gen_golden_generation_metrics.load_reference (its CUDA-only imports
are stub modules); nothing of it is copied.  One more shim: the module's own `from sklearn.neighbors import NearestNeighbors` is
commented out, so scikit-learn's class is put into the module's namespace -- as a subclass that also keeps the indices of every
query, from which this tool counts the per-cell Bernoulli variables (the reference uses them for the entropy but does not return them).

Recorded (arrays only), for the three input sets `sphere` (clouds normalised into the unit sphere), `cube` (uniform in the unit
cube: corners outside the sphere) and `outside` (points outside the cube), resolutions 28 and 9:
  pcs_<set>                       (10, 200, 3) f32
  grid_<R>_<0|1>                  unit_cube_grid_point_cloud(R, clip_sphere) flattened to (n, 3) f32
  counters_<set>_<R>_<0|1>        entropy_of_occupancy_grid(pcs, R, in_sphere)[1], f64
  bernoulli_<set>_<R>_<0|1>       clouds per cell, from the reference's query indices, f64
  entropy_<set>_<R>_<0|1>         entropy_of_occupancy_grid(pcs, R, in_sphere)[0], f64
  jsd_<setA>_<setB>_<R>           jsd_between_point_cloud_sets(pcs_A, pcs_B, R), f64
  min_margin                      smallest (second-nearest - nearest) squared distance to an admissible cell over every point, grid
                                  and mask, evaluated in float64

Fixture condition, checked here and again by tests/test_jsd_host.py: min_margin >= 1e-5, two orders above the error of an fp32
evaluation of these distances (about 1e-7), so an fp32 nearest-cell search must reproduce the counters exactly.  A point that does
not meet it is drawn again from its cloud's distribution (never dropped).

--time-reference S P: also time the reference's entropy_of_occupancy_grid once on S x P normalised points (context for
profiles/jsd.md: a CPU number from the authoring machine, not comparable with GPU timings elsewhere).

usage:  python tools/gen_golden_jsd.py [--reference DIR] [--seed 0] [--out tests/golden] [--time-reference 1000 2048]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

N_CLOUDS, POINTS = 10, 200
RESOLUTIONS = (28, 9)
MARGIN = 1e-5
SETS = ("sphere", "cube", "outside")


def load_reference(ref_root):
    from sklearn.neighbors import NearestNeighbors
    from gen_golden_generation_metrics import load_reference as load
    E = load(ref_root)
    queries = []

    class RecordingNearestNeighbors(NearestNeighbors):
        def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
            out = super().kneighbors(X, n_neighbors, return_distance)
            queries.append(np.asarray(out[1] if return_distance else out).reshape(-1).copy())
            return out

    E.NearestNeighbors = RecordingNearestNeighbors
    return E, queries


def draw_point(rs, kind, params):
    """one point of a cloud of the given set"""
    if kind == "cube":
        return rs.uniform(-0.5, 0.5, 3)
    scale, shift = params
    if kind == "outside":
        return rs.standard_normal(3) * scale + shift
    while True:  # sphere: an anisotropic Gaussian blob rejected to radius 0.5
        p = rs.standard_normal(3) * scale + shift
        if np.linalg.norm(p) <= 0.499:
            return p


def cloud_params(rs, kind):
    if kind == "sphere":
        return rs.uniform(0.08, 0.25, 3), rs.uniform(-0.1, 0.1, 3)
    if kind == "outside":
        return rs.uniform(0.3, 0.6, 3), rs.uniform(-0.3, 0.3, 3)
    return None


def margins(points, grids):
    """per point, the smallest float64 gap between the nearest and the second-nearest cell over all the grids"""
    p = points.astype(np.float64)
    out = np.full(len(p), np.inf)
    for g in grids:
        g = g.astype(np.float64)
        for s in range(0, len(p), 256):
            d = ((p[s:s + 256, None, :] - g[None]) ** 2).sum(-1)
            two = np.partition(d, 1, axis=1)[:, :2]
            out[s:s + 256] = np.minimum(out[s:s + 256], two[:, 1] - two[:, 0])
    return out


def make_set(rs, kind, grids):
    params = [cloud_params(rs, kind) for _ in range(N_CLOUDS)]
    pcs = np.stack([np.stack([draw_point(rs, kind, params[c]) for _ in range(POINTS)]) for c in range(N_CLOUDS)]).astype(np.float32)
    redrawn = 0
    while True:
        m = margins(pcs.reshape(-1, 3), grids).reshape(N_CLOUDS, POINTS)
        bad = np.argwhere(m < MARGIN)
        if not len(bad):
            return pcs, float(m.min()), redrawn
        for c, i in bad:
            pcs[c, i] = draw_point(rs, kind, params[c]).astype(np.float32)
            redrawn += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference tree (default: tools/ref_shims.REF)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--time-reference", type=int, nargs=2, default=None, metavar=("S", "P"))
    a = ap.parse_args()
    if a.reference is None:
        import ref_shims
        a.reference = ref_shims.REF
    E, queries = load_reference(a.reference)
    rs = np.random.RandomState(a.seed)
    if a.time_reference:
        S, P = a.time_reference
        x = rs.standard_normal((S, P, 3))
        x = (x / np.linalg.norm(x, axis=2).max(axis=1)[:, None, None] * 0.5).astype(np.float32)
        t0 = time.perf_counter()
        E.entropy_of_occupancy_grid(x, 28, True)
        print("reference entropy_of_occupancy_grid, %d x %d points, R 28, in_sphere: %.2f s on this CPU" % (S, P, time.perf_counter() - t0))
        return
    res = {"seed": np.int64(a.seed)}
    grids = []
    for R in RESOLUTIONS:
        for clip in (0, 1):
            g = E.unit_cube_grid_point_cloud(R, bool(clip))[0].reshape(-1, 3)
            assert g.dtype == np.float32
            res["grid_%d_%d" % (R, clip)] = g
            grids.append(g)
    margin = np.inf
    for kind in SETS:
        pcs, m, redrawn = make_set(rs, kind, grids)
        res["pcs_" + kind] = pcs
        margin = min(margin, m)
        norms = np.linalg.norm(pcs, axis=2)
        print("%-8s redrawn %d points, margin %.3e, max |coordinate| %.3f, max norm %.3f" % (kind, redrawn, m, np.abs(pcs).max(), norms.max()))
    assert np.linalg.norm(res["pcs_sphere"], axis=2).max() <= 0.5
    assert np.abs(res["pcs_cube"]).max() <= 0.5 and np.linalg.norm(res["pcs_cube"], axis=2).max() > 0.5
    assert np.abs(res["pcs_outside"]).max() > 0.5
    assert margin >= MARGIN
    res["min_margin"] = np.float64(margin)
    for kind in SETS:
        for R in RESOLUTIONS:
            for clip in (0, 1):
                del queries[:]
                ent, counters = E.entropy_of_occupancy_grid(res["pcs_" + kind], R, bool(clip))
                assert len(queries) == N_CLOUDS and counters.sum() == N_CLOUDS * POINTS
                bern = np.zeros(len(counters))
                for q in queries:
                    bern[np.unique(q)] += 1
                key = "%s_%d_%d" % (kind, R, clip)
                res["counters_" + key] = np.asarray(counters, np.float64)
                res["bernoulli_" + key] = bern
                res["entropy_" + key] = np.float64(ent)
    for i, ka in enumerate(SETS):
        for kb in SETS[i + 1:]:
            for R in RESOLUTIONS:
                res["jsd_%s_%s_%d" % (ka, kb, R)] = np.float64(E.jsd_between_point_cloud_sets(res["pcs_" + ka], res["pcs_" + kb], R))
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "golden_jsd.npz")
    np.savez_compressed(path, **res)
    print("wrote %s (%d bytes): min margin %.3e" % (path, os.path.getsize(path), margin))
    for k in sorted(res):
        if k.startswith(("entropy_", "jsd_")):
            print("  %-28s %.17g" % (k, float(res[k])))


if __name__ == "__main__":
    main()
