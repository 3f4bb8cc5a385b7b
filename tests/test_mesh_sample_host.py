"""CPU: the restatement of the mesh-sampling definition in tests/mesh_sample_cases.py -- that every bound tells the definition from
the nearest wrong arithmetics on the cases the GPU tests use, and that the generator behind it (counter layout, mulhi64 selection,
barycentric weights) draws what it should.  The statistical conditions are conditions on the generator at seed 0, not measurements."""
import numpy as np

import mesh_sample_cases as C

S_STAT = 65536


def _meshes():
    return {"ratio": C.ratio_mesh(), "random257": C.random_mesh(257), "random_degenerate": C.random_mesh(64, 40, seed=2, degenerate_every=3)}


def test_float32_areas_are_within_the_bound_of_float64():
    for name, (v, f) in _meshes().items():
        a32 = C.areas32(v, f)
        a64, e1e2 = C.areas64(v, f)
        err = np.abs(a32.astype(np.float64) - a64)
        print("%s: max area error / (e |e1| |e2|) %.3f, bound %.2f" % (name, (err[e1e2 > 0] / (C.E * e1e2[e1e2 > 0])).max(), C.AREA_C))
        assert (err <= C.area_bound(e1e2)).all()


def test_ratio_mesh_is_what_it_says():
    v, f = C.ratio_mesh()
    a, _ = C.areas64(v, f)
    live = np.delete(a, 4)
    assert a[4] == 0 and C.areas32(v, f)[4] == 0
    assert np.allclose(live / live[0], np.arange(1, 9), rtol=1e-6)
    q = C.quantise(C.areas32(v, f))
    assert q[4] == 0 and q[8] == 2 ** 32 and all(x > 0 for k, x in enumerate(q) if k != 4)


def test_point_bound_excludes_the_wrong_weights():
    for name, (v, f) in _meshes().items():
        good = C.sample(v, f, 2048)
        bound = C.point_bound(good["M"])
        for wrong in C.WRONG_POINT:
            off = np.abs(C.sample(v, f, 2048, wrong=wrong)["points"] - good["points"]).max(axis=1)
            frac = float((off > 1000 * bound).mean())
            print("%s / %s: %.3f of the samples move by more than 1000 bounds, median %.2e bounds" % (name, wrong, frac, np.median(off / bound)))
            assert frac > 0.9, (name, wrong)


def test_normal_bound_excludes_the_flipped_cross_product():
    for name, (v, f) in _meshes().items():
        good, bad = C.sample(v, f, 2048), C.sample(v, f, 2048, wrong="flipped")
        bound = C.face_normal_bound(good["e1e2"], good["nlen"])
        assert np.isfinite(bound).all() and bound.max() < 1e-3, (name, bound.max())
        off = np.abs(bad["normals_face"] - good["normals_face"]).max(axis=1)
        assert (off > 1000 * bound).all() and np.allclose(bad["normals_face"], -good["normals_face"])


def test_selection_differs_under_the_wrong_search_and_the_wrong_prefix():
    v, f = C.ratio_mesh()
    q = C.quantise(C.areas32(v, f))
    cdf, total = C.cdf_of(q)
    # draws whose t is exactly cdf[k] - 1 and cdf[k]: r = ceil(t 2^64 / total) gives mulhi64(r, total) = t
    words = []
    for k in (0, 2, 3, 4, 7):
        for t in (cdf[k] - 1, cdf[k]):
            if t < total:
                r = -((-t << 64) // total)
                assert (r * total) >> 64 == t and r < 2 ** 64
                words.append([r >> 32, r & 0xFFFFFFFF, 0x80000000, 0x40000000])
    words = np.array(words, np.uint64)
    good = C.select(words, cdf, total)
    assert list(good) == [0, 1, 2, 3, 3, 5, 3, 5, 7, 8]  # (t = cdf[3] and cdf[4], equal, both step over the zero-area row 4)
    lower = C.select(words, cdf, total, wrong="lower_bound")
    print("upper bound", list(good), "lower bound", list(lower))
    assert (lower[1::2] != good[1::2]).all() and np.array_equal(lower[0::2], good[0::2]) and not (good == 4).any()  # every t = cdf[k]
    ex_cdf, _ = C.cdf_of(q, exclusive=True)
    rnd = C.philox_words(2048, 0, 0, 0)
    g, x = C.select(rnd, cdf, total), C.select(rnd, ex_cdf, total)
    print("exclusive prefix: %d of 2048 random draws change their face" % int((g != x).sum()))
    assert (g != x).all()  # (no q but row 4's is 0, so the exclusive table shifts every draw)
    # across the zero-area run of the degenerate random mesh too
    v, f = C.random_mesh(64, 40, seed=2, degenerate_every=3)
    q = C.quantise(C.areas32(v, f))
    cdf, total = C.cdf_of(q)
    rnd = C.philox_words(4096, 0, 5, 1)
    g = C.select(rnd, cdf, total)
    assert all(q[k] > 0 for k in g) and set(g) == {k for k in range(64) if q[k] > 0}


def test_generator_statistics_at_seed_0():
    """Pearson's chi^2 of the face counts against q / total below the 0.999 quantile of chi^2(7); the zero-area face is never drawn;
    the mean of the points on the largest face within 4 standard errors of its centroid, per coordinate"""
    v, f = C.ratio_mesh()
    out = C.sample(v, f, S_STAT, seed=0)
    q = C.quantise(C.areas32(v, f))
    total = sum(q)
    counts = np.bincount(out["face"], minlength=9)
    assert counts[4] == 0 and counts.sum() == S_STAT
    live = [k for k in range(9) if k != 4]
    expect = np.array([q[k] / total for k in live]) * S_STAT
    chi2 = float((((counts[live] - expect) ** 2) / expect).sum())
    print("counts %s, expected %s, chi^2 %.2f (limit %.2f)" % (counts.tolist(), np.round(expect, 1).tolist(), chi2, C.CHI2_7_0999))
    assert chi2 < C.CHI2_7_0999
    pts = out["points"][out["face"] == 8]
    a, b, c = (v[f[8, k]].astype(np.float64) for k in range(3))
    se = np.sqrt(C.triangle_variance(a, b, c) / len(pts))
    dev = np.abs(pts.mean(axis=0) - (a + b + c) / 3) / se
    print("largest face: %d points, |mean - centroid| / standard error %s" % (len(pts), np.round(dev, 2).tolist()))
    assert (se > 0).all() and (dev < 4).all()
    # the weights are barycentric: non-negative and summing to 1
    w = out["weights"]
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1).max() < 1e-15


def test_streams_ids_and_seeds_are_different_draws():
    base = C.philox_words(64, 7, 3, 0)
    for other in (C.philox_words(64, 8, 3, 0), C.philox_words(64, 7, 4, 0), C.philox_words(64, 7, 3, 1), C.philox_words(64, 7 + (1 << 32), 3, 0)):
        assert (other != base).any(axis=1).all()
    assert np.array_equal(C.philox_words(64, 7, 3, 0)[:16], C.philox_words(16, 7, 3, 0))
