"""GPU: the all-pairs Chamfer kernel (slide_amd/csrc/chamfer_pairwise.hip through _ext.chamfer_pairwise) and
metrics_point_cloud.generation_metrics on it -- every entry bit-equal to the per-pair path chamfer_reduce(chamfer_nn(x[i], y[j])),
within 8 eps of a float64 brute force, independent of where a pair sits in the matrix and of the symmetric form; MMD / COV / 1-NNA
against the reference's results recorded in tests/golden/golden_generation_metrics.npz; scope errors and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

sys.path.insert(0, os.path.join(REPO, "pointnet2"))
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
KEYS = ("lgan_mmd-CD", "lgan_cov-CD", "lgan_mmd_smp-CD", "1-NN-CD-acc_t", "1-NN-CD-acc_f", "1-NN-CD-acc")


def _cloud(rs, B, P, grid=False, C=3):
    if grid:  # the 0.25 grid of test_hip_chamfer.py: duplicate points and exactly equidistant neighbours
        return (rs.randint(0, 4, (B, P, C)) * 0.25).astype(np.float32)
    return rs.standard_normal((B, P, C)).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _per_pair(xt, yt, pairs):
    """columns 0-1 of chamfer_reduce(chamfer_nn(x[i], y[j])) for the listed pairs, batched (a pair's numbers do not depend on its
    batch: test_hip_chamfer.py) -> (len(pairs), 2, 2)"""
    from slide_amd import _ext
    out = []
    for s in range(0, len(pairs), 64):
        ii = torch.tensor([p[0] for p in pairs[s:s + 64]], device=xt.device)
        jj = torch.tensor([p[1] for p in pairs[s:s + 64]], device=xt.device)
        d1, i1, d2, i2 = _ext.chamfer_nn(xt[ii].contiguous(), yt[jj].contiguous())
        out.append(_ext.chamfer_reduce(d1, None, d2, None)[:, :, :2])
    return torch.cat(out)


def _brute(x, y):
    """float64 directed sums (sum d, sum sqrt d) x -> y and y -> x of one pair, xyz only"""
    x, y = x.astype(np.float64), y.astype(np.float64)
    D = sum((x[:, None, c] - y[None, :, c]) ** 2 for c in range(3))
    a, b = D.min(1), D.min(0)
    return np.array([[a.sum(), np.sqrt(a).sum()], [b.sum(), np.sqrt(b).sum()]])


@pytest.mark.parametrize("M,N,P,Q", [(1, 1, 1, 1), (3, 5, 17, 1), (4, 3, 2047, 2049), (2, 2, 8192, 2048), (40, 24, 512, 300),
                                     (2, 3, 1500, 513)])
@pytest.mark.parametrize("kind", ["gauss", "grid", "gauss6"])
def test_pairwise_bit_equal_to_the_per_pair_path_and_close_to_float64(gpu_device, M, N, P, Q, kind):
    from slide_amd import _ext
    rs = np.random.RandomState(M * 7919 + N * 131 + P * 31 + Q)
    C = 6 if kind == "gauss6" else 3
    x, y = _cloud(rs, M, P, kind == "grid", C), _cloud(rs, N, Q, kind == "grid", C)
    if kind != "grid" and M > 1 and N > 1 and P == Q:
        y[-1] = x[0]  # an exact zero off the diagonal
    xt, yt = torch.from_numpy(x).to(gpu_device), torch.from_numpy(y).to(gpu_device)
    out = _ext.chamfer_pairwise(xt, yt)
    assert out.shape == (M, N, 2, 2) and out.dtype == torch.float32
    if M * N <= 64:
        pairs = [(i, j) for i in range(M) for j in range(N)]
    else:  # a fixed pseudo-random 64 pairs and the four corners (bounds the run time; position dependence is its own test)
        pairs = [(int(a), int(b)) for a, b in zip(rs.randint(0, M, 64), rs.randint(0, N, 64))]
        pairs += [(0, 0), (0, N - 1), (M - 1, 0), (M - 1, N - 1)]
    want = _per_pair(xt, yt, pairs)
    got = torch.stack([out[i, j] for i, j in pairs])
    assert torch.equal(_bits(got), _bits(want))
    # float64 brute force: each directed sum within 8 eps relative (a distance is within 4 eps -- test_hip_chamfer.py -- and so is
    # its square root; the sums run in double; one final rounding); zero distances are exactly zero
    o = out.cpu().numpy().astype(np.float64)
    for i, j in pairs[:12] + pairs[-4:]:
        ref = _brute(x[i], y[j])
        assert np.all(np.abs(o[i, j] - ref) <= 8 * EPS * ref), (i, j, o[i, j], ref)
        assert np.all(o[i, j][ref == 0] == 0)
    if kind != "grid" and M > 1 and N > 1 and P == Q:
        assert not out[0, N - 1].any()


def test_pairwise_does_not_depend_on_the_position_in_the_matrix(gpu_device):
    """slices that align with no blocking of the matrix over workgroups or XCDs"""
    from slide_amd import _ext
    rs = np.random.RandomState(5)
    x = torch.from_numpy(_cloud(rs, 19, 700)).to(gpu_device)
    y = torch.from_numpy(_cloud(rs, 21, 300)).to(gpu_device)
    full = _ext.chamfer_pairwise(x, y)
    for (a, b), (c, d) in (((3, 11), (5, 6)), ((5, 6), (3, 11)), ((0, 19), (20, 21)), ((18, 19), (0, 21)), ((1, 10), (9, 18))):
        part = _ext.chamfer_pairwise(x[a:b], y[c:d])
        assert torch.equal(_bits(part), _bits(full[a:b, c:d]))
    fs = _ext.chamfer_pairwise(x)
    for a, b in ((3, 11), (5, 6), (10, 19)):
        assert torch.equal(_bits(_ext.chamfer_pairwise(x[a:b])), _bits(fs[a:b, a:b]))


@pytest.mark.parametrize("M,P,grid", [(1, 5, False), (13, 300, False), (9, 2048, False), (11, 257, True)])
def test_pairwise_symmetric_form(gpu_device, M, P, grid):
    import metrics_point_cloud.generation_metrics as G
    from slide_amd import _ext
    rs = np.random.RandomState(M + P)
    x = torch.from_numpy(_cloud(rs, M, P, grid)).to(gpu_device)
    sym = _ext.chamfer_pairwise(x)
    gen = _ext.chamfer_pairwise(x, x.clone())
    assert torch.equal(_bits(sym), _bits(gen))
    assert torch.equal(_bits(sym.transpose(0, 1).flip(2)), _bits(sym))  # out[j, i, d] == out[i, j, 1 - d]
    assert not sym[torch.arange(M), torch.arange(M)].any()  # the diagonal is exactly zero
    cd = G.pairwise_cd(x)
    assert cd.shape == (M, M) and cd.dtype == torch.float32
    assert torch.equal(_bits(cd), _bits(cd.t()))
    assert torch.equal(_bits(cd), _bits(G.pairwise_cd(x, x.clone())))


def test_pairwise_cd_is_calc_cd_for_every_pair(gpu_device):
    """the matrix entry is calc_cd's cd_t of that pair, bitwise (6-channel inputs: xyz read in place through the stride)"""
    import metrics_point_cloud.generation_metrics as G
    from metrics_point_cloud.chamfer_and_f1 import calc_cd
    rs = np.random.RandomState(11)
    x = torch.from_numpy(_cloud(rs, 5, 640, C=6)).to(gpu_device)
    y = torch.from_numpy(_cloud(rs, 4, 200, C=6)).to(gpu_device)
    cd = G.pairwise_cd(x, y, batch_size=3)
    for i in range(5):
        # calc_cd(output, gt): direction 0 runs over gt's points
        want = calc_cd(y[:, :, :3].contiguous(), x[i:i + 1, :, :3].expand(4, -1, -1).contiguous())["cd_t"]
        assert torch.equal(_bits(cd[i]), _bits(want))


def _close(got, want):
    """8 eps relative; the recorded float64 numbers come from the reference's |a|^2 + |b|^2 - 2 a.b expansion, whose own
    cancellation error (a few 1e-16 x |a|^2, |a|^2 < 100 here) is far below the 1e-12 allowed for it"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.all(np.abs(got - want) <= 8 * EPS * np.abs(want) + 1e-12)


def test_compute_all_metrics_matches_the_reference_fixture(gpu_device):
    import metrics_point_cloud.generation_metrics as G
    g = load_golden("golden_generation_metrics.npz")
    s = torch.from_numpy(g["samples"]).to(gpu_device)
    r = torch.from_numpy(g["refs"]).to(gpu_device)
    M_rs, M_rr, M_ss = G.all_pairs_matrices(s, r)
    for got, key in ((M_rs, "M_rs"), (M_rr, "M_rr"), (M_ss, "M_ss")):
        assert got.dtype == torch.float32 and got.shape == g[key].shape
        assert _close(got.cpu().numpy(), g[key]), key
    cs, cr = (int(v) for v in g["copy_smp_ref"])
    assert float(M_rs[cr, cs]) == 0.0 and not M_rr.diagonal().any() and not M_ss.diagonal().any()  # exact zeros
    res = G.compute_all_metrics(s, r, batch_size=100)
    assert sorted(res) == sorted(KEYS)
    for v in res.values():
        assert v.dim() == 0 and v.is_cuda
    assert _close(float(res["lgan_mmd-CD"]), float(g["mmd_cov_lgan_mmd"]))
    assert _close(float(res["lgan_mmd_smp-CD"]), float(g["mmd_cov_lgan_mmd_smp"]))
    # ratios of integers, and the fixture separates every deciding minimum by > 1e-4: equal to the reference's values
    # (its coverage is a float32 ratio, its accuracies float64 ratios with 1e-10 in the denominator: rounded to float32 here)
    assert float(res["lgan_cov-CD"]) == float(g["mmd_cov_lgan_cov"])
    for k in ("acc_t", "acc_f", "acc"):
        assert float(res["1-NN-CD-" + k]) == float(np.float32(g["knn_" + k])), k
    one = G.knn(M_rr, M_rs, M_ss, 1)
    for k in ("tp", "fp", "fn", "tn"):
        assert float(one[k]) == float(g["knn_" + k]), k


def test_scope_errors(gpu_device):
    import metrics_point_cloud.generation_metrics as G
    from slide_amd import _ext
    x = torch.randn(3, 16, 3, device=gpu_device)
    with pytest.raises(RuntimeError):
        G.pairwise_cd(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError):
        G.pairwise_cd(x, x.cpu())
    with pytest.raises(RuntimeError):
        G.compute_all_metrics(x.cpu(), x)
    with pytest.raises(NotImplementedError):
        G.pairwise_cd(x.clone().requires_grad_(True), x)
    with pytest.raises(NotImplementedError):
        G.pairwise_cd(x, x.clone().requires_grad_(True))
    with torch.no_grad():
        G.pairwise_cd(x.clone().requires_grad_(True), x)  # forward only is fine where no graph is recorded
    with pytest.raises(ValueError):
        G.pairwise_cd(x[0], x)
    with pytest.raises(ValueError):
        G.pairwise_cd(x, x[:, :, :2])
    with pytest.raises(ValueError):
        G.pairwise_cd(x[:, :0], x)
    with pytest.raises(RuntimeError):
        _ext.chamfer_pairwise(x.double(), x)
    assert _ext.chamfer_pairwise(x[:0], x).shape == (0, 3, 2, 2)


def test_cli_end_to_end(gpu_device, tmp_path):
    """generation_evaluate.py in a fresh child process on two npz files: the JSON holds the six keys and the numbers of a direct
    compute_all_metrics call on the same (normalised) sets"""
    import metrics_point_cloud.generation_metrics as G
    from load_evaluate import normalize_point_cloud
    rs = np.random.RandomState(3)
    a = (rs.standard_normal((14, 200, 3)) * rs.uniform(0.5, 2.0, (14, 1, 3))).astype(np.float32)
    b = (rs.standard_normal((10, 160, 3)) * rs.uniform(0.5, 2.0, (10, 1, 3)) + 0.1).astype(np.float32)
    pa, pb, pj = str(tmp_path / "a.npz"), str(tmp_path / "b.npz"), str(tmp_path / "m.json")
    np.savez(pa, points=a)
    np.savez(pb, points=b)
    for extra, norm in (([], False), (["--normalize"], True)):
        r = subprocess.run([sys.executable, os.path.join(REPO, "pointnet2", "generation_evaluate.py"), "--samples", pa, "--ref", pb,
                            "--save", pj] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        got = json.load(open(pj))
        assert sorted(got) == sorted(KEYS)
        sa, sb = (normalize_point_cloud(a), normalize_point_cloud(b)) if norm else (a, b)
        want = G.compute_all_metrics(torch.from_numpy(np.ascontiguousarray(sa, dtype=np.float32)).to(gpu_device),
                                     torch.from_numpy(np.ascontiguousarray(sb, dtype=np.float32)).to(gpu_device))
        for k in KEYS:
            assert got[k] == float(want[k]), (k, got[k], float(want[k]))
            assert k in r.stdout
        assert "wall time" in r.stdout
