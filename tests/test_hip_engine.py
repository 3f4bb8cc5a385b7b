"""GPU parity: the fused denoiser engine + graph-captured samplers (C-ABI, HIP) vs golden vectors produced by the
REFERENCE's Python and vs the numpy oracle.  Tolerances: fp32-MFMA mode 1e-3 relative (north_star), asserted much
tighter; fp16-MFMA mode reported and bounded."""
import json

import numpy as np
import pytest
import torch

from conftest import NoiseStream, golden_spec, load_golden
from slide_amd import abi
from slide_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu


def _load(name):
    g = load_golden("golden_denoiser_%s.npz" % name)
    return g, json.loads(str(g["config_json"])), synth_state_dict(golden_spec(g))


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


@pytest.mark.parametrize("prec", ["fp32", "split"])
@pytest.mark.parametrize("name", ["pos", "feat"])
def test_denoiser_forward_fp32_matches_reference(gpu_device, name, prec):
    """the two fp32-grade modes against the reference goldens: "fp32" = fp32 MFMA; "split" (round 4) = the same plan with its
    contractions as two-term fp16 operand splits on the fp16 matrix pipe (include/slide_engine.h: SLIDE_PREC_SPLIT)"""
    from slide_amd.engine import DenoiserEngine
    g, hp, sd = _load(name)
    B = g["x_t0"].shape[0]
    eng = DenoiserEngine(hp, sd, B, gpu_device, prec=prec)
    for k in ["t0", "t1", "t500", "t999", "mixed"]:
        y = eng.forward(g["x_" + k], g["ts_" + k], g["label_" + k]).cpu().numpy()
        assert np.isfinite(y).all(), k
        assert _rel(y, g["eps_" + k]) <= 2e-4, (k, _rel(y, g["eps_" + k]))


@pytest.mark.parametrize("name,prec", [("pos", "split"), ("feat", "fp16")])
def test_benched_arithmetic_meets_1e3_on_reference_goldens(gpu_device, name, prec):
    """north_star / BASELINE.md section 4: generated latents within 1e-3 (relative, fp32).  `bench.py`'s default arrangement
    (round 5) runs the POSITION plan in the split arithmetic (fp32-grade) and the FEATURE plan in fp16 operands / fp32
    accumulation: every single forward of both against the reference goldens, <= 1e-3 in the relative L2 norm AND in the max-norm
    (max |difference| / max |reference|).  Round 6: no exemption for the fp16 feature plan -- the end of the network (FP0's second Mlp
    + the head, SLIDE_OP_POINT_CHAIN) runs in the split arithmetic; round 5 measured 8.7e-4 / 1.2e-3 with fp16 operands there."""
    from slide_amd.engine import DenoiserEngine
    g, hp, sd = _load(name)
    B = g["x_t0"].shape[0]
    eng = DenoiserEngine(hp, sd, B, gpu_device, prec=prec)
    worst = worst_max = 0.0
    for k in ["t0", "t1", "t500", "t999", "mixed"]:
        y = eng.forward(g["x_" + k], g["ts_" + k], g["label_" + k]).cpu().numpy()
        assert np.isfinite(y).all(), k
        ref = g["eps_" + k]
        worst = max(worst, float(np.linalg.norm(y - ref) / np.linalg.norm(ref)))
        worst_max = max(worst_max, _rel(y, ref))
    print("benched arithmetic (%s net, %s): relative L2 %.3e, max-norm %.3e vs reference" % (name, prec, worst, worst_max))
    assert worst <= 1e-3 and worst_max <= 1e-3, (worst, worst_max)


def test_optin_fp16_position_plan_is_bounded(gpu_device):
    """NOT the benched mode since round 5 (`bench.py --pos-prec fp16` / the CLIs' `--prec fp16` select it): the fp16 position
    plan's single forwards miss 1e-3 on the reference goldens (3.2e-3: every layer's operand rounding contributes and the error
    grows as the coordinates shrink).  Kept as an opt-in throughput plan; this test only bounds it."""
    from slide_amd.engine import DenoiserEngine
    g, hp, sd = _load("pos")
    B = g["x_t0"].shape[0]
    eng = DenoiserEngine(hp, sd, B, gpu_device, prec="fp16")
    worst = 0.0
    for k in ["t0", "t1", "t500", "t999", "mixed"]:
        y = eng.forward(g["x_" + k], g["ts_" + k], g["label_" + k]).cpu().numpy()
        assert np.isfinite(y).all(), k
        ref = g["eps_" + k]
        worst = max(worst, float(np.linalg.norm(y - ref) / np.linalg.norm(ref)))
    print("opt-in fp16 position plan, relative L2 error vs reference: %.3e" % worst)
    assert worst <= 4e-3, worst


_BENCHED_FEATURE_LAUNCH = {}  # B -> (oracle, fp32 engine, fp16 plan) outputs, shared by the two tests below


def _benched_feature_launch(gpu_device, B):
    if B not in _BENCHED_FEATURE_LAUNCH:
        from oracle import denoiser_np as D
        from slide_amd.engine import DenoiserEngine
        from slide_amd.synth import synth_keypoints
        g, hp, sd = _load("feat")
        rs = np.random.RandomState(B)
        x = rs.standard_normal((B, 16, 51)).astype(np.float32)
        x[:, :, :3] = synth_keypoints(B, seed=B)
        ts = rs.randint(0, 1000, B).astype(np.float32)
        label = rs.randint(0, 13, B).astype(np.int64)
        ref = np.concatenate([D.denoiser_forward(hp, sd, x[i:i + 32], ts[i:i + 32], label[i:i + 32]) for i in range(0, B, 32)])
        y32 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp32").forward(x, ts, label).cpu().numpy()
        y16 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp16").forward(x, ts, label).cpu().numpy()
        _BENCHED_FEATURE_LAUNCH[B] = (ref, y32, y16)
    return _BENCHED_FEATURE_LAUNCH[B]


@pytest.mark.parametrize("B", [88, 256])
def test_feature_denoiser_at_the_benched_launch_sizes_matches_oracle(gpu_device, B):
    """the goldens hold 2-3 samples; the benched launches hold 88 / 80 samples per feature sub-batch (and 256 in
    the single-chain arrangement) -- other tile maps, XCD groups, grid-size dependent kernel choices.  The exact-fp32 engine
    against the numpy oracle at those sizes (<= 2e-4 of the output's max, as at golden size), and the fp16 throughput plan
    against the same oracle output (<= 1e-3 relative L2, the single-forward criterion; its max-norm: the test below)."""
    ref, y32, y16 = _benched_feature_launch(gpu_device, B)
    assert np.isfinite(y32).all() and _rel(y32, ref) <= 2e-4, _rel(y32, ref)
    r16 = float(np.linalg.norm(y16 - ref) / np.linalg.norm(ref))
    per = np.linalg.norm((y16 - ref).reshape(B, -1), axis=1) / np.linalg.norm(ref.reshape(B, -1), axis=1)
    print("feature net, B = %d: fp32 engine vs oracle %.2e (max-norm); fp16 plan vs oracle %.2e relative L2 (per sample: median %.2e, "
          "max %.2e), max-norm %.2e" % (B, _rel(y32, ref), r16, np.median(per), per.max(), _rel(y16, ref)))
    assert np.isfinite(y16).all() and r16 <= 1e-3, r16


@pytest.mark.parametrize("B", [pytest.param(88, marks=pytest.mark.xfail(strict=True, reason=(
    "fp16 feature plan, max-norm vs the oracle at 88 samples: 1.46e-3 measured (relative L2 5.8e-4).  Form A, the same kernels "
    "as at 256 samples (7.4e-4), and every large-batch form computes the same samples bit for bit: the fp16 operand arithmetic, "
    "not a kernel -- single forwards meet 1e-3 in the L2 norm, not in the max-norm of every batch"))), 256])
def test_feature_fp16_plan_max_norm_at_the_benched_launch_sizes(gpu_device, B):
    """north_star's 1e-3 in the max-norm (max |difference| / max |oracle|) of the benched fp16 feature plan over a whole benched
    launch, as test_benched_arithmetic_meets_1e3_on_reference_goldens asserts it on the 2-3-sample goldens"""
    ref, _, y16 = _benched_feature_launch(gpu_device, B)
    print("feature net, B = %d: fp16 plan vs oracle max-norm %.2e" % (B, _rel(y16, ref)))
    assert _rel(y16, ref) <= 1e-3, _rel(y16, ref)


def test_position_denoiser_at_the_benched_launch_size_matches_oracle(gpu_device):
    """the position chain's launch size (256 samples): exact-fp32 engine vs the numpy oracle, <= 2e-4; the BENCHED position
    arithmetic (split, round 5) against the same output, <= 1e-3 relative L2, for two input families (chain start: N(0, 1);
    chain end: key-point-like coordinates -- where the opt-in fp16 plan is 1.5e-3 off)"""
    from oracle import denoiser_np as D
    from slide_amd.engine import DenoiserEngine
    from slide_amd.synth import synth_keypoints
    g, hp, sd = _load("pos")
    B = 256
    rs = np.random.RandomState(17)
    ts = rs.randint(0, 1000, B).astype(np.float32)
    label = rs.randint(0, 13, B).astype(np.int64)
    e32 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp32")
    e16 = DenoiserEngine(hp, sd, B, gpu_device, prec="split")
    for fam, x in (("normal", rs.standard_normal((B, 16, 3)).astype(np.float32)), ("keypoints", synth_keypoints(B, seed=3).astype(np.float32))):
        ref = D.denoiser_forward(hp, sd, x, ts, label)
        y32 = e32.forward(x, ts, label).cpu().numpy()
        assert np.isfinite(y32).all() and _rel(y32, ref) <= 2e-4, (fam, _rel(y32, ref))
        y16 = e16.forward(x, ts, label).cpu().numpy()
        r16 = float(np.linalg.norm(y16 - ref) / np.linalg.norm(ref))
        m16 = _rel(y16, ref)
        print("position net, B = 256, %s inputs: fp32 engine vs oracle %.2e; benched (split) plan vs oracle %.2e relative L2, %.2e max-norm"
              % (fam, _rel(y32, ref), r16, m16))
        assert np.isfinite(y16).all() and r16 <= 1e-3 and m16 <= 2e-4, (fam, r16, m16)


def test_denoiser_larger_batch_matches_oracle(gpu_device):
    """B=37 (ragged vs the 16-sample row tiles) and repeated calls (no state leaks between calls)."""
    from oracle import denoiser_np as D
    from slide_amd.engine import DenoiserEngine
    g, hp, sd = _load("pos")
    rs = np.random.RandomState(3)
    B = 37
    x = rs.standard_normal((B, 16, 3)).astype(np.float32)
    ts = rs.randint(0, 1000, B).astype(np.float32)
    label = rs.randint(0, 13, B).astype(np.int64)
    ref = D.denoiser_forward(hp, sd, x, ts, label)
    eng = DenoiserEngine(hp, sd, B, gpu_device, prec="fp32")
    y1 = eng.forward(x, ts, label).cpu().numpy()
    y2 = eng.forward(x, ts, label).cpu().numpy()
    assert np.array_equal(y1, y2)          # deterministic
    assert _rel(y1, ref) <= 2e-4, _rel(y1, ref)
    # batch independence: permuting the batch permutes the output
    perm = rs.permutation(B)
    y3 = eng.forward(x[perm], ts[perm], label[perm]).cpu().numpy()
    assert np.allclose(y3, y1[perm], rtol=0, atol=5e-6)  # same arithmetic per sample up to fp32 rounding


@pytest.mark.parametrize("name", ["pos", "feat"])
def test_ragged_batches_through_the_fp16_plan(gpu_device, name):
    """Batch sizes that leave row tiles and XCD groups partly empty (1, 5, 17, 100 samples: 16-row GEMM tiles of 64 rows,
    256-row tiles of one or two samples, eight-tile XCD groups) through the default fp16 plan -- pair tables, generated-X
    GEMMs, fused chains, dual launch -- against the exact fp32 engine at the same batch.  Feature net (the benched fp16 plan):
    north_star's 1e-3 in the relative L2 norm and the max-norm (measured <= 4.9e-4 / 7.4e-4).  Position net: the opt-in fp16 plan
    (not benched; its single forwards miss 1e-3, test_optin_fp16_position_plan_is_bounded): <= 2e-3 / 4e-3 (measured 1.0e-3 /
    1.4e-3 at one sample)."""
    from slide_amd.engine import DenoiserEngine
    g, hp, sd = _load(name)
    rs = np.random.RandomState(4)
    C = g["x_t0"].shape[2]
    tol_l2, tol_max = (1e-3, 1e-3) if name == "feat" else (2e-3, 4e-3)
    for B in (1, 5, 17, 100):
        x = rs.standard_normal((B, 16, C)).astype(np.float32)
        ts = rs.randint(0, 1000, B).astype(np.float32)
        label = rs.randint(0, 13, B).astype(np.int64)
        y16 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp16").forward(x, ts, label).cpu().numpy()
        y32 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp32").forward(x, ts, label).cpu().numpy()
        rel = float(np.linalg.norm(y16 - y32) / np.linalg.norm(y32))
        print("%s net, fp16 plan vs fp32 engine, B = %d: relative L2 %.2e, max-norm %.2e" % (name, B, rel, _rel(y16, y32)))
        assert np.isfinite(y16).all() and rel <= tol_l2 and _rel(y16, y32) <= tol_max, (B, rel, _rel(y16, y32))


@pytest.mark.parametrize("name", ["pos", "feat"])
def test_full_size_properties(gpu_device, name):
    """BASELINE batch (256 per GPU, and the 128-sample sub-batches the bench replays): size-independent properties.
    (1) fp16 throughput mode vs fp32 parity mode of the same engine: feature net (benched) <= 1e-3 relative L2 and max-norm
        (measured 4.7e-4 / 7.0e-4); position net (opt-in fp16 plan) <= 2e-3 / 4e-3 (measured 1.1e-3 / 2.6e-3);
    (2) sample independence at full size: a sample's output does not depend on where in the batch it sits, nor on the
        batch size it is launched with (256 vs 128: the same plan form, other grids and tile occupancy) -- bit for bit
        (the batch sizes that change the kernels: test_feature_plan_forms_agree_on_the_same_samples);
    (3) determinism of repeated launches."""
    from slide_amd.engine import DenoiserEngine
    g, hp, sd = _load(name)
    rs = np.random.RandomState(11)
    B, C = 256, g["x_t0"].shape[2]
    x = rs.standard_normal((B, 16, C)).astype(np.float32)
    ts = rs.randint(0, 1000, B).astype(np.float32)
    label = rs.randint(0, 13, B).astype(np.int64)
    e16 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp16")
    y16 = e16.forward(x, ts, label).cpu().numpy()
    assert np.isfinite(y16).all()
    assert np.array_equal(y16, e16.forward(x, ts, label).cpu().numpy())
    e32 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp32")
    y32 = e32.forward(x, ts, label).cpu().numpy()
    rel = float(np.linalg.norm(y16 - y32) / np.linalg.norm(y32))
    perm = rs.permutation(B)
    yp = e16.forward(x[perm], ts[perm], label[perm]).cpu().numpy()
    eh = DenoiserEngine(hp, sd, 128, gpu_device, prec="fp16")
    yh = eh.forward(x[:128], ts[:128], label[:128]).cpu().numpy()
    print("%s net, B = 256: fp16 vs fp32 relative L2 %.2e, max-norm %.2e; permuted: equal %s (%.2e); 128 vs 256: equal %s (%.2e)"
          % (name, rel, _rel(y16, y32), np.array_equal(yp, y16[perm]), _rel(yp, y16[perm]), np.array_equal(yh, y16[:128]),
             _rel(yh, y16[:128])))
    tol_l2, tol_max = (1e-3, 1e-3) if name == "feat" else (2e-3, 4e-3)
    assert rel <= tol_l2 and _rel(y16, y32) <= tol_max, (rel, _rel(y16, y32))
    # per-sample arithmetic is identical wherever the sample sits (GroupNorm statistics are per sample)
    assert np.array_equal(yp, y16[perm]), _rel(yp, y16[perm])
    assert np.array_equal(yh, y16[:128]), _rel(yh, y16[:128])


def _oracle_subset(B, seed=0):
    """the samples of a batch of B that the host oracle evaluates: the first 8 and the last 8 (the part-filled last tile), the
    first sample of each eighth of the batch (XCD group boundaries) and 24 seeded random others"""
    pick = set(range(min(8, B))) | set(range(max(0, B - 8), B)) | {(k * B) // 8 for k in range(8)}
    rs = np.random.RandomState(1000 + B + seed)
    return np.array(sorted(pick | set([int(i) for i in rs.permutation(B) if int(i) not in pick][:24])))


def _oracle_rows(hp, sd, x, ts, label, idx):
    """oracle/denoiser_np.py on the samples idx only: the network is per sample (GroupNorm statistics are per sample)"""
    from oracle import denoiser_np as D
    return np.concatenate([D.denoiser_forward(hp, sd, x[idx[i:i + 16]], ts[idx[i:i + 16]], label[idx[i:i + 16]])
                           for i in range(0, len(idx), 16)])


def _per_sample_max(y, ref):
    """max |difference| / max |reference| of every sample"""
    n = y.shape[0]
    return np.abs(y - ref).reshape(n, -1).max(axis=1) / np.abs(ref).reshape(n, -1).max(axis=1)


def _inputs(B, cx, seed, family="normal"):
    """x ~ N(0, 1) with the key-point channels from synth_keypoints (family "keypoints": the coordinates alone are key points),
    timesteps over [0, 1000), random labels"""
    from slide_amd.synth import synth_keypoints
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, 16, cx)).astype(np.float32)
    if family == "keypoints" or cx > 3:
        x[:, :, :3] = synth_keypoints(B, seed=seed)
    return x, rs.randint(0, 1000, B).astype(np.float32), rs.randint(0, 13, B).astype(np.int64)


# fp16 feature plan, batch sizes of forms B - F (tests/plan_forms.py): both sides of the 64- / 128-channel tile switch, the three
# feature sub-batch sizes of `bench.py --batch 1024 / 2048 / 4096` (344; 688; 1365 and 1364 share form D / E with 1025 / 1365),
# the first size with a separate finalise launch per threshold
FORM_SIZES = [257, 344, 513, 688, 1025, 1365, 2049]


@pytest.mark.parametrize("B", FORM_SIZES)
def test_every_feature_plan_form_matches_oracle(gpu_device, B):
    """The fp16 feature plan's kernels depend on the batch size (tests/plan_forms.py); the default selections otherwise never build
    it above 256 samples.  At a representative size of every large-batch form, on the oracle subset (_oracle_subset): the
    exact-fp32 engine within 2e-4 of the oracle in the max-norm of EVERY sample, and the fp16 plan within north_star's 1e-3 in the
    relative L2 norm and in the max-norm over the subset."""
    from plan_forms import expected_feature_fp16_signature, feature_fp16_form, form_signature
    from slide_amd.engine import DenoiserEngine
    _, hp, sd = _load("feat")
    x, ts, lab = _inputs(B, 51, seed=B)
    e16 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp16")
    assert form_signature(e16) == expected_feature_fp16_signature(B), (B, form_signature(e16))
    idx = _oracle_subset(B)
    ref = _oracle_rows(hp, sd, x, ts, lab, idx)
    y16 = e16.forward(x, ts, lab).cpu().numpy()
    del e16
    y32 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp32").forward(x, ts, lab).cpu().numpy()
    assert np.isfinite(y16).all() and np.isfinite(y32).all()
    p32 = _per_sample_max(y32[idx], ref)
    p16 = _per_sample_max(y16[idx], ref)
    l2 = float(np.linalg.norm(y16[idx] - ref) / np.linalg.norm(ref))
    mx = _rel(y16[idx], ref)
    print("feature net, form %s, B = %d (%d samples vs oracle): fp32 engine per-sample max-norm median %.2e, max %.2e; "
          "fp16 plan relative L2 %.2e, max-norm %.2e (per sample: median %.2e, max %.2e at sample %d)"
          % (feature_fp16_form(B), B, len(idx), np.median(p32), p32.max(), l2, mx, np.median(p16), p16.max(), idx[p16.argmax()]))
    assert p32.max() <= 2e-4, (B, p32.max(), idx[p32.argmax()])
    assert l2 <= 1e-3 and mx <= 1e-3, (B, l2, mx)


def test_feature_plan_forms_agree_on_the_same_samples(gpu_device):
    """The same 48 samples inside batches of every fp16 feature plan form (256: form A; FORM_SIZES: forms B - F), at different
    positions among seeded other samples.  The forms differ in launch fusion (dual launch, query GEMM riding on the SA chain, the
    GroupNorm finalisation inside the 16-row GEMM or as its own launch) and in the width of the generated-X tiles, never in the
    arithmetic of a sample: every sample's output is the same bits in every form.  (Before the two GroupNorm finalisations were
    compiled without FMA contraction, 4 of these 48 samples differed by up to 7.0e-4 between the fused and the separate one.)"""
    from plan_forms import feature_fp16_form
    from slide_amd.engine import DenoiserEngine
    _, hp, sd = _load("feat")
    n = 48
    xs, tss, labs = _inputs(n, 51, seed=4242)
    outs = {}
    for B in [256] + FORM_SIZES:
        x, ts, lab = _inputs(B, 51, seed=5000 + B)
        pos = np.sort(np.random.RandomState(B).choice(B, n, replace=False))
        pos[0], pos[-1] = 0, B - 1  # the first tile and the part-filled last one
        perm = np.random.RandomState(B + 1).permutation(n)
        x[pos], ts[pos], lab[pos] = xs[perm], tss[perm], labs[perm]
        y = DenoiserEngine(hp, sd, B, gpu_device, prec="fp16").forward(x, ts, lab).cpu().numpy()
        assert np.isfinite(y).all()
        out = np.empty((n,) + y.shape[1:], y.dtype)
        out[perm] = y[pos]
        outs[B] = out
    a = outs[256]
    diffs = {}
    for B in FORM_SIZES:
        d = _per_sample_max(outs[B], a)
        diffs[B] = (bool(np.array_equal(outs[B], a)), float(d.max()))
        print("form %s (B = %d) vs form A (B = 256), 48 samples: bit-identical %s, per-sample max-norm max %.2e, median %.2e"
              % (feature_fp16_form(B), B, diffs[B][0], d.max(), np.median(d)))
    for B in FORM_SIZES:
        assert diffs[B][0], (B, diffs[B])


@pytest.mark.parametrize("B", [512, 4096])
def test_position_split_plan_at_and_above_the_benched_launch_size(gpu_device, B):
    """The benched position chain runs the split plan at 512 samples per launch (`pos_batch_multiple: 2`); 4096 covers `--batch
    4096`'s sub-batches and beyond.  The split plan is one form at every size (tests/plan_forms.py), fp32-grade: on the oracle
    subset -- plus the sample where the split plan and the exact-fp32 engine differ most -- <= 2e-4 in every sample's max-norm
    (measured <= 1.4e-5), and within 2e-5 (max-norm) of the exact-fp32 engine at the same batch for both input families (chain
    start N(0, 1); chain end key-point-like coordinates) at 512 (measured 7.7e-6); 4096 key-point-like samples reach 2.6e-5
    (two fp32-grade summation orders, the worst of 4096 samples; both engines stay within 1.3e-5 of the oracle on the
    subset): 5e-5 there."""
    from slide_amd.engine import DenoiserEngine
    _, hp, sd = _load("pos")
    e32 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp32")
    esp = DenoiserEngine(hp, sd, B, gpu_device, prec="split")
    for fam in ("normal", "keypoints"):
        x, ts, lab = _inputs(B, 3, seed=B + 7, family=fam)
        y32 = e32.forward(x, ts, lab).cpu().numpy()
        ysp = esp.forward(x, ts, lab).cpu().numpy()
        assert np.isfinite(y32).all() and np.isfinite(ysp).all()
        worst = int(np.abs(ysp - y32).reshape(B, -1).max(axis=1).argmax())
        idx = np.union1d(_oracle_subset(B), [worst])
        ref = _oracle_rows(hp, sd, x, ts, lab, idx)
        psp = _per_sample_max(ysp[idx], ref)
        p32 = _per_sample_max(y32[idx], ref)
        vs32 = _rel(ysp, y32)
        print("position net, B = %d, %s inputs: split plan vs oracle per-sample max-norm median %.2e, max %.2e (fp32 engine %.2e); "
              "split vs fp32 engine %.2e (sample %d)" % (B, fam, np.median(psp), psp.max(), p32.max(), vs32, worst))
        assert psp.max() <= 2e-4 and p32.max() <= 2e-4, (fam, psp.max(), p32.max())
        assert vs32 <= (2e-5 if B <= 512 else 5e-5), (fam, vs32)


def _pos_cfg():
    return {"T": 1000, "beta_0": 0.0001, "beta_T": 0.02}


@pytest.mark.parametrize("use_graph", [False, True])
def test_position_sampler_tail_matches_reference(gpu_device, use_graph):
    from slide_amd.diffusion import PositionSampler, calc_diffusion_hyperparams
    g = load_golden("golden_sampler_pos.npz")
    _, hp, sd = _load("pos")
    dh = calc_diffusion_hyperparams(**_pos_cfg())
    for k in ["Beta", "Alpha", "Alpha_bar"]:
        assert np.array_equal(dh[k], g["sched_" + k])
    ns = NoiseStream(g["tail_seed"])
    size = g["tail_XT"].shape
    ns(size)
    step = int(g["tail_step"])
    x = g["tail_XT"] + dh["Sigma"][step] * ns(size)
    noise = np.stack([ns(size) for _ in range(step - 1)])
    smp = PositionSampler(hp, sd, size[0], gpu_device, _pos_cfg(), prec="fp32", noise=noise, use_graph=use_graph)
    x0 = smp.sample(g["label"], x, t_start=step - 1).cpu().numpy()
    assert _rel(x0, g["tail_x0"]) <= 1e-3, _rel(x0, g["tail_x0"])


FP16_TAIL = {}  # measured errors of the fp16 throughput mode over the golden 20-step segments (printed; asserted below)


def test_position_sampler_tail_fp16(gpu_device):
    """the bench's precision (fp16 operands / activation storage, fp32 accumulate) over the golden 20-step tail with the
    reference's injected noise.  One fp16 forward of eps is 1e-3 .. 4e-3 off, but the update scales eps by
    (1 - alpha_t) / sqrt(1 - alpha_bar_t): over the last 20 steps the STATE stays within BASELINE's 1e-3 of the reference
    (measured 1.7e-4) -- asserted.  Complete 1000-step chains: test_position_sampler_full_chain_fp16_matches_reference and
    test_feature_sampler_full_chain_matches_reference (both <= 1e-3 vs the reference's goldens; the reverse process contracts
    the per-step error, and no near-tie of a per-step kNN flipped on the golden chains)."""
    from slide_amd.diffusion import PositionSampler, calc_diffusion_hyperparams
    g = load_golden("golden_sampler_pos.npz")
    _, hp, sd = _load("pos")
    dh = calc_diffusion_hyperparams(**_pos_cfg())
    ns = NoiseStream(g["tail_seed"])
    size = g["tail_XT"].shape
    ns(size)
    step = int(g["tail_step"])
    x = g["tail_XT"] + dh["Sigma"][step] * ns(size)
    noise = np.stack([ns(size) for _ in range(step - 1)])
    smp = PositionSampler(hp, sd, size[0], gpu_device, _pos_cfg(), prec="fp16", noise=noise, use_graph=False)
    x0 = smp.sample(g["label"], x, t_start=step - 1).cpu().numpy()
    r = _rel(x0, g["tail_x0"])
    print("fp16 position sampler, 20-step tail: relative max error vs reference %.3e" % r)
    assert np.isfinite(x0).all() and r <= 1e-3, r


def test_feature_sampler_fp16(gpu_device):
    """fp16 throughput mode over the golden 20-step head (t = 999 .. 980) and tail (t = 19 .. 0) of
    denoise_and_reconstruct with the reference's injected noise; key points are a fixed condition, so no neighbour flips:
    measured 9e-5 / 8e-5, asserted <= 1e-3 (BASELINE's tolerance)"""
    from slide_amd.diffusion import FeatureSampler
    g = load_golden("golden_sampler_feat.npz")
    _, hp, sd = _load("feat")
    cfg = json.loads(str(g["config_json"]))
    size = g["head_x"].shape
    ns = NoiseStream(g["head_seed"])
    xT = ns(size)
    n = int(g["head_nsteps"])
    noise = np.stack([ns(size) for _ in range(n)])
    smp = FeatureSampler(hp, sd, size[0], gpu_device, cfg, prec="fp16", noise=noise, use_graph=False)
    x = smp.sample(g["label"], g["keypoint"], xT, n_steps=n).cpu().numpy()
    rh = _rel(x, g["head_x"])
    ns = NoiseStream(g["tail_seed"])
    cs = int(g["tail_curr_step"])
    noise = np.stack([ns(size) for _ in range(cs)])
    smp = FeatureSampler(hp, sd, size[0], gpu_device, cfg, prec="fp16", noise=noise, use_graph=False)
    x = smp.sample(g["label"], g["keypoint"], g["tail_x_in"], t_start=cs - 1).cpu().numpy()
    rt = _rel(x, g["tail_x0"])
    print("fp16 feature sampler: 20-step head %.3e, 20-step tail %.3e relative max error vs reference" % (rh, rt))
    assert rh <= 1e-3 and rt <= 1e-3, (rh, rt)


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_point_preparation_folded_into_the_update(gpu_device, monkeypatch, prec):
    """Feature DDPM (fixed key points): the update kernel writes the feature columns of the per-point table and of the
    concatenation buffers itself, SLIDE_OP_PREP_POINTS runs once per chain instead of once per step -- one launch less per
    step, and the SAME bits as the per-step preparation (same values, same conversions), over a chain with in-kernel noise
    and over a restarted chain (begin() must re-prime the tables)."""
    from slide_amd.diffusion import FeatureSampler
    g = load_golden("golden_sampler_feat.npz")
    _, hp, sd = _load("feat")
    cfg = json.loads(str(g["config_json"]))
    size = g["head_x"].shape
    rs = np.random.RandomState(2)
    xa, xb = rs.standard_normal(size).astype(np.float32), rs.standard_normal(size).astype(np.float32)
    kp2 = (g["keypoint"] + rs.standard_normal(g["keypoint"].shape).astype(np.float32) * 0.1).astype(np.float32)
    out = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("SLIDE_FUSE_PREP", fuse)
        smp = FeatureSampler(hp, sd, size[0], gpu_device, cfg, prec=prec, seed=77, use_graph=False)
        assert smp.fuse_prep == (fuse == "1")
        assert sum(1 for o in smp.step_ops if o.kind == abi.OP_PREP_POINTS) == (0 if fuse == "1" else 1)  # SLIDE_OP_PREP_POINTS
        a_ = smp.sample(g["label"], g["keypoint"], xa, t_start=40, n_steps=12).cpu().numpy()
        b_ = smp.sample(g["label"], kp2, xb, t_start=999, n_steps=7).cpu().numpy()  # a second chain, other key points
        out[fuse] = (a_, b_)
    assert np.isfinite(out["1"][0]).all() and np.array_equal(out["1"][0], out["0"][0]) and np.array_equal(out["1"][1], out["0"][1])


def test_head_and_update_as_one_launch(gpu_device, exp_lib, monkeypatch):
    """SLIDE_OP_HEAD_UPDATE: fc_lyaer's two per-point GEMMs (GroupNorm between them) and the DDPM update in one launch -- the
    prediction never leaves the registers.  Against the three-launch plan (SLIDE_HEAD_UPDATE=0: same arithmetic, other
    summation order in the K loops) over 10 steps with in-kernel noise: position and feature chains within 5e-4 relative
    max; the golden-chain tests run on the fused plan (the default)."""
    from slide_amd.diffusion import FeatureSampler, PositionSampler
    g = load_golden("golden_sampler_feat.npz")
    _, hpf, sdf = _load("feat")
    _, hpp, sdp = _load("pos")
    cfg = json.loads(str(g["config_json"]))
    size = g["head_x"].shape
    rs = np.random.RandomState(5)
    xf = rs.standard_normal(size).astype(np.float32)
    xp = rs.standard_normal((size[0], 16, 3)).astype(np.float32)
    out = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("SLIDE_HEAD_UPDATE", fuse)
        fs = FeatureSampler(hpf, sdf, size[0], gpu_device, cfg, prec="fp16", seed=9, use_graph=False)
        ps = PositionSampler(hpp, sdp, size[0], gpu_device, _pos_cfg(), prec="fp16", seed=9, use_graph=False)
        for smp in (fs, ps):
            kinds = [o.kind for o in smp.step_ops]
            assert (abi.OP_HEAD_UPDATE in kinds) == (fuse == "1") and ((abi.OP_UPDATE_POS in kinds) or (abi.OP_UPDATE_FEAT in kinds)) == (fuse == "0")
        out[fuse] = (fs.sample(g["label"], g["keypoint"], xf, t_start=60, n_steps=10).cpu().numpy(),
                     ps.sample(g["label"], xp, t_start=60, n_steps=10).cpu().numpy())
    for a_, b_ in zip(out["1"], out["0"]):
        assert np.isfinite(a_).all() and _rel(a_, b_) <= 5e-4, _rel(a_, b_)


def test_point_chain_launch_matches_its_four_layers(gpu_device, monkeypatch):
    """round 5: the feature sampler's step plan ends its network with ONE launch for the last FP block's second Mlp + the output head
    (SLIDE_OP_POINT_CHAIN, csrc/point_chain.hip: four dependent per-point GEMMs, weights in registers, activations through LDS) where
    SLIDE_POINT_CHAIN=0 launches the four GEMMs of the engine's plan; SLIDE_POINT_CHAIN_UPDATE=1 (opt-in: measured slower) also
    carries the DDPM update on that launch, its Philox draws in the shadow of the loads.  Same fp16 operands and roundings (the
    residual stays in fp32 inside the chain, the summation order of the K loops differs) and the SAME noise (same Philox counters):
    ragged batches (1, 3, 6 samples: partial 32-row workgroups), ten steps with in-kernel noise within 5e-4 relative max, the
    prediction of ONE step (eps) within 2e-3 of its scale, the fused update bit-identical to the chain + update launch, and an explicit
    noise tensor taking the same path."""
    from slide_amd.diffusion import FeatureSampler
    g = load_golden("golden_sampler_feat.npz")
    _, hpf, sdf = _load("feat")
    cfg = json.loads(str(g["config_json"]))
    for B in (1, 3, 6):
        rs = np.random.RandomState(11 + B)
        C = g["head_x"].shape[2]
        xf = rs.standard_normal((B, 16, C)).astype(np.float32)
        lab = np.resize(g["label"], B)
        kp = np.resize(g["keypoint"], (B,) + g["keypoint"].shape[1:])
        noise = rs.standard_normal((4, B, 16, C)).astype(np.float32)
        out, eps, nl, outn = {}, {}, {}, {}
        monkeypatch.setenv("SLIDE_POINT_CHAIN_WIDE", "0")  # like with like: the chain in the four layers' fp16 operands (round 6's default, the
        for tag, on, upd in (("fused", "1", "1"), ("chain", "1", "0"), ("plan", "0", "1")):  # split arithmetic, is compared below)
            monkeypatch.setenv("SLIDE_POINT_CHAIN", on)
            monkeypatch.setenv("SLIDE_POINT_CHAIN_UPDATE", upd)
            fs = FeatureSampler(hpf, sdf, B, gpu_device, cfg, prec="fp16", seed=9, use_graph=False)
            kinds = [o.kind for o in fs.step_ops]
            assert (abi.OP_POINT_CHAIN in kinds) == (on == "1") and (abi.OP_UPDATE_FEAT in kinds) == (tag != "fused"), kinds
            nl[tag] = len(kinds)
            x1 = fs.sample(lab, kp, xf, t_start=60, n_steps=1)
            eps[tag] = fs.engine.eps_pad.float().cpu().numpy().copy()
            out[tag] = fs.sample(lab, kp, xf, t_start=60, n_steps=10).cpu().numpy()
            assert torch.isfinite(x1).all()
            fn = FeatureSampler(hpf, sdf, B, gpu_device, cfg, prec="fp16", noise=noise, use_graph=False)
            outn[tag] = fn.sample(lab, kp, xf, t_start=3, n_steps=4).cpu().numpy()
        assert nl["plan"] - nl["chain"] == 3 and nl["chain"] - nl["fused"] == 1, nl  # four launches -> one; the update launch gone
        assert np.isfinite(out["fused"]).all() and np.array_equal(out["fused"], out["chain"]) and np.array_equal(outn["fused"], outn["chain"])
        assert np.array_equal(eps["fused"], eps["chain"])
        assert _rel(out["fused"], out["plan"]) <= 5e-4, (B, _rel(out["fused"], out["plan"]))
        assert _rel(outn["fused"], outn["plan"]) <= 5e-4, (B, _rel(outn["fused"], outn["plan"]))
        assert np.abs(eps["fused"] - eps["plan"]).max() <= 2e-3 * np.abs(eps["plan"]).max(), B
        # round 6: the chain's default form -- split arithmetic (fp32-grade products) -- against the fp16 layers: same network, fewer roundings
        monkeypatch.setenv("SLIDE_POINT_CHAIN_WIDE", "1")
        monkeypatch.setenv("SLIDE_POINT_CHAIN", "1")
        monkeypatch.setenv("SLIDE_POINT_CHAIN_UPDATE", "0")
        fw = FeatureSampler(hpf, sdf, B, gpu_device, cfg, prec="fp16", seed=9, use_graph=False)
        assert 37 in [o.kind for o in fw.step_ops] and len(fw.step_ops) == nl["chain"]
        fw.sample(lab, kp, xf, t_start=60, n_steps=1)
        ew = fw.engine.eps_pad.float().cpu().numpy()
        assert np.isfinite(ew).all() and np.abs(ew - eps["plan"]).max() <= 2e-3 * np.abs(eps["plan"]).max(), B


@pytest.mark.parametrize("prec", ["fp32", "split"])
def test_position_sampler_full_chain_matches_reference(gpu_device, prec):
    from slide_amd.diffusion import PositionSampler
    g = load_golden("golden_sampler_pos.npz")
    _, hp, sd = _load("pos")
    ns = NoiseStream(g["full_seed"])
    size = g["full_x0"].shape
    xT = ns(size)
    noise = np.stack([ns(size) for _ in range(999)])
    smp = PositionSampler(hp, sd, size[0], gpu_device, _pos_cfg(), prec=prec, noise=noise, use_graph=True)
    x0 = smp.sample(g["label"], xT).cpu().numpy()
    r = _rel(x0, g["full_x0"])
    print("1000-step position chain, relative max error vs reference: %.3e" % r)
    assert r <= 1e-3, r


def test_feature_sampler_matches_reference(gpu_device):
    from slide_amd.diffusion import FeatureSampler
    g = load_golden("golden_sampler_feat.npz")
    _, hp, sd = _load("feat")
    cfg = json.loads(str(g["config_json"]))
    size = g["head_x"].shape
    ns = NoiseStream(g["head_seed"])
    xT = ns(size)
    n = int(g["head_nsteps"])
    noise = np.stack([ns(size) for _ in range(n)])
    smp = FeatureSampler(hp, sd, size[0], gpu_device, cfg, prec="fp32", noise=noise, use_graph=True)
    x = smp.sample(g["label"], g["keypoint"], xT, n_steps=n).cpu().numpy()
    assert _rel(x, g["head_x"]) <= 1e-3, _rel(x, g["head_x"])
    ns = NoiseStream(g["tail_seed"])
    cs = int(g["tail_curr_step"])
    noise = np.stack([ns(size) for _ in range(cs)])
    smp = FeatureSampler(hp, sd, size[0], gpu_device, cfg, prec="fp32", noise=noise, use_graph=True)
    x = smp.sample(g["label"], g["keypoint"], g["tail_x_in"], t_start=cs - 1).cpu().numpy()
    assert _rel(x, g["tail_x0"]) <= 1e-3, _rel(x, g["tail_x0"])


def test_feature_sampler_full_chain_matches_reference(gpu_device):
    """The reference's COMPLETE 1000-step denoise_and_reconstruct chain (tests/golden/golden_sampler_feat_full.npz, generated by
    tools/gen_golden.py --only featfull from the imported reference with the noise stream injected): exact-fp32 mode AND the
    fp16 throughput mode within north_star's 1e-3"""
    from slide_amd.diffusion import FeatureSampler
    g = load_golden("golden_sampler_feat_full.npz")
    _, hp, sd = _load("feat")
    cfg = json.loads(str(g["config_json"]))
    size = g["full_x0"].shape
    ns = NoiseStream(g["full_seed"])
    xT = ns(size)
    noise = np.stack([ns(size) for _ in range(1000)])
    assert int(g["full_ndraws"]) == 1001
    for prec in ("fp32", "fp16"):
        smp = FeatureSampler(hp, sd, size[0], gpu_device, cfg, prec=prec, noise=noise, use_graph=(prec == "fp32"))
        x = smp.sample(g["label"], g["keypoint"], xT).cpu().numpy()
        r = _rel(x, g["full_x0"])
        print("1000-step feature chain, %s: relative max error vs reference %.3e" % (prec, r))
        assert np.isfinite(x).all() and r <= 1e-3, (prec, r)
        assert np.array_equal(x[:, :, :3], g["keypoint"])  # the key points are re-clamped every step (diffusion.py:383-385)


def test_feature_sampler_local_resampling_matches_reference(gpu_device):
    """--local_resampling: denoise_and_reconstruct(local_resampling=True) golden (tools/gen_golden.py --only resample)"""
    from slide_amd.diffusion import FeatureSampler
    g = load_golden("golden_sampler_feat_resample.npz")
    _, hp, sd = _load("feat")
    size = g["head_x"].shape
    for tag in ("head", "short"):
        cfg = json.loads(str(g[tag + "_config_json"]))
        n = int(g[tag + "_nsteps"])
        ns = NoiseStream(g[tag + "_seed"])
        xT = ns(size)
        noise = np.stack([ns(size) for _ in range(n)])
        smp = FeatureSampler(hp, sd, size[0], gpu_device, cfg, prec="fp32", noise=noise, use_graph=True, local_resampling=True)
        x = smp.sample(g["label"], g["keypoint"], xT, n_steps=n, complete_x0=g["complete_x0"],
                       keypoint_mask=g["keypoint_mask"]).cpu().numpy()
        assert _rel(x, g[tag + "_x"]) <= 1e-3, (tag, _rel(x, g[tag + "_x"]))
    # the same sampler without a mask behaves like plain generation (mask of ones)
    g2 = load_golden("golden_sampler_feat.npz")
    cfg = json.loads(str(g2["config_json"]))
    ns = NoiseStream(g2["head_seed"])
    xT = ns(size)
    n = int(g2["head_nsteps"])
    noise = np.stack([ns(size) for _ in range(n)])
    smp = FeatureSampler(hp, sd, size[0], gpu_device, cfg, prec="fp32", noise=noise, use_graph=False, local_resampling=True)
    x = smp.sample(g2["label"], g2["keypoint"], xT, n_steps=n).cpu().numpy()
    assert _rel(x, g2["head_x"]) <= 1e-3


def test_inkernel_rng_statistics(gpu_device):
    """Philox + Box-Muller noise path: one reverse step from x=0 with eps ignored is mean + sigma*z."""
    from slide_amd.diffusion import PositionSampler
    _, hp, sd = _load("pos")
    B = 256
    smp = PositionSampler(hp, sd, B, gpu_device, _pos_cfg(), prec="fp32", noise=None, seed=1234, use_graph=False)
    x1 = smp.sample(np.zeros(B, np.int64), np.zeros((B, 16, 3), np.float32), t_start=999, n_steps=1).cpu().numpy()
    x2 = smp.sample(np.zeros(B, np.int64), np.zeros((B, 16, 3), np.float32), t_start=999, n_steps=1).cpu().numpy()
    # every chain of a sampler has its own nonce in the Philox counter: the second batch of a generation run must NOT
    # replay the first one's noise trajectory (the reference draws fresh torch.randn per batch, util.py:252)
    assert not np.array_equal(x1, x2)
    z12 = np.corrcoef((x1 - x1.mean(0)).ravel(), (x2 - x2.mean(0)).ravel())[0, 1]
    assert abs(z12) < 0.05, z12
    smp_b = PositionSampler(hp, sd, B, gpu_device, _pos_cfg(), prec="fp32", noise=None, seed=1234, use_graph=False)
    x1b = smp_b.sample(np.zeros(B, np.int64), np.zeros((B, 16, 3), np.float32), t_start=999, n_steps=1).cpu().numpy()
    assert np.array_equal(x1, x1b)  # counter-based: same (seed, nonce, step, element) -> same draw
    # at t=999 the update is x = -c*eps/sqrt(alpha) + sigma*z ; all samples share eps statistics, so the
    # per-element spread across the batch is dominated by sigma*z
    z = (x1 - x1.mean(axis=0, keepdims=True)) / smp.dh["Sigma"][999]
    assert abs(z.std() - 1.0) < 0.15


def test_joint_graph_equals_separate_chains(gpu_device):
    """position + feature plans as two parallel branches of ONE hipGraph give bit-identical states to the two samplers run
    one after the other (same explicit noise)"""
    from slide_amd import configs
    from slide_amd.diffusion import FeatureSampler, JointSampler, PositionSampler
    _, hp_p, sd_p = _load("pos")
    _, hp_f, sd_f = _load("feat")
    B, n = 5, 6
    rs = np.random.RandomState(11)
    xp, xf = rs.standard_normal((B, 16, 3)).astype(np.float32), rs.standard_normal((B, 16, 51)).astype(np.float32)
    kp = rs.uniform(-0.7, 0.7, (B, 16, 3)).astype(np.float32)
    npos, nfeat = rs.standard_normal((n, B, 16, 3)).astype(np.float32), rs.standard_normal((n, B, 16, 51)).astype(np.float32)
    lab_p, lab_f = np.zeros(B, np.int64), np.full(B, 4, np.int64)
    fcfg = configs.feature_ddpm_config()["standard_diffusion_config"]
    for prec in ("fp32", "fp16"):
        pos = PositionSampler(hp_p, sd_p, B, gpu_device, _pos_cfg(), prec=prec, noise=npos)
        feat = FeatureSampler(hp_f, sd_f, B, gpu_device, fcfg, prec=prec, noise=nfeat)
        want_p = pos.sample(lab_p, xp, n_steps=n).cpu().numpy()
        want_f = feat.sample(lab_f, kp, xf, n_steps=n).cpu().numpy()
        joint = JointSampler(pos, feat)
        pos.begin(lab_p, xp); feat.begin(lab_f, kp, xf)
        joint.advance(n)
        joint.synchronize()
        assert np.array_equal(pos.state().cpu().numpy(), want_p), prec
        assert np.array_equal(feat.state().cpu().numpy(), want_f), prec


def test_split_sampler_equals_separate_chains(gpu_device):
    """bench.py's arrangement -- the position plan whole, the feature plan as two sub-batches, one step graph each launched
    round-robin (`SplitJointSampler`) -- gives bit-identical states to the three samplers run one after the other: the
    sub-batches are independent samples, only the schedule differs."""
    from slide_amd import configs
    from slide_amd.diffusion import FeatureSampler, JointSampler, PositionSampler, SplitJointSampler
    _, hp_p, sd_p = _load("pos")
    _, hp_f, sd_f = _load("feat")
    B, n = 6, 5
    sizes = [4, 2]
    rs = np.random.RandomState(23)
    xp, xf = rs.standard_normal((B, 16, 3)).astype(np.float32), rs.standard_normal((B, 16, 51)).astype(np.float32)
    kp = rs.uniform(-0.7, 0.7, (B, 16, 3)).astype(np.float32)
    npos = rs.standard_normal((n, B, 16, 3)).astype(np.float32)
    nfeat = [rs.standard_normal((n, b, 16, 51)).astype(np.float32) for b in sizes]
    lab_p, lab_f = np.zeros(B, np.int64), np.full(B, 4, np.int64)
    fcfg = configs.feature_ddpm_config()["standard_diffusion_config"]
    pos = PositionSampler(hp_p, sd_p, B, gpu_device, _pos_cfg(), prec="fp16", noise=npos)
    feats = [FeatureSampler(hp_f, sd_f, b, gpu_device, fcfg, prec="fp16", noise=nz) for b, nz in zip(sizes, nfeat)]
    lo = [0, sizes[0]]
    want_p = pos.sample(lab_p, xp, n_steps=n).cpu().numpy()
    want_f = [f.sample(lab_f[l:l + b], kp[l:l + b], xf[l:l + b], n_steps=n).cpu().numpy() for f, b, l in zip(feats, sizes, lo)]
    split = SplitJointSampler([JointSampler(pos, feats[0]), JointSampler(None, feats[1])])
    pos.begin(lab_p, xp)
    for f, b, l in zip(feats, sizes, lo):
        f.begin(lab_f[l:l + b], kp[l:l + b], xf[l:l + b])
    split.advance(n)
    split.synchronize()
    assert np.array_equal(pos.state().cpu().numpy(), want_p)
    for f, w in zip(feats, want_f):
        assert np.array_equal(f.state().cpu().numpy(), w)


def test_threaded_eager_sampler_equals_separate_chains(gpu_device):
    """bench.py's arrangements -- the position plan and three feature sub-batches replayed eagerly round-robin from one
    thread (`EagerChainsSampler`, the default), with one host thread per chain (`ThreadedEagerSampler`), or as one step
    graph per chain (`OwnGraphSampler`) -- give bit-identical states to the samplers run one after the other: only the
    schedule differs."""
    from slide_amd import configs
    from slide_amd.diffusion import (EagerChainsSampler, FeatureSampler, JointSampler, OwnGraphSampler, PositionSampler,
                                     SplitJointSampler, ThreadedEagerSampler)
    _, hp_p, sd_p = _load("pos")
    _, hp_f, sd_f = _load("feat")
    B, n = 7, 6
    sizes = [3, 2, 2]
    lo = [0, 3, 5]
    rs = np.random.RandomState(29)
    xp, xf = rs.standard_normal((B, 16, 3)).astype(np.float32), rs.standard_normal((B, 16, 51)).astype(np.float32)
    kp = rs.uniform(-0.7, 0.7, (B, 16, 3)).astype(np.float32)
    npos = rs.standard_normal((n, B, 16, 3)).astype(np.float32)
    nfeat = [rs.standard_normal((n, b, 16, 51)).astype(np.float32) for b in sizes]
    lab_p, lab_f = np.zeros(B, np.int64), np.full(B, 4, np.int64)
    fcfg = configs.feature_ddpm_config()["standard_diffusion_config"]

    def make(use_graph):
        p = PositionSampler(hp_p, sd_p, B, gpu_device, _pos_cfg(), prec="fp16", noise=npos, use_graph=use_graph)
        fs = [FeatureSampler(hp_f, sd_f, b, gpu_device, fcfg, prec="fp16", noise=nz, use_graph=use_graph)
              for b, nz in zip(sizes, nfeat)]
        return p, fs

    def begin(p, fs):
        p.begin(lab_p, xp)
        for f, b, l in zip(fs, sizes, lo):
            f.begin(lab_f[l:l + b], kp[l:l + b], xf[l:l + b])

    pos, feats = make(True)
    want_p = pos.sample(lab_p, xp, n_steps=n).cpu().numpy()
    want_f = [f.sample(lab_f[l:l + b], kp[l:l + b], xf[l:l + b], n_steps=n).cpu().numpy() for f, b, l in zip(feats, sizes, lo)]
    # graphs: the position chain as its own graph beside the feature graphs
    begin(pos, feats)
    split = SplitJointSampler([JointSampler(None, feats[0]), OwnGraphSampler(pos)] + [JointSampler(None, f) for f in feats[1:]])
    split.advance(n)
    split.synchronize()
    assert np.array_equal(pos.state().cpu().numpy(), want_p)
    for f, w in zip(feats, want_f):
        assert np.array_equal(f.state().cpu().numpy(), w)
    # eager, one host thread per chain: the first advance() runs on the caller's thread, the second on the threads
    pe, fe = make(False)
    thr = ThreadedEagerSampler([pe] + fe)
    begin(pe, fe)
    thr.advance(2)
    thr.advance(n - 2)
    thr.synchronize()
    assert np.array_equal(pe.state().cpu().numpy(), want_p)
    for f, w in zip(fe, want_f):
        assert np.array_equal(f.state().cpu().numpy(), w)
    # eager, all chains round-robin from one thread inside the library (bench.py's default)
    begin(pe, fe)
    rr = EagerChainsSampler([fe[0], pe] + fe[1:])
    rr.advance(n)
    rr.synchronize()
    assert np.array_equal(pe.state().cpu().numpy(), want_p)
    for f, w in zip(fe, want_f):
        assert np.array_equal(f.state().cpu().numpy(), w)
    # a chain that steps once per TWO rounds (slide_run_chains_every: a position chain over a multiple of the batch beside chains
    # over the batch): rounds 0, 2, ..., 2 n - 2 make the same n steps
    begin(pe, fe)
    rr = EagerChainsSampler([pe], every=[2])
    rr.advance(2 * n - 1)
    rr.synchronize()
    assert np.array_equal(pe.state().cpu().numpy(), want_p)


def test_x_stationary_kernel_bit_identical(gpu_device, exp_lib, monkeypatch):
    """csrc/gemm_xs.hip: input resident in LDS (gathered first layers: only the point table), a workgroup computes several
    column tiles from it -- the same MFMA / epilogue arithmetic in the same order as the ring kernels, so the denoiser output
    must be bit-identical in every mode (default policy, every eligible layer, 128-channel tiles, capped occupancy)"""
    from slide_amd.engine import DenoiserEngine
    monkeypatch.setenv("SLIDE_GX", "0")  # the round-2 plan (the X-stationary kernel reads stored K-expanded inputs)
    for name in ("pos", "feat"):
        g, hp, sd = _load(name)
        x, ts, lab = g["x_mixed"], g["ts_mixed"], g["label_mixed"]
        monkeypatch.setenv("SLIDE_XS", "")  # ring kernels only
        e0 = DenoiserEngine(hp, sd, x.shape[0], gpu_device, prec="fp16")
        assert not any(o.kind == abi.OP_GEMM and o.p[10] for o in e0.ops)
        ref = e0.forward(x, ts, lab).cpu().numpy()
        for mode, cbw, occ in (("auto", "2", ""), ("7,8", "2", ""), ("7,8", "4", "1"), ("8", "2", "2")):
            monkeypatch.setenv("SLIDE_XS", mode)
            monkeypatch.setenv("SLIDE_XS_CBW", cbw)
            monkeypatch.setenv("SLIDE_XS_OCC", occ) if occ else monkeypatch.delenv("SLIDE_XS_OCC", raising=False)
            e = DenoiserEngine(hp, sd, x.shape[0], gpu_device, prec="fp16")
            assert any(o.kind == abi.OP_GEMM and o.p[10] for o in e.ops)
            got = e.forward(x, ts, lab).cpu().numpy()
            assert np.array_equal(got, ref), (name, mode, cbw, occ, float(np.abs(got - ref).max()))


def test_fragment_major_layout_bit_identical(gpu_device, monkeypatch):
    """Round 6: the K-expanded inputs u / mo of the fused attention tails stored FRAGMENT-major (SLIDE_F_OUT_FM: inside every
    32-row group of a chunk the bytes are ordered as the MFMA fragments attn_tail_rx_kernel loads, 1 KB of consecutive memory
    per wave load) -- a pure re-layout between the producers' epilogue stores (generated-X GEMMs, SA chain) and
    the tail's loads: the denoiser output must be bit-identical to the chunk-major plan (SLIDE_FM=0), on the default
    (pair-decomposition) plan, with the two-launch Mlp tail instead of the SA chain, with separate instead of dual generated-X
    launches, and on ragged batches."""
    from slide_amd.engine import DenoiserEngine
    for name in ("feat", "pos"):
        g, hp, sd = _load(name)
        x, ts, lab = g["x_mixed"], g["ts_mixed"], g["label_mixed"]
        for knobs in ({}, {"SLIDE_SA_CHAIN": "0"}, {"SLIDE_GX_DUAL": "0"}):
            for k_, v_ in knobs.items():
                monkeypatch.setenv(k_, v_)
            for B in (x.shape[0], 9, 33):
                rep = (B + x.shape[0] - 1) // x.shape[0]
                xb, tb, lb = np.concatenate([x] * rep)[:B], np.concatenate([ts] * rep)[:B], np.concatenate([lab] * rep)[:B]
                monkeypatch.setenv("SLIDE_FM", "0")
                e0 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp16")
                assert not e0._fm and not any(o.kind == abi.OP_ATTN_TAIL and (int(o.f[1]) & abi.TAIL_FM) for o in e0.ops)
                ref = e0.forward(xb, tb, lb).cpu().numpy()
                monkeypatch.setenv("SLIDE_FM", "1")
                e1 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp16")
                tails = [o for o in e1.ops if o.kind == abi.OP_ATTN_TAIL]
                # (without the SA chain an SA block's rest_mlp is a ring GEMM over a stored h2: that block stays chunk-major)
                nfm = sum(1 for o in tails if int(o.f[1]) & abi.TAIL_FM)
                # (the position net's narrow blocks are outside the layout's conditions -- _tail_fm: its plan must simply not change)
                assert nfm == (0 if name == "pos" else 2 if "SLIDE_SA_CHAIN" in knobs else 4) and bool(e1._fm) == (nfm > 0), (name, knobs, B, nfm)
                got = e1.forward(xb, tb, lb).cpu().numpy()
                assert np.array_equal(got, ref), (name, knobs, B, float(np.abs(got - ref).max()))
            for k_ in knobs:
                monkeypatch.delenv(k_)


def test_chunk_major_layout_bit_identical(gpu_device, exp_lib, monkeypatch):
    """Chunk-major activations / weights ([k / 32][rows][32]: one LDS-DMA instruction reads 1 KB of consecutive memory) are a
    pure re-layout of the K-expanded buffers between GEMM epilogues and ring-kernel loaders: the denoiser output must be
    bit-identical to the row-major plan, with the gather-on-load first layers, the fused attention tail, and without either."""
    from slide_amd.engine import DenoiserEngine
    monkeypatch.setenv("SLIDE_GX", "0")  # the round-2 plan on both sides (the pair decomposition needs chunk-major weights)
    monkeypatch.setenv("SLIDE_GEMM_CHAIN", "0")  # (COPY launches between the per-point GEMMs change which of them form a chain)
    monkeypatch.setenv("SLIDE_POINT_CHAIN", "0")  # (... and whether forward() ends with the point chain, split arithmetic since round 6)
    for name in ("pos", "feat"):
        g, hp, sd = _load(name)
        x, ts, lab = g["x_mixed"], g["ts_mixed"], g["label_mixed"]
        for knobs in ({}, {"SLIDE_CM_TABLES": "1"}, {"SLIDE_GATHER": "0"}, {"SLIDE_ATTN_TAIL": "0"}, {"SLIDE_SPLIT_FIRST": "32"},
                      {"SLIDE_MERGE_Q": "0"}):
            for k_, v_ in knobs.items():
                monkeypatch.setenv(k_, v_)
            monkeypatch.setenv("SLIDE_CM", "0")
            monkeypatch.setenv("SLIDE_MERGE_Q", "0")  # (the reference plan is also the one-launch-per-query-GEMM plan
            monkeypatch.setenv("SLIDE_FOLD_COPIES", "0")  # with separate COPY launches for the concatenation columns)
            e0 = DenoiserEngine(hp, sd, x.shape[0], gpu_device, prec="fp16")
            n_copy0 = sum(1 for o in e0.ops if o.kind == abi.OP_COPY_COLS)
            monkeypatch.setenv("SLIDE_MERGE_Q", knobs.get("SLIDE_MERGE_Q", "1"))
            monkeypatch.setenv("SLIDE_FOLD_COPIES", "1")
            assert not e0._cm and not any(o.kind == abi.OP_GEMM and (o.i[8] & abi.GEMM_W_CM) for o in e0.ops)
            ref = e0.forward(x, ts, lab).cpu().numpy()
            monkeypatch.setenv("SLIDE_CM", "1")
            e1 = DenoiserEngine(hp, sd, x.shape[0], gpu_device, prec="fp16")
            assert e1._cm and any(o.kind == abi.OP_GEMM and (o.i[8] & abi.GEMM_W_CM) for o in e1.ops)
            assert sum(1 for o in e1.ops if o.kind == abi.OP_COPY_COLS) <= n_copy0 - 4  # skip-feature and xyz columns come from their producers
            got = e1.forward(x, ts, lab).cpu().numpy()
            assert np.array_equal(got, ref), (name, knobs, float(np.abs(got - ref).max()))
            for k_ in knobs:
                monkeypatch.delenv(k_)


def test_pair_decomposition_plan_variants(gpu_device, exp_lib, monkeypatch):
    """Round 3: the pair decomposition (csrc/gemm_gx.hip, block_body.hip) re-associates the blocks' first layers (a[q] + b[p]
    from 16-row GEMMs instead of 256- / 128-row ones) and runs the SA blocks in natural neighbour order, so it is NOT
    bit-identical to the round-2 plan; both are fp16 renderings of the same network.  Every combination of the round-3
    kernels (fused SA chain, block body, pair-table pass fused / v1 / v2, eight-wave tail, per-point layer chains) must agree with the reference golden
    within the fp16 forward bound (5e-3 of the output's L2 norm, as test_denoiser_forward_fp16_mfma) AND with each other
    within 4e-3 (measured <= 2e-3: different summation orders of fp16-rounded terms)."""
    from slide_amd.engine import DenoiserEngine
    for name in ("pos", "feat"):
        g, hp, sd = _load(name)
        x, ts, lab = g["x_mixed"], g["ts_mixed"], g["label_mixed"]
        ref = g["eps_mixed"]
        outs = {}
        for tag, knobs in (("round2", {"SLIDE_GX": "0"}), ("default", {}), ("block_body", {"SLIDE_BODY": "1"}),
                           ("no_chain", {"SLIDE_SA_CHAIN": "0"}),
                           ("pair_norm_v2", {"SLIDE_PAIR_NORM_V2": "1"}), ("tail8", {"SLIDE_TAIL8": "1"}),
                           ("two_launch_tables", {"SLIDE_PAIR_FUSED": "0"}), ("gemm_chains", {"SLIDE_GEMM_CHAIN": "256"}),
                           ("wide_key_tiles", {"SLIDE_GX_N64": "0"}), ("no_half_tiles_on_small_grids", {"SLIDE_GX_N64W": "0"}), ("no_dual_launch", {"SLIDE_GX_DUAL": "0"}), ("query_gemm_apart", {"SLIDE_CHAIN_P": "0"}), ("tail_occ3", {"SLIDE_TAIL_OCC3": "1"}), ("wide_tail", {"SLIDE_TAIL_WIDE": "8"}),
                           ("long_gemm_chains", {"SLIDE_GEMM_CHAIN": "100000"})):
            for k_, v_ in knobs.items():
                monkeypatch.setenv(k_, v_)
            e = DenoiserEngine(hp, sd, x.shape[0], gpu_device, prec="fp16")
            kinds = {o.kind for o in e.ops}
            if tag == "round2":
                assert not kinds & {abi.OP_GEMM_GX, abi.OP_PAIR_NORM, abi.OP_SA_CHAIN, abi.OP_BLOCK_BODY}
            elif tag in ("pair_norm_v2", "two_launch_tables"):
                assert abi.OP_PAIR_NORM in kinds and abi.OP_PAIR_FIRST not in kinds  # SLIDE_OP_PAIR_NORM after a 16-row GEMM
            else:
                assert abi.OP_PAIR_FIRST in kinds and abi.OP_PAIR_NORM not in kinds  # SLIDE_OP_PAIR_FIRST: GEMM + table pass in one launch
            assert (abi.OP_GEMM_CHAIN in kinds) == ("gemm_chain" in tag)  # SLIDE_OP_GEMM_CHAIN (opt-in): per-point layer chains, one launch each
            assert (abi.OP_BLOCK_BODY in kinds) == (tag == "block_body" and name == "feat")  # SLIDE_OP_BLOCK_BODY (opt-in since round 5): FP0 of the feature net
            outs[tag] = e.forward(x, ts, lab).cpu().numpy().astype(np.float64)
            for k_ in knobs:
                monkeypatch.delenv(k_)
            err = np.linalg.norm(outs[tag] - ref) / np.linalg.norm(ref)
            assert np.isfinite(outs[tag]).all() and err <= 5e-3, (name, tag, err)
        for tag, o in outs.items():
            d = np.linalg.norm(o - outs["default"]) / np.linalg.norm(outs["default"])
            assert d <= 4e-3, (name, tag, d)
        # the query GEMM riding on the Mlp chain's launch runs the same body on the same tiles: same bits
        assert np.array_equal(outs["query_gemm_apart"], outs["default"]), name
        # one launch for the two independent generated-X GEMMs of an FP block: the same two kernels' bodies, same bits
        assert np.array_equal(outs["no_dual_launch"], outs["default"]), name
        # the fused launch evaluates the table pass's arithmetic on the accumulators instead of a stored fp32 y: same bits
        assert np.array_equal(outs["two_launch_tables"], outs["default"]), name


def test_split_pair_decomposition_plan_variants(gpu_device, exp_lib, monkeypatch):
    """Round 5: the position DDPM's benched plan is the pair decomposition IN THE SPLIT ARITHMETIC (csrc/gemm_gxs.hip: float pair
    tables, generated-X split GEMMs on one accumulator set, PAIR residuals on float rows, the split attention tail).  Every
    variant -- the fp32-structured round-4 plan (SLIDE_GXS=0), the three-launch tail, the two generated-X GEMMs as separate
    launches, second_mlp and rest_mlp of the SA blocks as separate launches (no h2 in registers), the opt-in per-point stage kernel -- is fp32-grade: <= 2e-4 (max-norm) of the reference golden and <= 2e-5 of each
    other (different summation orders of fp32-grade terms), for both nets; the dual launch runs the same two kernel bodies on the
    same tiles: same bits."""
    from slide_amd.engine import DenoiserEngine
    for name in ("pos", "feat"):
        g, hp, sd = _load(name)
        x, ts, lab = g["x_mixed"], g["ts_mixed"], g["label_mixed"]
        ref = g["eps_mixed"]
        outs = {}
        for tag, knobs in (("default", {}), ("round4_plan", {"SLIDE_GXS": "0"}), ("three_launch_tail", {"SLIDE_TAIL_SPLIT": "0"}),
                           ("no_dual_launch", {"SLIDE_GX_DUAL": "0"}), ("no_layer_chain", {"SLIDE_GXS_CHAIN": "0"}),
                           ("no_chain_no_dual", {"SLIDE_GXS_CHAIN": "0", "SLIDE_GX_DUAL": "0"}), ("per_point_stage", {"SLIDE_PP": "1"})):
            for k_, v_ in knobs.items():
                monkeypatch.setenv(k_, v_)
            e = DenoiserEngine(hp, sd, x.shape[0], gpu_device, prec="split")
            kinds = [o.kind for o in e.ops]
            assert (abi.OP_GEMM_GX in kinds or abi.OP_GEMM_GX_DUAL in kinds) == (tag != "round4_plan")   # SLIDE_OP_GEMM_GX / _DUAL
            assert (abi.OP_ATTN_COMBINE in kinds) == (tag in ("round4_plan", "three_launch_tail"))  # SLIDE_OP_ATTN_COMBINE
            assert (abi.OP_PP_STAGE in kinds) == (tag == "per_point_stage")              # SLIDE_OP_PP_STAGE
            if tag == "default" and name == "pos":
                assert len(kinds) <= 30, len(kinds)  # (round 4: 49 launches + the t-embedding launch of the forward API)
            outs[tag] = e.forward(x, ts, lab).cpu().numpy().astype(np.float64)
            for k_ in knobs:
                monkeypatch.delenv(k_)
            assert np.isfinite(outs[tag]).all() and _rel(outs[tag], ref) <= 2e-4, (name, tag, _rel(outs[tag], ref))
        for tag, o in outs.items():
            assert _rel(o, outs["default"]) <= 2e-5, (name, tag, _rel(o, outs["default"]))
        assert np.array_equal(outs["no_dual_launch"], outs["default"]), name


@pytest.mark.parametrize("name", ["pos", "feat"])
def test_split_plan_on_ragged_batches(gpu_device, name):
    """the split pair-decomposition kernels own 256-row tiles: one 16 x 16-row sample, or TWO 16 x 8-row samples -- an odd batch leaves
    the last FP-block tile half empty, a batch of one leaves it with a single sample.  Split plan vs the exact-fp32 plan on random
    inputs for B = 1, 3, 5, 9: <= 2e-5 (max-norm), every output finite."""
    from slide_amd.engine import DenoiserEngine
    from slide_amd.synth import synth_keypoints
    g, hp, sd = _load(name)
    cx = 3 + hp["in_fea_dim"]
    for B in (1, 3, 5, 9):
        rs = np.random.RandomState(100 + B)
        x = rs.standard_normal((B, 16, cx)).astype(np.float32)
        x[:, :, :3] = synth_keypoints(B, seed=B)
        ts = rs.randint(0, 1000, B).astype(np.float32)
        lab = rs.randint(0, 13, B).astype(np.int64)
        y32 = DenoiserEngine(hp, sd, B, gpu_device, prec="fp32").forward(x, ts, lab).cpu().numpy()
        ysp = DenoiserEngine(hp, sd, B, gpu_device, prec="split").forward(x, ts, lab).cpu().numpy()
        assert np.isfinite(ysp).all() and _rel(ysp, y32) <= 2e-5, (name, B, _rel(ysp, y32))


def _full_chains(gpu_device, B, precs):
    """complete 1000-step position / feature chains of B shapes per arithmetic in `precs` = {name: (pos prec, feat prec)}"""
    from slide_amd.diffusion import FeatureSampler, PositionSampler
    from slide_amd.synth import synth_keypoints
    res = {}
    for tag, (pp, fp) in precs.items():
        if pp is not None:
            _, hp, sd = _load("pos")
            ps = PositionSampler(hp, sd, B, gpu_device, _pos_cfg(), prec=pp, seed=77, use_graph=True)
            xT = np.random.RandomState(4).standard_normal((B, 16, 3)).astype(np.float32)
            res["pos", tag] = ps.sample(np.zeros(B, np.int64), xT).cpu().numpy()
        if fp is not None:
            g, hp, sd = _load("feat")
            cfg = json.loads(str(load_golden("golden_sampler_feat.npz")["config_json"]))
            fs = FeatureSampler(hp, sd, B, gpu_device, cfg, prec=fp, seed=78, use_graph=True)
            xT = np.random.RandomState(5).standard_normal((B, 16, 51)).astype(np.float32)
            res["feat", tag] = fs.sample(np.full(B, 4, np.int64), synth_keypoints(B), xT).cpu().numpy()
    return res


def _chain_agreement(name, a, b, B):
    a, b = a.reshape(B, -1), b.reshape(B, -1)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    per_shape = np.abs(a - b).max(axis=1) / np.abs(b).max()
    a2, b2 = a.reshape(B * 16, -1), b.reshape(B * 16, -1)
    if name == "feat":  # the key-point channels are the clamped condition: identical
        assert np.array_equal(a2[:, :3], b2[:, :3])
        a2, b2 = a2[:, 3:], b2[:, 3:]
    sd_b = b2.std(axis=0) + 1e-6
    dm = np.abs(a2.mean(axis=0) - b2.mean(axis=0)) / sd_b
    ratio = a2.std(axis=0) / sd_b
    print("%s: per-shape relative max distance: median %.2e, 95 %% %.2e, 99 %% %.2e, max %.2e; shapes above 1e-3: %d of %d; "
          "|mean diff| / std <= %.1e, std ratio %.4f .. %.4f" % (name, np.median(per_shape), np.quantile(per_shape, 0.95),
                                                                 np.quantile(per_shape, 0.99), per_shape.max(),
                                                                 int((per_shape > 1e-3).sum()), B, dm.max(), ratio.min(), ratio.max()))
    return per_shape, dm, ratio


def test_benched_full_chains_follow_the_fp32_chains(gpu_device):
    """north_star's criterion on GENERATED LATENTS, over complete generations in the arithmetic `bench.py` times (round 5:
    position chain split, feature chain fp16 operands / fp32 accumulation) against the same chains in the exact-fp32 mode
    (pinned to the reference at <= 1e-3 above, measured 7e-7), 256 shapes, in-kernel Philox noise with equal seeds.
    Asserted per shape (relative max distance): <= 1e-3 for EVERY shape (round 6: no exemption -- rounds 4-5 allowed 1 % of the
    shapes up to 1e-2 for flipped kNN near-ties of the position chain; the split position plan does not flip any on these seeds:
    measured maximum 7.5e-4 position / 3.1e-4 feature); batch statistics must agree."""
    B = 256
    res = _full_chains(gpu_device, B, {"bench": ("split", "fp16"), "fp32": ("fp32", "fp32")})
    for name in ("pos", "feat"):
        per_shape, dm, ratio = _chain_agreement(name, res[name, "bench"], res[name, "fp32"], B)
        n_over = int((per_shape > 1e-3).sum())
        assert n_over == 0 and per_shape.max() <= 1e-3, (name, n_over, per_shape.max())
        assert dm.max() <= 0.01 and 0.99 <= ratio.min() and ratio.max() <= 1.01


def test_optin_fp16_position_chains_are_bounded(gpu_device):
    """the opt-in fp16 POSITION plan (`--pos-prec fp16`; not benched since round 5) over complete chains: the error does not
    accumulate (median 1.2e-4) but individual shapes reach 2.4e-3 -- bounded here at 95 % <= 1e-3, all <= 3e-3."""
    B = 256
    res = _full_chains(gpu_device, B, {"fp16": ("fp16", None), "fp32": ("fp32", None)})
    per_shape, dm, ratio = _chain_agreement("pos", res["pos", "fp16"], res["pos", "fp32"], B)
    assert per_shape.max() <= 3e-3 and np.quantile(per_shape, 0.95) <= 1e-3, (per_shape.max(), np.quantile(per_shape, 0.95))
    assert dm.max() <= 0.01 and 0.99 <= ratio.min() and ratio.max() <= 1.01


def test_position_sampler_full_chain_fp16_matches_reference(gpu_device):
    """the reference's own 1000-step position chain (golden, injected noise stream) in the throughput mode: <= 1e-3"""
    from slide_amd.diffusion import PositionSampler
    g = load_golden("golden_sampler_pos.npz")
    _, hp, sd = _load("pos")
    ns = NoiseStream(g["full_seed"])
    size = g["full_x0"].shape
    xT = ns(size)
    noise = np.stack([ns(size) for _ in range(999)])
    smp = PositionSampler(hp, sd, size[0], gpu_device, _pos_cfg(), prec="fp16", noise=noise, use_graph=True)
    r = _rel(smp.sample(g["label"], xT).cpu().numpy(), g["full_x0"])
    print("1000-step position chain in fp16, relative max error vs reference: %.3e" % r)
    assert r <= 1e-3, r


def test_feature_chain_at_a_form_c_sub_batch_follows_the_fp32_chain(gpu_device):
    """north_star's criterion on generated latents in the feature sub-batch size of `bench.py --batch 2048` (688 shapes: form C of
    the fp16 plan -- 128-channel generated-X tiles, the SA chain apart from its query GEMM, a separate GroupNorm finalise launch):
    one complete 1000-step chain in the benched fp16 arithmetic against the exact-fp32 chain, equal in-kernel seeds, <= 1e-3 per
    shape; batch statistics must agree."""
    from plan_forms import FEATURE_FP16_FORMS, feature_fp16_form, form_signature
    from slide_amd.diffusion import FeatureSampler
    import time
    B = 688
    assert feature_fp16_form(B) == "C"
    g, hp, sd = _load("feat")
    cfg = json.loads(str(load_golden("golden_sampler_feat.npz")["config_json"]))
    fs = FeatureSampler(hp, sd, B, gpu_device, cfg, prec="fp16", seed=78, use_graph=False)
    sig = form_signature(fs.engine)
    assert sig[2] == FEATURE_FP16_FORMS["C"][2][2] and sig[1]["OP_FINALIZE_GN"] == 1, sig  # (sampler mode: no t-embedding launch)
    del fs
    t0 = time.time()
    res = _full_chains(gpu_device, B, {"bench": (None, "fp16"), "fp32": (None, "fp32")})
    print("688-shape feature chains (fp16 + fp32): %.1f s" % (time.time() - t0))
    per_shape, dm, ratio = _chain_agreement("feat", res["feat", "bench"], res["feat", "fp32"], B)
    assert per_shape.max() <= 1e-3, (int((per_shape > 1e-3).sum()), per_shape.max())
    assert dm.max() <= 0.01 and 0.99 <= ratio.min() and ratio.max() <= 1.01
