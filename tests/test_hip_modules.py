"""GPU: the module-level drop-in API (`pointnet2_ops.*`, `PointNet2CloudCondition`) on HIP kernels vs golden vectors
produced by the REFERENCE modules."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden_spec, load_golden
from slide_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

# tolerances of the fp16-operand decode (the arithmetic bench.py's decode leg times and the generation CLIs run by default) against
# the reference's decode of golden_decode.npz.  Measured in round 6 (printed by the test): reference points -> own candidates 3.3e-6 /
# 1.0e-5 / 7.6e-6 per level (six channels, clouds in [-1, 1]^3); Chamfer per level <= 6.8e-8, end to end 2.0e-7.
DECODE_FP16_LEVEL_TOL = 1e-4
DECODE_FP16_CHAMFER_TOL = 1e-5


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _load(mod, g, prefix, tag, dev):
    spec = golden_spec(g, prefix)
    vals = synth_state_dict([(tag + n, s) for n, s in spec])
    mod.load_state_dict({n: torch.from_numpy(vals[tag + n]) for n, _ in spec})
    return mod.to(dev).eval()


def test_blocks_match_reference_modules(gpu_device):
    from pointnet2_ops import pointnet2_modules as PM
    from pointnet2_ops import pointnet2_utils as PU
    from pointnet2_ops.attention import AttentionModule
    g = load_golden("golden_blocks.npz")
    d = gpu_device
    xyz, feats = T(g["xyz"], d), T(g["feats"], d)
    fidx = PU.furthest_point_sample(xyz, g["fps_idx"].shape[1])
    assert np.array_equal(fidx.cpu().numpy(), g["fps_idx"])
    new_xyz = PU.gather_operation(xyz.transpose(1, 2).contiguous(), fidx).transpose(1, 2).contiguous()
    assert np.array_equal(new_xyz.cpu().numpy(), g["new_xyz"])
    o, c = PU.QueryAndGroup(0, 8, True, True, True, "nn")(xyz, new_xyz, feats, subset=True, return_counts=True)
    assert np.array_equal(o.cpu().numpy(), g["qg_nn"]) and np.array_equal(c.cpu().numpy(), g["qg_nn_counts"])
    qr = PU.QueryAndGroup(0.6, 8, True, True, False, "radius")
    o, c = qr(xyz, new_xyz, feats, subset=True, return_counts=True)
    assert np.array_equal(o.cpu().numpy(), g["qg_radius"]) and np.array_equal(c.cpu().numpy(), g["qg_radius_counts"])
    o, c = qr(xyz, T(g["q2"], d), feats, subset=False, return_counts=True)
    assert np.allclose(o.cpu().numpy(), g["qg_radius_nosubset"], atol=1e-7)
    assert np.allclose(PU.group_knn(new_xyz, xyz, feats, 6, transpose=True).cpu().numpy(), g["group_knn"], rtol=1e-5, atol=1e-6)
    dist, i3 = PU.three_nn(xyz, new_xyz)
    assert np.array_equal(i3.cpu().numpy(), g["three_nn_idx"]) and np.allclose(dist.cpu().numpy(), g["three_nn_dist"], atol=1e-6)
    C = feats.shape[1]
    fp = _load(PM.PointnetFPModule(mlp=[C + 7, 16, 16], bn=True, include_t=False, bias=True, res_connect=True), g, "fp_spec", "fpmod.", d)
    out = fp(xyz, new_xyz, T(g["fp_unknown_feats"], d), T(g["fp_known_feats"], d))
    assert np.allclose(out.cpu().numpy(), g["fp_out"], atol=5e-5)
    att = {"use_attention_module": True, "attention_bn": True, "transform_grouped_feat_out": True, "last_activation": True}
    sa = _load(PM.PointnetSAModule(mlp=[C, 16, 16, 32], npoint=12, radius=0, nsample=8, bn=True, use_xyz=True, t_dim=24,
                                   include_t=True, include_abs_coordinate=True, include_center_coordinate=True, bias=True,
                                   res_connect=True, include_condition=True, condition_dim=10, neighbor_def="nn",
                                   attention_setting=att), g, "sa_spec", "samod.", d)
    nx, nf = sa(xyz, feats, t_emb=T(g["sa_t_emb"], d), condition_emb=T(g["sa_cond_emb"], d))
    assert np.array_equal(nx.cpu().numpy(), g["sa_new_xyz"]) and np.allclose(nf.cpu().numpy(), g["sa_new_features"], atol=5e-5)
    am = _load(AttentionModule(C, C + 6, C, C + 6, 32, True, True, True), g, "att_spec", "attmod.", d)
    a = am(T(g["att_query"], d), T(g["qg_radius"], d), T(g["att_grouped_feat_out"], d), T(g["qg_radius_counts"], d))
    assert np.allclose(a.cpu().numpy(), g["att_out"], atol=5e-5)


@pytest.mark.parametrize("name", ["pos", "feat"])
def test_denoiser_module_path_and_state_dict(gpu_device, name):
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    g = load_golden("golden_denoiser_%s.npz" % name)
    hp = json.loads(str(g["config_json"]))
    spec = golden_spec(g)
    net = PointNet2CloudCondition(hp)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(spec)  # checkpoint compatibility
    sd = synth_state_dict(spec)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(gpu_device).eval()
    for k in ["t0", "t999", "mixed"]:
        x, ts, lab = T(g["x_" + k], gpu_device), T(g["ts_" + k], gpu_device), T(g["label_" + k], gpu_device)
        y = net(x, ts=ts, label=lab).cpu().numpy()
        ref = g["eps_" + k]
        assert np.abs(y - ref).max() <= 2e-4 * np.abs(ref).max(), k
        yf = net(x, ts=ts, label=lab, fused=True).cpu().numpy()
        assert np.abs(yf - ref).max() <= 2e-4 * np.abs(ref).max(), k


@pytest.mark.parametrize("name", ["fp3nn", "bnfirst", "fp3nn_bnfirst", "nobn"])
def test_denoiser_configuration_branches_match_reference(gpu_device, name):
    """The configuration branches no shipped latent-DDPM config takes (VERDICT r5 "missing" 3): the three-nearest-neighbour FP module
    (`use_knn_FP` False), `bn_first` (GroupNorm -> ReLU -> conv Mlps with a leading convolution in SA0, activation + conv output head)
    and `bn` False -- PointNet2CloudCondition.forward on the module path against the reference's forward of the same configuration
    (golden_denoiser_variants.npz, tools/gen_golden.py; reference pointnet2_with_pcld_condition.py:226-277, pointnet2_ssg_sem.py:56-177),
    checkpoint-compatible state dict; the fused plan declines them."""
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    g = load_golden("golden_denoiser_variants.npz")
    hp = json.loads(str(g[name + "_config_json"]))
    spec = golden_spec(g, name + "_spec")
    net = PointNet2CloudCondition(hp)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(spec)
    sd = synth_state_dict(spec)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(gpu_device).eval()
    x, ts, lab = T(g[name + "_x"], gpu_device), T(g[name + "_ts"], gpu_device), T(g[name + "_label"], gpu_device)
    y = net(x, ts=ts, label=lab).cpu().numpy()
    ref = g[name + "_eps"]
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print("variant %s: max-norm error vs reference %.2e" % (name, err))
    assert y.shape == ref.shape and err <= 2e-4, (name, err)
    with pytest.raises(NotImplementedError):
        net(x, ts=ts, label=lab, fused=True)


@pytest.mark.parametrize("name", ["local", "global", "both"])
def test_denoiser_with_a_condition_cloud_matches_reference(gpu_device, name):
    """The condition-cloud form of the denoiser (VERDICT r5 "missing" 2; reference pointnet2_with_pcld_condition.py:94-260, :301-447):
    local features through the feature-transfer modules of a second PointNet++ over the condition cloud, the Pnet2Stage global
    feature, both -- module path against the reference's forward (golden_denoiser_condition.npz, tools/gen_golden.py `--only
    condition`; a small architecture under the reference's keys: no shipped configuration sets these branches); the retained-feature
    path: a second call with other x / t re-uses the first call's condition features, as the reference's does."""
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    g = load_golden("golden_denoiser_condition.npz")
    hp = json.loads(str(g[name + "_config_json"]))
    spec = golden_spec(g, name + "_spec")
    net = PointNet2CloudCondition(hp)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(spec)
    sd = synth_state_dict(spec)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(gpu_device).eval()
    d = gpu_device
    x, cond, ts, lab = (T(g[name + "_" + k], d) for k in ("x", "cond", "ts", "label"))
    ref, ref2 = g[name + "_eps"], g[name + "_eps2"]
    y = net(x, condition=cond, ts=ts, label=lab).cpu().numpy()
    err = np.abs(y - ref).max() / np.abs(ref).max()
    net.reset_cond_features()
    y1 = net(x, condition=cond, ts=ts, label=lab, use_retained_condition_feature=True).cpu().numpy()
    y2 = net(T(g[name + "_x2"], d), condition=cond, ts=T(g[name + "_ts2"], d), label=lab, use_retained_condition_feature=True).cpu().numpy()
    err2 = np.abs(y2 - ref2).max() / np.abs(ref2).max()
    print("condition cloud %s: max-norm error vs reference %.2e, retained second call %.2e" % (name, err, err2))
    assert err <= 2e-4 and np.array_equal(y1, y) and err2 <= 2e-4, (name, err, err2)
    with pytest.raises(AssertionError):  # a configuration with a condition cloud needs one
        net(x, ts=ts, label=lab)


@pytest.mark.parametrize("name", ["swish_pe_ga", "concat_partial"])
def test_denoiser_parent_project_switches_match_reference(gpu_device, name):
    """The completion / refinement parent project's switches of PointNet2CloudCondition (reference :47-93, :119-126, :243-257, :302-347):
    swish activation + NeRF-style position encoding of the coordinates + global attention behind both levels + the up-sampling output
    head (out_dim x 2), and the condition cloud concatenated to the noisy cloud behind an indicator channel -- module path against the
    reference's forward (golden_denoiser_switches.npz, tools/gen_golden.py `--only switches`)."""
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.pointnet2_with_pcld_condition import PointNet2CloudCondition
    g = load_golden("golden_denoiser_switches.npz")
    hp = json.loads(str(g[name + "_config_json"]))
    spec = golden_spec(g, name + "_spec")
    net = PointNet2CloudCondition(hp)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(spec)
    sd = synth_state_dict(spec)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(gpu_device).eval()
    d = gpu_device
    kw = {"condition": T(g[name + "_cond"], d)} if name == "concat_partial" else {}
    y = net(T(g[name + "_x"], d), ts=T(g[name + "_ts"], d), label=T(g[name + "_label"], d), **kw).cpu().numpy()
    ref = g[name + "_eps"]
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print("switches %s: output %s, max-norm error vs reference %.2e" % (name, y.shape, err))
    assert y.shape == ref.shape and err <= 2e-4, (name, err)


def test_encoder_parent_project_switches_match_reference(gpu_device):
    """PointNet2Encoder (the autoencoder's encoder class, reference pointnet2_feature_extractor.py:25-218) with swish, position
    encoding, bn_first and global attention behind level 0 (128 -> 64 -> 16 points with FPS) against the reference's forward
    (golden_encoder_switches.npz, tools/gen_golden.py `--only switches`): FPS selections bit-equal, features <= 2e-4."""
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.pointnet2_feature_extractor import PointNet2Encoder
    g = load_golden("golden_encoder_switches.npz")
    hp = json.loads(str(g["config_json"]))
    spec = golden_spec(g)
    net = PointNet2Encoder(hp)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(spec)
    sd = synth_state_dict(spec)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(gpu_device).eval()
    y, l_xyz, _ = net(T(g["pointcloud"], gpu_device), ts=None, label=T(g["label"], gpu_device))
    assert np.array_equal(l_xyz[-1].cpu().numpy(), g["xyz_last"])
    err = np.abs(y.cpu().numpy() - g["out"]).max() / np.abs(g["out"]).max()
    print("encoder switches: max-norm error vs reference %.2e" % err)
    assert err <= 2e-4, err


def test_autoencoder_decode_matches_reference(gpu_device):
    """config 5: latents -> 256 -> 1024 -> 2048 x 6 on the HIP module path vs the reference's decode (FPS start index 0)."""
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.autoencoder import PointAutoencoder
    from oracle import denoiser_np as D
    g = load_golden("golden_decode.npz")
    decs = json.loads(str(g["decoder_configs_json"]))
    spec = golden_spec(g)
    ae = PointAutoencoder(None, decs, apply_kl_regularization=True)
    assert {k: tuple(v.shape) for k, v in ae.state_dict().items()} == dict(spec)  # decode-side checkpoint compatibility
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])
    ae.load_state_dict({n: torch.from_numpy(vals["ae." + n]) for n, _ in spec})
    ae = ae.to(gpu_device).eval()
    d = gpu_device
    kp, feat, lab = T(g["keypoint"], d), T(g["feature"], d), T(g["label"], d)
    B = kp.shape[0]
    start = torch.zeros(B, dtype=torch.int32, device=d)
    l1 = ae.keypoint_encoder.upsample_points(feat, kp, start)
    assert np.abs(l1.cpu().numpy() - g["level1"]).max() <= 1e-5
    # level by level, each fed with the reference's previous level (FPS selection order is perturbation-fragile)
    f2, l2 = ae.decoder.decoders[0](kp, feat, T(g["level1"], d), label=lab, fps_start_idx=start)
    f3, l3 = ae.decoder.decoders[1](T(g["level1"], d)[:, :, :3].contiguous(), f2, T(g["level2"], d), label=lab, fps_start_idx=start)
    for b in range(B):
        err, bij = D.match_point_sets(l2[b].cpu().numpy(), g["level2"][b])
        assert bij and err <= 1e-4, ("level2", err)
        err, bij = D.match_point_sets(l3[b].cpu().numpy(), g["level3"][b])
        assert bij and err <= 1e-4, ("level3", err)
    # end to end (own previous levels, own FPS order): Chamfer vs the reference cloud
    full = ae.decode(kp, feat, label=lab, fps_start_idx=start).cpu().numpy()
    assert full.shape == (B, 2048, 6)
    cd = max(D.chamfer(full[b], g["level3"][b]) for b in range(B))
    print("decode end-to-end Chamfer (sum of both directions, squared) vs reference: %.3e" % cd)
    assert cd <= 1e-5
    # random-start variant runs and stays on the same surface
    full_r = ae.decode(kp, feat, label=lab).cpu().numpy()
    assert max(D.chamfer(full_r[b], g["level3"][b]) for b in range(B)) <= 1e-3


def test_autoencoder_decode_fp16_operands_matches_reference(gpu_device, monkeypatch):
    """The TIMED decode arithmetic (bench.py's decode leg and the generation CLIs' default `--prec mixed`: SLIDE_MODULE_PREC=fp16 =
    fp16 MFMA operands, fp32 accumulation / GroupNorm statistics / soft-max) against the reference's decode of the same latents
    (golden_decode.npz, FPS start index 0; reference: pointnet2/models/autoencoder.py:42-45,
    point_upsample_decoder.py:184-190).  A decoder level is [feature extractor -> upsampling to 2x the points -> plain FPS down to
    the level's size].  The FPS step selects a SUBSET of the upsampled candidates and a 1e-3 perturbation of the candidates can
    change which near-equidistant candidate is picked, so at this precision the selected sets are not compared point for point
    (the fp32 module mode is: test_autoencoder_decode_matches_reference).  What is asserted, per level, each level fed with the
    reference's previous level:
      * every point the REFERENCE selected has one of this path's upsampled CANDIDATES (the tensor handed to the FPS kernel)
        within DECODE_FP16_LEVEL_TOL in all six channels (nearest by xyz) -- the arithmetic of the level, FPS taken out;
      * the level's selected cloud has Chamfer distance <= DECODE_FP16_CHAMFER_TOL to the reference's level;
    and end to end (own previous levels, own FPS order): Chamfer <= DECODE_FP16_CHAMFER_TOL to the reference cloud (sum of both
    directions, mean squared distances; the clouds span [-1, 1]^3)."""
    monkeypatch.setenv("SLIDE_MODULE_PREC", "fp16")
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models import point_upsample_decoder as PUD
    from models.autoencoder import PointAutoencoder
    from oracle import denoiser_np as D
    g = load_golden("golden_decode.npz")
    decs = json.loads(str(g["decoder_configs_json"]))
    spec = golden_spec(g)
    ae = PointAutoencoder(None, decs, apply_kl_regularization=True)
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])
    ae.load_state_dict({n: torch.from_numpy(vals["ae." + n]) for n, _ in spec})
    ae = ae.to(gpu_device).eval()
    d = gpu_device
    kp, feat, lab = T(g["keypoint"], d), T(g["feature"], d), T(g["label"], d)
    B = kp.shape[0]
    start = torch.zeros(B, dtype=torch.int32, device=d)
    cands = []
    real_fps = PUD._hip.sample_farthest_points

    def recording_fps(pts, *a, **k):  # the candidates of every plain-FPS call, in call order
        cands.append(pts.detach().cpu().numpy())
        return real_fps(pts, *a, **k)

    monkeypatch.setattr(PUD._hip, "sample_farthest_points", recording_fps)
    l1 = ae.keypoint_encoder.upsample_points(feat, kp, start)
    f2, l2 = ae.decoder.decoders[0](kp, feat, T(g["level1"], d), label=lab, fps_start_idx=start)
    f3, l3 = ae.decoder.decoders[1](T(g["level1"], d)[:, :, :3].contiguous(), f2, T(g["level2"], d), label=lab, fps_start_idx=start)
    assert len(cands) == 3
    worst_lvl = worst_cd = 0.0
    for name, own, cand in (("level1", l1, cands[0]), ("level2", l2, cands[1]), ("level3", l3, cands[2])):
        ref = g[name]
        assert cand.shape[1] >= ref.shape[1] and own.shape == ref.shape
        e = max(D.match_point_sets(ref[b], cand[b])[0] for b in range(B))       # reference selections -> own candidates
        cd = max(D.chamfer(own[b].cpu().numpy(), ref[b]) for b in range(B))
        same = sum(D.match_point_sets(own[b].cpu().numpy(), ref[b])[1] for b in range(B))
        print("fp16-operand decode, %s: reference points -> own candidates max %.3e; Chamfer of the selected cloud %.3e; "
              "selected SET identical for %d of %d shapes" % (name, e, cd, same, B))
        worst_lvl, worst_cd = max(worst_lvl, e), max(worst_cd, cd)
    monkeypatch.setattr(PUD._hip, "sample_farthest_points", real_fps)
    full = ae.decode(kp, feat, label=lab, fps_start_idx=start).cpu().numpy()
    assert full.shape == (B, 2048, 6) and np.isfinite(full).all()
    cd = max(D.chamfer(full[b], g["level3"][b]) for b in range(B))
    print("fp16-operand decode end to end: Chamfer vs the reference cloud %.3e" % cd)
    assert worst_lvl <= DECODE_FP16_LEVEL_TOL, worst_lvl
    assert max(worst_cd, cd) <= DECODE_FP16_CHAMFER_TOL, (worst_cd, cd)


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_decode_of_a_shape_does_not_depend_on_its_batch(gpu_device, monkeypatch, prec):
    """BASELINE configs[4] shards the decode over ranks and batches: a shape's cloud must not depend on the batch it is decoded in
    (the reference decodes per rank, mesh_evaluation.py:113-118; the CLI test compares one rank with two bit for bit).  Seven shapes at
    once against the same shapes as batches of 3, 3 and 1 -- small batches, where samples straddle row tiles and the query side of the
    split q / k attention takes its statistics outside the GEMM epilogue -- over several latent sets: bit-identical, both module
    precisions.  (Round 6: torch.sum's batch-dependent reduction order there turned into re-ordered clouds through FPS near-ties.)"""
    monkeypatch.setenv("SLIDE_MODULE_PREC", prec)
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.autoencoder import PointAutoencoder
    from slide_amd.synth import synth_keypoints
    g = load_golden("golden_decode.npz")
    decs = json.loads(str(g["decoder_configs_json"]))
    spec = golden_spec(g)
    ae = PointAutoencoder(None, decs, apply_kl_regularization=True)
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])
    ae.load_state_dict({n: torch.from_numpy(vals["ae." + n]) for n, _ in spec})
    ae = ae.to(gpu_device).eval()
    d = gpu_device
    B = 7
    for seed in range(4 if prec == "fp16" else 1):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        kp = torch.from_numpy(synth_keypoints(B)).float() + 0.01 * torch.randn(B, 16, 3, generator=gen)
        feat = 0.5 * torch.randn(B, 16, 48, generator=gen)
        kp, feat = kp.to(d), feat.to(d)
        lab = torch.zeros(B, dtype=torch.long, device=d)
        start = torch.zeros(B, dtype=torch.int32, device=d)
        ref = ae.decode(kp, feat, label=lab, fps_start_idx=start)
        parts = torch.cat([ae.decode(kp[a:b], feat[a:b], label=lab[a:b], fps_start_idx=start[a:b]) for a, b in ((0, 3), (3, 6), (6, 7))])
        assert ref.shape == (B, 2048, 6) and torch.isfinite(ref).all()
        assert torch.equal(parts, ref), (prec, seed, (parts - ref).abs().flatten(1).max(1).values.tolist())


def test_autoencoder_encode_matches_reference(gpu_device):
    """2048 x 6 cloud -> PointNet2Encoder (FPS 1024/256/64/32, kNN-32 SA stack) -> key-point encoder ->
    (B,16,48) latent features, HIP module path vs the reference's `PointAutoencoder.encode` (posterior mode).  FPS runs on
    the INPUT coordinates only, so the selected points are bit-exact and the features compare element-wise."""
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.autoencoder import PointAutoencoder
    g = load_golden("golden_encode.npz")
    enc, decs = json.loads(str(g["encoder_config_json"])), json.loads(str(g["decoder_configs_json"]))
    spec = golden_spec(g)
    ae = PointAutoencoder(enc, decs, apply_kl_regularization=True)
    have = {k: tuple(v.shape) for k, v in ae.state_dict().items()}
    assert {k: v for k, v in have.items() if k.startswith(("encoder.", "keypoint_encoder."))} == dict(spec)  # checkpoint keys
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])
    ae.load_state_dict({n: torch.from_numpy(vals["ae." + n]) for n, _ in spec}, strict=False)
    ae = ae.to(gpu_device).eval()
    d = gpu_device
    pc, kp, lab = T(g["pointcloud"], d), T(g["keypoint"], d), T(g["label"], d)
    out, l_xyz, _ = ae.encoder(pc, ts=None, label=lab)
    assert np.array_equal(l_xyz[-1].cpu().numpy(), g["encoder_xyz_last"])  # four FPS levels, bit-exact selections
    ref = g["encoder_out"]
    assert np.abs(out.cpu().numpy() - ref).max() <= 2e-4 * np.abs(ref).max()
    feat = ae.encode(pc, kp, ts=None, label=lab, sample_posterior=False).cpu().numpy()
    ref = g["feature_at_keypoint"]
    assert feat.shape == ref.shape == (pc.shape[0], 16, 48)
    assert np.abs(feat - ref).max() <= 2e-4 * np.abs(ref).max(), np.abs(feat - ref).max()
    # the sampled posterior differs from the mode by std * N(0,1) only
    fs = ae.encode(pc, kp, ts=None, label=lab, sample_posterior=True).cpu().numpy()
    assert np.isfinite(fs).all() and fs.shape == ref.shape
    # encode -> decode round trip runs end to end on the module path
    rec = ae.decode(kp, T(feat, d), label=lab, fps_start_idx=torch.zeros(pc.shape[0], dtype=torch.int32, device=d))
    assert rec.shape == (pc.shape[0], 2048, 6) and bool(torch.isfinite(rec).all())


def test_module_path_fp16_operands(gpu_device, monkeypatch):
    """SLIDE_MODULE_PREC=fp16 (throughput mode of the module-level path: fp16 GEMM operands, fp32 accumulate / outputs):
    encode within 5e-3 relative L2 of the reference, FPS selections unchanged (they depend on the input coordinates only)."""
    monkeypatch.setenv("SLIDE_MODULE_PREC", "fp16")
    sys.path.insert(0, os.path.join(REPO, "pointnet2"))
    from models.autoencoder import PointAutoencoder
    g = load_golden("golden_encode.npz")
    enc, decs = json.loads(str(g["encoder_config_json"])), json.loads(str(g["decoder_configs_json"]))
    spec = golden_spec(g)
    ae = PointAutoencoder(enc, decs, apply_kl_regularization=True)
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])
    ae.load_state_dict({n: torch.from_numpy(vals["ae." + n]) for n, _ in spec}, strict=False)
    ae = ae.to(gpu_device).eval()
    d = gpu_device
    pc, kp, lab = T(g["pointcloud"], d), T(g["keypoint"], d), T(g["label"], d)
    out, l_xyz, _ = ae.encoder(pc, ts=None, label=lab)
    assert np.array_equal(l_xyz[-1].cpu().numpy(), g["encoder_xyz_last"])
    feat = ae.encode(pc, kp, ts=None, label=lab, sample_posterior=False).cpu().numpy()
    ref = g["feature_at_keypoint"]
    rel = float(np.linalg.norm(feat - ref) / np.linalg.norm(ref))
    assert rel <= 5e-3, rel


def test_sample_farthest_points(gpu_device):
    from oracle import ops as O
    from slide_amd import _ext
    rs = np.random.RandomState(4)
    for (B, n, K) in [(2, 512, 256), (3, 2048, 1024), (1, 4096, 2048), (2, 100, 100)]:
        p = rs.uniform(-1, 1, (B, n, 6)).astype(np.float32)
        p[:, 5] = p[:, 1]
        start = rs.randint(0, n, B).astype(np.int32)
        ro, ri = O.sample_farthest_points(p, K, start)
        go, gi = _ext.sample_farthest_points(T(p, gpu_device), K=K, start_idx=torch.from_numpy(start))
        assert np.array_equal(gi.cpu().numpy(), ri) and np.array_equal(go.cpu().numpy(), ro)


def _randomise(m, dev, seed=11):
    g2 = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g2) * (0.3 if p.dim() > 1 else 0.5) + (1.0 if n.endswith("group_norm.weight") else 0.0))
    return m.to(dev).eval()


def _sd(m, prefix):
    return {prefix + "." + k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_row_major_modules_against_the_oracle(gpu_device, monkeypatch, prec):
    """The row-major module programs (slide_amd.rows kernels + MFMA GEMMs) vs the numpy restatement of the reference
    modules (oracle/denoiser_np.py) on random weights: multi-scale grouping, fewer points than npoint (no FPS), odd channel
    counts (pad columns, un-normalised GroupNorm tail channels), 48 neighbours, kNN feature propagation with skip features,
    the autoencoder's feature mapper."""
    from oracle import denoiser_np as O
    from pointnet2_ops import pointnet2_modules as PM
    monkeypatch.setenv("SLIDE_MODULE_PREC", prec)
    # fp16 rows: measured worst |got - oracle| / (1 + |oracle|) over the four module programs 7.3e-3 (printed below); the tolerance is
    # twice that (the margin is for another seed's draw).  It was 4e-2 until the row ops had references of their own
    # (tests/test_hip_rows_arith.py).
    tol = dict(atol=3e-4, rtol=2e-4) if prec == "fp32" else dict(atol=1.46e-2, rtol=1.46e-2)
    d = gpu_device
    gen = torch.Generator().manual_seed(5)
    B, N, C = 3, 200, 13
    xyz = torch.rand(B, N, 3, generator=gen)
    feats = torch.randn(B, C, N, generator=gen)
    temb, cemb = torch.randn(B, 24, generator=gen), torch.randn(B, 10, generator=gen)
    npy = lambda t: t.detach().cpu().numpy()
    att = {"use_attention_module": True, "attention_bn": True, "transform_grouped_feat_out": True, "last_activation": True}

    worst = [0.0]

    def close(a, b):
        # allclose with atol == rtol == t asks |a - b| <= t (1 + |b|): the measured figure is the largest |a - b| / (1 + |b|)
        worst[0] = max(worst[0], float((np.abs(a - b) / (1 + np.abs(b))).max()))
        assert a.shape == b.shape and np.allclose(a, b, **tol), float(np.abs(a - b).max())

    # two scales (5 and 48 neighbours), t and class embeddings, res_connect through a convolution
    sa = _randomise(PM.PointnetSAModuleMSG(npoint=50, radii=[0, 0], nsamples=[5, 48], mlps=[[C, 20, 20, 45], [C, 16, 24, 33]],
                                           bn=True, use_xyz=True, t_dim=24, include_t=True, include_abs_coordinate=True,
                                           include_center_coordinate=True, bias=True, res_connect=True, include_condition=True,
                                           condition_dim=10, neighbor_def="nn", attention_setting=att), d)
    nx, nf = sa(xyz.to(d), feats.to(d), t_emb=temb.to(d), condition_emb=cemb.to(d))
    sd = _sd(sa, "sa")
    from oracle import ops as oops
    fidx = oops.furthest_point_sampling(npy(xyz), 50)
    ctr = np.ascontiguousarray(oops.gather_points(np.ascontiguousarray(npy(xyz).transpose(0, 2, 1)), fidx).transpose(0, 2, 1))
    q = oops.gather_points(npy(feats), fidx)
    want = []
    for i, K in enumerate((5, 48)):
        grouped, _, _ = O.query_and_group_nn(npy(xyz), ctr, npy(feats), K)
        h = O.mlp_plus_t_emb(grouped, sd, "sa.mlps.%d" % i, npy(temb), npy(cemb))
        want.append(O.attention_module(q, grouped, h, sd, "sa.attention_modules.%d" % i))
    assert np.array_equal(npy(nx), ctr)
    close(npy(nf), np.concatenate(want, axis=1))
    # fewer points than npoint: every point is a centre, the queries are the input features; identity res_connect
    sa = _randomise(PM.PointnetSAModule(mlp=[C, 16, 16, C + 9], npoint=512, radius=0, nsample=16, bn=True, use_xyz=True,
                                        include_t=False, include_abs_coordinate=True, include_center_coordinate=True, bias=False,
                                        res_connect=True, neighbor_def="nn", attention_setting=att), d)
    nx, nf = sa(xyz.to(d), feats.to(d))
    wx, wf = O.sa_module(npy(xyz), npy(feats), _sd(sa, "sa"), "sa", 512, 16, None, None)
    assert nx.shape == (B, N, 3)
    close(npy(nf), wf)
    # kNN feature propagation: 40 known points -> 200 unknown points, skip features, t / class embeddings
    known, kf = xyz[:, :40].contiguous(), torch.randn(B, 21, 40, generator=gen)
    fp = _randomise(PM.PointnetKnnFPModule(mlp1=[21, 24, 24, 30], mlp2=[30 + C, 36, 36], K=7, bn=True, t_dim=24, include_t=True,
                                           bias=True, res_connect=True, include_condition=True, condition_dim=10,
                                           attention_setting=att), d)
    out = fp(xyz.to(d), known.to(d), feats.to(d), kf.to(d), t_emb=temb.to(d), condition_emb=cemb.to(d))
    close(npy(out), O.knn_fp_module(npy(xyz), npy(known), npy(feats), npy(kf), _sd(fp, "fp"), "fp", 7, npy(temb), npy(cemb)))
    # feature mapper of the autoencoder: features of 200 points mapped onto 16 key points
    fm = _randomise(PM.FeatureMapModule([C, 32, 32, 48], 0, 12, use_xyz=True, include_abs_coordinate=True,
                                        include_center_coordinate=True, bn=True, bn_first=False, bias=True, res_connect=True,
                                        neighbor_def="nn", attention_setting=att, query_feature_dim=19), d)
    keypts, qf = xyz[:, 100:116].contiguous(), torch.randn(B, 19, 16, generator=gen)
    out = fm(xyz.to(d), feats.to(d), keypts.to(d), subset=False, record_neighbor_stats=True, features_at_new_xyz=qf.to(d))
    close(npy(out), O.feature_map_module(npy(xyz), npy(feats), npy(keypts), npy(qf), _sd(fm, "fm"), "fm", 12))
    assert float(fm.mapper.neighbor_stats[0]) == 12.0
    print("row-major modules %s: worst |got - oracle| / (1 + |oracle|) %.3e (tolerance %.1e)" % (prec, worst[0], tol["atol"]))


def test_general_module_programs_against_torch(gpu_device):
    """What the stage interpreter does not cover -- GroupNorm BEFORE the convolution, swish, pooling instead of attention,
    ball-query grouping with partially filled balls -- against a plain PyTorch fp32 restatement of the same arithmetic."""
    import torch.nn.functional as F
    from pointnet2_ops import pointnet2_modules as PM
    from pointnet2_ops import pointnet2_utils as PU
    d = gpu_device
    gen = torch.Generator().manual_seed(9)
    B, N, C, npnt, K = 2, 96, 10, 24, 12
    xyz = torch.rand(B, N, 3, generator=gen)
    feats = torch.randn(B, C, N, generator=gen)
    temb = torch.randn(B, 16, generator=gen)
    cpu = lambda t: t.detach().cpu()

    def gn(x, m):  # MyGroupNorm on a CPU tensor: tail channels pass through
        n = m.num_channels
        y = F.group_norm(x[:, :n], m.num_groups, cpu(m.group_norm.weight), cpu(m.group_norm.bias), 1e-5)
        return torch.cat([y, x[:, n:]], dim=1)

    def seq(s, x):
        for l in s:
            if isinstance(l, PM.MyGroupNorm):
                x = gn(x, l)
                x = F.relu(x) if l.fused_relu else x
            elif isinstance(l, PM.HipConv1x1):
                x = F.conv2d(x, cpu(l.weight), None if l.bias is None else cpu(l.bias))
            elif isinstance(l, PM.Swish):
                x = x * torch.sigmoid(x)
            elif isinstance(l, torch.nn.ReLU):
                x = F.relu(x)
        return x

    def mlp_ref(m, x, t):
        h = seq(m.first_mlp, x)
        if m.include_t:
            h = h + F.linear(t, cpu(m.fc.weight), cpu(m.fc.bias))[:, :, None, None]
        h = seq(m.second_mlp, h)
        if m.rest_mlp is not None:
            h = seq(m.rest_mlp, h)
        if m.res_connect_bool:
            h = h + (F.conv2d(x, cpu(m.res_connect.weight), cpu(m.res_connect.bias)) if m.res_connect is not None else x)
        return h

    for bn_first, activation, pooling in ((True, "swish", "max"), (False, "relu", "avg"), (True, "relu", "avg_max")):
        sa = _randomise(PM.PointnetSAModule(mlp=[C, 16, 24, 30], npoint=npnt, radius=0.35, nsample=K, bn=True, use_xyz=True, t_dim=16,
                                            include_t=True, include_abs_coordinate=True, bn_first=bn_first, bias=True,
                                            res_connect=True, neighbor_def="radius", activation=activation), d)
        assert sa.mlps[0].rows_ok() == (not bn_first and activation == "relu")
        nx, nf = sa(xyz.to(d), feats.to(d), t_emb=temb.to(d), pooling=pooling)
        grouped, counts = PU.QueryAndGroup(0.35, K, True, True, False, "radius")(xyz.to(d), nx, feats.to(d), return_counts=True)
        counts = cpu(counts).long()
        assert counts.min() < K and counts.max() == K  # partially filled balls are part of the case
        h = mlp_ref(sa.mlps[0], cpu(grouped), temb)
        mask = (torch.arange(K)[None, None, :] < counts.clamp(min=1)[:, :, None])[:, None].float()
        avg = (h * mask).sum(-1) / counts.clamp(min=1)[:, None].float()
        mx = h.max(dim=-1)[0]
        half_c = h.shape[1] // 2
        want = {"max": mx, "avg": avg, "avg_max": torch.cat([mx[:, :half_c], avg[:, half_c:]], dim=1)}[pooling]
        assert torch.allclose(cpu(nf), want, atol=3e-4, rtol=2e-4), (bn_first, activation, pooling, float((cpu(nf) - want).abs().max()))


def test_empty_batch_flows_through_the_modules(gpu_device):
    """B = 0 (the short last rank of a sharded run can be empty): every kernel launch is skipped, shapes are kept"""
    from pointnet2_ops import pointnet2_modules as PM
    att = {"use_attention_module": True, "attention_bn": True, "transform_grouped_feat_out": True, "last_activation": True}
    d = gpu_device
    sa = _randomise(PM.PointnetSAModule(mlp=[5, 16, 16, 32], npoint=8, radius=0, nsample=4, bn=True, use_xyz=True,
                                        include_abs_coordinate=True, bias=True, res_connect=True, neighbor_def="nn",
                                        attention_setting=att), d)
    nx, nf = sa(torch.zeros(0, 20, 3, device=d), torch.zeros(0, 5, 20, device=d))
    assert nx.shape == (0, 8, 3) and nf.shape == (0, 32, 8)
    fp = _randomise(PM.PointnetKnnFPModule(mlp1=[32, 16, 16], mlp2=[16 + 5, 16, 16], K=3, bn=True, bias=True, res_connect=True,
                                           attention_setting=att), d)
    out = fp(torch.zeros(0, 20, 3, device=d), nx, torch.zeros(0, 5, 20, device=d), nf)
    assert out.shape == (0, 16, 20)


def test_rows_conv_plan_follows_bias_updates(gpu_device):
    """The row-major path packs a convolution's weight AND bias once per parameter version (rows.conv's plan cache): an
    in-place update of the bias alone (an optimiser step, an EMA copy_) must re-pack -- the key carries the bias' version
    and storage and the device."""
    from pointnet2_ops import pointnet2_modules as PM
    from slide_amd import rows as R
    d = gpu_device
    conv = PM.HipConv1x1(40, 24, bias=True).to(d)
    x = torch.randn(2, 40, 64, 1, device=d)
    want = lambda: torch.nn.functional.conv2d(x, conv.weight, conv.bias)
    y0 = R.to_ncx(R.conv(R.from_ncx(x, half=False), conv), spatial=(64, 1))
    assert torch.allclose(y0, want(), atol=1e-4, rtol=1e-4)
    with torch.no_grad():
        conv.bias.add_(3.0)
    y1 = R.to_ncx(R.conv(R.from_ncx(x, half=False), conv), spatial=(64, 1))
    assert torch.allclose(y1, want(), atol=1e-4, rtol=1e-4) and float((y1 - y0).mean()) > 2.9
    with torch.no_grad():
        conv.weight.mul_(0.5)
    y2 = R.to_ncx(R.conv(R.from_ncx(x, half=False), conv), spatial=(64, 1))
    assert torch.allclose(y2, want(), atol=1e-4, rtol=1e-4)
    # the NCHW tensor-program path (HipConv1x1.forward / HipLinear.forward) caches a packed plan the same way
    with torch.no_grad():
        conv.bias.sub_(1.5)
    assert torch.allclose(conv(x), want(), atol=1e-4, rtol=1e-4)
    lin = PM.HipLinear(12, 20).to(d)
    z = torch.randn(5, 12, device=d)
    a0 = lin(z).clone()
    with torch.no_grad():
        lin.bias.add_(2.0)
    assert torch.allclose(lin(z), torch.nn.functional.linear(z, lin.weight, lin.bias), atol=1e-4, rtol=1e-4)
    assert float((lin(z) - a0).mean()) > 1.9


@pytest.mark.parametrize("npnt,K", [(256, 8), (64, 32), (16, 16)])
def test_attention_without_the_concatenation(gpu_device, monkeypatch, npnt, K):
    """round 5, fp16 module path: AttentionModule evaluates relu(weight_conv.2(GN(relu([q | k])))) WITHOUT building the concatenation --
    joint GroupNorm statistics from the two producers' GEMM epilogues (SLIDE_OP_ROWS_GN_JOINT, groups straddling the q / k boundary
    included: C1 = 48 of 32 groups over 112 channels), the q half of weight_conv.2 once per point and added ahead of the ReLU.  Same
    layer as the three-pass form (SLIDE_MODULE_SPLIT_QK=0) up to fp16 operand rounding (<= 3e-3 relative L2), both within 6e-3 of an
    fp64 restatement; ball-query counts (masked slots) take the same path.  Levels with fewer points than one 256-row tile per sample
    (npnt = 64 / 16) take the q side's sums from small elementwise passes instead of the GEMM epilogue."""
    from pointnet2_ops.attention import AttentionModule
    monkeypatch.setenv("SLIDE_MODULE_PREC", "fp16")
    d = gpu_device
    B, Cq, Cg, Cout = 2, 40, 70, 96
    am = _randomise(AttentionModule(Cq, Cg, 48, 64, Cout), d, seed=5)
    gen = torch.Generator().manual_seed(9)
    feat = torch.randn(B, Cq, npnt, generator=gen).to(d)
    gfeat = torch.randn(B, Cg, npnt, K, generator=gen).to(d)
    gout = torch.randn(B, Cout, npnt, K, generator=gen).to(d)
    count = torch.randint(0, K + 1, (B, npnt), generator=gen).to(d)
    for cnt in ("all", count):
        outs = {}
        for v in ("1", "0"):
            monkeypatch.setenv("SLIDE_MODULE_SPLIT_QK", v)
            outs[v] = am(feat, gfeat, gout, cnt).double()
        # fp64 restatement of attention.py:70-96
        gn = lambda x, m: torch.cat([torch.nn.functional.group_norm(x[:, :m.num_channels], m.num_groups, m.group_norm.weight.double(),
                                                                     m.group_norm.bias.double(), 1e-5), x[:, m.num_channels:]], 1)
        c2 = lambda x, m: torch.nn.functional.conv2d(x, m.weight.double(), m.bias.double())
        q = c2(feat.double()[..., None], am.feat_conv).expand(-1, -1, -1, K)
        k = c2(gfeat.double(), am.grouped_feat_conv)
        wc = list(am.weight_conv)
        u = c2(gn(torch.cat([q, k], 1).relu(), wc[1]), wc[2])
        sc = c2(gn(u.relu(), wc[4]), wc[5])
        fo = list(am.feat_out_conv)
        val = gn(c2(gout.double(), fo[0]), fo[1]).relu()
        if not isinstance(cnt, str):
            mask = (torch.arange(K, device=d)[None, None, :] < cnt.clamp(min=1)[..., None]).double()[:, None]
            sc = sc * mask + (-1e9) * (1 - mask)
        ref = (torch.softmax(sc, dim=-1) * val).sum(-1)
        rel = lambda a, b: float(((a - b).norm() / b.norm()).detach())
        assert torch.isfinite(outs["1"]).all() and rel(outs["1"], outs["0"]) <= 3e-3, rel(outs["1"], outs["0"])
        assert rel(outs["1"], ref) <= 6e-3 and rel(outs["0"], ref) <= 6e-3, (rel(outs["1"], ref), rel(outs["0"], ref))


@pytest.mark.parametrize("npnt,K", [(64, 4), (32, 8), (64, 16), (16, 32), (256, 32)])
def test_attention_fused_score_gemm_and_attend(gpu_device, monkeypatch, npnt, K):
    """round 6, fp16 module path: the score convolution of an AttentionModule, the soft-max over the K neighbours and the weighted sum
    of the values as ONE launch (SLIDE_OP_GEMM_ATTEND: the score map stays in the accumulators) against the two-launch form
    (SLIDE_MODULE_FUSE_ATTEND=0: scores stored in fp16, rows_attn_kernel) and an fp64 restatement of attention.py:70-96, with and
    without ball-query counts.  The fused form soft-maxes fp32 scores, the two-launch form fp16-rounded ones: they agree to <= 3e-3
    relative L2 and the fused form is not further from the restatement than the two-launch form (+ 10 %).
    (The launch itself, elementwise against float64 at every argument form: tests/test_hip_attend.py.)"""
    from pointnet2_ops.attention import AttentionModule
    monkeypatch.setenv("SLIDE_MODULE_PREC", "fp16")
    d = gpu_device
    B, Cq, Cg, Cout = 2, 40, 70, 96
    am = _randomise(AttentionModule(Cq, Cg, 48, 64, Cout), d, seed=6)
    gen = torch.Generator().manual_seed(10 + K)
    feat = torch.randn(B, Cq, npnt, generator=gen).to(d)
    gfeat = torch.randn(B, Cg, npnt, K, generator=gen).to(d)
    gout = torch.randn(B, Cout, npnt, K, generator=gen).to(d)
    count = torch.randint(0, K + 1, (B, npnt), generator=gen).to(d)
    from slide_amd import rows as R
    launched = []
    real_run = R._run
    monkeypatch.setattr(R, "_run", lambda op: (launched.append(op.kind), real_run(op))[1])
    for cnt in ("all", count):
        outs = {}
        for v in ("1", "0"):
            monkeypatch.setenv("SLIDE_MODULE_FUSE_ATTEND", v)
            del launched[:]
            outs[v] = am(feat, gfeat, gout, cnt).double()
            fusable = (npnt * K) % 256 == 0
            assert (R.OP_GEMM_ATTEND in launched) == (v == "1" and fusable) and (R.OP_ROWS_ATTN in launched) == (v == "0" or not fusable), launched
        gn = lambda x, m: torch.cat([torch.nn.functional.group_norm(x[:, :m.num_channels], m.num_groups, m.group_norm.weight.double(),
                                                                     m.group_norm.bias.double(), 1e-5), x[:, m.num_channels:]], 1)
        c2 = lambda x, m: torch.nn.functional.conv2d(x, m.weight.double(), m.bias.double())
        q = c2(feat.double()[..., None], am.feat_conv).expand(-1, -1, -1, K)
        k = c2(gfeat.double(), am.grouped_feat_conv)
        wc = list(am.weight_conv)
        u = c2(gn(torch.cat([q, k], 1).relu(), wc[1]), wc[2])
        sc = c2(gn(u.relu(), wc[4]), wc[5])
        fo = list(am.feat_out_conv)
        val = gn(c2(gout.double(), fo[0]), fo[1]).relu()
        if not isinstance(cnt, str):
            mask = (torch.arange(K, device=d)[None, None, :] < cnt.clamp(min=1)[..., None]).double()[:, None]
            sc = sc * mask + (-1e9) * (1 - mask)
        ref = (torch.softmax(sc, dim=-1) * val).sum(-1)
        rel = lambda a, b: float(((a - b).norm() / b.norm()).detach())
        assert torch.isfinite(outs["1"]).all() and rel(outs["1"], outs["0"]) <= 3e-3, rel(outs["1"], outs["0"])
        assert rel(outs["1"], ref) <= 6e-3 and rel(outs["1"], ref) <= 1.1 * rel(outs["0"], ref) + 1e-4, (rel(outs["1"], ref), rel(outs["0"], ref))


@pytest.mark.parametrize("layout", ["sa", "sa_abs_ctr", "fp", "xyz_only"])
def test_pair_decomposition_of_the_module_path(gpu_device, monkeypatch, layout):
    """round 6, fp16 module path: a 1 x 1 convolution over a GROUPED input evaluated without the grouped matrix (slide_amd.rows.LazyGroup /
    _pair_conv, SLIDE_OP_ROWS_PAIR_EXPAND: per-source-point feature table + fp32 coordinate terms) against the materialised form
    (SLIDE_MODULE_PAIR=0: grouping kernel + GEMM) and an fp64 restatement of conv(QueryAndGroup / group_knn) (reference
    pointnet2_utils.py:383-430, :497-524): raw / ReLU'd outputs, the per-tile channel sums handed to the following GroupNorm, cross-set
    grouping (centres != sources), ragged last tile.  The pair form evaluates the coordinate channels in fp32 where the grouped matrix
    held them in fp16: it is at least as close to the restatement as the materialised form."""
    from slide_amd import rows as R
    from slide_amd.nn_ops import HipConv1x1
    monkeypatch.setenv("SLIDE_MODULE_PREC", "fp16")
    d = gpu_device
    gen = torch.Generator().manual_seed(21)
    B, N, npnt, K, C, O = 3, 200, 72, 8, (0 if layout == "xyz_only" else 45), 70
    xyz = torch.rand(B, N, 3, generator=gen).to(d) * 2 - 1
    ctr = (torch.rand(B, npnt, 3, generator=gen).to(d) * 2 - 1) if layout != "sa" else xyz[:, :npnt].contiguous()
    feat = torch.randn(B, C, N, generator=gen).to(d) if C else None
    idx = torch.randint(0, N, (B, npnt, K), generator=gen).to(d)
    flags = {"sa": 0, "sa_abs_ctr": R.GROUP_ABS | R.GROUP_CENTER, "fp": R.GROUP_FP, "xyz_only": R.GROUP_ABS}[layout]
    d2 = (torch.rand(B, npnt, K, generator=gen).to(d) * 0.5 + 1e-3) if layout == "fp" else None
    ncoord = 11 if layout == "fp" else 3 + (3 if flags & R.GROUP_ABS else 0) + (3 if flags & R.GROUP_CENTER else 0)
    conv = _randomise(HipConv1x1(C + ncoord, O), d, seed=3)
    # fp64 restatement
    q = torch.gather(xyz.double(), 1, idx.reshape(B, -1, 1).expand(-1, -1, 3)).reshape(B, npnt, K, 3)
    c = ctr.double()[:, :, None, :].expand(-1, -1, K, -1)
    parts = []
    if C:
        parts.append(torch.gather(feat.double().transpose(1, 2), 1, idx.reshape(B, -1, 1).expand(-1, -1, C)).reshape(B, npnt, K, C))
    if layout == "fp":
        w = 1.0 / (d2.double() + 1e-8)
        parts += [d2.double()[..., None], (w / w.sum(-1, keepdim=True))[..., None], q, q - c, c]
    else:
        parts.append(q - c)
        if flags & R.GROUP_ABS:
            parts.append(q)
        if flags & R.GROUP_CENTER:
            parts.append(c)
    g = torch.cat(parts, -1)
    W = conv.weight.double().reshape(O, -1)
    ref = g @ W.T + conv.bias.double()
    rel = lambda a, b: float(((a - b).norm() / b.norm()).detach())
    for stats in (None, "raw", "relu"):
        outs = {}
        for v in ("1", "0"):
            monkeypatch.setenv("SLIDE_MODULE_PAIR", v)
            fr = R.from_ncx(feat) if C else None
            gr = R.group(xyz, ctr, fr, idx, flags, d2=d2)
            assert isinstance(gr, R.LazyGroup) == (v == "1")
            y = R.conv(gr, conv, stats=stats)
            assert (getattr(gr, "_buf", 0) is None) == (v == "1")  # the pair form never built the grouped matrix
            outs[v] = (y.data.double()[:, :O].reshape(B, npnt, K, O), y.stats)
        want = ref.relu() if stats == "relu" else ref
        e1, e0 = rel(outs["1"][0], want), rel(outs["0"][0], want)
        assert e1 <= 2e-3 and e1 <= 1.1 * e0 + 1e-4, (layout, stats, e1, e0)
        if stats is not None and (npnt * K) % 256 == 0:
            assert outs["1"][1] is not None
    # tile statistics (samples of whole tiles): sums and sums of squares per 256-row tile
    npnt2 = 64
    idx2 = torch.randint(0, N, (B, npnt2, K), generator=gen).to(d)
    ctr2 = torch.rand(B, npnt2, 3, generator=gen).to(d)
    d22 = (torch.rand(B, npnt2, K, generator=gen).to(d) * 0.5 + 1e-3) if layout == "fp" else None
    res = {}
    for v in ("1", "0"):
        monkeypatch.setenv("SLIDE_MODULE_PAIR", v)
        y = R.conv(R.group(xyz, ctr2, R.from_ncx(feat) if C else None, idx2, flags, d2=d22), conv, stats="relu")
        assert y.stats is not None and y.stats[2] is True
        res[v] = (y.data.double(), y.stats[0].double(), y.stats[1].double())
    t = res["1"][0].reshape(-1, 256, res["1"][0].shape[1])
    assert rel(res["1"][1], t.sum(1)) <= 2e-3 and rel(res["1"][2], (t * t).sum(1)) <= 4e-3
    assert rel(res["1"][1], res["0"][1]) <= 3e-3 and rel(res["1"][2], res["0"][2]) <= 6e-3


def test_deferred_normalisation_matches_the_materialised_path(gpu_device, monkeypatch):
    """fp16 module path: a GroupNorm whose consumer is a GEMM is DEFERRED -- the producer's raw output stays in memory and the
    consumer's loader applies relu(x * scale + shift) + add from per-sample fp16 vectors in LDS (csrc/gemm_ring.hip, AFF
    loaders) -- where SLIDE_MODULE_DEFER=0 normalises in fp32 arithmetic first and stores the fp16 result.  The two differ by
    the fp16 rounding of scale / shift / add (2^-11 relative each) and of the affine's result: bounded here on activations
    with a large mean (|shift| = mean * rstd ~ 6) and large embedding rows (|add| up to 50), where that rounding is at its
    worst: <= 3e-3 of the output's L2 norm, and both within 6e-3 of the fp32 arithmetic."""
    from pointnet2_ops import pointnet2_modules as PM
    from slide_amd import rows as R
    monkeypatch.setenv("SLIDE_MODULE_PREC", "fp16")
    d = gpu_device
    gen = torch.Generator().manual_seed(3)
    B, S, C, O_ = 3, 512, 64, 96
    x = (torch.randn(B, C, S, 1, generator=gen) * 5 + 30).to(d)
    add = (torch.rand(B, C, generator=gen) * 100 - 50).to(d)
    gn = PM.HipGroupNorm(8, C).to(d)
    conv = PM.HipConv1x1(C, O_, bias=True).to(d)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 2.0, generator=None); gn.bias.uniform_(-1, 1)
    outs = {}
    for defer in ("1", "0"):
        monkeypatch.setenv("SLIDE_MODULE_DEFER", defer)
        r = R.from_ncx(x)
        assert r.half
        r = R.norm_act(r, gn=gn, relu=True, addvec=add, defer=True)
        assert (r.pending is not None) == (defer == "1")
        outs[defer] = R.to_ncx(R.conv(r, conv), spatial=(S, 1)).double()
    h = torch.nn.functional.group_norm(x.double(), 8, gn.weight.double(), gn.bias.double(), 1e-5).relu() + add.double()[:, :, None, None]
    ref = torch.nn.functional.conv2d(h, conv.weight.double(), conv.bias.double())
    rel = lambda a, b: float(((a - b).norm() / b.norm()).detach())
    assert rel(outs["1"], outs["0"]) <= 3e-3, rel(outs["1"], outs["0"])
    assert rel(outs["1"], ref) <= 6e-3 and rel(outs["0"], ref) <= 6e-3, (rel(outs["1"], ref), rel(outs["0"], ref))
