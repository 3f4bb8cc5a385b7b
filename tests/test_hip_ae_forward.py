"""GPU: PointAutoencoder.forward, the reference's evaluation forward (pointnet2/models/autoencoder.py:48-87), against
tests/golden/golden_ae_forward.npz (the reference's forward on golden_encode.npz's clouds, airplane AE config, posterior mode, every
farthest point sampling started at index 0)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from slide_amd.synth import synth_state_dict

sys.path.insert(0, os.path.join(REPO, "pointnet2"))
pytestmark = pytest.mark.gpu

LOSS_KEYS = ("cd_p", "cd_t", "cd_feature_p", "cd_feature_t", "f1", "kl_loss", "training_loss")


def _ae(dev):
    from models.autoencoder import PointAutoencoder
    ge, gf = load_golden("golden_encode.npz"), load_golden("golden_ae_forward.npz")
    enc, decs = json.loads(str(ge["encoder_config_json"])), json.loads(str(ge["decoder_configs_json"]))
    ae = PointAutoencoder(enc, decs, apply_kl_regularization=True, kl_weight=float(gf["kl_weight"]),
                          feature_weight=[float(v) for v in gf["feature_weight"]])
    spec = [(k, tuple(v.shape)) for k, v in ae.state_dict().items()]
    vals = synth_state_dict([("ae." + n, s) for n, s in spec])  # the generator's weights: a function of the names
    ae.load_state_dict({n: torch.from_numpy(vals["ae." + n]) for n, _ in spec})
    return ae.to(dev).eval(), ge, gf


def _inputs(ge, d):
    return (torch.from_numpy(ge["pointcloud"]).to(d), torch.from_numpy(ge["keypoint"]).to(d),
            torch.from_numpy(ge["label"]).to(d))


def test_metrics_on_the_reference_levels_match_loss_list(gpu_device):
    """the reference's own decoded levels through OUR calc_cd against OUR farthest-point-sampled input: loss_list to 1e-6;
    training_loss recombined with the feature weights and, at the last level, the reference's KL term"""
    import metrics_point_cloud.chamfer_and_f1 as C
    from slide_amd import _ext
    d = gpu_device
    g = load_golden("golden_ae_forward.npz")
    pc = torch.from_numpy(load_golden("golden_encode.npz")["pointcloud"]).to(d)
    B = pc.shape[0]
    start = torch.zeros(B, dtype=torch.int32, device=d)
    n_lv = int(g["levels"])
    fw = g["feature_weight"]
    for i in range(1, n_lv):
        uvw = torch.from_numpy(g["level%d" % i]).to(d)
        down, _ = _ext.sample_farthest_points(pc, K=uvw.shape[1], start_idx=start)
        r = C.calc_cd(uvw, down, calc_f1=True, f1_threshold=1e-4, normal_loss_type='mse')
        for k in ("cd_p", "cd_t", "cd_feature_p", "cd_feature_t", "f1"):
            want = g["loss%d_%s" % (i - 1, k)]
            got = r[k].cpu().numpy()
            assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (i, k, got, want)
        loss = (r["cd_p"] + r["cd_feature_p"] * float(fw[i - 1])).cpu().numpy().astype(np.float64)
        if i == n_lv - 1:
            loss = loss + float(g["kl_weight"]) * g["loss%d_kl_loss" % (i - 1)].astype(np.float64)
        want = g["loss%d_training_loss" % (i - 1)]
        assert np.all(np.abs(loss - want) <= 1e-6 * np.abs(want)), (i, loss, want)


# End-to-end tolerance, derived from what the decode parity pins (test_hip_modules.py::test_autoencoder_decode_matches_reference):
# the end-to-end decoded cloud's Chamfer distance to the reference cloud (squared, sum of both directions) is at most CH = 1e-5.
# A level L of ours and the reference's L' then satisfy mean_a min_b |a - b|^2 <= CH in each direction, so (Cauchy-Schwarz) the mean
# displacement of a point to the other cloud is at most sqrt(CH).  Nearest-neighbour distances are 1-Lipschitz in the query point,
# so each direction's mean distance to the (shared, bit-exact) down-sampled input moves by at most sqrt(CH):
#     |cd_p - cd_p'| <= sqrt(CH)
# and with |d^2 - d'^2| = |d - d'| (d + d') and Cauchy-Schwarz once more, per direction at most 2 sqrt(CH) sqrt(cd_t') + CH, so
#     |cd_t - cd_t'| <= 2 (2 sqrt(CH) sqrt(cd_t') + CH)
# (the Lipschitz steps pair every point with its counterpart: the level comparisons of that test are bijections).
# The normal terms are not Lipschitz in the positions (a point whose nearest neighbour changes picks up another normal) and F1 is a
# count at a threshold: those follow the same perturbation only statistically and are held to the relative bound REL_STAT, the
# fraction of points a displacement of sqrt(CH) can move across a neighbour change or the threshold, taken as 1e-2.
# The KL term comes from the encoder alone (no FPS-order fragility): it is held to the encode parity's 2e-4 relative.
CH = 1e-5
REL_STAT = 1e-2
KL_REL = 2e-4


def test_forward_end_to_end_matches_reference(gpu_device):
    ae, ge, g = _ae(gpu_device)
    pc, kp, lab = _inputs(ge, gpu_device)
    start = torch.zeros(pc.shape[0], dtype=torch.int32, device=gpu_device)
    with torch.no_grad():
        l_xyz, loss_list, feat = ae(pc, kp, ts=None, label=lab, loss_type='cd_p', sample_posterior=False,
                                    return_keypoint_feature=True, fps_start_idx=start)
    n_lv = int(g["levels"])
    assert len(l_xyz) == n_lv and len(loss_list) == n_lv - 1 and feat.shape == (pc.shape[0], 16, 48)
    for i in range(n_lv):
        assert tuple(l_xyz[i].shape) == g["level%d" % i].shape
    sq = np.sqrt(CH)
    for i, dct in enumerate(loss_list):
        assert sorted(dct) == sorted(LOSS_KEYS), sorted(dct)
        r = {k: v.cpu().numpy().astype(np.float64) for k, v in dct.items()}
        w = {k: g["loss%d_%s" % (i, k)].astype(np.float64) for k in LOSS_KEYS}
        print("level %d:" % (i + 1), {k: float(np.abs(r[k] - w[k]).max()) for k in LOSS_KEYS})
        assert np.all(np.abs(r["cd_p"] - w["cd_p"]) <= sq), i
        assert np.all(np.abs(r["cd_t"] - w["cd_t"]) <= 2 * (2 * sq * np.sqrt(w["cd_t"]) + CH)), i
        for k in ("cd_feature_p", "cd_feature_t"):
            assert np.all(np.abs(r[k] - w[k]) <= REL_STAT * np.abs(w[k])), (i, k)
        assert np.all(np.abs(r["f1"] - w["f1"]) <= REL_STAT), i
        if i == n_lv - 2:
            assert np.all(np.abs(r["kl_loss"] - w["kl_loss"]) <= KL_REL * np.abs(w["kl_loss"])), (r["kl_loss"], w["kl_loss"])
        else:
            assert not r["kl_loss"].any()
        want_loss = r["cd_p"] + float(g["feature_weight"][i]) * r["cd_feature_p"] + (float(g["kl_weight"]) * r["kl_loss"])
        assert np.allclose(r["training_loss"], want_loss, rtol=1e-6, atol=0)
        assert np.all(np.abs(r["training_loss"] - w["training_loss"]) <=
                      sq + float(g["feature_weight"][i]) * REL_STAT * np.abs(w["cd_feature_p"]) + float(g["kl_weight"]) * KL_REL *
                      np.abs(w["kl_loss"])), i


def test_forward_with_grad_still_raises(gpu_device):
    ae, ge, _ = _ae(gpu_device)
    pc, kp, lab = _inputs(ge, gpu_device)
    assert any(p.requires_grad for p in ae.parameters())
    with pytest.raises(NotImplementedError, match="training"):
        ae(pc, kp, ts=None, label=lab)
