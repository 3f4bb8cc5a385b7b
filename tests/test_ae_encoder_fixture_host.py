"""CPU: tests/golden/golden_ae_encoder_train.npz (tools/gen_golden_ae_encoder_train.py: the reference's training step of a reduced
autoencoder with KL) keeps its margins and reaches the new branches; TrainableAutoencoder's state dict carries exactly the names and
shapes of the module path's PointAutoencoder, for the fixture's configs and for the shipped ones, and loads into it and from it
strictly; configurations outside the family raise in the constructor; pointnet2/train_autoencoder.py resolves its arguments and
config files as the reference's CLI does."""
import copy
import json
import os
import sys

import numpy as np
import pytest

from conftest import REPO, golden_spec, load_golden

sys.path.insert(0, os.path.join(REPO, "pointnet2"))


def _stringify(d):
    """lists as strings, the way the reference's JSON files store them"""
    return {k: (_stringify(v) if isinstance(v, dict) else str(v) if isinstance(v, list) else v) for k, v in d.items()}


def test_recorded_selections_meet_their_margins():
    g = load_golden("golden_ae_encoder_train.npz")
    names, gaps, need = [str(n) for n in g["margin_names"]], g["margin_gaps"], g["margin_required"]
    assert float(g["given_sep"]) == 1e-6 and float(g["sep"]) >= 1e-5
    assert {n.split("/")[2] for n in names} == {"knn", "fps", "sample", "chamfer"}
    for n, gap, req in zip(names, gaps, need):
        run, _, kind, where = n.split("/")
        # the encoder and the key-point level search the given clouds, as the loss's down-sampling does; the decoder chain runs on
        # computed points
        assert where == ("computed" if run == "chain" else "given"), n
        assert req == (float(g["given_sep"]) if where == "given" else float(g["sep"])) and gap >= req, (n, gap, req)
    assert len(names) == sum(1 for k in g.files if "_sel" in k) + sum(1 for k in g.files if k.endswith("_i1"))
    assert {n.split("/")[0] for n in names} == {"enc", "kp", "chain", "loss"}


def test_ambiguous_relu_decisions_and_the_kl_term():
    g = load_golden("golden_ae_encoder_train.npz")
    assert float(g["relu_sep"]) >= 8.4e-6 and float(g["relu_tol_norm"]) <= 0.5 * 1e-3 and int(g["relu_ambiguous"]) > 0
    assert float(g["relu_shift"][0]) <= float(g["relu_tol_norm"])
    # kl_weight is large enough that the KL term moves the recorded gradients, and both posteriors sample
    assert float(g["kl_gradient_share"]) > 1e-2 and float(g["kl_weight"]) > 0 and (g["kl_loss"] > 0).all()
    assert g["eps0"].shape == (2, 16, 16) and g["eps1"].shape == (2, 16, 32) and g["eps0"].std() > 0.5


def test_fixture_reaches_the_new_branches_and_stays_small():
    g = load_golden("golden_ae_encoder_train.npz")
    enc, decs = json.loads(str(g["encoder_config_json"])), json.loads(str(g["decoder_configs_json"]))
    assert g["keypoint"].shape == (2, 16, 3) and len(set(g["label"].tolist())) == 2 and g["pointcloud"].shape[2] == 6
    n = g["pointcloud"].shape[1]
    assert n > enc["architecture"]["npoint"][0] > enc["architecture"]["npoint"][1] and len(enc["architecture"]["npoint"]) == 2
    k = decs[0]
    assert k["include_global_feature"] and k["include_class_condition"] and not k["attention_setting"]["last_activation"]
    assert "decoder_feature_dim" not in k["architecture"]
    names = [str(s) for s in g["grad_names"]]
    kept = [f[len("grad__"):] for f in g.files if f.startswith("grad__")]
    for kind in ("global_pnet", "fc_second_condition", "feature_mapper.attention_module.feat_out_conv.0", "encoder.SA_modules"):
        assert any(kind in s for s in kept), kind
    assert not any("feat_out_conv.1" in s for s in names if s.startswith("keypoint_encoder."))   # no last GroupNorm + ReLU there
    gn = dict(zip(names, g["grad_norms"]))
    for kind in ("global_pnet", "fc_second_condition", "encoder.SA_modules.0", "keypoint_encoder.feature_mapper"):
        assert max(v for s, v in gn.items() if kind in s) > 0, kind
    assert all(gn[s] == 0 for s in names if ".fc_t" in s)            # the t-embedding layers exist and nothing reads them
    size = lambda f: os.path.getsize(os.path.join(REPO, "tests", "golden", f))
    assert size("golden_ae_encoder_train.npz") <= size("golden_ae_decoder_train.npz")


def _configs(which):
    if which == "fixture":
        g = load_golden("golden_ae_encoder_train.npz")
    else:
        g = load_golden("golden_encode.npz")
    return json.loads(str(g["encoder_config_json"])), json.loads(str(g["decoder_configs_json"]))


@pytest.mark.parametrize("which,kl", [("fixture", True), ("shipped", True), ("shipped", False)])
def test_state_dict_names_equal_the_module_paths(which, kl):
    import torch
    from models.autoencoder import PointAutoencoder
    from slide_amd.train.encoder import TrainableAutoencoder
    enc, decs = _configs(which)
    ref = PointAutoencoder(copy.deepcopy(enc), copy.deepcopy(decs), apply_kl_regularization=kl)
    ae = TrainableAutoencoder(enc, decs, apply_kl_regularization=kl).reset_parameters(1)
    a = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in ae.state_dict().items()} == a
    assert sorted(n for n, _ in ae.named_parameters()) == sorted(a)
    assert {k.split(".")[0] for k in a} == {"encoder", "keypoint_encoder", "decoder"}
    ref.load_state_dict(ae.state_dict(), strict=True)               # a state dict saved here loads into the module path
    ae.load_state_dict(ref.state_dict(), strict=True)                # and a full PointAutoencoder state dict loads here
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in ae.state_dict().items())
    if which == "fixture":
        assert a == dict(golden_spec(load_golden("golden_ae_encoder_train.npz")))


def test_configurations_outside_the_family_raise_in_the_constructor():
    from slide_amd.train.encoder import TrainableAutoencoder, TrainableEncoder
    enc, decs = _configs("shipped")
    TrainableEncoder(copy.deepcopy(enc))
    for path, value in ((("include_t",), True), (("bn_first",), True), (("res_connect",), False), (("transform_output",), True),
                        (("architecture", "neighbor_definition"), "radius"), (("architecture", "mlp_depth"), 2),
                        (("attention_setting", "use_attention_module"), False), (("include_class_condition",), False),
                        (("activation",), "swish")):
        bad = copy.deepcopy(enc)
        d = bad
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] = value
        with pytest.raises(AssertionError):
            TrainableEncoder(bad)
    with pytest.raises(AssertionError):   # a key-point level that extracts with a PointNet2CloudCondition is a decoder level
        TrainableAutoencoder(enc, [decs[1]] + decs[1:], apply_kl_regularization=True)
    bad = copy.deepcopy(decs)
    bad[0]["feature_mapper_setting"]["neighbor_definition"] = "radius"
    with pytest.raises(AssertionError):
        TrainableAutoencoder(enc, bad, apply_kl_regularization=True)


def _write_configs(tmp_path, dataset=None, train=None):
    enc, decs = _configs("fixture")
    os.makedirs(tmp_path / "lv", exist_ok=True)
    (tmp_path / "lv" / "enc.json").write_text(json.dumps({"pointnet_config": _stringify(enc)}))
    for i, d in enumerate(decs):
        (tmp_path / "lv" / ("d%d.json" % i)).write_text(json.dumps({"pointnet_config": _stringify(d)}))
    cfg = {"pointnet_config": {"model_name": "ae_test", "apply_kl_regularization": True, "kl_weight": 1e-5, "encoder_config_file": "lv/enc.json",
                               "decoder_config_file": "['lv/d0.json', 'lv/d1.json', 'lv/d2.json']", "feature_weight": "[0,0,0.1]"},
           "train_config": dict({"task": "autoencode", "root_directory": "exps/ae", "output_directory": "checkpoint", "ckpt_iter": "max",
                                 "epochs_per_ckpt": 2, "iters_per_logging": 1, "n_epochs": 3, "learning_rate": 0.001}, **(train or {})),
           "shapenet_psr_dataset_config": dict({"batch_size": 2, "num_keypoints": 16, "keypoint_noise_magnitude": 0.04,
                                                "keypoints_source": "farthest_points_sampling"}, **(dataset or {}))}
    (tmp_path / "ae.json").write_text(json.dumps(cfg))
    return str(tmp_path / "ae.json"), enc, decs


def test_cli_arguments_and_config_handling(tmp_path):
    import train_autoencoder as T
    path, enc, decs = _write_configs(tmp_path)
    a = T.parse_args(["-c", path, "--dataset_npz", "clouds.npz"])
    s = T.resolve(a, per_epoch=4)
    assert s["encoder_config"] == enc and s["decoder_config_list"] == decs          # the string lists are restored
    assert s["apply_kl_regularization"] is True and s["kl_weight"] == 1e-5 and s["feature_weight"] == [0, 0, 0.1]
    assert s["out_dir"] == os.path.join("exps/ae", "ae_test", "checkpoint")
    assert (s["batch_size"], s["num_keypoints"], s["keypoint_noise"], s["add_centroid"], s["random_subsample"]) == (2, 16, 0.04, True, False)
    assert (s["n_iters"], s["iters_per_ckpt"], s["learning_rate"], s["ckpt_iter"]) == (12, 8, 0.001, "max")
    a = T.parse_args(["-c", path, "--dataset_npz", "x.npz", "--n_iters", "3", "--iters_per_ckpt", "3", "--root_directory", str(tmp_path / "o")])
    s = T.resolve(a, per_epoch=4)
    assert (s["n_iters"], s["iters_per_ckpt"]) == (3, 3) and s["out_dir"] == str(tmp_path / "o" / "ae_test" / "checkpoint")
    with pytest.raises(SystemExit):
        T.parse_args(["--dataset_npz", "x.npz"])                                      # the config is required
    path, _, _ = _write_configs(tmp_path, dataset={"add_centroid_to_keypoints": False, "random_sample_keypoints": True})
    s = T.resolve(T.parse_args(["-c", path, "--dataset_npz", "x.npz"]))
    assert s["random_subsample"] and not s["add_centroid"] and "n_iters" not in s
    path, _, _ = _write_configs(tmp_path, dataset={"random_sample_keypoints": True})
    with pytest.raises(ValueError):
        T.resolve(T.parse_args(["-c", path, "--dataset_npz", "x.npz"]))
    path, _, _ = _write_configs(tmp_path, dataset={"keypoints_source": "skeleton"})
    with pytest.raises(ValueError):
        T.resolve(T.parse_args(["-c", path, "--dataset_npz", "x.npz"]))


def test_find_max_ckpt_resumes_from_the_highest(tmp_path):
    from slide_amd.train.trainer import find_max_ckpt
    assert find_max_ckpt(str(tmp_path / "none")) == -1
    for i in (2, 11, 5):
        (tmp_path / ("pointnet_ckpt_%d.pkl" % i)).write_bytes(b"")
    assert find_max_ckpt(str(tmp_path)) == 11
