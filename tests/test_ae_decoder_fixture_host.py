"""CPU: tests/golden/golden_ae_decoder_train.npz (tools/gen_golden_ae_train.py: the reference's decode-side training step on a reduced
two-level decoder) -- every selection the reference made keeps its margin over the runner-up, and the trainable decoder's state dict
carries exactly the decode-side keys of the reference's PointAutoencoder for those configs."""
import json

import numpy as np

from conftest import golden_spec, load_golden


def test_recorded_selections_meet_their_margins():
    g = load_golden("golden_ae_decoder_train.npz")
    names, gaps, need = [str(n) for n in g["margin_names"]], g["margin_gaps"], g["margin_required"]
    assert float(g["given_sep"]) == 1e-6 and float(g["sep"]) >= 1e-5
    kinds = {n.split("/")[2] for n in names}
    assert kinds == {"knn", "fps", "sample", "chamfer"}
    for n, gap, req in zip(names, gaps, need):
        where = n.split("/")[3]
        assert req == (float(g["given_sep"]) if where == "given" else float(g["sep"])), n
        assert gap >= req, (n, gap, req)
    # selections on computed coordinates: thinning FPS, Chamfer neighbours, everything of the chained run; the loss's down-sampling
    # of the input cloud and the in-level searches of the per-level runs see given coordinates
    for n in names:
        run, _, kind, where = n.split("/")
        assert where == ("computed" if (run == "chain" or kind in ("sample", "chamfer")) and run != "loss" else "given"), n
    # every recorded selection array has its margin entry
    n_sel = sum(1 for k in g.files if "_sel" in k)
    n_cd = sum(1 for k in g.files if k.endswith("_i1"))
    assert len(names) == n_sel + n_cd


def test_ambiguous_relu_decisions_do_not_move_the_gradients():
    """ReLU decisions on computed values are selections too (the gradient jumps at 0): with every decision whose input lies within
    relu_sep of its tensor's root mean square flipped at once, the reference's own gradient norms and input gradients of the chained
    run and of each level moved by less than half the tolerances the GPU test holds them to"""
    g = load_golden("golden_ae_decoder_train.npz")
    assert float(g["relu_sep"]) >= 8.4e-6               # the feature disagreement measured on the GPU (profiles/decoder_training.md)
    assert float(g["relu_tol_norm"]) <= 0.5 * 1e-3 and float(g["relu_tol_full"]) <= 0.5 * 2e-3
    assert [str(r) for r in g["relu_shift_runs"]] == ["chain", "lvl0", "lvl1"] and int(g["relu_ambiguous_chain"]) > 0
    for run, (d_norm, _, d_in) in zip(g["relu_shift_runs"], g["relu_shift"]):
        assert d_norm <= float(g["relu_tol_norm"]) and d_in <= float(g["relu_tol_full"]), (str(run), d_norm, d_in)


def test_fixture_reaches_every_branch():
    g = load_golden("golden_ae_decoder_train.npz")
    cfgs = json.loads(str(g["decoder_configs_json"]))
    assert g["keypoint"].shape == (2, 16, 3) and len(set(g["label"].tolist())) == 2 and g["pointcloud"].shape[2] == 6
    assert cfgs[0]["in_position_and_normal_dim"] == 3 < cfgs[0]["out_dim"]             # the head zero-pads
    sizes = [g["lvl0_new_xyz"].shape[1], g["lvl1_new_xyz"].shape[1]]
    forms = []
    for c, n in zip(cfgs[1:], sizes):
        a, fm, up = c["architecture"], c["feature_mapper_setting"], c["upsampling_setting"]
        assert n > a["npoint"][0] and a["npoint"][0] <= a["npoint"][1]                  # one SA level with FPS, one without
        assert fm["nsample"] not in a["nsample"] and a["K"] == 8 and a["use_knn_FP"]
        assert all(w % 32 == 0 for w in a["feature_dim"] + a["decoder_feature_dim"] + [fm["out_dim"]])
        factor = up["point_upsample_factor"] - (1 if up["include_displacement_center_to_final_output"] else 0)
        made = n * factor + (n if up["include_displacement_center_to_final_output"] else 0)
        forms.append((up["first_refine_coarse_points"], made > up["num_output_points"]))
        assert made >= up["num_output_points"]
    assert forms == [(True, True), (False, False)]                                      # a thinned level and one that hits its size
    assert g["feature_weight"].tolist()[:2] == [0, 0] and g["feature_weight"][2] > 0


def test_state_dict_names_are_the_references_decode_side_keys():
    from slide_amd.train.decoder import TrainableDecoder
    g = load_golden("golden_ae_decoder_train.npz")
    spec = golden_spec(g)
    assert all(n.startswith("keypoint_encoder.fc_layer.") or n.startswith("decoder.decoders.") for n, _ in spec)
    dec = TrainableDecoder(json.loads(str(g["decoder_configs_json"])))
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == dict(spec)
    assert sorted(n for n, _ in dec.named_parameters()) == sorted(n for n, _ in spec)
