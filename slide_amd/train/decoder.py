"""The trainable DECODE side of the autoencoder (pointnet2/models/autoencoder.py:11-45 `decode`: key points + latent features ->
256 -> 1024 -> 2048 x 6) on the differentiable row-major layers: differentiable in every decode-side parameter, in the latent
features and in the key points, along the reference's own gradient paths (a level's points reach the level after them through its
feature mapper's centres and its splitting head; the reference's feature extractor detaches its input cloud, cloudnet.py).

TrainableDecoderLevel = PointUpsampleDecoder without KL (point_upsample_decoder.py:24-190): the feature extractor (cloudnet.py), the
feature mapper (FeatureMapModule: 'nn' QueryAndGroup of the level before around the new points, an Mlp without embeddings,
attention whose queries are the extracted features), fc_layer, point_upsample in its three first_refine_coarse_points /
include_displacement_center_to_final_output forms, the zero padding where the input points carry fewer channels than the output,
and the thinning to num_output_points by farthest point sampling (selection without gradient, the gather differentiable).

TrainableDecoder = the key-point level's splitting head (`keypoint_encoder.fc_layer.*`, what the module path builds with
decode_only=True) + the KeypointDecoder levels (`decoder.decoders.{i}.*`).  State-dict names are the reference's: the decode-side keys
of a PointAutoencoder checkpoint load with load_state_dict(..., strict=True) after filtering, and a state dict saved here loads into
the module path's PointAutoencoder(None, decoder_config_list).  The encoder, the key-point level's propagate_feature and its KL
posteriors are encoder.py, whose TrainableAutoencoder builds on this class."""
import numpy as np
import torch
import torch.nn as nn

from .. import _ext, model_spec
from . import functions as F
from .cloudnet import RowsNet, TrainableCloudNet, check_decoder_level_family
from .grouping import query_and_group_rows


def level_feature_dim(cfg):
    arch = cfg["architecture"]
    base = arch["decoder_feature_dim"][0] if "decoder_feature_dim" in arch else arch["feature_dim"][-1]
    return base + cfg["feature_mapper_setting"]["out_dim"]


def upsample_factor(up):
    """the number of out_dim-wide groups fc_layer emits per point (point_upsample_decoder.py:64-72)"""
    factor = up["point_upsample_factor"]
    if up["first_refine_coarse_points"]:
        factor += 0 if up["include_displacement_center_to_final_output"] else 1
    else:
        assert not up["include_displacement_center_to_final_output"]
    return factor


def point_upsample(coarse, displacement, factor, include_displacement_center_to_final_output, output_scale_factor_value,
                   first_refine_coarse_points):
    """pointnet2/models/point_upsample_module.py:4-46: every coarse point emits children = parent + displacement x scale /
    sqrt(factor); with first_refine_coarse_points the first F displacement channels move the parent itself first, and with
    include_displacement_center_to_final_output the refined parents are appended behind the children.  Elementwise torch ops."""
    B, N, Fd = coarse.shape
    assert first_refine_coarse_points or not include_displacement_center_to_final_output
    parents = coarse
    if first_refine_coarse_points:
        parents = coarse + displacement[:, :, :Fd] * output_scale_factor_value
        displacement = displacement[:, :, Fd:]
    n_child = displacement.shape[2] // Fd
    children = parents.unsqueeze(2) + (displacement * (1.0 / np.sqrt(factor))).reshape(B, N, n_child, Fd) * output_scale_factor_value
    children = children.reshape(B, N * n_child, Fd)
    if include_displacement_center_to_final_output:
        children = torch.cat([children, parents], dim=1)
    return children.contiguous()


def _head_spec(hp):
    arch = hp["architecture"]
    query_dim = arch["decoder_feature_dim"][0] if "decoder_feature_dim" in arch else arch["feature_dim"][-1]
    cin = query_dim + hp["feature_mapper_setting"]["out_dim"] + hp["in_fea_dim"] + 3
    cout = int(hp["out_dim"] * upsample_factor(hp["upsampling_setting"]))
    return [("fc_layer.weight", (cout, cin, 1)), ("fc_layer.bias", (cout,))]


def _mapper_spec(hp, in_dim):
    fm = hp["feature_mapper_setting"]
    spec = [in_dim + 9] + [fm["out_dim"]] * fm["mlp_depth"]
    out = []
    model_spec._mlp(spec, "feature_mapper.mlp", False, 0, False, 0, out)
    model_spec._attention("feature_mapper.attention_module", hp["architecture"]["decoder_feature_dim"][0], spec[0], spec[-1], out)
    return out


def _upsample(net, hp, final_feature, new_xyz, fps_start_idx):
    """upsample_points (point_upsample_decoder.py:146-190): final_feature rows [B * N, ld] with C valid channels given as a (rows, C)
    pair, new_xyz (B, N, in_position_and_normal_dim) -> (B, num_output_points, out_dim)"""
    rows, C = final_feature
    up = hp["upsampling_setting"]
    B, N = new_xyz.shape[:2]
    x = F.pad_cols(torch.cat([rows[:, :C], new_xyz.reshape(B * N, -1)], dim=1))
    factor = upsample_factor(up)
    split = F.conv_rows(x, net._p("fc_layer.weight"), net._p("fc_layer.bias"))[:, :hp["out_dim"] * factor].reshape(B, N, -1)
    in_dim = hp.get("in_position_and_normal_dim", hp["out_dim"])
    coarse = new_xyz[:, :, 0:in_dim]
    if in_dim < hp["out_dim"]:  # key points carry no normals: they are generated from scratch
        coarse = torch.cat([coarse, coarse.new_zeros(B, N, hp["out_dim"] - in_dim)], dim=2)
    pts = point_upsample(coarse, split, factor, include_displacement_center_to_final_output=up["include_displacement_center_to_final_output"],
                         output_scale_factor_value=up["output_scale_factor"], first_refine_coarse_points=up["first_refine_coarse_points"])
    n_out = up["num_output_points"]
    assert pts.shape[1] >= n_out
    if pts.shape[1] > n_out:  # the selection carries no gradient; the selected points do
        with torch.no_grad():
            _, idx = _ext.sample_farthest_points(pts.detach(), K=n_out, random_start_point=fps_start_idx is None, start_idx=fps_start_idx)
        pts = torch.gather(pts, 1, idx.unsqueeze(-1).expand(-1, -1, pts.shape[2]))
    return pts


class TrainableDecoderLevel(RowsNet):
    def __init__(self, hp, in_dim):
        check_decoder_level_family(hp)
        fm = hp["feature_mapper_setting"]
        assert fm["neighbor_definition"] == "nn" and fm["mlp_depth"] == 2, "the feature mapper of the family: 'nn' grouping, a two-layer Mlp"
        super().__init__(_mapper_spec(hp, in_dim) + _head_spec(hp))
        self.hp, self.in_dim = hp, in_dim
        self.feature_extractor = TrainableCloudNet(hp)

    def propagate_feature(self, xyz, features, new_xyz, label):
        """xyz (B, N1, 3) with features (B, N1, in_dim) -> features at new_xyz (B, N2, 3 + in_fea_dim) as (rows [B * N2, ld], C):
        [extracted | mapped]"""
        hp, fm = self.hp, self.hp["feature_mapper_setting"]
        B, N1 = xyz.shape[:2]
        N2 = new_xyz.shape[1]
        q = self.feature_extractor(new_xyz, label)
        cq = self.feature_extractor.out_channels
        g, idx, _ = query_and_group_rows(xyz.contiguous(), new_xyz[:, :, 0:3].contiguous(), F.pad_cols(features.reshape(B * N1, self.in_dim)),
                                         self.in_dim, fm["nsample"], "nn", include_abs_coordinate=True, include_center_coordinate=True)
        K = idx.shape[2]
        h = self._mlp(g, "feature_mapper.mlp", B, N2 * K, None, None)
        mapped, cm = self._attention(q, g, h, "feature_mapper.attention_module", B, N2 * K, K)
        return F.pad_cols(torch.cat([q[:, :cq], mapped[:, :cm]], dim=1)), cq + cm

    def forward(self, xyz, features, new_xyz, label, fps_start_idx=None):
        """-> (final_feature (B, N2, C), output points (B, num_output_points, out_dim))"""
        rows, C = self.propagate_feature(xyz, features, new_xyz, label)
        B, N2 = new_xyz.shape[:2]
        return rows[:, :C].reshape(B, N2, C), _upsample(self, self.hp, (rows, C), new_xyz, fps_start_idx)


class TrainableDecoder(nn.Module):
    def __init__(self, decoder_config_list, state_dict=None):
        super().__init__()
        self.configs = decoder_config_list
        self.keypoint_encoder = RowsNet(_head_spec(decoder_config_list[0]))
        self.decoder = nn.Module()
        self.decoder.decoders = nn.ModuleList()
        dim = level_feature_dim(decoder_config_list[0])
        for cfg in decoder_config_list[1:]:
            self.decoder.decoders.append(TrainableDecoderLevel(cfg, dim))
            dim = level_feature_dim(cfg)
        if state_dict is not None:
            self.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict.items()})

    def reset_parameters(self, seed=0):
        for k, m in enumerate(m for m in self.modules() if isinstance(m, RowsNet)):
            m.reset_parameters(seed + k)
        return self

    def decode(self, keypoint, feature_at_keypoint, label, fps_start_idx=None):
        """keypoint (B, 16, 3 | 6), feature_at_keypoint (B, 16, C), label (B,) -> l_xyz_decoder: [key points (B, 16, 3), level 1, ...]"""
        B, N = keypoint.shape[:2]
        hp0 = self.configs[0]
        keypoint, feats = keypoint.float(), feature_at_keypoint.float()
        C = feats.shape[2]
        new_xyz = _upsample(self.keypoint_encoder, hp0, (F.pad_cols(feats.reshape(B * N, C)), C), keypoint, fps_start_idx)
        l_xyz = [keypoint[:, :, 0:3], new_xyz]
        for i, level in enumerate(self.decoder.decoders):
            feats, pts = level(l_xyz[i][:, :, 0:3], feats, l_xyz[i + 1], label, fps_start_idx)
            l_xyz.append(pts)
        return l_xyz

    forward = decode
