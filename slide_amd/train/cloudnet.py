"""Trainable PointNet2CloudCondition for ANY input size (pointnet2/models/pointnet2_with_pcld_condition.py:286-489 on
pointnet2_ssg_sem.py:34-177) on the differentiable row-major layers of functions.py -- the configuration family of the shipped
DECODER-LEVEL configs (autoencoder_configs/*/decoder_level_2.json, decoder_level_3.json): set-abstraction levels with farthest
point sampling where N > npoint and none where N <= npoint, 'nn' grouping with `nsample` neighbours among the level's source
points, kNN feature propagation with K = 8 ACROSS levels, attention everywhere, class condition without t, per-point features out
(transform_output false), no condition cloud.  Anything else raises in the constructor.

TrainableDenoiser is the 16-point special case (no FPS, one shared 16 x 16 neighbour table, S = 16 K); its layer helpers are used
here as they are (RowsNet), except the two that hard-wire its sizes: the attention block takes its row count, and the class-embedding
term of an Mlp is functions.add_vec_rows, whose backward is the per-sample column-sum kernel (S reaches 256 centres x 32 neighbours
= 8192 rows per sample here; TrainableDenoiser keeps its torch expression and its step graphs).

Selections -- FPS picks, kNN tables -- run without gradients on the existing kernels; for the selected rows everything is
differentiable: query features are gathered by GroupRows with K = 1 and no coordinate columns (a row gather whose backward is
slide_group_rows_bwd), grouping goes through grouping.query_and_group_rows / group_knn_rows.  The INPUT cloud itself receives no
gradient from this network, as in the reference, which assembles xyz and the input features under torch.no_grad(); in a decoder
level the new points get their gradient from the feature mapper's centre columns and from the splitting head."""
import torch
import torch.nn as nn

from .. import _ext, model_spec
from ..abi import GROUP_NO_XYZ, ru
from . import functions as F
from .denoiser import TrainableDenoiser
from .grouping import group_knn_rows, query_and_group_rows


class RowsNet(nn.Module):
    """a parameter tree under the reference's dotted names + the layer helpers of TrainableDenoiser (its own functions, unchanged)"""
    _register = TrainableDenoiser._register
    _p = TrainableDenoiser._p
    _has = TrainableDenoiser._has
    _shared = TrainableDenoiser._shared
    _mlp = TrainableDenoiser._mlp
    reset_parameters = TrainableDenoiser.reset_parameters

    def __init__(self, spec):
        super().__init__()
        self._names = []
        for name, shape in spec:
            self._register(name, nn.Parameter(torch.zeros(*shape)))

    @staticmethod
    def _add_vec(x, vec, B, S):
        """x[(b, s)][c] += vec[b][c]; dvec = the per-sample column sums of the gradient (slide_col_sums_seg)"""
        return F.add_vec_rows(x, vec, B, S)

    def _attention(self, feat, grouped, out, prefix, B, S, K):
        """AttentionModule.forward (attention.py:70-96) on S = points x K rows per sample, 'nn' grouping: every neighbour counts"""
        P = self._p
        q = F.conv_rows(feat, P(prefix + ".feat_conv.weight"), P(prefix + ".feat_conv.bias"))
        k = F.conv_rows(grouped, P(prefix + ".grouped_feat_conv.weight"), P(prefix + ".grouped_feat_conv.bias"))
        C1, C2 = P(prefix + ".feat_conv.weight").shape[0], P(prefix + ".grouped_feat_conv.weight").shape[0]
        s = F.concat_qk(q, k, K, C1, C2)                                             # relu(cat([q.expand, k]))
        s = F.gn_rows(s, P(prefix + ".weight_conv.1.group_norm.weight"), P(prefix + ".weight_conv.1.group_norm.bias"),
                      B, S, min(32, C1 + C2), False, False)
        s = F.conv_rows(s, P(prefix + ".weight_conv.2.weight"), P(prefix + ".weight_conv.2.bias"))
        inter = P(prefix + ".weight_conv.2.weight").shape[0]
        s = F.gn_rows(s, P(prefix + ".weight_conv.4.group_norm.weight"), P(prefix + ".weight_conv.4.group_norm.bias"),
                      B, S, min(32, inter), True, False)                             # ReLU, then MyGroupNorm
        scores = F.conv_rows(s, P(prefix + ".weight_conv.5.weight"), P(prefix + ".weight_conv.5.bias"))
        cout = P(prefix + ".weight_conv.5.weight").shape[0]
        v = F.conv_rows(out, P(prefix + ".feat_out_conv.0.weight"), P(prefix + ".feat_out_conv.0.bias"))
        v = F.gn_rows(v, P(prefix + ".feat_out_conv.1.group_norm.weight"), P(prefix + ".feat_out_conv.1.group_norm.bias"),
                      B, S, min(32, cout), False, True)
        return F.attend_rows(scores, v, K, cout), cout


def gather_rows(rows, idx, B, N, C):
    """rows [B * N, ld] with C valid channels, idx (B, m) integer -> [B * m, ru(C)]: rows[(b, idx[b][j])], differentiable in the rows
    (GroupRows with K = 1 and no coordinate columns: the forward is the grouping kernel, the backward slide_group_rows_bwd)"""
    m = idx.shape[1]
    z = torch.zeros(B, max(N, m), 3, device=rows.device)  # (the coordinate arguments of a launch that writes no coordinate column)
    out = F.group_rows(rows, z[:, :N], z[:, :m], idx.long().reshape(B, m, 1).contiguous(), None, GROUP_NO_XYZ, C)
    return out if out.shape[1] == ru(C) else out[:, :ru(C)].contiguous()


def check_decoder_level_family(hp):
    """the configuration family of the shipped decoder-level configs; raises AssertionError for anything else"""
    arch = hp["architecture"]
    assert "decoder_feature_dim" in arch, "a level without decoder_feature_dim extracts with a PointNet2Encoder (the key-point level)"
    assert not hp.get("include_local_feature", False) and not hp.get("include_global_feature", False)
    assert arch["neighbor_definition"] == "nn" and arch.get("use_knn_FP", False) and not arch.get("include_grouper", False)
    assert arch["K"] == 8 and len(arch["decoder_feature_dim"]) == len(arch["npoint"]) + 1 == len(arch["feature_dim"])
    assert arch["decoder_feature_dim"][-1] == arch["feature_dim"][-1]
    assert hp["attach_position_to_input_feature"] and hp["include_abs_coordinate"] and hp.get("include_center_coordinate", False)
    assert hp["model.use_xyz"] and hp["bias"] and hp["res_connect"] and not hp["bn_first"] and hp.get("bn", True)
    assert not hp["include_t"] and hp["include_class_condition"] and not hp.get("transform_output", True)
    assert hp.get("activation", "relu") == "relu" and not hp.get("use_position_encoding", False)
    assert not hp.get("concate_partial_with_noisy_input", False) and hp.get("global_attention_setting") is None
    att = hp["attention_setting"]
    assert att["use_attention_module"] and att["attention_bn"] and att["transform_grouped_feat_out"] and att["last_activation"]
    assert att["add_attention_to_FeatureMapper_module"]


def cloudnet_param_spec(hp):
    """the reference's state-dict names and shapes of the extractor: the denoiser's, without its output head (transform_output false)"""
    return [(n, s) for n, s in model_spec.denoiser_param_spec(hp) if not n.startswith("fc_lyaer.")]


class TrainableCloudNet(RowsNet):
    def __init__(self, hp):
        check_decoder_level_family(hp)
        super().__init__(cloudnet_param_spec(hp))
        self.hp = hp
        self.out_channels = hp["architecture"]["decoder_feature_dim"][0]
        for name in self._names:  # the Mlps' embeddings and residuals the helpers rely on
            assert ".fc." not in name
        for name, _ in cloudnet_param_spec(hp):
            if name.endswith(".first_mlp.0.weight"):
                assert self._has(name[:-len("first_mlp.0.weight")] + "res_connect.weight"), "identity res_connect is not in the family"

    def forward(self, pointcloud, label):
        """pointcloud (B, N, 3 + in_fea_dim), label (B,) -> per-point features as rows [B * N, ru(C)], C = decoder_feature_dim[0]"""
        hp, arch = self.hp, self.hp["architecture"]
        B, N = pointcloud.shape[:2]
        assert pointcloud.shape[2] == 3 + hp["in_fea_dim"]
        # the reference assembles the network's input -- the attached positions, xyz, the input features -- under torch.no_grad()
        # (pointnet2_with_pcld_condition.py:321-349): the extractor is differentiable in its parameters, NOT in its input cloud
        pc = pointcloud.detach().float()
        pc = torch.cat([pc, pc[:, :, 0:3]], dim=2)                                   # attach_position_to_input_feature
        xyz = pc[:, :, 0:3].contiguous()
        C0 = pc.shape[2] - 3
        cond = self._p("class_emb.weight")[label.long()]
        l_xyz, feats, chans = [xyz], [F.pad_cols(pc[:, :, 3:].reshape(B * N, C0))], [C0]
        for i, npoint in enumerate(arch["npoint"]):                                    # PointnetSAModule (pointnet2_modules.py:222-292)
            pfx = "SA_modules.%d" % i
            src, n_src = l_xyz[i], l_xyz[i].shape[1]
            if n_src <= npoint:                                                        # nothing to sub-sample: every point is a centre
                centres, query = src, feats[i]
            else:
                with torch.no_grad():  # (the coordinates are constants of the input cloud: nothing to differentiate)
                    picked = _ext.furthest_point_sampling(src.contiguous(), npoint)
                    centres = _ext.gather_rows(src, picked)
                query = gather_rows(feats[i], picked, B, n_src, chans[i])
            g, idx, _ = query_and_group_rows(src, centres, feats[i], chans[i], arch["nsample"][i], "nn", include_abs_coordinate=True,
                                             include_center_coordinate=True)
            n_c, K = idx.shape[1:]
            out = self._mlp(g, pfx + ".mlps.0", B, n_c * K, None, cond)
            o, c = self._attention(query, g, out, pfx + ".attention_modules.0", B, n_c * K, K)
            l_xyz.append(centres); feats.append(o); chans.append(c)
        nfp = len(arch["decoder_feature_dim"]) - 1
        for i in range(-1, -(nfp + 1), -1):                                            # PointnetKnnFPModule (:771-873)
            pfx = "FP_modules.%d" % (nfp + i)
            unknown, known = l_xyz[i - 1], l_xyz[i]
            U, CU, Kf, C2 = feats[i - 1], chans[i - 1], feats[i], chans[i]
            n = unknown.shape[1]
            g = group_knn_rows(unknown, known, Kf, C2, arch["K"])
            out = self._mlp(g, pfx + ".mlp1", B, n * arch["K"], None, None)
            interp, c = self._attention(U, g, out, pfx + ".attention_module", B, n * arch["K"], arch["K"])
            z = F.pad_cols(torch.cat([interp[:, :c], U[:, :CU], unknown.reshape(B * n, 3)], dim=1))
            feats[i - 1] = self._mlp(z, pfx + ".mlp2", B, n, None, cond)
            chans[i - 1] = self._p(pfx + ".mlp2.res_connect.weight").shape[0]
        assert chans[0] == self.out_channels
        return feats[0]
