"""The trainable ENCODE side of the autoencoder and the whole autoencoder on top of it (pointnet2/models/autoencoder.py:48-87): the
input cloud -> PointNet2Encoder (pointnet2_feature_extractor.py; the shipped config_encoder.json: 2048 -> 1024 -> 256 -> 64 -> 32
points, K = 32) -> the key-point level's propagate_feature (point_upsample_decoder.py:96-147; decoder_level_1.json: a PointNet2Encoder
on the 16 key points conditioned on a Pnet2Stage global feature and on the class embedding, a feature mapper onto the encoder's
last level, and -- with apply_kl_regularization -- a diagonal Gaussian posterior over each of the two) -> feature_at_keypoint ->
TrainableDecoder.decode.

TrainableEncoder is cloudnet.TrainableCloudNet's set-abstraction loop without the feature-propagation half.  What the key-point
level adds to the layers of RowsNet lives HERE, in EncoderRowsNet (TrainableDenoiser._mlp / _attention stay as they are for the
configurations they serve):
  * Mlp_plus_t_emb with a SECOND condition term, added after rest_mlp (pointnet2_modules.py:159-165): the global feature goes through
    fc_condition, the class embedding through fc_second_condition;
  * Mlp_plus_t_emb without res_connect (Pnet2Stage) and with the identity one where mlp_spec[0] == mlp_spec[-1];
  * remove_last_activation (pnet.py:20-28: second_mlp keeps its convolution only);
  * attention without its last GroupNorm + ReLU (attention_setting.last_activation false: feat_out_conv is one convolution);
  * the maxima over a sample's points (functions.col_max_seg) and the posterior with its KL term (functions.gauss_posterior).
Anything outside the family raises in the constructor.  State-dict names are the reference's (`encoder.*`, `keypoint_encoder.*`,
`decoder.decoders.{i}.*`): a full PointAutoencoder state dict loads with strict=True, and a state dict saved here loads into the
module path's PointAutoencoder(encoder_config, decoder_config_list, apply_kl_regularization=...).  The reference assembles the
encoder's input under no_grad: the input cloud gets no gradient."""
import copy

import torch
import torch.nn as nn

from .. import _ext, model_spec
from . import functions as F
from .cloudnet import RowsNet, gather_rows
from .decoder import TrainableDecoder, _head_spec
from .grouping import query_and_group_rows


# ---------------------------------------------------------------------------------------------------- parameter specs
def _mlp_spec(spec, pfx, cond_dim, second_dim, out, res_connect=True, last_activation=True):
    """Mlp_plus_t_emb(spec, bn=True, include_t=False, bias=True) -> (name, shape) list; cond_dim / second_dim None: no such term"""
    assert 3 <= len(spec) <= 4, "an Mlp of the family has three or four widths (rest_mlp is one layer)"
    if cond_dim is not None:
        out += [(pfx + ".fc_condition.weight", (spec[2], cond_dim)), (pfx + ".fc_condition.bias", (spec[2],))]
    if second_dim is not None:
        out += [(pfx + ".fc_second_condition.weight", (spec[-1], second_dim)), (pfx + ".fc_second_condition.bias", (spec[-1],))]
    if res_connect and spec[0] != spec[-1]:
        out += [(pfx + ".res_connect.weight", (spec[-1], spec[0], 1, 1)), (pfx + ".res_connect.bias", (spec[-1],))]
    layers = [("first_mlp", spec[0], spec[1], True), ("second_mlp", spec[1], spec[2], last_activation)]
    if len(spec) > 3:
        layers.append(("rest_mlp", spec[2], spec[3], True))
    for n, i, o, gn in layers:
        out += [("%s.%s.0.weight" % (pfx, n), (o, i, 1, 1)), ("%s.%s.0.bias" % (pfx, n), (o,))]
        if gn:
            c = model_spec._gn_channels(o)
            out += [("%s.%s.1.group_norm.weight" % (pfx, n), (c,)), ("%s.%s.1.group_norm.bias" % (pfx, n), (c,))]


def _attention_spec(pfx, c_in1, c_in2, c_out, last_activation, out):
    part = []
    model_spec._attention(pfx, c_in1, c_in2, c_out, part)
    out += [(n, s) for n, s in part if last_activation or ".feat_out_conv.1." not in n]


def check_encoder_family(hp):
    """the PointNet2Encoder family of the shipped config_encoder.json and decoder_level_1.json; AssertionError for anything else"""
    arch = hp["architecture"]
    assert "decoder_feature_dim" not in arch, "a level with decoder_feature_dim extracts with a PointNet2CloudCondition (cloudnet.py)"
    assert arch["neighbor_definition"] == "nn" and arch["mlp_depth"] == 3 and len(arch["feature_dim"]) == len(arch["npoint"]) + 1
    assert len(arch["nsample"]) == len(arch["npoint"])
    assert hp["attach_position_to_input_feature"] and hp["include_abs_coordinate"] and hp.get("include_center_coordinate", False)
    assert hp["model.use_xyz"] and hp["bias"] and hp["res_connect"] and not hp["bn_first"] and hp.get("bn", True)
    assert not hp["include_t"] and hp["include_class_condition"] and not hp.get("transform_output", False)
    assert hp.get("activation", "relu") == "relu" and not hp.get("use_position_encoding", False)
    assert hp.get("global_attention_setting") is None and hp.get("pooling", "max") == "max"
    att = hp["attention_setting"]
    assert att["use_attention_module"] and att["attention_bn"] and att["transform_grouped_feat_out"]
    if hp.get("include_global_feature", False):
        pa = hp["pnet_global_feature_architecture"]
        assert len(pa) == 2 and len(pa[0]) >= 3 and len(pa[1]) >= 2, "Pnet2Stage: two Mlps of at least two layers"


def encoder_param_spec(hp):
    """the reference's state-dict names and shapes of a PointNet2Encoder of the family"""
    arch = hp["architecture"]
    C0 = hp["in_fea_dim"] + 3
    cdim = hp["class_condition_dim"]
    t = hp["t_dim"]
    last = hp["attention_setting"]["last_activation"]
    out = [("class_emb.weight", (hp["num_class"], cdim))]
    cond_dim, second_dim = cdim, None
    if hp.get("include_global_feature", False):
        pa = hp["pnet_global_feature_architecture"]
        keep = not hp.get("global_feature_remove_last_activation", True)
        mlp1 = [C0] + list(pa[0][1:])  # (the reference corrects the configured input width, pointnet2_feature_extractor.py:73-75)
        _mlp_spec(mlp1, "global_pnet.mlp1", None, None, out, res_connect=False, last_activation=keep)
        _mlp_spec([2 * mlp1[-1]] + list(pa[1]), "global_pnet.mlp2", None, None, out, res_connect=False, last_activation=keep)
        cond_dim, second_dim = pa[1][-1], cdim
    # (the t-embedding layers exist in every PointNet2Encoder; with include_t false nothing reads them and they get no gradient)
    out += [("fc_t1.weight", (4 * t, t)), ("fc_t1.bias", (4 * t,)), ("fc_t2.weight", (4 * t, 4 * t)), ("fc_t2.bias", (4 * t,))]
    f = arch["feature_dim"]
    for i in range(len(arch["npoint"])):
        c_in = C0 if i == 0 else f[i]
        spec = [c_in + 9, f[i], f[i], f[i + 1]]
        _mlp_spec(spec, "SA_modules.%d.mlps.0" % i, cond_dim, second_dim, out)
        _attention_spec("SA_modules.%d.attention_modules.0" % i, c_in, spec[0], spec[-1], last, out)
    return out


def keypoint_mapper_spec(hp, in_dim, kl):
    """FeatureMapModule of a level whose extractor is a PointNet2Encoder (point_upsample_decoder.py:56-72): the query is the
    extractor's (sampled) output, feature_dim[-1] channels; with KL the mapper emits (mean | logvar)"""
    fm = hp["feature_mapper_setting"]
    spec = [in_dim + 9] + [fm["out_dim"] * kl] * fm["mlp_depth"]
    out = []
    _mlp_spec(spec, "feature_mapper.mlp", None, None, out)
    _attention_spec("feature_mapper.attention_module", hp["architecture"]["feature_dim"][-1], spec[0], spec[-1],
                    hp["attention_setting"]["last_activation"], out)
    return out


# ---------------------------------------------------------------------------------------------------- layers
class EncoderRowsNet(RowsNet):
    """RowsNet + the Mlp and attention forms of the key-point level (module docstring); which form a block takes follows from the
    parameters it has, and the identity residual from `identity_res` (prefixes whose Mlp has res_connect with equal widths)"""

    def __init__(self, spec, identity_res=()):
        super().__init__(spec)
        self.identity_res = frozenset(identity_res)

    def _vec(self, x, prefix, emb, B, S):
        return F.add_vec_rows(x, torch.nn.functional.linear(emb, self._p(prefix + ".weight"), self._p(prefix + ".bias")), B, S)

    def _mlp(self, x, prefix, B, S, cond_emb=None, second_emb=None):
        """Mlp_plus_t_emb.forward without t (pointnet2_modules.py:119-176)"""
        assert not self._has(prefix + ".fc.weight")
        h = self._shared(x, prefix + ".first_mlp", B, S)
        if self._has(prefix + ".second_mlp.1.group_norm.weight"):
            h = self._shared(h, prefix + ".second_mlp", B, S)
        else:  # remove_last_activation: the convolution alone
            h = F.conv_rows(h, self._p(prefix + ".second_mlp.0.weight"), self._p(prefix + ".second_mlp.0.bias"))
        if self._has(prefix + ".fc_condition.weight"):
            h = self._vec(h, prefix + ".fc_condition", cond_emb, B, S)
        if self._has(prefix + ".rest_mlp.0.weight"):
            h = self._shared(h, prefix + ".rest_mlp", B, S)
        if self._has(prefix + ".fc_second_condition.weight"):
            h = self._vec(h, prefix + ".fc_second_condition", second_emb, B, S)
        if self._has(prefix + ".res_connect.weight"):
            h = h + F.conv_rows(x, self._p(prefix + ".res_connect.weight"), self._p(prefix + ".res_connect.bias"))
        elif prefix in self.identity_res:
            h = h + x
        return h

    def _attention(self, feat, grouped, out, prefix, B, S, K):
        """AttentionModule.forward (attention.py:70-96); without feat_out_conv.1 the values are the convolution's output as it is"""
        if self._has(prefix + ".feat_out_conv.1.group_norm.weight"):
            return RowsNet._attention(self, feat, grouped, out, prefix, B, S, K)
        P = self._p
        q = F.conv_rows(feat, P(prefix + ".feat_conv.weight"), P(prefix + ".feat_conv.bias"))
        k = F.conv_rows(grouped, P(prefix + ".grouped_feat_conv.weight"), P(prefix + ".grouped_feat_conv.bias"))
        C1, C2 = P(prefix + ".feat_conv.weight").shape[0], P(prefix + ".grouped_feat_conv.weight").shape[0]
        s = F.concat_qk(q, k, K, C1, C2)
        s = F.gn_rows(s, P(prefix + ".weight_conv.1.group_norm.weight"), P(prefix + ".weight_conv.1.group_norm.bias"),
                      B, S, min(32, C1 + C2), False, False)
        s = F.conv_rows(s, P(prefix + ".weight_conv.2.weight"), P(prefix + ".weight_conv.2.bias"))
        inter = P(prefix + ".weight_conv.2.weight").shape[0]
        s = F.gn_rows(s, P(prefix + ".weight_conv.4.group_norm.weight"), P(prefix + ".weight_conv.4.group_norm.bias"),
                      B, S, min(32, inter), True, False)
        scores = F.conv_rows(s, P(prefix + ".weight_conv.5.weight"), P(prefix + ".weight_conv.5.bias"))
        cout = P(prefix + ".weight_conv.5.weight").shape[0]
        v = F.conv_rows(out, P(prefix + ".feat_out_conv.0.weight"), P(prefix + ".feat_out_conv.0.bias"))
        return F.attend_rows(scores, v, K, cout), cout


class TrainablePnet2Stage:
    """Pnet2Stage.forward (pointnet2/models/pnet.py:32-40) on the parameters `prefix`.mlp1 / .mlp2 of an EncoderRowsNet: per-point Mlp,
    max over the points, [per-point | global] Mlp, max over the points.  The maxima are functions.col_max_seg; the global half of the
    concatenation is a per-sample vector added to zero columns (functions.add_vec_rows: its gradient is slide_col_sums_seg)."""

    def __init__(self, net, prefix):
        self.net, self.prefix = net, prefix
        width = lambda m: net._p("%s.%s.%s.0.weight" % (prefix, m, "rest_mlp" if net._has("%s.%s.rest_mlp.0.weight" % (prefix, m))
                                                          else "second_mlp")).shape[0]
        self.c1, self.out_channels = width("mlp1"), width("mlp2")

    def __call__(self, x, B, N):
        """x rows [B * N, ld] -> [B, out_channels]"""
        net, c1 = self.net, self.c1
        f = net._mlp(x, self.prefix + ".mlp1", B, N)
        g, _ = F.col_max_seg(f, B, N, c1)
        wide = F.pad_cols(f[:, :c1], F.ru(2 * c1))
        vec = torch.cat([g.new_zeros(B, c1), g[:, :c1]], dim=1)
        f = net._mlp(F.add_vec_rows(wide, vec, B, N), self.prefix + ".mlp2", B, N)
        return F.col_max_seg(f, B, N, self.out_channels)[0][:, :self.out_channels]


class TrainableEncoder(EncoderRowsNet):
    def __init__(self, hp):
        check_encoder_family(hp)
        arch = hp["architecture"]
        f = arch["feature_dim"]
        C0 = hp["in_fea_dim"] + 3
        ident = ["SA_modules.%d.mlps.0" % i for i in range(len(arch["npoint"])) if (C0 if i == 0 else f[i]) + 9 == f[i + 1]]
        super().__init__(encoder_param_spec(hp), ident)
        self.hp = hp
        self.out_channels = f[-1]
        self.global_pnet_stage = TrainablePnet2Stage(self, "global_pnet") if hp.get("include_global_feature", False) else None

    def forward(self, pointcloud, label):
        """pointcloud (B, N, 3 + in_fea_dim), label (B,) -> (last-level features as rows [B * n, ru(C)], last-level points (B, n, 3));
        C = out_channels"""
        hp, arch = self.hp, self.hp["architecture"]
        B, N = pointcloud.shape[:2]
        assert pointcloud.shape[2] == 3 + hp["in_fea_dim"], (pointcloud.shape, hp["in_fea_dim"])
        # the reference assembles the network's input under torch.no_grad() (pointnet2_feature_extractor.py:150-166)
        pc0 = pointcloud.detach().float()
        pc = torch.cat([pc0, pc0[:, :, 0:3]], dim=2)                                  # attach_position_to_input_feature
        xyz = pc[:, :, 0:3].contiguous()
        C0 = pc.shape[2] - 3
        cond, second = self._p("class_emb.weight")[label.long()], None
        if self.global_pnet_stage is not None:  # the global feature conditions first, the class embedding second (:182-190)
            cond, second = self.global_pnet_stage(F.pad_cols(pc0.reshape(B * N, pc0.shape[2])), B, N), cond
        l_xyz, feats, chans = [xyz], [F.pad_cols(pc[:, :, 3:].reshape(B * N, C0))], [C0]
        for i, npoint in enumerate(arch["npoint"]):                                    # PointnetSAModule (pointnet2_modules.py:222-292)
            pfx = "SA_modules.%d" % i
            src, n_src = l_xyz[i], l_xyz[i].shape[1]
            if n_src <= npoint:                                                        # nothing to sub-sample: every point is a centre
                centres, query = src, feats[i]
            else:
                with torch.no_grad():
                    picked = _ext.furthest_point_sampling(src.contiguous(), npoint)
                    centres = _ext.gather_rows(src, picked)
                query = gather_rows(feats[i], picked, B, n_src, chans[i])
            g, idx, _ = query_and_group_rows(src, centres, feats[i], chans[i], arch["nsample"][i], "nn", include_abs_coordinate=True,
                                             include_center_coordinate=True)
            n_c, K = idx.shape[1:]
            out = self._mlp(g, pfx + ".mlps.0", B, n_c * K, cond, second)
            o, c = self._attention(query, g, out, pfx + ".attention_modules.0", B, n_c * K, K)
            l_xyz.append(centres); feats.append(o); chans.append(c)
        assert chans[-1] == self.out_channels
        return feats[-1], l_xyz[-1]


class TrainableKeypointEncoder(EncoderRowsNet):
    """the key-point level (PointUpsampleDecoder whose extractor is a PointNet2Encoder): feature_extractor.*, feature_mapper.*, and
    the splitting head fc_layer.* that TrainableDecoder.keypoint_encoder holds"""

    def __init__(self, hp, in_dim, apply_kl_regularization):
        arch = hp["architecture"]
        assert "decoder_feature_dim" not in arch, "the key-point level extracts with a PointNet2Encoder"
        fm = hp["feature_mapper_setting"]
        assert fm["neighbor_definition"] == "nn" and fm["mlp_depth"] == 2, "the feature mapper of the family: 'nn' grouping, a two-layer Mlp"
        assert hp["attention_setting"]["add_attention_to_FeatureMapper_module"]
        kl = 2 if apply_kl_regularization else 1
        ident = ["feature_mapper.mlp"] if in_dim + 9 == fm["out_dim"] * kl else []
        ext = copy.deepcopy(hp)
        ext["architecture"]["feature_dim"][-1] *= kl
        feature_extractor = TrainableEncoder(ext)  # (raises outside the family, before any parameter of this level exists)
        super().__init__(keypoint_mapper_spec(hp, in_dim, kl) + _head_spec(hp), ident)
        self.hp, self.in_dim, self.kl = hp, in_dim, apply_kl_regularization
        self.feature_extractor = feature_extractor

    def propagate_feature(self, xyz, feat_rows, new_xyz, label, eps=None, sample_posterior=True):
        """xyz (B, N1, 3) with features as rows [B * N1, ld] (in_dim channels) -> features at the key points new_xyz (B, N2, 3) as
        (rows [B * N2, ld], C) = [extracted | mapped], and the summed KL of the two posteriors (B,) (None without KL).  eps: the pair
        of standard-normal tensors (B, N2, C_extracted), (B, N2, C_mapped) of the two posteriors; with sample_posterior false
        (the posterior's mode) it is not read."""
        fm = self.hp["feature_mapper_setting"]
        B, N1 = xyz.shape[:2]
        N2 = new_xyz.shape[1]
        q, _ = self.feature_extractor(new_xyz, label)
        cq = self.feature_extractor.out_channels
        kl = None
        if self.kl:
            cq //= 2
            q, kl = F.gauss_posterior(q, self._eps_rows(eps, 0, B, N2, cq, sample_posterior), B, N2, cq)
        g, idx, _ = query_and_group_rows(xyz.contiguous(), new_xyz[:, :, 0:3].contiguous(), feat_rows, self.in_dim, fm["nsample"], "nn",
                                         include_abs_coordinate=True, include_center_coordinate=True)
        K = idx.shape[2]
        h = self._mlp(g, "feature_mapper.mlp", B, N2 * K)
        mapped, cm = self._attention(q, g, h, "feature_mapper.attention_module", B, N2 * K, K)
        if self.kl:
            cm //= 2
            mapped, kl2 = F.gauss_posterior(mapped, self._eps_rows(eps, 1, B, N2, cm, sample_posterior), B, N2, cm)
            kl = kl + kl2
        return (F.pad_cols(torch.cat([q[:, :cq], mapped[:, :cm]], dim=1)), cq + cm), kl

    @staticmethod
    def _eps_rows(eps, which, B, N, C, sample):
        if not sample:
            return None
        e = eps[which]
        assert tuple(e.shape) == (B, N, C), (tuple(e.shape), (B, N, C))
        return F.pad_cols(e.detach().float().reshape(B * N, C))


class TrainableAutoencoder(TrainableDecoder):
    """PointAutoencoder(encoder_config, decoder_config_list, apply_kl_regularization, kl_weight, feature_weight) for training"""

    def __init__(self, encoder_config, decoder_config_list, apply_kl_regularization=False, kl_weight=0, feature_weight=None,
                 state_dict=None):
        super().__init__(decoder_config_list)
        self.apply_kl_regularization, self.kl_weight, self.feature_weight = apply_kl_regularization, kl_weight, feature_weight
        self.encoder = TrainableEncoder(copy.deepcopy(encoder_config))
        self.keypoint_encoder = TrainableKeypointEncoder(copy.deepcopy(decoder_config_list[0]), self.encoder.out_channels,
                                                         apply_kl_regularization)
        if state_dict is not None:
            self.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict.items()})

    def posterior_shapes(self, B, n):
        """the shapes of the two eps tensors propagate_feature takes for B samples of n key points"""
        hp0 = self.configs[0]
        return (B, n, hp0["architecture"]["feature_dim"][-1]), (B, n, hp0["feature_mapper_setting"]["out_dim"])

    def encode(self, pointcloud, keypoint, label, eps=None, sample_posterior=True):
        """pointcloud (B, N, 3 + in_fea_dim), keypoint (B, 16, 3) -> (feature_at_keypoint (B, 16, C), kl (B,) or None)"""
        B, N2 = keypoint.shape[:2]
        keypoint = keypoint.float()
        if self.apply_kl_regularization and sample_posterior and eps is None:
            eps = tuple(torch.randn(s, device=keypoint.device) for s in self.posterior_shapes(B, N2))
        feat, last_xyz = self.encoder(pointcloud, label)
        (rows, C), kl = self.keypoint_encoder.propagate_feature(last_xyz, feat, keypoint, label, eps, sample_posterior)
        return rows[:, :C].reshape(B, N2, C), kl

    def forward(self, pointcloud, keypoint, label, eps=None, sample_posterior=True, fps_start_idx=None):
        """-> (l_xyz_decoder, feature_at_keypoint, kl)"""
        feature_at_keypoint, kl = self.encode(pointcloud, keypoint, label, eps, sample_posterior)
        return self.decode(keypoint, feature_at_keypoint, label, fps_start_idx=fps_start_idx), feature_at_keypoint, kl
