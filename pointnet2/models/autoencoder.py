"""`PointAutoencoder` (reference: pointnet2/models/autoencoder.py:11-45).  DECODE: 16 key points + 48-dim latent features ->
256 -> 1024 -> 2048 points x 6 (xyz + normal).  ENCODE (built when an encoder config is given; SURVEY.md section 8(f) item
1): 2048 x 6 input cloud -> `PointNet2Encoder` (2048 -> 1024 -> 256 -> 64 -> 32 points, K = 32) -> the key-point encoder's
`propagate_feature` -> 48-dim latent features at the 16 key points.  Parameter names follow the reference (`encoder.*`,
`keypoint_encoder.*`, `decoder.decoders.{i}.*`) so `load_state_dict(ckpt['model_state_dict'])` fills it from a released
checkpoint.  `forward` is the reference's EVALUATION forward (autoencoder.py:48-87: reconstruction levels + Chamfer / F1 /
normal / KL losses per level, scored by metrics_point_cloud.chamfer_and_f1 on the HIP Chamfer kernels) without autograd; training
(a forward with grad, the backward) is out of scope."""
import torch
import torch.nn as nn

from models.keypoint_decoder import KeypointDecoder, level_feature_dim
from models.point_upsample_decoder import PointUpsampleDecoder
from models.pointnet2_feature_extractor import PointNet2Encoder
from metrics_point_cloud.chamfer_and_f1 import calc_cd
from slide_amd import _ext as _hip


class PointAutoencoder(nn.Module):
    def __init__(self, encoder_config, decoder_config_list, apply_kl_regularization=False, kl_weight=0, feature_weight=None):
        super().__init__()
        self.apply_kl_regularization, self.kl_weight, self.feature_weight = apply_kl_regularization, kl_weight, feature_weight
        enc_dim = encoder_config["architecture"]["feature_dim"][-1] if encoder_config is not None else 0
        self.has_encoder = encoder_config is not None
        if self.has_encoder:
            self.encoder = PointNet2Encoder(encoder_config)
        self.keypoint_encoder = PointUpsampleDecoder(decoder_config_list[0], in_dim=enc_dim,
                                                     apply_kl_regularization=apply_kl_regularization,
                                                     decode_only=not self.has_encoder)
        self.decoder = KeypointDecoder(decoder_config_list[1:], level_feature_dim(decoder_config_list[0]))

    @torch.no_grad()
    def encode(self, pointcloud, keypoint, ts=None, label=None, sample_posterior=True):
        """pointcloud (B,N,6), keypoint (B,16,3) -> latent features at the key points (B,16,48)"""
        if not self.has_encoder:
            raise NotImplementedError("this autoencoder was built decode-only (no encoder config)")
        out, l_xyz, _ = self.encoder(pointcloud, ts=ts, label=label)
        feat, _ = self.keypoint_encoder.propagate_feature(l_xyz[-1], out, keypoint, ts=ts, label=label,
                                                          sample_posterior=sample_posterior)
        return feat

    def forward(self, pointcloud, keypoint, ts=None, label=None, loss_type='cd_p', sample_posterior=True,
                return_keypoint_feature=False, fps_start_idx=None):
        """the reference's forward for EVALUATION (autoencoder.py:48-87), under torch.no_grad() or with no parameter requiring grad:
        pointcloud (B,N,3|6), keypoint (B,16,3) -> (l_xyz_decoder, loss_list[, feature_at_keypoint]).  l_xyz_decoder = [key points,
        every decoder level]; loss_list[i-1] scores level i >= 1 against the input cloud farthest-point-sampled to the level's size:
        the dict of calc_cd(level, downsampled, calc_f1=True, f1_threshold=1e-4, normal_loss_type='mse') plus 'training_loss'
        (cd_p or cd_t + feature_weight[i-1] x the matching feature term) and, with KL regularisation and kl_weight > 0, 'kl_loss'
        (the key-point encoder's KL at the last level, zeros before it; added to the last level's training_loss x kl_weight).
        fps_start_idx (B,) int: the start point of every farthest point sampling (decoder levels and input down-sampling); None
        draws random starts like the reference's random_start_point=True."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("training (reconstruction / KL losses) is out of scope (SURVEY.md section 8(f) item 4)")
        if not self.has_encoder:
            raise NotImplementedError("this autoencoder was built decode-only (no encoder config)")
        with torch.no_grad():
            out, l_xyz_encoder, _ = self.encoder(pointcloud, ts=ts, label=label)
            feature_at_keypoint, kl_loss = self.keypoint_encoder.propagate_feature(
                l_xyz_encoder[-1], out, keypoint, ts=ts, label=label, sample_posterior=sample_posterior, return_kl=True)
            new_xyz = self.keypoint_encoder.upsample_points(feature_at_keypoint, keypoint, fps_start_idx)
            l_xyz_decoder = self.decoder(keypoint[:, :, 0:3], feature_at_keypoint, new_xyz, ts=ts, label=label,
                                         fps_start_idx=fps_start_idx)
            assert pointcloud.shape[2] in [3, 6]
            loss_list = []
            for i in range(1, len(l_xyz_decoder)):
                # level 0 is the user's key points: not supervised
                uvw = l_xyz_decoder[i]
                downsampled, _ = _hip.sample_farthest_points(pointcloud.contiguous(), K=uvw.shape[1],
                                                             random_start_point=fps_start_idx is None, start_idx=fps_start_idx)
                loss_dict = calc_cd(uvw, downsampled, calc_f1=True, f1_threshold=0.0001, normal_loss_type='mse')
                feature_weight = 0 if self.feature_weight is None else self.feature_weight[i - 1]
                if loss_type not in ('cd_p', 'cd_t'):
                    raise Exception('loss type %s is not supported yet' % loss_type)
                loss = loss_dict[loss_type]
                if 'cd_feature_p' in loss_dict:  # (the reference requires features: a 3-channel cloud raised a KeyError there)
                    loss = loss + loss_dict['cd_feature_' + loss_type[-1]] * feature_weight
                if self.apply_kl_regularization and self.kl_weight > 0:
                    # the KL term is added once, at the last level
                    if i == len(l_xyz_decoder) - 1:
                        loss_dict['kl_loss'] = kl_loss
                        loss = loss + self.kl_weight * loss_dict['kl_loss']
                    else:
                        loss_dict['kl_loss'] = torch.zeros_like(loss)
                loss_dict['training_loss'] = loss
                loss_list.append(loss_dict)
        if return_keypoint_feature:
            return l_xyz_decoder, loss_list, feature_at_keypoint
        return l_xyz_decoder, loss_list

    @torch.no_grad()
    def decode(self, keypoint, feature_at_keypoint, ts=None, label=None, fps_start_idx=None):
        new_xyz = self.keypoint_encoder.upsample_points(feature_at_keypoint, keypoint, fps_start_idx)
        return self.decoder(keypoint[:, :, 0:3], feature_at_keypoint, new_xyz, ts=ts, label=label,
                            fps_start_idx=fps_start_idx)[-1]
