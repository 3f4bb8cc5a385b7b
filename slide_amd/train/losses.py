"""Training losses of the two latent DDPMs, restated from the reference (forward = slide_amd.train.denoiser.TrainableDenoiser or any
callable net(x_t, ts, label) -> eps prediction).  Random timesteps and noise are drawn here unless they are passed in (the parity
tests inject the reference's); and the autoencoder's Chamfer losses (calc_cd_loss, autoencoder_losses) on the differentiable
Chamfer sums of functions.ChamferCD, with the decode side's training loss (decoder_training_loss) and the whole autoencoder's
(autoencoder_training_loss) on top; and the refinement network's grid loss through DPSR (psr_grid_loss)."""
import numpy as np
import torch

from ..diffusion import calc_diffusion_hyperparams, get_beta_schedule

_TABLES = {}  # (schedule, device) -> alpha_bar table on the device (an upload per step would be a blocking host -> device copy)


def _table(key, device, make):
    key = (key, str(device))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.as_tensor(np.asarray(make(), dtype=np.float64), device=device).float()
    return t


def position_training_loss(net, X, diffusion_config, label, steps=None, z=None):
    """util.training_loss (pointnet2/util.py:262-300) with nn.MSELoss: x_t = sqrt(abar_t) x_0 + sqrt(1 - abar_t) z,
    loss = mean((eps_theta(x_t, t, label) - z)^2) over every element of the batch.  X (B, N, 3)."""
    T = int(diffusion_config["T"])
    abar = _table(("ddpm",) + tuple(sorted(diffusion_config.items())), X.device,
                  lambda: np.asarray(calc_diffusion_hyperparams(**diffusion_config)["Alpha_bar"]))
    B = X.shape[0]
    if steps is None:
        steps = torch.randint(T, size=(B,), device=X.device)
    if z is None:
        z = torch.randn_like(X)
    a = abar[steps.long()].reshape(B, 1, 1)
    x_t = torch.sqrt(a) * X + torch.sqrt(1 - a) * z
    eps = net(x_t, steps.reshape(B).float(), label)
    return torch.nn.functional.mse_loss(eps, z)


def latent_training_loss(net, x, keypoint, label, standard_diffusion_config, steps=None, z=None):
    """LatentDiffusion.train_loss (pointnet2/diffusion_utils/diffusion.py:319-341) on given latents x (B, N, kd + F) = [key points |
    features] (the reference gets them from its frozen autoencoder's encode()): with keypoint_conditional the key points are not
    diffused and their loss weight is 0; per-sample loss = mean over points of
    w_kp * sum_{c < kd} (eps - z)^2 + w_feat * mean_{c >= kd} (eps - z)^2.  -> (B,)"""
    cfg = standard_diffusion_config
    sched = (cfg["beta_schedule"], cfg["beta_start"], cfg["beta_end"], cfg["num_diffusion_timesteps"])
    ac = _table(sched, x.device, lambda: np.cumprod(1.0 - get_beta_schedule(*sched), axis=0))  # extract(): float64 table cast to float32
    conditional = cfg.get("keypoint_conditional", False)
    w_kp = 0.0 if conditional else cfg.get("keypoint_position_loss_weight", 1.0)
    w_f = cfg.get("feature_loss_weight", 1.0)
    B = x.shape[0]
    kd = keypoint.shape[2]
    if steps is None:
        steps = torch.randint(int(cfg["num_diffusion_timesteps"]), size=(B,), device=x.device)
    if z is None:
        z = torch.randn_like(x)
    a = ac[steps.long()].reshape(B, 1, 1)
    x_t = torch.sqrt(a) * x + torch.sqrt(1 - a) * z
    if conditional:
        x_t = torch.cat([keypoint, x_t[:, :, kd:]], dim=2)
    out = net(x_t, steps.float(), label) * cfg.get("model_output_scale_factor", 1.0)
    mse = (out - z) ** 2
    loss = w_kp * mse[:, :, :kd].sum(dim=2) + w_f * mse[:, :, kd:].mean(dim=2)
    return loss.mean(dim=1)


def calc_cd_loss(output, gt, calc_f1=False, f1_threshold=1e-4, normal_loss_type='mse'):
    """differentiable calc_cd (pointnet2/metrics_point_cloud/chamfer_and_f1.py:242-265) of output vs gt (B, N, C >= 3; xyz = channels
    0:3, features behind them): the reference's dict -- cd_p, cd_t, with features cd_feature_p / cd_feature_t of the `mse` term, with
    calc_f1 the (non-differentiable) F-score -- each (B,), values bit-equal to metrics_point_cloud.chamfer_and_f1.calc_cd, gradients
    into both clouds through functions.ChamferCD (one backward launch).  Where two points coincide (or their features do) the square
    root in cd_p / cd_feature_p contributes the subgradient 0; the reference's autograd yields NaN there.
    normal_loss_type='cos' has no backward kernel: NotImplementedError."""
    from .functions import chamfer_cd
    if normal_loss_type != 'mse':
        if normal_loss_type == 'cos':
            raise NotImplementedError("calc_cd_loss: the `cos` feature term has no backward kernel (normal_loss_type='mse' only)")
        raise ValueError("normal_loss_type must be 'mse' or 'cos'")
    red = chamfer_cd(output, gt, f1_threshold)
    n_gt, n_out = gt.shape[1], output.shape[1]
    result = {}
    result['cd_p'] = (red[:, 0, 1] / n_gt + red[:, 1, 1] / n_out) / 2
    result['cd_t'] = red[:, 0, 0] / n_gt + red[:, 1, 0] / n_out
    if gt.shape[2] > 3:
        result['cd_feature_p'] = (red[:, 0, 4] / n_gt + red[:, 1, 4] / n_out) / 2
        result['cd_feature_t'] = red[:, 0, 3] / n_gt + red[:, 1, 3] / n_out
    if calc_f1:
        cnt = red.detach()
        p1 = cnt[:, 0, 2] / n_gt
        p2 = cnt[:, 1, 2] / n_out
        f = 2 * p1 * p2 / (p1 + p2)
        result['f1'] = torch.where(torch.isnan(f), torch.zeros_like(f), f)
    return result


def autoencoder_losses(l_xyz_decoder, pointcloud, feature_weight, loss_type='cd_p', kl_loss=None, kl_weight=0,
                       apply_kl_regularization=False, fps_start_idx=None):
    """the loss loop of PointAutoencoder.forward (pointnet2/models/autoencoder.py:60-87) on given decoder levels: l_xyz_decoder =
    [key points, level 1, ...]; every level i >= 1 is scored against `pointcloud` (B, N, 3 | 6) farthest-point-sampled to the level's
    size (not differentiated; fps_start_idx (B,) int pins the start, None draws it) with calc_cd_loss(..., calc_f1=True,
    normal_loss_type='mse'); training_loss = cd_p | cd_t + feature_weight[i-1] x the matching feature term (feature_weight None: 0)
    and, with KL regularisation and kl_weight > 0, + kl_weight x kl_loss at the last level only.  -> loss_list of the reference's
    dicts; gradients flow into the levels and kl_loss."""
    from .. import _ext
    assert pointcloud.shape[2] in [3, 6]
    if loss_type not in ('cd_p', 'cd_t'):
        raise Exception('loss type %s is not supported yet' % loss_type)
    has_feature = pointcloud.shape[2] > 3
    loss_list = []
    for i in range(1, len(l_xyz_decoder)):
        uvw = l_xyz_decoder[i]
        with torch.no_grad():
            downsampled, _ = _ext.sample_farthest_points(pointcloud.detach().contiguous(), K=uvw.shape[1],
                                                         random_start_point=fps_start_idx is None, start_idx=fps_start_idx)
        loss_dict = calc_cd_loss(uvw, downsampled, calc_f1=True, f1_threshold=0.0001, normal_loss_type='mse')
        w = 0 if feature_weight is None else feature_weight[i - 1]
        loss = loss_dict[loss_type]
        if has_feature:
            loss = loss + loss_dict['cd_feature_' + loss_type[-1]] * w
        if apply_kl_regularization and kl_weight > 0:
            if i == len(l_xyz_decoder) - 1:  # the KL term is added once, at the last level
                loss_dict['kl_loss'] = kl_loss
                loss = loss + kl_weight * loss_dict['kl_loss']
            else:
                loss_dict['kl_loss'] = torch.zeros_like(loss)
        loss_dict['training_loss'] = loss
        loss_list.append(loss_dict)
    return loss_list


def _sum_of_level_means(loss_list):
    loss = loss_list[0]['training_loss'].mean()
    for d in loss_list[1:]:
        loss = loss + d['training_loss'].mean()
    return loss


def autoencoder_training_loss(ae, pointcloud, keypoint, label, eps=None, loss_type='cd_p', sample_posterior=True, fps_start_idx=None):
    """the training loss of the whole autoencoder (slide_amd.train.encoder.TrainableAutoencoder): the reference's forward
    (pointnet2/models/autoencoder.py:48-87: encode, the key-point level's posteriors and KL, decode, autoencoder_losses with the KL
    term at the last level) and loss = the sum over the levels of training_loss.mean() (pointnet2/train_autoencoder.py:179-181).
    -> (loss, loss_list); loss_list[-1] also carries 'feature_at_keypoint' (detached).  eps: the pair of standard-normal tensors of
    the two posteriors (ae.posterior_shapes); None draws them with torch.randn on the device.  Capturable: under
    GraphedTrainingStep pass static eps tensors and refill them (normal_()) between replays -- the kernels never draw numbers."""
    l_xyz_decoder, feature_at_keypoint, kl = ae(pointcloud, keypoint, label, eps=eps, sample_posterior=sample_posterior,
                                                fps_start_idx=fps_start_idx)
    loss_list = autoencoder_losses(l_xyz_decoder, pointcloud, ae.feature_weight, loss_type=loss_type, kl_loss=kl, kl_weight=ae.kl_weight,
                                   apply_kl_regularization=ae.apply_kl_regularization, fps_start_idx=fps_start_idx)
    loss_list[-1]['feature_at_keypoint'] = feature_at_keypoint.detach()
    return _sum_of_level_means(loss_list), loss_list


def decoder_training_loss(decoder, keypoint, feature_at_keypoint, label, pointcloud, feature_weight, loss_type='cd_p', fps_start_idx=None):
    """the training loss of the decode side (slide_amd.train.decoder.TrainableDecoder): l_xyz_decoder = decoder.decode(keypoint,
    feature_at_keypoint, label), loss_list = autoencoder_losses on its levels against `pointcloud`, loss = the sum over the levels of
    training_loss.mean() (pointnet2/train_autoencoder.py:179-181).  -> (loss, loss_list); gradients reach every decode-side parameter,
    the latent features and the key points.  Capturable: GraphedTrainingStep(decoder, optimizer, lambda: decoder_training_loss(...)[0])
    with a fixed fps_start_idx tensor or None (drawn on the device)."""
    l_xyz_decoder = decoder.decode(keypoint, feature_at_keypoint, label, fps_start_idx=fps_start_idx)
    loss_list = autoencoder_losses(l_xyz_decoder, pointcloud, feature_weight, loss_type=loss_type, fps_start_idx=fps_start_idx)
    return _sum_of_level_means(loss_list), loss_list


def psr_grid_loss(points, normals, psr_gt, dpsr, scale=1, explicit_normalize=False, psr_tanh=False):
    """the refinement network's training loss on given refined points: the tail of network_output_to_dpsr_grid
    (pointnet2/dpsr_evaluation.py:77-84: shapenet_psr_normalize or the division by the dataset scale, clamp(x / 1.2 + 0.5, 0, 0.99),
    DPSR) and the loss of pointnet2/train_upsampler.py (tanh on both grids with psr_tanh, then nn.MSELoss).  points / normals
    (B, N, 3) fp32 CUDA, psr_gt (B, r, r, r), dpsr a pointnet2 dpsr_utils.dpsr.DPSR -> scalar; differentiable in points and normals
    (the clamp and the tanh are torch ops, DPSR is functions.DpsrGrid)."""
    if explicit_normalize:
        minn = points.min(dim=1, keepdim=True)[0]
        maxx = points.max(dim=1, keepdim=True)[0]
        points = (points - (maxx + minn) / 2) / (maxx - minn).max(dim=2, keepdim=True)[0] * 0.99  # shapenet_psr_normalize
    else:
        points = points / scale / 2
    points = torch.clamp(points / 1.2 + 0.5, min=0, max=0.99)
    psr_grid = dpsr(points.contiguous(), normals.contiguous())
    if psr_tanh:
        psr_grid, psr_gt = torch.tanh(psr_grid), torch.tanh(psr_gt)
    return torch.nn.functional.mse_loss(psr_grid, psr_gt)
