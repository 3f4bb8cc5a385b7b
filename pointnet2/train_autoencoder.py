#!/usr/bin/env python
"""Autoencoder training CLI on the HIP training path -- counterpart of the reference's pointnet2/train_autoencoder.py: the whole
PointAutoencoder (encoder, key-point level with its KL posteriors, decoder levels) is trained on the reconstruction losses of
every level plus the KL term (slide_amd.train.losses.autoencoder_training_loss on slide_amd.train.encoder.TrainableAutoencoder).
Same JSON config as the reference (pointnet_config with encoder_config_file / decoder_config_file / apply_kl_regularization /
kl_weight / feature_weight, train_config, shapenet_psr_dataset_config) and the same checkpoint files (`pointnet_ckpt_{iter}.pkl`:
iter, model_state_dict, optimizer_state_dict, training_time_seconds; resumed from the highest), which
`models.autoencoder.PointAutoencoder` loads strictly and load_evaluate.py scores.  Adam; one process per GPU under
torch.distributed.run, gradients averaged with slide_amd.train.dp.allreduce_gradients.
Not the reference's: the ShapeNet loader and its augmentation (clouds come from `--dataset_npz`: points, normals, label),
tensorboard, the evaluation passes inside the loop."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", type=str, required=True)
    ap.add_argument("--dataset_npz", type=str, required=True, help="training clouds: points (n, P, 3), normals (n, P, 3), label (n,)")
    ap.add_argument("--n_iters", type=int, default=None, help="default: train_config n_epochs x the batches of an epoch")
    ap.add_argument("--iters_per_ckpt", type=int, default=None, help="default: train_config epochs_per_ckpt x the batches of an epoch")
    ap.add_argument("--root_directory", type=str, default=None)
    ap.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def resolve(a, per_epoch=None):
    """everything the loop needs from the arguments and the config files, without a device: the network's constructor arguments, the
    output directory, the key-point settings and -- given the batches of an epoch -- the iteration counts"""
    from slide_amd.json_reader import autoencoder_read_config, read_json_file
    cfg = read_json_file(a.config)
    hp, tc, dc = cfg["pointnet_config"], cfg["train_config"], cfg["shapenet_psr_dataset_config"]
    if dc.get("keypoints_source", "farthest_points_sampling") != "farthest_points_sampling":
        raise ValueError("keypoints_source %r is not supported: key points come from farthest point sampling" % dc["keypoints_source"])
    enc, decs = autoencoder_read_config(os.path.dirname(os.path.abspath(a.config)), cfg)
    r = dict(encoder_config=enc, decoder_config_list=decs, apply_kl_regularization=bool(hp.get("apply_kl_regularization", False)),
             kl_weight=float(hp.get("kl_weight", 0)), feature_weight=hp.get("feature_weight"),
             out_dir=os.path.join(a.root_directory or tc["root_directory"], hp.get("model_name", "autoencoder"), tc["output_directory"]),
             batch_size=int(dc["batch_size"]), num_keypoints=int(dc["num_keypoints"]),
             add_centroid=bool(dc.get("add_centroid_to_keypoints", True)), random_subsample=bool(dc.get("random_sample_keypoints", False)),
             keypoint_noise=float(dc.get("keypoint_noise_magnitude", 0)), learning_rate=float(tc["learning_rate"]),
             ckpt_iter=tc.get("ckpt_iter", "max"), iters_per_logging=int(tc.get("iters_per_logging", 50)))
    if r["random_subsample"] and r["add_centroid"]:
        raise ValueError("random_sample_keypoints needs add_centroid_to_keypoints false")
    if per_epoch is not None:
        r["n_iters"] = a.n_iters if a.n_iters is not None else int(tc["n_epochs"]) * per_epoch
        r["iters_per_ckpt"] = a.iters_per_ckpt if a.iters_per_ckpt is not None else int(tc["epochs_per_ckpt"]) * per_epoch
        if r["iters_per_ckpt"] < 1:
            raise ValueError("iters_per_ckpt must be at least 1")
    return r


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    import torch
    from slide_amd.generation import init_distributed
    from slide_amd.train.dp import allreduce_gradients, broadcast_parameters
    from slide_amd.train.encoder import TrainableAutoencoder
    from slide_amd.train.losses import autoencoder_training_loss
    from slide_amd.train.trainer import find_max_ckpt, npz_batches, sample_keypoints

    rank, world, dev, _ = init_distributed()
    torch.manual_seed(a.seed + rank)
    log = print if rank == 0 else (lambda *_: None)
    s = resolve(a)
    B = s["batch_size"]
    batches = npz_batches(a.dataset_npz, B, rank, world, seed=a.seed)
    s = resolve(a, max(1, len(batches)))
    net = TrainableAutoencoder(s["encoder_config"], s["decoder_config_list"], apply_kl_regularization=s["apply_kl_regularization"],
                               kl_weight=s["kl_weight"], feature_weight=s["feature_weight"]).reset_parameters(a.seed).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=s["learning_rate"])
    time0 = time.time()
    ckpt_iter = find_max_ckpt(s["out_dir"]) if s["ckpt_iter"] == "max" else s["ckpt_iter"]
    n_iter = 0
    if ckpt_iter is not None and int(ckpt_iter) >= 0:
        ck = torch.load(os.path.join(s["out_dir"], "pointnet_ckpt_%d.pkl" % int(ckpt_iter)), map_location="cpu")
        net.load_state_dict(ck["model_state_dict"])
        opt.load_state_dict(ck["optimizer_state_dict"])
        time0 -= ck.get("training_time_seconds", 0)
        n_iter = int(ck["iter"]) + 1
        log("checkpoint of iteration %d loaded (trained for %d s)" % (int(ck["iter"]), ck.get("training_time_seconds", 0)))
    broadcast_parameters(net)
    bucket, t_log, it = None, time.time(), iter(batches)
    while n_iter < s["n_iters"]:
        try:
            batch = next(it)
        except StopIteration:
            it = iter(batches)  # next epoch
            batch = next(it)
        # train_autoencoder.py:160-177: renormalised normals, key points from the positions (+ noise), the cloud = [xyz | normal]
        X = torch.as_tensor(batch["points"], dtype=torch.float32, device=dev)
        normals = torch.as_tensor(batch["normals"], dtype=torch.float32, device=dev)
        normals = normals / torch.norm(normals, p=2, dim=2, keepdim=True)
        label = torch.as_tensor(batch["label"] if "label" in batch else np.zeros(B, np.int64)).to(dev)
        keypoint, _ = sample_keypoints(X, s["num_keypoints"], add_centroid=s["add_centroid"], random_subsample=s["random_subsample"])
        if s["keypoint_noise"] > 0:
            keypoint = keypoint + s["keypoint_noise"] * torch.randn_like(keypoint)
        opt.zero_grad(set_to_none=False)
        loss, loss_list = autoencoder_training_loss(net, torch.cat([X, normals], dim=2), keypoint.contiguous(), label, loss_type="cd_p")
        loss.backward()
        bucket = allreduce_gradients(net, bucket)
        opt.step()
        if n_iter % s["iters_per_logging"] == 0:
            kl = loss_list[-1].get("kl_loss")
            log("iteration: %d \tloss: %.6f \tkl: %s \ttime: %.2fs" % (n_iter, float(loss), "-" if kl is None else "%.4f" % float(kl.mean()),
                                                                    time.time() - t_log))
            t_log = time.time()
        if n_iter > 0 and (n_iter + 1) % s["iters_per_ckpt"] == 0 and rank == 0:
            os.makedirs(s["out_dir"], exist_ok=True)
            torch.save({"iter": n_iter, "model_state_dict": {k: v.detach().cpu() for k, v in net.state_dict().items()},
                        "optimizer_state_dict": opt.state_dict(), "training_time_seconds": int(time.time() - time0)},
                       os.path.join(s["out_dir"], "pointnet_ckpt_%d.pkl" % n_iter))
            log("model at iteration %d is saved" % n_iter)
        n_iter += 1
    log("trained to iteration %d; checkpoints in %s" % (n_iter - 1, s["out_dir"]))


if __name__ == "__main__":
    main()
