"""Training step of the latent DDPMs on the HIP row-major path, and the autoencoder's Chamfer losses.

functions.py  torch.autograd.Functions over the module path's forward kernels and the backward kernels of csrc/train_ops.hip
              (include/slide_train.h): 1x1 convolution / linear, MyGroupNorm (+ ReLUs), grouping, relu([q | k]), softmax-weighted sum
denoiser.py   PointNet2CloudCondition (pointnet2/models/pointnet2_with_pcld_condition.py:286-489) built from them, with the
              reference's parameter names
              (pad columns zero); ChamferCD: the fused Chamfer sums with csrc/chamfer_bwd.hip as their backward
grouping.py   query_and_group_rows / group_knn_rows: QueryAndGroup and group_knn on rows (search without gradients, then the grouping
              layer), differentiable in the features and in both coordinate tensors (csrc/group_coord_bwd.hip)
losses.py     util.training_loss (pointnet2/util.py:262-300) and LatentDiffusion.train_loss
              (pointnet2/diffusion_utils/diffusion.py:319-341); calc_cd_loss and autoencoder_losses, the differentiable calc_cd and the
              autoencoder's loss loop (pointnet2/models/autoencoder.py:60-87) on given decoder levels
cloudnet.py   TrainableCloudNet: PointNet2CloudCondition of the decoder-level configs for any input size (FPS levels, cross-level
              kNN feature propagation), on the same layers; add_vec_rows (functions.py) carries the class embedding, its backward is
              slide_col_sums_seg
decoder.py    TrainableDecoderLevel / TrainableDecoder: the decode side of the autoencoder with the reference's state-dict names;
              losses.decoder_training_loss puts autoencoder_losses on its levels
encoder.py    TrainableEncoder (PointNet2Encoder), TrainablePnet2Stage, TrainableKeypointEncoder (the key-point level: extractor, feature
              mapper, the two KL posteriors) and TrainableAutoencoder; functions.col_max_seg / gauss_posterior on csrc/encoder_ops.hip;
              losses.autoencoder_training_loss is the reference's forward plus its loss
dp.py         data-parallel gradient averaging: bucketed all-reduce over torch.distributed (RCCL over xGMI; gloo in the CPU tests),
              the counterpart of pointnet2/distributed.py:99-151
There is no CPU fallback: every Function launches kernels of libslide_hip.so."""
from .grouping import group_knn_rows, query_and_group_rows  # noqa: E402,F401
