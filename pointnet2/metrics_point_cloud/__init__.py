"""Point-cloud metrics (reference: pointnet2/metrics_point_cloud/): Chamfer distance and F-score on the HIP kernels of
slide_amd/csrc/chamfer.hip, and the set-level generation metrics (MMD-CD / COV-CD / 1-NNA-CD, reference:
pointnet2/models/pvd/metrics/evaluation_metrics.py) on slide_amd/csrc/chamfer_pairwise.hip."""
