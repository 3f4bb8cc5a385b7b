"""Point-cloud metrics (reference: pointnet2/metrics_point_cloud/): Chamfer distance and F-score on the HIP kernels of
slide_amd/csrc/chamfer.hip."""
