"""Point-cloud metrics (reference: pointnet2/metrics_point_cloud/): Chamfer distance and F-score on the HIP kernels of
slide_amd/csrc/chamfer.hip, and the set-level generation metrics (reference: pointnet2/models/pvd/metrics/evaluation_metrics.py):
MMD-CD / COV-CD / 1-NNA-CD on slide_amd/csrc/chamfer_pairwise.hip, the JSD on slide_amd/csrc/occupancy_grid.hip, and the approximate
Earth Mover's Distance (emd.py; MMD-EMD / COV-EMD / 1-NNA-EMD in generation_metrics.py) on slide_amd/csrc/emd_pairwise.hip.

The JSD functions are also reachable from the package (resolved on first use, so importing the package stays free of side effects)."""
__all__ = ["unit_cube_grid_point_cloud", "entropy_of_occupancy_grid", "jensen_shannon_divergence", "jsd_between_point_cloud_sets"]


def __getattr__(name):
    if name in __all__:
        from . import generation_metrics
        return getattr(generation_metrics, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
