"""CPU: the product library exports the DPSR backward entry points of include/slide_hip.h Part 5, the ctypes layer lists them, and
their argument checks run on the host before any launch."""
from slide_amd import _lib, build

NAMES = ("slide_dpsr_bwd_sums", "slide_dpsr_bwd_dpre", "slide_dpsr_spectral_adj", "slide_dpsr_bwd_points", "slide_dpsr_grid_bwd")


def test_dpsr_backward_symbols_exported():
    build.build()
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(L, n), n


def test_dpsr_backward_entry_points_reject_bad_arguments_without_a_launch():
    """-2 for a size outside the kernels' scope or a NULL array, 0 for an empty batch -- every call returns before a launch"""
    build.build()
    L = _lib.lib()
    z = None
    ws = (z,) * 12
    assert L.slide_dpsr_bwd_sums(1, 1, z, z, z, z, z) == -2 and L.slide_dpsr_bwd_sums(1, 1025, z, z, z, z, z) == -2
    assert L.slide_dpsr_bwd_sums(-1, 16, z, z, z, z, z) == -2 and L.slide_dpsr_bwd_sums(1, 16, z, z, z, z, z) == -2  # NULL
    assert L.slide_dpsr_bwd_sums(0, 16, z, z, z, z, z) == 0
    assert L.slide_dpsr_bwd_dpre(1, 4, 1, z, z, z, z, z, 1, 1, z, z) == -2 and L.slide_dpsr_bwd_dpre(1, 0, 16, z, z, z, z, z, 1, 1, z, z) == -2
    assert L.slide_dpsr_bwd_dpre(1, 4, 16, z, z, z, z, z, 0, 0, z, z) == -2  # NULL
    assert L.slide_dpsr_bwd_dpre(0, 4, 16, z, z, z, z, z, 1, 1, z, z) == 0
    assert L.slide_dpsr_bwd_points(1, 4, 1, z, z, z, z, z, z, 1, 1, z, z, z, z) == -2
    assert L.slide_dpsr_bwd_points(1, -1, 16, z, z, z, z, z, z, 1, 1, z, z, z, z) == -2
    assert L.slide_dpsr_bwd_points(0, 4, 16, z, z, z, z, z, z, 1, 1, z, z, z, z) == 0
    assert L.slide_dpsr_bwd_points(1, 4, 16, z, z, z, z, z, z, 1, 1, z, z, z, z) == 0  # neither gradient is asked for
    for r in (8, 24, 48, 100, 512):
        assert L.slide_dpsr_spectral_adj(1, r, z, z, z, z) == -2, r
        assert L.slide_dpsr_grid_bwd(1, 4, r, z, z, z, z, z, z, 1, 1, *ws) == -2, r
    for r in (16, 32, 64, 128, 256):
        assert L.slide_dpsr_spectral_adj(1, r, z, z, z, z) == -2 and L.slide_dpsr_spectral_adj(0, r, z, z, z, z) == 0
        assert L.slide_dpsr_grid_bwd(0, 4, r, z, z, z, z, z, z, 1, 1, *ws) == 0
        assert L.slide_dpsr_grid_bwd(1, 4, r, z, z, z, z, z, z, 1, 1, *ws) == 0  # neither gradient is asked for
    assert L.slide_dpsr_grid_bwd(1, 0, 16, z, z, z, z, z, z, 1, 1, *ws) == -2 and L.slide_dpsr_grid_bwd(-1, 4, 16, z, z, z, z, z, z, 1, 1, *ws) == -2
    # NULL arrays with a gradient asked for: a non-NULL dv that is never written (the call returns before any launch)
    import ctypes
    buf = (ctypes.c_float * 12)()
    assert L.slide_dpsr_grid_bwd(1, 4, 16, z, z, z, z, z, z, 1, 1, z, z, z, z, z, z, z, z, buf, z, z, z) == -2
    assert L.slide_dpsr_bwd_points(1, 4, 16, z, z, z, z, z, z, 1, 1, buf, z, z, z) == -2
    assert all(v == 0.0 for v in buf)
