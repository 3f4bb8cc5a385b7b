"""CPU: the product library exports the DPSR entry points of include/slide_hip.h Part 5, the ctypes layer lists them, and their
argument checks run on the host before any launch."""
from slide_amd import _lib, build

NAMES = ("slide_point_rasterize", "slide_grid_fixed_to_float", "slide_grid_interp", "slide_fft3_r2c", "slide_fft3_c2r",
         "slide_dpsr_spectral", "slide_dpsr_finish", "slide_dpsr_grid")


def test_dpsr_symbols_exported():
    build.build()
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(L, n), n


def test_dpsr_entry_points_reject_bad_arguments_without_a_launch():
    """-2 for a size outside the kernels' scope or a NULL array, 0 for an empty batch -- every call returns before a launch"""
    build.build()
    L = _lib.lib()
    z = None
    assert L.slide_point_rasterize(1, 4, 2, 16, z, z, z, z, z) == -2  # nf
    assert L.slide_point_rasterize(1, 4, 3, 1, z, z, z, z, z) == -2 and L.slide_point_rasterize(1, 4, 3, 1025, z, z, z, z, z) == -2
    assert L.slide_point_rasterize(1, 4, 3, 16, z, z, z, z, z) == -2  # NULL
    assert L.slide_point_rasterize(0, 4, 3, 16, z, z, z, z, z) == 0 and L.slide_point_rasterize(2, 0, 1, 16, z, z, z, z, z) == 0
    assert L.slide_grid_fixed_to_float(-1, z, z, z) == -2 and L.slide_grid_fixed_to_float(0, z, z, z) == 0
    assert L.slide_grid_fixed_to_float(8, z, z, z) == -2
    assert L.slide_grid_interp(1, 4, 0, 16, z, z, z, z, z) == -2 and L.slide_grid_interp(1, 4, 1, 16, z, z, z, z, z) == -2
    assert L.slide_grid_interp(0, 4, 1, 16, z, z, z, z, z) == 0
    for r in (8, 24, 48, 100, 512):
        assert L.slide_fft3_r2c(1, r, z, 0, z, z) == -2 and L.slide_fft3_c2r(1, r, z, z, z) == -2, r
        assert L.slide_dpsr_spectral(1, r, z, z, z, z) == -2 and L.slide_dpsr_grid(1, 4, r, z, z, z, 1, 1, z, z, z, z, z, z, z, z) == -2, r
    for r in (16, 32, 64, 128, 256):
        assert L.slide_fft3_r2c(1, r, z, 0, z, z) == -2 and L.slide_fft3_c2r(1, r, z, z, z) == -2  # NULL
        assert L.slide_fft3_r2c(0, r, z, 1, z, z) == 0 and L.slide_fft3_c2r(0, r, z, z, z) == 0
        assert L.slide_dpsr_spectral(0, r, z, z, z, z) == 0
    assert L.slide_dpsr_finish(1, 4, 16, z, 1, 1, z, z, z) == -2 and L.slide_dpsr_finish(1, 0, 16, z, 1, 1, z, z, z) == -2
    assert L.slide_dpsr_finish(1, 4, 16, z, 0, 0, z, z, z) == 0 and L.slide_dpsr_finish(0, 4, 16, z, 1, 1, z, z, z) == 0
    assert L.slide_dpsr_grid(1, 0, 16, z, z, z, 1, 1, z, z, z, z, z, z, z, z) == -2
    assert L.slide_dpsr_grid(1, 4, 16, z, z, z, 1, 1, z, z, z, z, z, z, z, z) == -2
    assert L.slide_dpsr_grid(0, 4, 16, z, z, z, 1, 1, z, z, z, z, z, z, z, z) == 0
