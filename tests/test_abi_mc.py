"""CPU: the product library exports the marching-cubes entry points of include/slide_hip.h Part 6, the ctypes layer lists them, and
their argument checks run on the host before any launch."""
import ctypes

from slide_amd import _lib, build

NAMES = ("slide_mc_bricks", "slide_mc_count", "slide_mc_emit")


def test_mc_symbols_exported():
    build.build()
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(L, n), n


def test_mc_bricks():
    """a brick is 4 x 8 x 16 grid points (csrc/marching_cubes.hip)"""
    build.build()
    L = _lib.lib()
    assert L.slide_mc_bricks(1) == -2 and L.slide_mc_bricks(257) == -2 and L.slide_mc_bricks(-3) == -2
    for r in (2, 13, 16, 17, 64, 100, 128, 256):
        assert L.slide_mc_bricks(r) == -(-r // 4) * -(-r // 8) * -(-r // 16), r


def test_mc_entry_points_reject_bad_arguments_without_a_launch():
    """-2 for r outside [2, 256], a negative b or a NULL array with b > 0; 0 for an empty batch -- every call returns before a launch"""
    build.build()
    L = _lib.lib()
    z = None
    buf = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))  # a non-NULL pointer no call may get as far as using
    for r in (-1, 0, 1, 257, 1024):
        assert L.slide_mc_count(1, r, buf, 0.0, buf, buf, z) == -2, r
        assert L.slide_mc_emit(1, r, buf, 0.0, buf, buf, buf, buf, buf, buf, z) == -2, r
        assert L.slide_mc_count(0, r, z, 0.0, z, z, z) == -2, r  # (the size is checked first)
    for r in (2, 13, 16, 128, 256):
        assert L.slide_mc_count(-1, r, buf, 0.0, buf, buf, z) == -2 and L.slide_mc_emit(-1, r, buf, 0.0, buf, buf, buf, buf, buf, buf, z) == -2
        assert L.slide_mc_count(0, r, z, 0.0, z, z, z) == 0 and L.slide_mc_emit(0, r, z, 0.0, z, z, z, z, z, z, z) == 0
        assert L.slide_mc_count(1, r, z, 0.0, z, z, z) == -2 and L.slide_mc_emit(1, r, z, 0.0, z, z, z, z, z, z, z) == -2
        for k in range(3):  # every single NULL array
            a = [buf] * 3
            a[k] = z
            assert L.slide_mc_count(2, r, a[0], 0.0, a[1], a[2], z) == -2, (r, k)
        for k in range(7):
            a = [buf] * 7
            a[k] = z
            assert L.slide_mc_emit(2, r, a[0], 0.0, a[1], a[2], a[3], a[4], a[5], a[6], z) == -2, (r, k)
    # more workgroups than a launch can have: 2^31 / slide_mc_bricks(256) = 65536 grids
    assert L.slide_mc_count(65536, 256, buf, 0.0, buf, buf, z) == -2
