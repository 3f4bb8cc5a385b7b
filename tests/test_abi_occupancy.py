"""CPU: the product library exports the occupancy-grid entry point of include/slide_hip.h Part 4 (the JSD metric's counters), the
ctypes layer lists it, and its argument checks run on the host before any launch."""
import ctypes

from slide_amd import _lib, build


def test_occupancy_symbol_exported():
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "slide_occupancy_grid")
    assert "slide_occupancy_grid" in _lib.EXPORTS


def test_occupancy_entry_point_rejects_bad_arguments_without_a_launch():
    """(s, p, pts, sp, r, axis, rowmask, counts, clouds, cells, flag, stream): a point stride below 3, a resolution outside
    [2, 32], more than 2^31 - 1 points or a NULL array -> -2; an empty set or empty clouds are a no-op (also with NULL arrays)"""
    lib = ctypes.CDLL(build.build())
    f = lib.slide_occupancy_grid
    null = None
    assert f(2, 4, null, 2, 28, null, null, null, null, null, null, null) == -2
    assert f(2, 4, null, 3, 1, null, null, null, null, null, null, null) == -2
    assert f(2, 4, null, 3, 33, null, null, null, null, null, null, null) == -2
    assert f(2, 4, null, 3, 28, null, null, null, null, null, null, null) == -2
    assert f(1 << 20, 1 << 12, null, 3, 28, null, null, null, null, null, null, null) == -2
    assert f(0, 4, null, 3, 28, null, null, null, null, null, null, null) == 0
    assert f(2, 0, null, 3, 2, null, null, null, null, null, null, null) == 0
    assert f(0, 0, null, 3, 32, null, null, null, null, null, null, null) == 0
