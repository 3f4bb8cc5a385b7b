"""CPU: the product library exports the Chamfer / F1 entry points of include/slide_hip.h Part 4, and the ctypes layer lists them."""
import ctypes

from slide_amd import _lib, build


def test_chamfer_symbols_exported():
    lib = ctypes.CDLL(build.build())
    for name in ("slide_chamfer_nn", "slide_chamfer_reduce"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS


def test_chamfer_entry_points_reject_bad_arguments_without_a_launch():
    """argument checks run on the host before any launch (no device needed): a point stride below 3 or an unknown term mode -> -2;
    empty batches are a no-op"""
    lib = ctypes.CDLL(build.build())
    null = None
    assert lib.slide_chamfer_nn(1, 4, 4, null, 2, null, 3, null, null, null, null, null, null, null) == -2
    assert lib.slide_chamfer_nn(0, 4, 4, null, 3, null, 3, null, null, null, null, null, null, null) == 0
    assert lib.slide_chamfer_reduce(1, 4, 4, null, null, null, null, null, null, ctypes.c_float(1e-4), 3, 7, null, 3, null, 3,
                                    null, null) == -2
    assert lib.slide_chamfer_reduce(1, 4, 4, null, null, null, null, null, null, ctypes.c_float(1e-4), 3, 1, null, 3, null, 3,
                                    null, null) == -2
