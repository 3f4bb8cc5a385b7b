"""CPU: the product library exports the Chamfer backward entry point of include/slide_train.h, the ctypes layer lists it, and its
argument checks run on the host before any launch (no device needed)."""
import ctypes

from slide_amd import _lib, build


def test_chamfer_bwd_symbol_exported():
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "slide_chamfer_cd_bwd")
    assert "slide_chamfer_cd_bwd" in _lib.EXPORTS


def _call(lib, b, n1, n2, f, sx, sy, inputs=True, dx=True, dy=True):
    buf = ctypes.create_string_buffer(64)  # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    i = p if inputs else None
    return lib.slide_chamfer_cd_bwd(b, n1, n2, f, i, sx, i, sy, i, i, i, i, i, p if dx else None, p if dy else None, None)


def test_chamfer_bwd_rejects_bad_arguments_without_a_launch():
    lib = ctypes.CDLL(build.build())
    assert _call(lib, 1, 4, 4, 0, 2, 3) == -2    # a point stride below 3 + f
    assert _call(lib, 1, 4, 4, 3, 6, 5) == -2
    assert _call(lib, 1, 4, 4, -1, 6, 6) == -2   # a negative or unsupported channel count
    assert _call(lib, 1, 4, 4, 17, 32, 32) == -2
    assert _call(lib, 1, 4, 4, 3, 6, 6, inputs=False) == -2  # NULL inputs


def test_chamfer_bwd_empty_batch_is_a_no_op():
    lib = ctypes.CDLL(build.build())
    assert _call(lib, 0, 4, 4, 3, 6, 6) == 0
    assert _call(lib, 0, 4, 4, 3, 6, 6, inputs=False) == 0
    assert _call(lib, 1, 4, 4, 3, 6, 6, dx=False, dy=False) == 0  # no output requested: nothing to launch
