"""CPU: the product library exports the grouping layer's coordinate backward (include/slide_train.h slide_group_rows_coord_bwd), the
ctypes layer lists it, and its argument checks and no-op returns happen on the host before any launch (no device needed)."""
import ctypes

from slide_amd import _lib, build

FP, ABS, CENTER, NO_XYZ = 1, 2, 4, 8


def test_group_coord_bwd_symbol_exported():
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "slide_group_rows_coord_bwd")
    assert "slide_group_rows_coord_bwd" in _lib.EXPORTS


def _call(lib, B=1, N=4, np_=4, K=2, C=5, ldg=32, flags=0, null=(), d2=True, dxyz=True, dnew=True):
    buf = ctypes.create_string_buffer(64)  # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = {n: (None if n in null else p) for n in ("xyz", "new_xyz", "idx", "dout")}
    return lib.slide_group_rows_coord_bwd(B, N, np_, K, C, ldg, flags, a["xyz"], a["new_xyz"], a["idx"], p if d2 else None, None, a["dout"],
                                          p if dxyz else None, p if dnew else None, None)


def test_group_coord_bwd_rejects_bad_arguments_without_a_launch():
    lib = ctypes.CDLL(build.build())
    for ldg in (0, -32, 24, 48, 1056):       # not a positive multiple of 32 up to 1024
        assert _call(lib, ldg=ldg) == -3, ldg
    assert _call(lib, C=-1) == -3
    assert _call(lib, C=30, flags=0) == -3                       # 30 + 3 > 32
    assert _call(lib, C=27, flags=ABS) == -3                     # 27 + 6
    assert _call(lib, C=24, flags=ABS | CENTER) == -3            # 24 + 9
    assert _call(lib, C=22, flags=FP) == -3                      # 22 + 11
    assert _call(lib, C=33, flags=NO_XYZ) == -3                  # C alone
    assert _call(lib, K=0) == -3
    assert _call(lib, K=-2) == -3
    for name in ("xyz", "new_xyz", "idx", "dout"):
        assert _call(lib, null=(name,)) == -3, name
    assert _call(lib, C=5, flags=FP, d2=False) == -3             # the FP form needs d2


def test_group_coord_bwd_no_op_returns():
    lib = ctypes.CDLL(build.build())
    assert _call(lib, B=0) == 0
    assert _call(lib, N=0) == 0
    assert _call(lib, np_=0) == 0
    assert _call(lib, B=-1) == 0
    assert _call(lib, flags=NO_XYZ) == 0                         # no coordinate columns
    assert _call(lib, dxyz=False, dnew=False) == 0               # no output requested
    assert _call(lib, flags=FP, C=21, dxyz=False, dnew=False) == 0
