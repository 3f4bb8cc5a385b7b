"""CPU: the product library exports the per-sample column-sum entry point of include/slide_train.h, the ctypes layer lists it with
the header's signature, and its argument checks run on the host before any launch (no device needed)."""
import ctypes

import col_sums_seg_cases as K
from slide_amd import _lib, abi, build


def test_col_sums_seg_symbol_exported():
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "slide_col_sums_seg")
    assert "slide_col_sums_seg" in _lib.EXPORTS


def test_col_sums_seg_signature():
    # (int B, long long S, int ld, const float *x, float *out, float *scratch, slide_stream_t stream) -> int
    restype, argtypes = abi.PROTOTYPES["slide_col_sums_seg"]
    assert restype is ctypes.c_int
    assert argtypes == (ctypes.c_int, ctypes.c_longlong, ctypes.c_int) + (ctypes.c_void_p,) * 4


def test_col_sums_seg_status_codes_without_a_launch():
    lib = abi.bind(ctypes.CDLL(build.build()), False)
    buf = ctypes.create_string_buffer(64)  # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name, kw, status in K.STATUS_CASES:
        args = [p if kw.get(k, True) else None for k in ("x", "out", "scratch")]
        assert lib.slide_col_sums_seg(kw["B"], kw["S"], kw["ld"], *args, None) == status, name
