"""CPU: the product library exports slide_philox_normal_selftest (include/slide_hip.h), the ctypes layer lists it with the
header's prototype, and its argument checks run on the host before any launch."""
import ctypes

from slide_amd import _lib, abi, build

NAME = "slide_philox_normal_selftest"


def test_selftest_symbol_exported_and_declared():
    build.build()
    L = _lib.lib()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    restype, argtypes = abi.PROTOTYPES[NAME]
    assert restype is ctypes.c_int
    assert argtypes == (ctypes.c_int,) * 6 + (ctypes.c_void_p,) * 2  # seed_lo, seed_hi, step, nonce, elem0, n, out, stream


def test_selftest_rejects_bad_arguments_without_a_launch():
    """-2 for a negative count or a NULL output with n > 0, 0 for n == 0 -- every call returns before a launch.  Words above 2^31
    cross as the int that carries their bit pattern."""
    build.build()
    fn = getattr(_lib.lib(), NAME)
    assert fn(0, 0, 0, 0, 0, -1, None, None) == -2
    assert fn(0, 0, 0, 0, 0, 16, None, None) == -2
    assert fn(0, 0, 0, 0, 0, 0, None, None) == 0
    hi = ctypes.c_int32(0x9E3779B9).value
    assert hi < 0 and fn(hi, hi, hi, hi, hi, 0, None, None) == 0
