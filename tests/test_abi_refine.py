"""CPU: the product library exports the refine-front entry points of include/slide_hip.h Part 9, the ctypes layer lists them, and the
launchers refuse by status before any launch."""
import ctypes

from slide_amd import _lib, build

NAMES = ("slide_refine_span", "slide_mirror_concat", "slide_refine_to_dpsr")


def test_refine_symbols_exported():
    build.build()
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(L, n), n


def test_refine_span():
    """256 output rows per workgroup (csrc/refine_front.hip; tests/refine_cases.py TILE)"""
    import refine_cases
    build.build()
    L = _lib.lib()
    assert L.slide_refine_span(0) == 256 == refine_cases.TILE
    assert L.slide_refine_span(1) == -2 and L.slide_refine_span(-1) == -2


def test_refine_entry_points_refuse_by_status_without_a_launch():
    build.build()
    L = _lib.lib()
    z = None
    raw = ctypes.create_string_buffer(64 + 8)
    base = ctypes.addressof(raw)
    buf = ctypes.c_void_p(base + (-base) % 8)  # an 8-byte aligned non-NULL pointer no call may get as far as using
    odd = ctypes.c_void_p(buf.value + 4)

    def mirror(b=2, n=8, c=6, axis=2, label=1, a=None):
        a = a or [buf] * 5  # x perm out center flag
        return L.slide_mirror_concat(b, n, c, a[0], axis, label, a[1], a[2], a[3], a[4], z)

    assert mirror(b=-1) == -2 and mirror(b=65536) == -2 and mirror(n=-1) == -2 and mirror(c=2) == -2
    assert mirror(axis=-1) == -2 and mirror(axis=3) == -2
    assert mirror(b=0, a=[z] * 5) == 0 and mirror(n=0, a=[z] * 5) == 0
    for k in (0, 2, 3, 4):  # (perm may be NULL)
        a = [buf] * 5
        a[k] = z
        assert mirror(a=a) == -2, k

    def refine(b=2, m=8, ldx=6, dw=30, rows=8, factor=5, first=0, center=0, mode=0, a=None):
        a = a or [buf] * 7  # X disp points normals bbox partials flag
        return L.slide_refine_to_dpsr(b, m, ldx, dw, rows, a[0], a[1], factor, first, center, 0.001, mode, 1.0, a[2], a[3], a[4], a[5],
                                      a[6], z)

    assert refine(b=-1) == -2 and refine(b=65536) == -2 and refine(m=-1) == -2 and refine(rows=9) == -2 and refine(rows=-1) == -2
    assert refine(mode=2) == -2 and refine(mode=-1) == -2
    assert refine(ldx=5) == -3 and refine(ldx=8) == -3
    assert refine(dw=36) == -4 and refine(first=1, dw=30) == -4 and refine(first=1, center=1, dw=36) == -4
    assert refine(center=1) == -5
    assert refine(factor=0, dw=0) == -6
    assert refine(b=0, a=[z] * 7) == 0 and refine(rows=0, a=[z] * 7) == 0
    assert refine(first=1, center=1, factor=1, dw=6, rows=0, a=[z] * 7) == 0
    for k in range(7):
        a = [buf] * 7
        a[k] = z
        assert refine(a=a) == -2, k
    # the wide loads need 8-byte aligned rows: disp always, X with 6 channels
    assert refine(a=[buf, odd] + [buf] * 5) == -2 and refine(a=[odd] + [buf] * 6) == -2
    # (ldx 7 passes the alignment check: its status would be a launch's, so it is not called here)
