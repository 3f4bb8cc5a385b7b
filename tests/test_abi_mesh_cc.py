"""CPU: the product library exports the mesh-component entry points of include/slide_hip.h Part 8, the ctypes layer lists them, and
their argument checks run on the host before any launch."""
import ctypes

from slide_amd import _lib, build

NAMES = ("slide_mesh_cc_span", "slide_mesh_cc_label", "slide_mesh_cc_stats", "slide_mesh_cc_select", "slide_mesh_cc_compact")


def test_mesh_cc_symbols_exported():
    build.build()
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(L, n), n


def test_mesh_cc_spans():
    """256 threads per workgroup of the per-face / per-vertex launches; 4 elements per thread, 64 threads per wave and 1024 threads
    per workgroup in the per-mesh scans (csrc/mesh_components.hip)"""
    build.build()
    L = _lib.lib()
    assert [L.slide_mesh_cc_span(k) for k in (0, 1, 2)] == [256, 256, 4096]
    assert L.slide_mesh_cc_span(-1) == -2 and L.slide_mesh_cc_span(3) == -2


def test_mesh_cc_entry_points_reject_bad_arguments_without_a_launch():
    """-2 for a count out of range or a NULL array, 0 for an empty batch or no vertices -- every call returns before a launch"""
    build.build()
    L = _lib.lib()
    z = None
    buf = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))  # a non-NULL pointer no call may get as far as using
    info = (ctypes.c_int * 4)(7, 7, 7, 7)
    pinfo = ctypes.addressof(info)

    def label(b, nv, nf, a=None, group=4, cap=10, inf=pinfo):
        a = a or [buf] * 5  # faces voff foff labels state
        return L.slide_mesh_cc_label(b, nv, nf, a[0], a[1], a[2], a[3], a[4], group, cap, inf, z)

    def stats(b, nv, nf, a=None):
        a = a or [buf] * 11  # faces voff foff labels cnt_v cnt_f rank cid nverts nfaces totals
        return L.slide_mesh_cc_stats(b, nv, nf, *a, z)

    def select(b, nv, nf, a=None, by=0, min_size=0, keep_all=0):
        a = a or [buf] * 9  # faces voff foff labels cnt_v cnt_f | vnew fnew totals
        return L.slide_mesh_cc_select(b, nv, nf, a[0], a[1], a[2], a[3], a[4], a[5], by, min_size, keep_all, a[6], a[7], a[8], z)

    def compact(b, nv, nf, a=None):
        a = a or [buf] * 13  # verts normals faces voff foff vnew fnew ovoff ofoff out_verts out_normals out_faces vert_idx
        return L.slide_mesh_cc_compact(b, nv, nf, *a, z)

    for call in (label, stats, select, compact):
        assert call(-1, 4, 4) == -2 and call(2, -1, 4) == -2 and call(2, 4, -1) == -2, call.__name__
        assert call(2, 2 ** 31, 4) == -2 and call(2, 4, 2 ** 31) == -2 and call(65536, 4, 4) == -2, call.__name__
        n = {"label": 5, "stats": 11, "select": 9, "compact": 13}[call.__name__]
        assert call(0, 0, 0, [z] * n) == 0 and call(0, 5, 5) == 0 and call(3, 0, 0, [z] * n) == 0, call.__name__
    assert label(2, 4, 4, group=0) == -2 and label(2, 4, 4, cap=0) == -2 and label(2, 4, 4, inf=z) == -2
    assert label(0, 0, 0) == 0 and list(info) == [0, 0, 0, 0]  # an empty call reports no rounds
    assert select(2, 4, 4, by=2) == -2 and select(2, 4, 4, by=-1) == -2
    # every single NULL array (compact: normals without out_normals, or the reverse, is refused too)
    for call, n in ((label, 5), (stats, 11), (select, 9), (compact, 13)):
        for k in range(n):
            a = [buf] * n
            a[k] = z
            assert call(2, 5, 5, a) == -2, (call.__name__, k)
