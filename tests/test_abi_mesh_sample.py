"""CPU: the product library exports the mesh-sampling entry points of include/slide_hip.h Part 7, the ctypes layer lists them, and
their argument checks run on the host before any launch."""
import ctypes

from slide_amd import _lib, build

NAMES = ("slide_mesh_cdf_span", "slide_mesh_face_cdf", "slide_mesh_sample")


def test_mesh_sample_symbols_exported():
    build.build()
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(L, n), n


def test_mesh_cdf_spans():
    """4 faces per thread, 64 threads per wave, 1024 threads per workgroup (csrc/mesh_sample.hip)"""
    build.build()
    L = _lib.lib()
    assert [L.slide_mesh_cdf_span(k) for k in (0, 1, 2)] == [4, 256, 4096]
    assert L.slide_mesh_cdf_span(-1) == -2 and L.slide_mesh_cdf_span(3) == -2


def test_mesh_entry_points_reject_bad_arguments_without_a_launch():
    """-2 for a negative count or a NULL array, 0 for an empty batch, no faces or no samples -- every call returns before a launch"""
    build.build()
    L = _lib.lib()
    z = None
    buf = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))  # a non-NULL pointer no call may get as far as using

    def cdf(b, nf, a=None):
        a = a or [buf] * 7
        return L.slide_mesh_face_cdf(b, nf, a[0], a[1], a[2], a[3], a[4], a[5], a[6], z)

    def smp(b, s, a=None, vertex=0, opt=(None, None, None)):
        # required arrays: verts faces voff foff cdf points valid; opt: vnormals, normals, face_idx
        a = a or [buf] * 7
        return L.slide_mesh_sample(b, s, a[0], a[1], opt[0], a[2], a[3], a[4], 1, 2, 3, z, z, vertex, a[5], opt[1], opt[2], a[6], z)

    assert cdf(-1, 4) == -2 and cdf(2, -1) == -2 and cdf(2, 2 ** 31) == -2
    assert cdf(0, 0, [z] * 7) == 0 and cdf(0, 5) == 0 and cdf(3, 0, [z] * 7) == 0
    for k in range(7):  # every single NULL array
        a = [buf] * 7
        a[k] = z
        assert cdf(2, 5, a) == -2, k
    assert smp(-1, 4) == -2 and smp(2, -1) == -2 and smp(65536, 4) == -2
    assert smp(0, 4, [z] * 7) == 0 and smp(3, 0, [z] * 7) == 0 and smp(0, 0) == 0
    for k in range(7):
        a = [buf] * 7
        a[k] = z
        assert smp(2, 5, a) == -2, k
    # vertex normals need the vertex-normal array and the output
    assert smp(2, 5, vertex=1) == -2 and smp(2, 5, vertex=1, opt=(buf, None, None)) == -2 and smp(2, 5, vertex=1, opt=(None, buf, None)) == -2
