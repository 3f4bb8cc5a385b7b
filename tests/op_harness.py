"""Helpers of the tests that run hand-built SlideOps through slide_run_ops on synthetic data (no engine, no sampler):
tests/test_hip_update_ops.py, tests/test_hip_point_chain.py, tests/test_hip_front_ops.py."""
import ctypes

import numpy as np

import update_cases as uc

SENTINEL = 1234.5  # (exact in fp16 and fp32)


class Dev:
    """device buffers of one launch: everything put() uploads stays alive with the object"""

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device
        self.keep = []

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.keep.append(t)
        return t

    def t_dev(self, t, step, nonce=0, offset=0):
        return self.put(np.array([t, step, 0, uc.as_i32(nonce), offset, 0, 0, 0], np.int32))


def run(ops, times=1, graph=False):
    """launches the ops `times` times back to back on one side stream with no host synchronisation in between"""
    import torch
    from slide_amd import _lib, abi
    L = _lib.lib()
    arr = (abi.SlideOp * len(ops))(*ops)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        if graph:
            _lib.check(L.slide_graph_begin(s.cuda_stream), "graph_begin")
            st = L.slide_run_ops(arr, len(ops), s.cuda_stream)
            g = ctypes.c_void_p()
            st2 = L.slide_graph_end(s.cuda_stream, ctypes.byref(g))
            _lib.check(st, "slide_run_ops(capture)")
            _lib.check(st2, "graph_end")
            try:
                for _ in range(times):
                    _lib.check(L.slide_graph_launch(g, s.cuda_stream), "graph_launch")
                s.synchronize()
            finally:
                L.slide_graph_destroy(g)
        else:
            for _ in range(times):
                _lib.check(L.slide_run_ops(arr, len(ops), s.cuda_stream), "slide_run_ops")
            s.synchronize()


def status(op):
    """the status slide_run_ops returns for one op on torch's current stream (a refusal: negative, nothing launched)"""
    import torch
    from slide_amd import _lib, abi
    st = _lib.lib().slide_run_ops((abi.SlideOp * 1)(op), 1, _lib.stream_of())
    torch.cuda.synchronize()
    return st


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])
