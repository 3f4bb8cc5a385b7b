"""The case matrix of the per-sample column sums (csrc/train_ops.hip col_sums_seg_kernel, include/slide_train.h slide_col_sums_seg), a
numpy restatement of the kernel's ORDER of additions, the error bound that follows from it, and the nearest wrong variants --
shared by tests/test_col_sums_seg_host.py (CPU) and tests/test_hip_col_sums_seg.py (GPU).  Nothing of the code under test is called.

The order (seg_map): ld / 4 threads cover a row, rt = 256 / (ld / 4) rows are in flight.  S >= 128: n = min(256, S / 64) chunks of
rpc = ceil(S / n) consecutive rows (n recomputed as ceil(S / rpc)); inside a chunk lane p adds rows p, p + rt, ... in ascending
order from 0, then the rt lane sums are added in ascending lane from 0; the second pass runs the same order over the n partial
rows of the sample (one chunk of n rows).  S < 128: the one chunk is the result.

Bound.  An element of the result is the root of a tree of additions whose longest path from a leaf is
    L = ceil(rpc / rt) + rt            (+ ceil(n / rt) + rt with the second pass)
additions long (the first addition of every chain is 0 + x: exact, counted all the same).  Every addition on the path of a term
scales it by (1 + d), |d| <= u = 2^-24, so |err| <= ((1 + u)^L - 1) sum|x| <= 1.01 L u sum|x| for L u < 0.01: the bound is
linear in the LONGEST CHAIN, not in S -- at S = 8195, ld = 32 it is 71 u, where a row-after-row sum would carry 8195 u.
Integer data whose partial sums stay below 2^24 is added exactly in any order: bound 0."""
import zlib

import numpy as np

U = 2.0 ** -24
B = 3
SIZES = (1, 5, 127, 128, 130, 1000, 8195)
LDS = (32, 96, 1024)
CASES = [dict(name="s%d_ld%d" % (S, ld), B=B, S=S, ld=ld) for S in SIZES for ld in LDS]
# (B, S, ld, x, out, scratch) -> status: the argument check of the entry point, no launch behind any of them
STATUS_CASES = (
    ("b0", dict(B=0, S=40, ld=32), 0), ("b0_null", dict(B=0, S=40, ld=32, x=False, out=False, scratch=False), 0),
    ("bad_ld_0", dict(B=2, S=40, ld=0), -3), ("bad_ld_mod32", dict(B=2, S=40, ld=48), -3), ("bad_ld_1056", dict(B=2, S=40, ld=1056), -3),
    ("bad_b_neg", dict(B=-1, S=40, ld=32), -3), ("bad_b_65536", dict(B=65536, S=40, ld=32), -3), ("bad_s_neg", dict(B=2, S=-1, ld=32), -3),
    ("bad_null_out", dict(B=2, S=40, ld=32, out=False), -3), ("bad_null_x", dict(B=2, S=40, ld=32, x=False), -3),
    ("bad_null_out_s0", dict(B=2, S=0, ld=32, out=False), -3),
    ("bad_null_scratch_s128", dict(B=2, S=128, ld=32, scratch=False), -3))


def seg_map(S, ld):
    """the stage map of slide_col_sums_seg"""
    rt = 256 // (ld // 4)
    n = min(256, max(1, S // 64))
    rpc = (S + n - 1) // n
    n = (S + rpc - 1) // rpc
    chain = -(-rpc // rt) + rt + ((-(-n // rt) + rt) if n > 1 else 0)
    return dict(rt=rt, nchunk=n, rpc=rpc, stages=2 if n > 1 else 1, chain=chain, scratch_floats=n * ld if n > 1 else 0)


def scratch_floats(B, S, ld):
    """what the header documents: nothing below 128 rows, else B * min(256, S / 64) * ld floats"""
    return B * min(256, S // 64) * ld if S >= 128 else 0


def _chunk_sum(x, rt, dtype):
    """one workgroup: lane p adds rows p, p + rt, ... from 0, then the lane sums are added in ascending lane from 0"""
    lanes = np.zeros((rt,) + x.shape[1:], dtype)
    for r in range(x.shape[0]):
        lanes[r % rt] = lanes[r % rt] + x[r]
    a = np.zeros(x.shape[1:], dtype)
    for p in range(rt):
        a = a + lanes[p]
    return a


def ordered_sums(x, B, S, ld, dtype=np.float32, mutant=None):
    """out [B, ld] in the kernel's order of additions, in `dtype` arithmetic (float32: what the kernel computes, bit for bit
    unless the compiler reassociates -- it may not).  mutant: one of MUTANTS, the nearest wrong variants."""
    m = seg_map(S, ld)
    x = np.asarray(x, dtype).reshape(B * S, ld)
    out = np.zeros((B, ld), dtype)
    for b in range(B):
        lo, hi = b * S, (b + 1) * S
        if mutant == "segment_shift" and b > 0:
            lo, hi = lo - 1, hi - 1          # a segment boundary one row early: the sample before leaks in, its own last row is lost
        if mutant == "drop_last_row":
            hi -= 1
        seg = x[lo:hi]
        parts = [_chunk_sum(seg[c * m["rpc"]:(c + 1) * m["rpc"]], m["rt"], dtype) for c in range(m["nchunk"])]
        if mutant == "drop_last_chunk":
            parts = parts[:-1] if len(parts) > 1 else [np.zeros(ld, dtype)]
        out[b] = parts[0] if m["nchunk"] == 1 else _chunk_sum(np.stack(parts), m["rt"], dtype)
    return out


MUTANTS = ("drop_last_row", "drop_last_chunk", "segment_shift")


def bound(x, B, S, ld):
    """elementwise bound [B, ld] on |kernel - float64 sum|, from the longest chain of additions (module docstring)"""
    L = seg_map(S, ld)["chain"]
    assert L * U < 0.01
    return 1.01 * L * U * np.abs(np.asarray(x, np.float64).reshape(B, S, ld)).sum(axis=1)


def make_data(case, dist):
    """x [B * S, ld] float32: `normal` (mean 0.5, so that a lost row shows against the sum) or `ints` (integers of [-8, 8]: every
    partial sum is an integer below 2^24, exact in fp32)"""
    rs = np.random.RandomState(zlib.crc32(("%s_%s" % (case["name"], dist)).encode()) & 0x7FFFFFFF)
    shape = (case["B"] * case["S"], case["ld"])
    if dist == "ints":
        return rs.randint(-8, 9, size=shape).astype(np.float32)
    return (rs.standard_normal(shape) + 0.5).astype(np.float32)


def ratio(got, ref, bnd):
    """worst |got - ref| / bound over the elements (an element with bound 0 must be exact: inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0
