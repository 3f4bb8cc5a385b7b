"""Shared by tests/test_emd_host.py, tests/test_hip_emd.py and tools/gen_golden_emd.py: the numpy restatement of the approximate
Earth Mover's Distance that slide_amd/csrc/emd_pairwise.hip computes (the reference's approxmatch + matchcost, written from the
algorithm and not from its source), the case list, and the tolerance rule.

The reference's kernels cannot be compiled without CUDA, so this restatement in float64 is the yardstick; the reference's two-point
known answer (KNOWN_*: 0.71, the sum of the crossed squared distances) pins it to the reference.

For one ordered pair, xyz1 (n points) against xyz2 (m points), d(k, l) the squared distance:

    multiL, multiR = (1, n // m) if n >= m else (m // n, 1)
    remainL[k] = multiL, remainR[l] = multiR, cost = 0
    for level in LEVELS:                                    # -(4 ** j), j = 7 ... -1, then 0: ten levels
      A: ratioL[k] = remainL[k] / (1e-9 + sum_l exp(level d(k,l)) remainR[l])
      B: sumr[l]   = remainR[l] sum_k exp(level d(k,l)) ratioL[k]
         ratioR[l] = min(remainR[l] / (sumr[l] + 1e-9), 1) remainR[l];  remainR[l] = max(0, remainR[l] - sumr[l])
      C: w(k,l) = exp(level d(k,l)) ratioL[k] ratioR[l];  cost += sum_kl d(k,l) w(k,l);  remainL[k] = max(0, remainL[k] - sum_l w(k,l))

Tolerance: |got - ref64| <= R (|ref64| + S), S = n * mean_kl d(k, l) -- the cost of the uniform plan, a scale that survives when
the cost itself is near zero.  R = 8 x the largest |f32 - f64| / (|f64| + S) of this same restatement evaluated in float32 arrays
over CASES: the kernel's exponentials are the hardware's approximate base-2 form (argument error about |level d| 2^-23) and its
sums run in another order, the emulation's exponentials are correctly rounded -- hence the margin of 8."""
import functools

import numpy as np

LEVELS = tuple(-(4.0 ** j) for j in range(7, -2, -1)) + (0.0,)
assert len(LEVELS) == 10 and LEVELS[0] == -16384.0 and LEVELS[-2] == -0.25

# measured with `python tests/emd_cases.py` (float32 emulation against float64 over CASES): the largest ratio is 4.285e-07, at
# case ('cube', 96, 48); the next are 3.05e-07 at ('dup', 1025, 1025) and 1.28e-07 at ('gauss3', 64, 64)
R_EMULATION = 4.285e-7
R = 8 * R_EMULATION  # 3.4e-06

KNOWN_XYZ1 = np.array([[1.7, -0.1, 0.1], [0.1, 1.2, 0.3]], np.float32)
KNOWN_XYZ2 = np.array([[0.3, 1.8, 0.2], [1.2, -0.2, 0.3]], np.float32)
KNOWN_COST = 0.71  # d(0,1) + d(1,0) = 0.30 + 0.41: the plan crosses

SIZES = ((1, 1), (2, 2), (64, 64), (96, 48), (50, 130), (257, 255), (300, 1030), (1025, 1025))
KINDS = ("cube", "gauss3", "dup", "apart")
CASES = tuple((kind, n, m) for n, m in SIZES for kind in KINDS) + (("known", 2, 2),)


def sqdist(x1, x2, dtype=np.float64):
    """(n, m) squared distances of the xyz channels, in dtype, by the kernel's recipe dx dx + dy dy + dz dz"""
    a, b = np.asarray(x1)[:, :3].astype(dtype), np.asarray(x2)[:, :3].astype(dtype)
    dx, dy, dz = (a[:, None, c] - b[None, :, c] for c in range(3))
    return dx * dx + dy * dy + dz * dz


def emd_ref(x1, x2, dtype=np.float64, return_match=False):
    """the raw cost (a python float) of xyz1 = x1 (n, C >= 3) against xyz2 = x2 (m, C >= 3), every array and scalar in dtype; with
    return_match also the (n, m) match matrix sum over the levels of w(k, l) (the transpose of the reference's layout)"""
    d = sqdist(x1, x2, dtype)
    n, m = d.shape
    multiL, multiR = (1, n // m) if n >= m else (m // n, 1)
    remainL, remainR = np.full(n, multiL, dtype), np.full(m, multiR, dtype)
    eps, zero, one = dtype(1e-9), dtype(0), dtype(1)
    cost = dtype(0)
    match = np.zeros((n, m), dtype) if return_match else None
    for level in LEVELS:
        e = np.exp(dtype(level) * d)
        ratioL = remainL / (eps + e @ remainR)
        sumr = remainR * (ratioL @ e)
        ratioR = np.minimum(remainR / (sumr + eps), one) * remainR
        remainR = np.maximum(zero, remainR - sumr)
        w = e * ratioL[:, None] * ratioR[None, :]
        cost = cost + (d * w).sum(dtype=dtype)
        remainL = np.maximum(zero, remainL - w.sum(1, dtype=dtype))
        if return_match:
            match += w
    assert cost.dtype == dtype
    return (float(cost), match) if return_match else float(cost)


def scale(x1, x2):
    """S = n * mean_kl d(k, l) in float64"""
    return float(len(x1) * sqdist(x1, x2).mean())


def within(got, ref64, S):
    return abs(float(got) - ref64) <= R * (abs(ref64) + S)


def make_pair(kind, n, m, channels=3):
    """the clouds of a case, float32 (n, channels) and (m, channels); channels beyond xyz are noise the kernel must not read"""
    if kind == "known":
        a, b = KNOWN_XYZ1.copy(), KNOWN_XYZ2.copy()
    else:
        rs = np.random.RandomState(KINDS.index(kind) * 1000003 + n * 4099 + m)
        if kind == "gauss3":
            a, b = 3.0 * rs.standard_normal((n, 3)), 3.0 * rs.standard_normal((m, 3))
        else:
            a, b = rs.uniform(0, 1, (n, 3)), rs.uniform(0, 1, (m, 3))
        if kind == "dup":  # half of the smaller cloud's size are exact copies of points of the other cloud
            h = (min(n, m) + 1) // 2
            b[:h] = a[:h]
        if kind == "apart":
            b[:, 0] += 10.0
        a, b = a.astype(np.float32), b.astype(np.float32)
    if channels > 3:
        rs = np.random.RandomState(n + m)
        a = np.concatenate([a, rs.standard_normal((len(a), channels - 3)).astype(np.float32)], 1)
        b = np.concatenate([b, rs.standard_normal((len(b), channels - 3)).astype(np.float32)], 1)
    return a, b


@functools.lru_cache(maxsize=None)
def case_reference(kind, n, m):
    """(ref64, S) of a case, computed once per process"""
    a, b = make_pair(kind, n, m)
    return emd_ref(a, b), scale(a, b)


def separation(M_rs, M_rr, M_ss):
    """(smallest relative gap (runner-up - minimum) / minimum over every column whose arg-min decides a 1-NN vote, the same over
    the columns that decide coverage): coverage takes each sample's nearest reference (columns of M_rs (N_ref, N_sample)), the
    1-NN test each element's nearest other element (columns of the full matrix, diagonal excluded)"""
    def gaps(A):
        srt = np.sort(A, axis=0)
        return float(((srt[1] - srt[0]) / np.maximum(np.abs(srt[0]), 1e-300)).min())

    full = np.block([[M_rr, M_rs], [M_rs.T, M_ss]]).astype(np.float64)
    np.fill_diagonal(full, np.inf)
    return gaps(full), gaps(M_rs)


if __name__ == "__main__":  # the measurement behind R_EMULATION
    worst = (0.0, None)
    for case in CASES:
        a, b = make_pair(*case)
        r64, S = case_reference(*case)
        r32 = emd_ref(a, b, np.float32)
        den = abs(r64) + S  # 0 for ('dup', 1, 1), one point against itself: the cost is exactly 0 in any arithmetic
        ratio = abs(r32 - r64) / den if den else float(r32 != r64)
        print("%-22s ref64 %.9e  S %.4e  f32 ratio %.3e" % (case, r64, S, ratio), flush=True)
        worst = max(worst, (ratio, case))
    print("largest ratio %.3e at %s" % worst)
