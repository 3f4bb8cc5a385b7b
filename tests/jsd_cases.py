"""Shared by tests/test_jsd_host.py and tests/test_hip_occupancy.py: the cases of tests/golden/golden_jsd.npz and the float64 bounds.

An entropy is a sum of n <= 32 768 non-negative terms t = -p log p, each evaluated within a few ulp; a float64 sum of n non-negative
terms, in any order, is within (n - 1) u of their exact sum relative to it (u = 2^-53).  Two correct evaluations of an entropy H
(the reference's scipy sum, ours) therefore differ by at most 2 (n + 8) u H.  The JSD is e_sum - (e1 + e2) / 2 and cancels, so
its bound is ABSOLUTE: the sum of the three entropies' bounds."""
import numpy as np

U = 2.0 ** -53
SETS = ("sphere", "cube", "outside")
RESOLUTIONS = (28, 9)


def entropy_bound(n, h):
    """two float64 evaluations of an entropy h (a sum of n terms)"""
    return 2.0 * (n + 8) * U * h


def _entropy2(c):
    p = c[c > 0] / c.sum()
    return float(-(p * np.log2(p)).sum())


def jsd_bound(P, Q):
    """two float64 evaluations of the JSD of the counters P and Q"""
    M = P / P.sum() + Q / Q.sum()
    return entropy_bound(len(P), _entropy2(P) + _entropy2(Q) + _entropy2(M))
