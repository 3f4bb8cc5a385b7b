"""Shared by the Chamfer-backward tests (no test in here): a float64 numpy restatement of the gradient that
include/slide_train.h's slide_chamfer_cd_bwd defines, its deliberately wrong variants, and the elementwise error bound.

Convention of the fused path: x = gt, y = output, direction 0 over x's points (i1: their neighbours in y), direction 1 over y's.

THE BOUND.  An element of a gradient is a sum of 1 + m terms (its own, and one per incoming source; m = the point's in-degree), each
a product k e with e = p - q one coordinate difference and k = 2 (g0 + g1 / (2 sqrt d)).  Rounding steps of one term in the kernel,
in units u = 2^-24 of relative error against the exact value from the same fp32 inputs:
  e = fl(p - q)                                                   1
  d: three squares of such differences, summed (the forward's)    2 + 1 + 2 = 5, halved by the square root: 2.5
  sqrt, the division, the addition g0 + ...                       3      (2 x is exact)
  the product k e                                                 1
that is 7.5 for a coordinate; a feature channel has t = sum of F squares in place of d: (2 + 1 + F - 1) / 2 = (F + 2) / 2 = 2.5 for
F = 3, the same 7.5.  dred itself may arrive through an fp32 autograd chain (division by the point count, the feature weight's fp32
value and its product): 2.5 more.  So R = 10 roundings per term, relative to |k| |e| with |k| taken as 2 (|g0| + |g1| / (2 sqrt d))
(no cancellation credit), and the sequential sum of 1 + m terms adds m roundings relative to the sum of their magnitudes:
    |err| <= gamma(R + m) S,   gamma(n) = n u / (1 - n u),   S = sum of the magnitudes of the element's terms.
For F > 3 feature channels R grows by (F - 3) / 2.  Nothing here is fitted to a result."""
import numpy as np

U = 2.0 ** -24
MUTANTS = ("no_scatter", "scatter_sign", "no_factor_2", "no_sqrt_factor")


def rounding_steps(F):
    return 10.0 + max(F - 3, 0) / 2.0


def tolerance(S, indeg, F):
    n = (rounding_steps(F) + indeg[..., None]) * U
    return n / (1 - n) * S


def _coef(g0, g1, v, mutant):
    with np.errstate(divide="ignore", invalid="ignore"):
        part = g1 if mutant == "no_sqrt_factor" else g1 / (2 * np.sqrt(v))
        mag = np.abs(g1) / (2 * np.sqrt(v))
    pos = v > 0
    return g0 + np.where(pos, part, 0.0), np.abs(g0) + np.where(pos, mag, 0.0)


def _direction(p, q, idx, g, mutant):
    """own points p (B,P,C), other cloud q (B,Q,C), idx (B,P), g (B,5) -> (own terms (B,P,C), their magnitudes)"""
    e = p - np.take_along_axis(q, idx[:, :, None], axis=1)
    two = 1.0 if mutant == "no_factor_2" else 2.0
    a, am = _coef(g[:, None, 0], g[:, None, 1], (e[:, :, :3] ** 2).sum(-1), mutant)
    v, vm = two * a[:, :, None] * e[:, :, :3], 2 * am[:, :, None] * np.abs(e[:, :, :3])
    if p.shape[2] > 3:
        c, cm = _coef(g[:, None, 3], g[:, None, 4], (e[:, :, 3:] ** 2).sum(-1), mutant)
        v = np.concatenate([v, two * c[:, :, None] * e[:, :, 3:]], axis=2)
        vm = np.concatenate([vm, 2 * cm[:, :, None] * np.abs(e[:, :, 3:])], axis=2)
    return v, vm


def restate(x, y, i1, i2, dred, mutant=None):
    """float64 gradient of sum(red * dred), red = chamfer_reduce(chamfer_nn(x, y), mse features) -> (dx, dy, Sx, Sy, mx, my): the
    gradients, the per-element sums of term magnitudes and the per-point in-degrees.  mutant: one of MUTANTS (a wrong formula)"""
    x, y, dred = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(dred, np.float64)
    v1, m1 = _direction(x, y, i1, dred[:, 0], mutant)
    v2, m2 = _direction(y, x, i2, dred[:, 1], mutant)
    dx, dy, Sx, Sy = v1.copy(), v2.copy(), m1.copy(), m2.copy()
    mx, my = np.zeros(x.shape[:2], np.int64), np.zeros(y.shape[:2], np.int64)
    sign = {"no_scatter": 0.0, "scatter_sign": 1.0}.get(mutant, -1.0)
    for b in range(x.shape[0]):
        np.add.at(dy[b], i1[b], sign * v1[b])
        np.add.at(Sy[b], i1[b], m1[b])
        np.add.at(my[b], i1[b], 1)
        np.add.at(dx[b], i2[b], sign * v2[b])
        np.add.at(Sx[b], i2[b], m2[b])
        np.add.at(mx[b], i2[b], 1)
    return dx, dy, Sx, Sy, mx, my


def dred_of_loss(B, n_gt, n_out, tag, w):
    """d mean_b(cd_<tag> + w cd_feature_<tag>) / d red, (B, 2, 5) float64 (tag 'p': the square-root columns 1 and 4, 't': 0 and 3)"""
    g = np.zeros((B, 2, 5))
    n = np.array([n_gt, n_out], np.float64)
    if tag == "p":
        g[:, :, 1] = 1.0 / (2 * n * B)
        g[:, :, 4] = w / (2 * n * B)
    else:
        g[:, :, 0] = 1.0 / (n * B)
        g[:, :, 3] = w / (n * B)
    return g


def nearest(x, y):
    """float64 brute-force neighbours of x's points in y and of y's in x (xyz = channels 0:3) -> (i1, i2, D (B,P1,P2))"""
    D = ((np.asarray(x, np.float64)[:, :, None, :3] - np.asarray(y, np.float64)[:, None, :, :3]) ** 2).sum(-1)
    return D.argmin(2), D.argmin(1), D
