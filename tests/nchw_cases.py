"""The SLIDE_OP_TRANSPOSE and SLIDE_OP_GROUPNORM_NCHW case matrices, their references, bounds and mutants -- shared by
tests/test_nchw_ops_host.py (CPU) and tests/test_hip_nchw_ops.py (GPU).  The two launches of csrc/engine.hip behind
slide_amd.nn_ops.HipConv1x1 / HipGroupNorm (reference-layout tensors of the module-level path), until now covered through module
outputs only.

TRANSPOSE  out[b][c][r] = in[b][r][c] over fp32 input [B][R][in_ld] (batch stride in_bs) into fp32 or fp16 [B][C][out_ld] (batch
  stride out_bs), 32 x 32 tiles.  A mover: the fp32 destination is BIT-equal to the input (NaN payloads, -0.0 included), the fp16
  destination bit-equal to numpy's round-to-nearest-even astype(float16) -- among the data: fp16 ties (both ways), values in fp16's
  subnormal range (2^-25 is a tie to zero), +-65504, 65520 (a tie that rounds to inf), 65519.996 (stays 65504), -0.0 and NaN.  Row
  pads [C, in_ld) and batch gaps of the input hold a value that must not appear; pads and gaps of the output keep SENTINEL.
  Mutants: swap_ld (the destination indexed with in_ld) | batch_stride_of_other_side | tile_edge_off_by_one (the last row of a
  matrix with R % 32 == 1 dropped) | truncate_fp16 (fp16 by truncation).

GROUPNORM_NCHW  x (B, C, HW) fp32: channels [0, n_norm) in G groups of gs = n_norm / G (a group is one run of n = gs HW floats), the
  rest copied -- or max(x, 0) with the ReLU -- exactly.  Reference in float64; bound: the GN derivation of tests/rows_cases.py on an
  exact fp32 input (imported: rows_cases.gn_stats gives m, rstd, dm, dr of the same values laid out as rows),
      dm = (d + 2) u mean|x|     dv = 4 (d + 2) u mean(x^2)     dr = rstd (0.6 dv / (v + eps) + 4 u)     d = ceil(log2 n) + 2
      b' = |gamma| rstd dm + |gamma| |x - m| dr + 3 u (|x g| + |m g| + |beta|),   g = gamma rstd;     store fp32: b' + u |ref|
  The kernel sums n / 256 values per thread, then a butterfly over the wave and four wave totals (chains of <= 16 + 8 links here,
  inside d + 2 >= 10), takes v = E[x^2] - m^2 clamped at 0 and evaluates ((x - m) rstd) gamma + beta: four roundings,
  <= 3 u |(x - m) g| + u |y|, which the 3 u (...) term and dm's share cover (|x - m| <= |x| + |m|).
  Mutants: unbiased_var | tail_normalised | tail_relu_dropped | neighbour_sample | gamma_within_group (the channel index without
  g gs) | count_hw_only (n taken as HW).  One below a case's resolution is in GN_EXEMPT with the case that shows it."""
import zlib

import numpy as np

from rows_cases import EPS, U, gn_stats, r32, ratio, store  # noqa: F401  (ratio is re-exported to the test modules)
from slide_amd.abi import ru

IN_PAD = -4321.0  # what the input's row pads and batch gaps hold


def _rs(name):
    return np.random.RandomState(zlib.crc32(("nchw_" + name).encode()) & 0x7fffffff)


# ------------------------------------------------------------------------------------------------------------- TRANSPOSE
TR_CASES = []


def _tr(name, B, R, C, in_ld=None, out_ld=None, in_gap=0, out_gap=0):
    in_ld, out_ld = in_ld or C, out_ld or R
    for f16 in (False, True):
        TR_CASES.append(dict(name="%s_%s" % (name, "f16" if f16 else "f32"), B=B, R=R, C=C, in_ld=in_ld, out_ld=out_ld, in_bs=R * in_ld + in_gap,
                             out_bs=C * out_ld + out_gap, f16=f16))


_tr("b1_1x1", 1, 1, 1)
_tr("b2_33x31", 2, 33, 31)
_tr("b3_32x64", 3, 32, 64)
_tr("b2_65x40", 2, 65, 40)
_tr("b1_16x1568", 1, 16, 1568)
_tr("b2_33x31_in_ld", 2, 33, 31, in_ld=40)
_tr("b2_65x40_out_ld", 2, 65, 40, out_ld=72)
_tr("b3_33x31_gaps", 3, 33, 31, in_ld=37, out_ld=41, in_gap=5, out_gap=11)
# the two shapes HipConv1x1.forward builds (B = 2, 35 -> 51 channels, P = 50 pixels): (B, C, P) -> [B * P][kp], [B * P][op_] -> (B, O, P)
_tr("conv_in", 2, 35, 50, in_ld=50, out_ld=ru(35))
_tr("conv_out", 2, 50, 51, in_ld=ru(51), out_ld=50)
TR_BY_NAME = {c["name"]: c for c in TR_CASES}
assert len(TR_BY_NAME) == len(TR_CASES)

SPECIALS = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2049.0, 2051.0, 1e-6, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24,
                     6.1e-5, 65504.0, -65504.0, 65520.0, 65519.996, -0.0, np.nan], np.float32)


def tr_sizes(c):
    return (c["B"] - 1) * c["in_bs"] + c["R"] * c["in_ld"], (c["B"] - 1) * c["out_bs"] + c["C"] * c["out_ld"]


def tr_data(c):
    """the flat fp32 input buffer: N(0, 30) with the special values planted, IN_PAD in the row pads and batch gaps"""
    rs = _rs(c["name"])
    B, R, C = c["B"], c["R"], c["C"]
    x = (rs.standard_normal((B, R, C)) * 30).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 2 * SPECIALS.size:
        flat[rs.choice(flat.size, SPECIALS.size, replace=False)] = SPECIALS
    buf = np.full(tr_sizes(c)[0], IN_PAD, np.float32)
    b, r, cc = np.meshgrid(np.arange(B), np.arange(R), np.arange(C), indexing="ij")
    buf[b * c["in_bs"] + r * c["in_ld"] + cc] = x
    return dict(x=x, buf=buf)


def tr_expected(c, d, sentinel, mutant=None):
    """the whole destination buffer after the launch (fp32 or fp16 array), or None where the mutant writes outside it"""
    B, R, C = c["B"], c["R"], c["C"]
    dt = np.float16 if c["f16"] else np.float32
    out = np.full(tr_sizes(c)[1], sentinel, dt)
    b, r, cc = np.meshgrid(np.arange(B), np.arange(R), np.arange(C), indexing="ij")
    ld = c["in_ld"] if mutant == "swap_ld" else c["out_ld"]
    bs = c["in_bs"] if mutant == "batch_stride_of_other_side" else c["out_bs"]
    idx = b * bs + cc * ld + r
    x = d["x"]
    with np.errstate(over="ignore"):
        if c["f16"] and mutant == "truncate_fp16":
            h = x.astype(np.float16)
            big = np.abs(h.astype(np.float32)) > np.abs(x)  # rounded away from zero: step back towards it
            v = np.where(big, np.nextafter(h, np.float16(0)), h)
        else:
            v = x.astype(dt)
    keep = np.ones(idx.shape, bool)
    if mutant == "tile_edge_off_by_one" and R % 32 == 1:
        keep[:, R - 1, :] = False
    if idx.max() >= out.size:
        return None
    out[idx[keep]] = v[keep]
    return out


def tr_mutants(c):
    m = []
    if c["in_ld"] != c["out_ld"] and c["C"] > 1:
        m.append("swap_ld")
    if c["in_bs"] != c["out_bs"] and c["B"] > 1:
        m.append("batch_stride_of_other_side")
    if c["R"] % 32 == 1 and c["R"] > 1:
        m.append("tile_edge_off_by_one")
    if c["f16"] and c["R"] * c["C"] >= 2 * SPECIALS.size:
        m.append("truncate_fp16")
    return m


# -------------------------------------------------------------------------------------------------------- GROUPNORM_NCHW
def _gn(name, B, C, HW, G, n_norm, relu, dist="normal"):
    assert n_norm % G == 0 and 0 < n_norm <= C
    return dict(name=name, B=B, C=C, HW=HW, G=G, n_norm=n_norm, relu=relu, dist=dist)


GN_CASES = [
    _gn("n64", 3, 16, 16, 4, 16, False),                 # fewer values than threads; no tail workgroup
    _gn("n300_tail_relu", 3, 8, 100, 2, 6, True),         # n no multiple of 256; the tail is max(x, 0)
    _gn("hw1_gs4_tail", 3, 35, 1, 8, 32, False),          # HW = 1; the tail is a copy
    _gn("n4096_relu", 2, 8, 1024, 2, 8, True),
    _gn("g1", 3, 6, 37, 1, 6, False),
    _gn("common", 3, 16, 64, 4, 16, False, "common"),     # mean 30, std 1: E[x^2] - m^2 cancels 900 x the variance
    _gn("const_group", 3, 12, 50, 3, 12, False, "const"),  # one group constant: the variance clamps to 0, the output is beta
]
GN_BY_NAME = {c["name"]: c for c in GN_CASES}
# (case, mutant) -> the case where that mutant IS visible
GN_EXEMPT = {}


def gn_mutants(c):
    gs = c["n_norm"] // c["G"]
    m = ["unbiased_var", "neighbour_sample"]
    if c["n_norm"] < c["C"]:
        m.append("tail_normalised")
        if c["relu"]:
            m.append("tail_relu_dropped")
    if c["G"] > 1:
        m.append("gamma_within_group")
    if gs > 1:
        m.append("count_hw_only")
    return m


def gn_data(c):
    rs = _rs(c["name"])
    B, C, HW = c["B"], c["C"], c["HW"]
    x = rs.standard_normal((B, C, HW)).astype(np.float32)
    if c["dist"] == "common":
        x = (x + np.float32(30.0)).astype(np.float32)
    elif c["dist"] == "const":
        gs = c["n_norm"] // c["G"]
        x[:, gs:2 * gs, :] = np.float32(3.7)
    return dict(x=x, gamma=(1 + 0.2 * rs.standard_normal(c["n_norm"])).astype(np.float32),
                beta=(0.5 * rs.standard_normal(c["n_norm"])).astype(np.float32))


def gn_forward(c, d, mutant=None):
    """float64 reference of the case (or of a mutant): dict(y (B, C, HW), b, stored); b = 0 marks the exact tail"""
    B, C, HW, G, n_norm = c["B"], c["C"], c["HW"], c["G"], c["n_norm"]
    gs = n_norm // G
    x = d["x"].astype(np.float64)
    rows = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(B * HW, C)  # the same values as [B * HW][C] rows
    st = gn_stats(dict(B=B, S=HW, ld=C, G=G, n_norm=n_norm, tiles=False, flags=0, half=False), dict(x=rows), mutant)
    m, rstd = st["m"], st["rstd"]
    if mutant == "count_hw_only":
        xg = x[:, :n_norm].reshape(B, G, gs * HW)
        m = xg.sum(2) / HW
        rstd = 1 / np.sqrt(np.maximum((xg * xg).sum(2) / HW - m * m, 0) + EPS)
    ch = np.arange(n_norm) // gs
    e = lambda a: a[:, ch][:, :, None]  # [B][G] -> [B][n_norm][1]
    gi = np.arange(n_norm) % gs if mutant == "gamma_within_group" else np.arange(n_norm)
    gam, bet = d["gamma"].astype(np.float64)[gi][None, :, None], d["beta"].astype(np.float64)[gi][None, :, None]
    part = x[:, :n_norm]
    g = gam * e(rstd)
    y = x.copy()
    b = np.zeros_like(x)
    y[:, :n_norm] = (part - e(m)) * g + bet
    b[:, :n_norm] = (np.abs(gam) * e(st["rstd"]) * e(st["dm"]) + np.abs(gam) * np.abs(part - e(st["m"])) * e(st["dr"]) +
                     3 * U * (np.abs(part * g) + np.abs(e(st["m"]) * g) + np.abs(bet)))
    if mutant == "tail_normalised" and n_norm < C:
        y[:, n_norm] = (x[:, n_norm] - m[:, -1:]) * rstd[:, -1:]
    if c["relu"]:
        y[:, :n_norm] = np.maximum(y[:, :n_norm], 0)
        if mutant != "tail_relu_dropped":
            y[:, n_norm:] = np.maximum(y[:, n_norm:], 0)
    return store(dict(y=y, b=b), False)
