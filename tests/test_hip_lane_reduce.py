"""The transposing lane reduction of the GroupNorm epilogues (slide_amd/csrc/lane_reduce.h) against the all-reduce it replaced,
through slide_lane_reduce_selftest: one 64-lane wave sums NV values per lane over each 32-lane half wave both ways.

The kernels' results must not change, so the comparison is BITWISE: every total the new reduction leaves in a lane equals the
all-reduce's total of that value, and both equal a numpy float32 restatement of the tree.  The tree, written out: every lane adds
the value of lane ^ 1, then lane ^ 2, lane ^ 4, lane ^ 8 and lane ^ 16, one rounded fp32 addition per level (x + y and y + x
are the same number, so both partners hold the same partial after a level).  The new reduction keeps the total of value i in the
lanes whose number, bit-reversed over the first min(log2 NV, 5) bits, gives the top bits of i (lane_reduce_index).

The CPU test makes the GPU test meaningful: with the inputs used here, a tree with any two levels swapped differs from the right
one in at least one bit for every NV, so a reduction that pairs the lanes in another order cannot pass."""
import itertools

import numpy as np
import pytest

NVS = (4, 8, 16, 32, 64)
LEVELS = (1, 2, 4, 8, 16)  # partner = lane ^ k, in this order
SEED = 20240611


def _inputs(nv):
    """(64, nv) fp32: magnitudes spread over 2^-8 .. 2^8, mixed signs"""
    rs = np.random.RandomState(SEED + nv)
    mag = np.exp2(rs.uniform(-8.0, 8.0, (64, nv)))
    return (mag * rs.choice((-1.0, 1.0), (64, nv))).astype(np.float32)


def _tree(x, order=LEVELS):
    """what every lane holds after the all-reduce: (64, nv) fp32"""
    v = x.astype(np.float32).copy()
    lanes = np.arange(64)
    for k in order:
        v = (v + v[lanes ^ k]).astype(np.float32)
    return v


def _index(nv, lane):
    """number of the value whose total lane `lane` holds in register 0 (lane_reduce_index<NV>)"""
    nbits = nv.bit_length() - 1
    nl = min(nbits, 5)
    rev = sum(((lane >> k) & 1) << (nl - 1 - k) for k in range(nl))
    return rev << (nbits - nl)


def _regs(nv):
    return max(nv // 32, 1)


def test_index_covers_every_value_once_per_half_wave():
    for nv in NVS:
        for half in (0, 1):
            held = [_index(nv, lane) + j for lane in range(32 * half, 32 * half + 32) for j in range(_regs(nv))]
            assert sorted(set(held)) == list(range(nv))
            assert len(held) == max(nv, 32)  # nv < 32: 32 / nv lanes hold copies of a total


def test_swapped_levels_change_the_bits():
    for nv in NVS:
        x = _inputs(nv)
        assert np.abs(x).min() >= 2.0 ** -8 and np.abs(x).max() <= 2.0 ** 8 and (x < 0).any() and (x > 0).any()
        want = _tree(x)
        for a, b in itertools.combinations(range(len(LEVELS)), 2):
            order = list(LEVELS)
            order[a], order[b] = order[b], order[a]
            mutant = _tree(x, order)
            assert (mutant.view(np.uint32) != want.view(np.uint32)).any(), (nv, order)
            np.testing.assert_allclose(mutant, want, rtol=1e-3, atol=1e-2)  # (the same sums, in another order)


@pytest.mark.gpu
@pytest.mark.parametrize("nv", NVS)
def test_new_reduction_is_bitwise_the_all_reduce(gpu_device, nv):
    import torch
    from slide_amd import _lib
    x = _inputs(nv)
    nr = _regs(nv)
    xin = torch.from_numpy(x).to(gpu_device)
    out_new = torch.full((64, nr), float("nan"), device=gpu_device)
    out_old = torch.full((64, nv), float("nan"), device=gpu_device)
    _lib.check(_lib.lib().slide_lane_reduce_selftest(_lib.ptr(xin), _lib.ptr(out_new), _lib.ptr(out_old), nv, _lib.stream_of()),
               "slide_lane_reduce_selftest")
    torch.cuda.synchronize()
    new, old = out_new.cpu().numpy().view(np.uint32), out_old.cpu().numpy().view(np.uint32)
    want = _tree(x).view(np.uint32)
    assert (old == want).all(), "the all-reduce is not the tree of the docstring"
    for lane in range(64):
        for j in range(nr):
            i = _index(nv, lane) + j
            assert new[lane, j] == old[lane, i], (lane, j, i)
            assert new[lane, j] == want[lane, i], (lane, j, i)


@pytest.mark.gpu
def test_selftest_rejects_other_sizes(gpu_device):
    import torch
    from slide_amd import _lib
    buf = torch.zeros(64 * 64, device=gpu_device)
    for nv in (0, 2, 12, 128):
        assert _lib.lib().slide_lane_reduce_selftest(_lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), nv, _lib.stream_of()) == -2
    assert _lib.lib().slide_lane_reduce_selftest(None, _lib.ptr(buf), _lib.ptr(buf), 4, _lib.stream_of()) == -2
