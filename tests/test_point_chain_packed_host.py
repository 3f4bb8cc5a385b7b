"""CPU: the packed weight buffer of SLIDE_OP_POINT_CHAIN (slide_amd/chain_pack.py, SlidePointChainArgs.wpk_bytes) holds, for every lane
of every wave, exactly the halves the row-major addressing of slide_amd/csrc/point_chain.hip reads, in the order the kernel consumes
them.

Two independent models meet here.  The DECODER is the packed kernel's addressing: lane l of wave w reads bytes [16 l, 16 l + 16) of
fragment j of the wave's slice, the slices follow each other.  The ROW-MAJOR model is the other kernel's pointer arithmetic, written
out per lane on the flat arrays: W + (32 w + (l & 31)) * K + 8 (l >> 5) + 16 s (Wz: + 128 K for res_connect).  The matrices hold random 16-bit
patterns, so a permutation error cannot hide; two mutant packers (the k-halves of a fragment swapped;
first_mlp and res_connect swapped) must be caught."""
import numpy as np
import pytest

from slide_amd import chain_pack

CASES = [(kz, n1c, wide) for kz in (32, 96, 192) for n1c in (1, 2) for wide in (False, True)]
K0 = 160


def _matrices(kz, n1c, wide):
    """fp16 arrays of random 16-bit patterns (compared as bits: a NaN pattern is as good as any)"""
    shapes = dict(Wz=(256, kz), W2=(128, 128), W0=(128, K0), W1=(32 * n1c, 128))
    rs = np.random.RandomState(kz + 7 * n1c + wide)
    names = list(shapes) + ([k + "_lo" for k in shapes] if wide else [])
    return {n: rs.randint(0, 1 << 16, shapes[n[:2]]).astype(np.uint16).view(np.float16) for n in names}


def _lane_read(flat, K, row0, w, s, l):
    """the eight halves lane l of wave w loads for k16 step s of a row-major [.][K] matrix (point_chain.hip: wp + s2 * 16)"""
    off = (row0 + 32 * w + (l & 31)) * K + 8 * (l >> 5) + 16 * s
    return flat[off:off + 8]


def _consumed(m, kz, n1c, w, wide):
    """[fragment][lane][8] as uint16: what wave w's lanes hold, in the order the packed kernel issues its loads"""
    flat = {k: v.reshape(-1).view(np.uint16) for k, v in m.items()}
    frags = []
    rd = lambda name, K, row0, s: frags.append([_lane_read(flat[name], K, row0, w, s, l) for l in range(64)])
    for s in range(kz // 16):
        rd("Wz", kz, 0, s)
        rd("Wz", kz, 128, s)
        if wide:
            rd("Wz_lo", kz, 0, s)
            rd("Wz_lo", kz, 128, s)
    for s in range(8):
        rd("W2", 128, 0, s)
    if wide:
        for s in range(8):
            rd("W2_lo", 128, 0, s)
    for s in range(K0 // 16):
        rd("W0", K0, 0, s)
    if w < n1c:
        for s in range(8):
            rd("W1", 128, 0, s)
    if wide:
        for s in range(K0 // 16):
            rd("W0_lo", K0, 0, s)
        if w < n1c:
            for s in range(8):
                rd("W1_lo", 128, 0, s)
    return np.array(frags, np.uint16)


def _decode(buf, kz, n1c, wide):
    """the packed kernel's view: per wave [fragment][lane][8]; slices back to back, sizes as the kernel computes them"""
    halves = np.ascontiguousarray(buf).view(np.uint16)
    lw, n2, nk0 = (4, 16, K0 // 16) if wide else (2, 8, K0 // 16)
    per_wave = (kz // 16) * lw + n2 + nk0 * (2 if wide else 1)
    out = []
    for w in range(4):
        base = w * per_wave + min(w, n1c) * n2
        n = per_wave + (n2 if w < n1c else 0)
        out.append(halves[base * 512:(base + n) * 512].reshape(n, 64, 8))
    assert (4 * per_wave + n1c * n2) * 512 == halves.size
    return out


def _pack(m, wide):
    return chain_pack.pack(m["Wz"], m["W2"], m["W0"], m["W1"], [m[k + "_lo"] for k in ("Wz", "W2", "W0", "W1")] if wide else None)


def _matches(buf, m, kz, n1c, wide):
    dec = _decode(buf, kz, n1c, wide)
    return all(d.shape == c.shape and (d == c).all() for d, c in ((dec[w], _consumed(m, kz, n1c, w, wide)) for w in range(4)))


@pytest.mark.parametrize("kz,n1c,wide", CASES)
def test_packed_buffer_is_what_the_row_major_kernel_reads(kz, n1c, wide):
    m = _matrices(kz, n1c, wide)
    buf = _pack(m, wide)
    assert buf.dtype == np.float16 and buf.size == 512 * chain_pack.n_fragments(kz, K0, n1c, wide)
    assert buf.size * 2 == 1024 * (4 * (2 * (kz // 16) + 8 + K0 // 16) + 8 * n1c) * (2 if wide else 1)  # (the launcher's formula)
    assert _matches(buf, m, kz, n1c, wide)
    # a permutation: nothing invented, nothing lost
    src = np.sort(np.concatenate([v.reshape(-1).view(np.uint16) for v in m.values()]))
    assert (np.sort(buf.view(np.uint16)) == src).all()


@pytest.mark.parametrize("kz,n1c,wide", [(32, 1, False), (192, 2, True)])
def test_mutant_packers_are_caught(monkeypatch, kz, n1c, wide):
    m = _matrices(kz, n1c, wide)
    good_fragment, good_order = chain_pack.fragment, chain_pack.wave_order
    # the two k-halves of every fragment swapped (lanes 32.. hold k 0..7)
    monkeypatch.setattr(chain_pack, "fragment", lambda W, w, s: good_fragment(W, w, s).reshape(2, 32, 8)[::-1].reshape(-1))
    assert not _matches(_pack(m, wide), m, kz, n1c, wide)
    monkeypatch.setattr(chain_pack, "fragment", good_fragment)
    # first_mlp and res_connect swapped
    swap = lambda *a: [(n, 128 - r0 if n.startswith("Wz") else r0, s) for n, r0, s in good_order(*a)]
    monkeypatch.setattr(chain_pack, "wave_order", swap)
    assert not _matches(_pack(m, wide), m, kz, n1c, wide)
    monkeypatch.setattr(chain_pack, "wave_order", good_order)
    assert _matches(_pack(m, wide), m, kz, n1c, wide)
