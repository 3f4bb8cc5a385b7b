"""The PACKED weight buffer of SLIDE_OP_POINT_CHAIN (SlidePointChainArgs.wpk_bytes, include/slide_engine.h; csrc/point_chain.hip).

The chain's kernel keeps every weight in MFMA A-fragment registers: wave w owns channel block w (32 channels) of every layer, and for
the k16 step s of a matrix W [channels][k] lane l holds the eight halves W[32 w + (l & 31)][16 s + 8 (l >> 5) : + 8].  Row-major
storage makes one load instruction read 32 B from each of 32 rows; the packed buffer stores every fragment as the 1 KB the instruction
reads, lane l at byte 16 l, and a wave's fragments in the order the kernel consumes them:

  for s < kz/16:  Wz rows 0.. (first_mlp) | Wz rows 128.. (res_connect) | wide: Wz_lo rows 0.. | Wz_lo rows 128..
  W2 s = 0..7 | wide: W2_lo s = 0..7
  W0 s < k0/16
  W1 s = 0..7                      (waves w < n1c only)
  wide: W0_lo s < k0/16 | W1_lo s = 0..7 (w < n1c)

The four waves' slices follow each other without gaps.  A plain index permutation of the fp16 values: nothing is computed."""
import numpy as np

FRAG = 512  # halves per fragment (1 KB)


def fragment(W, w, s):
    """the 512 halves of channel block w, k16 step s of W [channels][k], in lane order"""
    return W[32 * w:32 * w + 32, 16 * s:16 * s + 16].reshape(32, 2, 8).transpose(1, 0, 2).reshape(-1)


def n_fragments(kz, k0, n1c, wide):
    """fragments of the whole buffer (the launcher checks wpk_bytes against 1024 times this)"""
    return (4 * (2 * (kz // 16) + 8 + k0 // 16) + 8 * n1c) * (2 if wide else 1)


def wave_order(kz, k0, n1c, w, wide):
    """[(matrix name, first row of the 128-row matrix half, k16 step)] of wave w's slice, in storage order"""
    out = []
    for s in range(kz // 16):
        out += [("Wz", 0, s), ("Wz", 128, s)] + ([("Wz_lo", 0, s), ("Wz_lo", 128, s)] if wide else [])
    out += [("W2", 0, s) for s in range(8)] + ([("W2_lo", 0, s) for s in range(8)] if wide else [])
    out += [("W0", 0, s) for s in range(k0 // 16)]
    if w < n1c:
        out += [("W1", 0, s) for s in range(8)]
    if wide:
        out += [("W0_lo", 0, s) for s in range(k0 // 16)]
        if w < n1c:
            out += [("W1_lo", 0, s) for s in range(8)]
    return out


def pack(Wz, W2, W0, W1, lo=None):
    """fp16 arrays Wz [256][kz], W2 [128][128], W0 [128][k0], W1 [32 n1c][128] (+ lo = their four low-fragment arrays: the WIDE
    form) -> the packed buffer, a flat fp16 array of n_fragments(...) * 512 halves"""
    m = dict(Wz=Wz, W2=W2, W0=W0, W1=W1)
    if lo is not None:
        m.update(zip(("Wz_lo", "W2_lo", "W0_lo", "W1_lo"), lo))
    m = {k: np.ascontiguousarray(v, np.float16) for k, v in m.items()}
    kz, k0, n1c = m["Wz"].shape[1], m["W0"].shape[1], m["W1"].shape[0] // 32
    assert m["Wz"].shape == (256, kz) and kz % 32 == 0 and m["W2"].shape == (128, 128) and m["W0"].shape == (128, k0) and k0 % 16 == 0
    assert m["W1"].shape == (32 * n1c, 128) and all(m[k + "_lo"].shape == m[k].shape for k in ("Wz", "W2", "W0", "W1") if lo is not None)
    out = [fragment(m[name][r0:], w, s) for w in range(4) for name, r0, s in wave_order(kz, k0, n1c, w, lo is not None)]
    out = np.concatenate(out)
    assert out.size == FRAG * n_fragments(kz, k0, n1c, lo is not None)
    return out
