"""The DDPM update launches (SLIDE_OP_UPDATE_FEAT / SLIDE_OP_UPDATE_POS, slide_amd/csrc/engine.hip + ddpm_update.h): numpy restatements,
the case list and the noise generator's reference and bound -- shared by tests/test_hip_update_ops.py.

ARITHMETIC.  The kernels are compiled with contraction off, so every step is ONE correctly rounded IEEE float32 operation (the division
of the position update included), and a numpy float32 restatement in the same operation order gives the same bits:
  feature:   x0 = rc[t] x - rm1[t] eps;  [clamp > 0: x0 = min(max(x0, -clamp), clamp)];  [x0 = x0 m + complete_x0 (1 - m)];
             v = c1[t] x0 + c2[t] x;  [t > 0: v = v + std[t] z];  channels < kdim: the key-point condition
  position:  v = (x - c_eps[t] eps) / sqrt_alpha[t];  [t > 0: v = v + sigma[t] z]
The comparison is therefore BITWISE.  Tables have T = 8 entries; t_dev = [t, step, workgroup counter, nonce, first global sample, 3 spare].

NOISE.  philox_normal(seed, step, elem, nonce) = Box-Muller on the first two words of Philox4x32-10 keyed with (seed_lo, seed_hi) on the
counter (elem, step, 0x243F6A88 ^ nonce, 0x85A308D3).  The restatement runs Philox in integers and forms the two uniforms
u = (float32(w >> 8) + 0.5f) 2^-24 with the kernel's own two float32 operations (w >> 8 < 2^24 converts exactly; the addition rounds
once, the power of two scales exactly), so u1, u2 are the kernel's values bit for bit; the normal itself is evaluated in float64,
z = sqrt(-2 ln u1) cos(2 pi u2).  The kernel's value differs from it by the roundings of its four float32 steps.  With e = 2^-24 (half
an ulp, relative) and the library functions within ONE ulp (2 e relative) of the true function of their float32 argument:
  L = logf(u1):            |dL| <= 2 e |L|;     a = -2 L is exact
  s = sqrtf(a):            the argument's error halves under the root, the root itself is taken within one ulp (half an ulp when
                           the division / square root are correctly rounded, which is not assumed): |ds| <= (e + 2 e) s = 3 e s
  th = fl(fl(2 pi) u2):    the constant is rounded once, the product once: |dth| <= 2 e th <= 2 e 2 pi
  c = cosf(th):            |dc| <= |dth| |sin| + 2 e |c| <= 2 e 2 pi + 2 e
  z = fl(s c):             |dz| <= s |dc| + |c| |ds| + e |z| <= e s (4 pi + 2 + 3 + 1)
NORMAL_BOUND is that, with 1 % for the products of two errors: |z_kernel - z_float64| <= 1.01 e (4 pi + 6) sqrt(-2 ln u1), at most 6.6e-6
(u1 >= 2^-25).  A generator that mixes up two counter words draws unrelated normals, off by O(1): test_hip_update_ops.py checks on the
CPU that such a mutant misses the bound."""
import ctypes
import itertools

import numpy as np

F32 = np.float32
T = 8  # entries of the synthetic schedule tables
C, KDIM = 51, 3
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------ schedule tables
def feat_tables(seed=11):
    """(rc, rm1, c1, c2, std), T entries each: magnitudes of a real schedule, no structure the arithmetic could hide behind"""
    rs = np.random.RandomState(seed)
    return [rs.uniform(lo, hi, T).astype(F32) for lo, hi in ((1.0, 3.0), (0.2, 2.5), (0.05, 0.9), (0.1, 0.95), (0.01, 0.8))]


def pos_tables(seed=12):
    """(c_eps, sqrt_alpha, sigma)"""
    rs = np.random.RandomState(seed)
    return [rs.uniform(lo, hi, T).astype(F32) for lo, hi in ((0.01, 0.6), (0.7, 0.9999), (0.01, 0.5))]


# ------------------------------------------------------------------------------------------------------------ restatements
def feat_step(x, eps, keypoint, tabs, t, z, clamp=0.0, complete_x0=None, kmask=None, kdim=KDIM):
    """one feature update.  x (npts, C), eps (npts, >= C) with the prediction of channel c in column c, keypoint (npts, kdim),
    z (npts, C) or None at t == 0, complete_x0 (npts, C) and kmask (npts) or None.  Returns the new x; float32 throughout."""
    rc, rm1, c1, c2, std = (tab[t] for tab in tabs)
    assert all(a.dtype == F32 for a in (x, eps, keypoint, rc, rm1, c1, c2, std))
    c = x.shape[1]
    xv, ev = x[:, kdim:], eps[:, kdim:c]
    x0 = rc * xv - rm1 * ev
    if clamp > 0:
        x0 = np.minimum(np.maximum(x0, F32(-clamp)), F32(clamp))
    if complete_x0 is not None:
        m = kmask.astype(F32)[:, None]
        x0 = x0 * m + complete_x0[:, kdim:] * (F32(1) - m)
    v = c1 * x0 + c2 * xv
    if t > 0:
        v = v + std * z[:, kdim:]
    out = np.concatenate([keypoint, v], axis=1)
    assert out.dtype == F32
    return out


def pos_step(x, eps, tabs, t, z):
    """one position update on flat arrays: x (n), eps (n) gathered to the elements, z (n) or None at t == 0"""
    c_eps, sqrt_alpha, sigma = (tab[t] for tab in tabs)
    v = (x - c_eps * eps) / sqrt_alpha
    if t > 0:
        v = v + sigma * z
    assert v.dtype == F32
    return v


# ------------------------------------------------------------------------------------------------------------ the noise
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words; returns the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def philox_uniforms(seed_lo, seed_hi, step, nonce, elem0, n, order=(0, 1, 2, 3)):
    """(u1, u2) float32, the kernel's values bit for bit.  `order` permutes the four counter words (a mutant: (1, 0, 2, 3) swaps the
    element number and the step)"""
    elem = (np.uint64(elem0) + np.arange(n, dtype=np.uint64)) & M32
    words = [elem, np.full(n, step, np.uint64), np.full(n, 0x243F6A88 ^ (nonce & 0xFFFFFFFF), np.uint64), np.full(n, 0x85A308D3, np.uint64)]
    w0, w1, _, _ = philox4x32_10(*[words[k] for k in order], seed_lo, seed_hi)
    scale = F32(1.0 / 16777216.0)
    return [((w >> np.uint64(8)).astype(F32) + F32(0.5)) * scale for w in (w0, w1)]


def philox_normal_ref(seed_lo, seed_hi, step, nonce, elem0, n, order=(0, 1, 2, 3)):
    """(z, bound): the float64 normals of the kernel's uniforms and NORMAL_BOUND per element (module docstring)"""
    u1, u2 = (u.astype(np.float64) for u in philox_uniforms(seed_lo, seed_hi, step, nonce, elem0, n, order))
    s = np.sqrt(-2.0 * np.log(u1))
    e = 2.0 ** -24
    return s * np.cos(2.0 * np.pi * u2), 1.01 * e * (4.0 * np.pi + 6.0) * s


def as_i32(word):
    """a 32-bit unsigned word as the C int that carries its bit pattern"""
    return ctypes.c_int32(int(word) & 0xFFFFFFFF).value


# ------------------------------------------------------------------------------------------------------------ the feature cases
# npts: 816 elements (under one workgroup of any mapping), 2448, 17136 (several workgroups, a ragged last one)
# copies: () = none, or (n, ld, kind) per descriptor; kind 1 (a coordinate copy) is not the update's to write; n < C - kdim leaves
# the columns beyond n alone
COPIES_1 = ((C - KDIM, 72, 0),)
COPIES_3 = ((C - KDIM, 56, 0), (3, 5, 1), (20, 40, 0))
FEAT_CASES = [
    # name,            npts, eps_ld, clamp, t, resample, feat0 (None / "f16" / "f32"), copies
    ("n16_plain",        16, 0,  0.0, 5, False, None,  ()),
    ("n16_t0_f16_c3",    16, 64, 1.5, 0, True,  "f16", COPIES_3),
    ("n48_f32_c1",       48, 0,  1.5, 3, True,  "f32", COPIES_1),
    ("n48_f16_c0",       48, 64, 0.0, 7, False, "f16", ()),
    ("n336_f16_c3",     336, 0,  1.5, 2, True,  "f16", COPIES_3),
    ("n336_t0_f32_c3",  336, 64, 0.0, 0, False, "f32", COPIES_3),
    ("n336_f32_c1",     336, 64, 1.5, 6, False, "f32", COPIES_1),
    ("n336_resample",   336, 0,  0.0, 4, True,  None,  ()),
]
POS_CASES = [(n, eps_ld, t) for (n, eps_ld), t in zip(itertools.product((48, 288), (0, 8)), (5, 0, 3, 7))]


def feat_inputs(npts, eps_ld, resample, seed):
    """x, eps (npts, max(eps_ld, C)), keypoint, complete_x0 / kmask (or None), as float32 arrays"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((npts, C)).astype(F32)
    eps = rs.standard_normal((npts, eps_ld or C)).astype(F32)
    keypoint = rs.uniform(-1, 1, (npts, KDIM)).astype(F32)
    cx0 = rs.standard_normal((npts, C)).astype(F32) if resample else None
    kmask = (rs.uniform(size=npts) < 0.5).astype(F32) if resample else None
    return x, eps, keypoint, cx0, kmask
