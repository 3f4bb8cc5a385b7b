"""The batch-size forms of the fused denoiser plan, shared by tests/test_host_logic.py (the thresholds, built on the CPU) and
tests/test_hip_engine.py (every form against the oracle).

DenoiserEngine picks kernels from the number of tiles a launch has, so the batch size decides what runs.  The fp16 feature
plan has six forms:
  A   1 - 256   two dual generated-X launches, the SA chains with their query GEMM riding along (sa_chain_p_kernel)
  B 257 - 512   one FP block's dual launch splits into two 128-channel-tile launches (engine.py: the 64-channel tiles only
                while the grid is <= 256 tiles)
  C 513 - 1024  no dual launch; sa_chain_kernel<8> with its query GEMM apart; one SLIDE_OP_FINALIZE_GN (the 16-row kernel
                finalises GroupNorm statistics itself only up to 1024 tiles)
  D 1025 - 1364 a second SLIDE_OP_FINALIZE_GN
  E 1365 - 2048 sa_chain_kernel<4> with its query GEMM apart; a third SLIDE_OP_FINALIZE_GN
  F >= 2049     a fourth SLIDE_OP_FINALIZE_GN
The split position plan and the fp32 plans have one form at every batch size."""
import collections

from slide_amd import engine as E

_OP_NAMES = {v: k for k, v in vars(E).items() if k.startswith("OP_") and isinstance(v, int)}


def form_signature(e):
    """what a plan runs: its launch count, the multiset of its op kinds and the multiset of its named kernels"""
    return (len(e.ops), dict(collections.Counter(_OP_NAMES[o.kind] for o in e.ops)),
            dict(collections.Counter(e.kernel_names.values())))


_PAIR_FIRST = {"pair_first_kernel<false>": 2, "pair_first_kernel<true>": 2, "gemm_gx_n64_kernel<8, 3, 1>": 2}
_GX128 = {"gemm_gx_kernel<7, 2, 1>": 1, "gemm_gx_kernel<7, 3, 0>": 1}
_BASE_KINDS = {"OP_PREP_POINTS": 1, "OP_COPY_COLS": 1, "OP_TEMB": 1, "OP_ATTN_TAIL": 4, "OP_PAIR_FIRST": 4}


def _form(n, gemm, fin, gx, dual, sa_chain, chain_p, kernels):
    kinds = dict(_BASE_KINDS, OP_GEMM=gemm, OP_GEMM_GX=gx, OP_FINALIZE_GN=fin, OP_GEMM_GX_DUAL=dual, OP_SA_CHAIN=sa_chain,
                 OP_SA_CHAIN_P=chain_p)
    return n, {k: v for k, v in kinds.items() if v}, dict(_PAIR_FIRST, **kernels)


# form -> (first batch size, last batch size or None, expected form_signature) of the fp16 feature plan
FEATURE_FP16_FORMS = {
    "A": (1, 256, _form(25, 8, 0, 2, 2, 0, 2, {"gemm_gx_dual_kernel<7>": 2, "sa_chain_p_kernel<8>": 1, "sa_chain_p_kernel<4>": 1})),
    "B": (257, 512, _form(26, 8, 0, 4, 1, 0, 2, dict(_GX128, **{"gemm_gx_dual_kernel<7>": 1, "sa_chain_p_kernel<8>": 1,
                                                                  "sa_chain_p_kernel<4>": 1}))),
    "C": (513, 1024, _form(29, 9, 1, 6, 0, 1, 1, {"gemm_gx_kernel<7, 2, 1>": 1, "gemm_gx_kernel<7, 3, 0>": 2,
                                                   "gemm_gx_kernel<7, 3, 1>": 1, "sa_chain_kernel<8>": 1, "sa_chain_p_kernel<4>": 1})),
    "D": (1025, 1364, _form(30, 9, 2, 6, 0, 1, 1, {"gemm_gx_kernel<7, 2, 1>": 1, "gemm_gx_kernel<7, 3, 0>": 2,
                                                    "gemm_gx_kernel<7, 3, 1>": 1, "sa_chain_kernel<8>": 1, "sa_chain_p_kernel<4>": 1})),
    "E": (1365, 2048, _form(32, 10, 3, 6, 0, 2, 0, {"gemm_gx_kernel<7, 2, 1>": 1, "gemm_gx_kernel<7, 3, 0>": 2,
                                                     "gemm_gx_kernel<7, 3, 1>": 1, "sa_chain_kernel<8>": 1, "sa_chain_kernel<4>": 1})),
    "F": (2049, None, _form(33, 10, 4, 6, 0, 2, 0, {"gemm_gx_kernel<7, 2, 1>": 1, "gemm_gx_kernel<7, 3, 0>": 2,
                                                     "gemm_gx_kernel<7, 3, 1>": 1, "sa_chain_kernel<8>": 1, "sa_chain_kernel<4>": 1})),
}


def feature_fp16_form(B):
    """the form letter the fp16 feature plan of B samples must have"""
    for name, (lo, hi, _) in FEATURE_FP16_FORMS.items():
        if lo <= B and (hi is None or B <= hi):
            return name
    raise ValueError(B)


def expected_feature_fp16_signature(B):
    return FEATURE_FP16_FORMS[feature_fp16_form(B)][2]
