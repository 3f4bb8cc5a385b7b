"""The C ABI of libslide_hip.so as Python sees it: the ONE restatement of include/slide_hip.h, slide_engine.h, slide_train.h and
include/experiments/slide_resident.h -- constants, ctypes struct mirrors, function prototypes -- and the small helpers every
caller of the library needs.  tests/test_abi_mirror.py compiles the headers with the host C compiler and compares every value,
offset, size and prototype below with them, on the CPU: a renumbered op, a field added to a descriptor or a parameter that
changes width fails there, before anything runs on a GPU.

(The four structs of the experiments header live next to their only user, experiments/resident.py, and are checked by the same
test.)"""
import ctypes
from ctypes import c_float, c_int32, c_uint32, c_void_p

import torch

# ------------------------------------------------------------------------------------------------------------ constants
# enumerators and #defines of the headers, under the header's name minus the SLIDE_ prefix
EPI_RAW, EPI_NORM, EPI_STATS = 0, 1, 2
F_PRE_RELU, F_POST_RELU, F_OUT_F32, F_RES_PAIR, F_RES_PAIR_NBR, F_OUT_FM = 1, 2, 4, 8, 16, 32
# PREC_SPLIT: the fp32 plan (float storage, same ops) with its contractions on the fp16 matrix pipe as two-term operand splits --
# fp32-grade results
PREC_F32, PREC_F16, PREC_SPLIT = 0, 1, 2
PREC = {"fp32": PREC_F32, "fp16": PREC_F16, "split": PREC_SPLIT}
EPI_PACKED_VECS = 1  # bit 0 of a descriptor-array pointer: the blocks' [bias | gamma | beta] values follow the descriptors

OP_GEMM = 1
OP_PREP_POINTS = 2
OP_ASSEMBLE_SA = 3
OP_ASSEMBLE_FP = 4
OP_FINALIZE_GN = 5
OP_ATTN_COMBINE = 6
OP_COPY_COLS = 7
OP_TEMB = 8
OP_COND = 9
OP_UPDATE_POS = 10
OP_UPDATE_FEAT = 11
OP_ADVANCE_T = 12
OP_GROUPNORM_NCHW = 13
OP_SYNC = 14
OP_TRANSPOSE = 15
OP_ATTN_TAIL = 16
OP_GEMM_GX = 17
OP_PAIR_NORM = 18
OP_SA_CHAIN = 19
OP_ROWS_FROM_NCX = 20
OP_ROWS_TO_NCX = 21
OP_ROWS_GROUP = 22
OP_ROWS_GN = 23
OP_ROWS_CONCAT_QK = 24
OP_ROWS_ATTN = 25
OP_ROWS_POOL = 26
OP_ROWS_GN_JOINT = 27
OP_BLOCK_BODY = 30
OP_PAIR_FIRST = 31
OP_GEMM_CHAIN = 32
OP_HEAD_UPDATE = 33
OP_GEMM_GX_DUAL = 34
OP_SA_CHAIN_P = 35
OP_PP_STAGE = 36
OP_POINT_CHAIN = 37
OP_GEMM_ATTEND = 38
OP_ROWS_PAIR_EXPAND = 39

# status of an op whose kernel is not in the product library.  NOT in a header under include/ (csrc/launch.h defines it): unchecked
ST_EXPERIMENT = -20

# flag sets the headers describe in comments only (unchecked): SLIDE_OP_ROWS_GROUP i[7], SLIDE_OP_ROWS_GN i[5], SLIDE_OP_ROWS_POOL i[5],
# slide_chamfer_reduce's mode, SLIDE_OP_GEMM i[8] (LDS-DMA ring kernels | chunk-major W | a block carries a PAIR residual) and
# SLIDE_OP_ATTN_TAIL f[1] (chunk-major weights | two-stage ring | split arithmetic | fragment-major u / mo)
GROUP_FP, GROUP_ABS, GROUP_CENTER, GROUP_NO_XYZ, GROUP_IDX32 = 1, 2, 4, 8, 16
GN_PRE_RELU, GN_POST_RELU, GN_STATS_ONLY, GN_APPLY_ONLY = 1, 2, 4, 8
POOL_MAX, POOL_AVG, POOL_MAX_AVG = 0, 1, 2
CHAMFER_TERM = {None: 0, "mse": 1, "cos": 2}
GEMM_LDS_DMA, GEMM_W_CM, GEMM_PAIR_RES = 1, 2, 4
TAIL_W_CM, TAIL_TWO_STAGE, TAIL_SPLIT, TAIL_FM = 1, 2, 8, 16


# ------------------------------------------------------------------------------------------------------------ struct mirrors
def _fields(ctype, names):
    return [(n, ctype) for n in names.split()]


class SlideEpi(ctypes.Structure):
    _fields_ = (_fields(c_int32, "mode flags gs n_norm") + _fields(c_float, "inv_count stats_scale")
                + _fields(c_int32, "out_ld res_ld addvec_bs stats_bs pre_add_ld pre_add_shift addvec_idx_stride pad0")
                + _fields(c_void_p, "bias gamma beta addvec addvec_idx residual pre_add out stats_sum stats_sq res_b res_vd res_vw"))


class SlideGnFin(ctypes.Structure):
    _fields_ = (_fields(c_void_p, "sum sq gid gstart gend gamma beta scale shift") + [("inv_count", c_float)]
                + _fields(c_int32, "C bs G"))


class SlidePrepCopy(ctypes.Structure):
    _fields_ = [("dst", c_void_p)] + _fields(c_int32, "ld kind n pad")


class SlideChainLayer(ctypes.Structure):
    _fields_ = _fields(c_void_p, "X W epi") + _fields(c_int32, "x_ld k_pad n_cob pad")


class SlideHeadArgs(ctypes.Structure):
    _fields_ = (_fields(c_void_p, "X W0 W1 v0 b1 eps_out")
                + _fields(c_int32, "rows x_ld k0 n1c eps_ld kind C kdim ldf half_out n_copies")
                + [("clamp", c_float), ("seed_lo", c_uint32), ("seed_hi", c_uint32)]
                + _fields(c_void_p, "x noise t_dev keypoint t0 t1 t2 t3 t4 complete_x0 kmask feat0 copies"))


class SlidePointChainArgs(ctypes.Structure):
    _fields_ = (_fields(c_void_p, "Z Wz W2 W0 W1 vz v2 v0 b1 tvec t_idx cvec X eps Wz_lo W2_lo W0_lo W1_lo")
                + _fields(c_int32, "rows z_ld kz x_ld k0 n1c eps_ld t_stride t_bs c_bs fuse_update wpk_bytes")
                + [("upd", SlideHeadArgs)])


class SlideOp(ctypes.Structure):
    _fields_ = [("kind", c_int32), ("i", c_int32 * 11), ("f", c_float * 4), ("p", c_void_p * 14)]


# The argument blocks of SLIDE_OP_BLOCK_BODY.  Their C definition is in csrc/experiments/block_body.hip, not in a header, so the
# mirror test does NOT cover them: same field order, natural alignment on both sides, kept in step by hand.
class BodySlot(ctypes.Structure):
    _fields_ = [("src", c_void_p)] + _fields(c_int32, "chunk_stride nrows kind nvalid")


class BodyArgs(ctypes.Structure):
    _fields_ = [("slots", c_void_p), ("n_slots", c_int32),
                ("ta", c_void_p), ("tb", c_void_p),
                ("t_ld", c_int32), ("off1", c_int32), ("k1", c_int32), ("offr", c_int32), ("offk", c_int32), ("kk", c_int32),
                ("vv", c_void_p), ("vbs", c_int32), ("rv", c_void_p),
                ("nbr", c_void_p), ("d2", c_void_p), ("w", c_void_p),
                ("add0", c_void_p), ("add0_idx", c_void_p), ("add0_stride", c_int32), ("add0_bs", c_int32),
                ("sc", c_void_p), ("sh", c_void_p), ("aff_bs", c_int32),
                ("P", c_void_p), ("p_ld", c_int32),
                ("vec1", c_void_p), ("n1", c_int32), ("gs1", c_int32), ("inv1", c_float),
                ("add1", c_void_p), ("add1_bs", c_int32),
                ("vecm", c_void_p), ("n_mo", c_int32), ("gsm", c_int32), ("invm", c_float),
                ("addm", c_void_p), ("addm_bs", c_int32),
                ("vecu", c_void_p), ("n_u", c_int32), ("gsu", c_int32), ("nnu", c_int32), ("invu", c_float),
                ("vect", c_void_p), ("n_out", c_int32), ("gsv", c_int32), ("nnv", c_int32), ("invv", c_float),
                ("out", c_void_p), ("out_ld", c_int32), ("out2", c_void_p), ("out2_ld", c_int32), ("out2_n", c_int32),
                ("B", c_int32), ("dbg", c_void_p)]


UNCHECKED_STRUCTS = ("BodySlot", "BodyArgs")

# ------------------------------------------------------------------------------------------------------------ prototypes
# One letter per parameter: i = int, q = long long, f = float, p = any pointer or slide_stream_t.  c_void_p for every pointer
# keeps None, a Python int (data_ptr(), cuda_stream), a c_void_p, a ctypes array and byref(...) all valid arguments -- and converts
# the ints at full width: without argtypes ctypes passes a Python int as a 32-bit C int.
_CTYPE = {"i": ctypes.c_int, "q": ctypes.c_longlong, "f": c_float, "p": c_void_p}


def _proto(args, restype=ctypes.c_int):
    return restype, tuple(_CTYPE[a] for a in args)


PROTOTYPES = {name: _proto(args) for name, args in {
    # include/slide_hip.h
    "gather_points_kernel_wrapper": "iiiipppp",
    "gather_points_grad_kernel_wrapper": "iiiipppp",
    "furthest_point_sampling_kernel_wrapper": "iiipppp",
    "query_ball_point_kernel_wrapper": "iiifippppp",
    "group_points_kernel_wrapper": "iiiiipppp",
    "group_points_grad_kernel_wrapper": "iiiiipppp",
    "three_nn_kernel_wrapper": "iiippppp",
    "three_interpolate_kernel_wrapper": "iiiippppp",
    "three_interpolate_grad_kernel_wrapper": "iiiippppp",
    "slide_knn_points": "iiiipppppp",
    "slide_knn_gather": "iiiiipppp",
    "slide_sample_farthest_points": "iiippppp",
    "slide_gather_rows": "iiiipppp",
    "slide_chamfer_nn": "iiipipippppppp",
    "slide_chamfer_reduce": "iiippppppfiipipipp",
    "slide_chamfer_pairwise": "iiiipipiipp",
    "slide_emd_pairwise": "iiiipipiipp",
    "slide_occupancy_grid": "iipiippppppp",
    "slide_point_rasterize": "iiiippppp",
    "slide_grid_fixed_to_float": "qppp",
    "slide_grid_interp": "iiiippppp",
    "slide_fft3_r2c": "iipipp",
    "slide_fft3_c2r": "iippp",
    "slide_dpsr_spectral": "iipppp",
    "slide_dpsr_finish": "iiipiippp",
    "slide_dpsr_grid": "iiipppiipppppppp",
    "slide_dpsr_bwd_sums": "iippppp",
    "slide_dpsr_bwd_dpre": "iiipppppiipp",
    "slide_dpsr_spectral_adj": "iipppp",
    "slide_dpsr_bwd_points": "iiippppppiipppp",
    "slide_dpsr_grid_bwd": "iiippppppii" + "p" * 12,
    "slide_mc_bricks": "i",
    "slide_mc_count": "iipfppp",
    "slide_mc_emit": "iipfppppppp",
    "slide_mesh_cdf_span": "i",
    "slide_mesh_face_cdf": "iqpppppppp",
    "slide_mesh_sample": "ii" + "pppppp" + "iii" + "pp" + "i" + "ppppp",
    "slide_mesh_cc_span": "i",
    "slide_mesh_cc_label": "iqq" + "ppppp" + "ii" + "pp",
    "slide_mesh_cc_stats": "iqqppp" + "pppppppp" + "p",
    "slide_mesh_cc_select": "iqqppp" + "ppp" + "iqi" + "ppp" + "p",
    "slide_mesh_cc_compact": "iqq" + "ppp" + "pp" + "pp" + "pp" + "pppp" + "p",
    "slide_refine_span": "i",
    "slide_mirror_concat": "iiipiippppp",
    "slide_refine_to_dpsr": "iiiii" + "pp" + "iii" + "fif" + "pppppp",
    "slide_hip_device_ok": "",
    "slide_lane_reduce_selftest": "pppip",
    "slide_philox_normal_selftest": "iiiiiipp",
    # include/slide_engine.h
    "slide_run_ops": "pip",
    "slide_run_ops2": "pipp",
    "slide_run_chains": "pppii",
    "slide_run_chains_every": "ppppii",
    "slide_run_ops_repeat": "pippi",
    "slide_run_ops_timed": "pipp",
    "slide_graph_begin": "p",
    "slide_graph_end": "pp",
    "slide_graph_launch": "pp",
    "slide_graph_destroy": "p",
    "slide_event_create": "p",
    "slide_event_record": "pp",
    "slide_event_elapsed_ms": "ppp",
    "slide_event_destroy": "p",
    "slide_stream_create_cu_mask": "pip",
    "slide_stream_destroy": "p",
    "slide_sizeof_epi": "",
    "slide_sizeof_op": "",
    # include/slide_train.h
    "slide_gn_rows_bwd": "iiiiiipppppppppp",
    "slide_col_sums": "qipppp",
    "slide_col_sums_seg": "iqipppp",
    "slide_group_rows_bwd": "iiiiiiippppp",
    "slide_group_rows_coord_bwd": "iiiiiiippppppppp",
    "slide_concat_qk_bwd": "qiiiiiippppp",
    "slide_attn_rows_bwd": "qiiiiippppppp",
    "slide_chamfer_cd_bwd": "iiiipipipppppppp",
    "slide_col_max_seg": "iiiipppp",
    "slide_col_max_seg_bwd": "iiipppp",
    "slide_gauss_posterior_fwd": "iiiiippppp",
    "slide_gauss_posterior_bwd": "iiiiipppppp",
    # include/experiments/slide_resident.h
    "slide_resident_run": "pp",
    "slide_sizeof_rop": "",
    "slide_sizeof_rstrip": "",
    "slide_sizeof_rargs": "",
}.items()}
PROTOTYPES["slide_hip_version"] = _proto("", ctypes.c_char_p)
# the entry points of include/experiments/: only libslide_hip_exp.so exports them
EXPERIMENT_FUNCTIONS = frozenset(("slide_resident_run", "slide_sizeof_rop", "slide_sizeof_rstrip", "slide_sizeof_rargs"))


def bind(handle, experiments):
    """sets restype / argtypes of every function of PROTOTYPES on a loaded library (a missing symbol is an AttributeError)"""
    for name, (restype, argtypes) in PROTOTYPES.items():
        if experiments or name not in EXPERIMENT_FUNCTIONS:
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = restype, argtypes
    return handle


# ------------------------------------------------------------------------------------------------------------ helpers
def ru(x, m=32):
    return (x + m - 1) // m * m


def make_op(kind, i=(), f=(), p=()):
    o = SlideOp()
    o.kind = kind
    for k, v in enumerate(i):
        o.i[k] = int(v)
    for k, v in enumerate(f):
        o.f[k] = float(v)
    for k, v in enumerate(p):
        o.p[k] = None if v is None else int(v)
    return o


def ptr(t):
    """device address of a tensor (None stays None: a NULL pointer)"""
    return None if t is None else c_void_p(t.data_ptr())


def stream_of(t=None):
    """torch's current stream as a slide_stream_t"""
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def run_op(op):
    """launches one op on torch's current stream"""
    _lib.check(_lib.lib().slide_run_ops((SlideOp * 1)(op), 1, stream_of()), "slide_run_ops")


# the loader applies PROTOTYPES to every library it opens and run_op launches through it: the two modules import each other, so this
# import comes LAST, when everything ._lib reads from here exists
from . import _lib  # noqa: E402
