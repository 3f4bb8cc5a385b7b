"""Host side of the fused denoiser engine (include/slide_engine.h).

`DenoiserEngine` turns a reference `pointnet_config` + a reference-named state dict
 into a *plan*: packed MFMA weights, per-32-channel epilogue tables and a
flat list of `SlideOp` launches that computes PointNet2CloudCondition.forward
(pointnet2/models/pointnet2_with_pcld_condition.py:286-489) for the configuration family every shipped
DDPM config uses (16 latent points, 'nn' grouping, kNN feature propagation, attention, GroupNorm,
bias, res_connect, no condition cloud).  The plan is replayed eagerly or from a captured hipGraph.

torch is used for device memory and streams only; all arithmetic runs in libslide_hip.so.
"""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import chain_pack, knobs
from ._lib import SlideHipError, check, lib
# the C side of include/slide_engine.h -- every OP_* / EPI_* / F_* constant, PREC, the struct mirrors, make_op and ru -- is declared
# in abi.py; all of it stays importable from this module
from .abi import *  # noqa: F401,F403


class GnLayout(NamedTuple):
    """physical channel layout of a GroupNorm'ed (or plain) segment, see gn_layout"""
    index: np.ndarray  # physical channel of every logical channel
    width: int         # physical channels
    n_norm: int        # physical channels that are normalised (the leading ones)
    gs: int            # group size, physical: a power of two
    gs_logical: int    # group size, logical: what the statistics are divided by

    @classmethod
    def plain(cls, C):
        """C channels where they are, none normalised"""
        return cls(np.arange(C), C, 0, 1, 1)

    @property
    def unpermuted(self):
        """every channel where it logically is (no padded groups)"""
        return np.array_equal(self.index, np.arange(len(self.index)))

    @property
    def identity(self):
        """unpermuted and every channel normalised"""
        return self.unpermuted and self.width == len(self.index) and self.n_norm == len(self.index)

    def raw(self):
        """the same columns, no normalisation"""
        return GnLayout(self.index, self.width, 0, 1, 1)


def gn_layout(C):
    """MyGroupNorm(min(32, C), C) (pointnet2_modules.py:24-42): the first n_norm = C - C % G channels are
    normalised in G groups, the rest pass through.  Returns the PHYSICAL channel layout the engine uses so that
    every group is a power-of-two run inside one 32-channel block:
    (phys_index[c] for logical c, C_phys, n_norm_phys, gs_phys, gs_logical)."""
    G = min(32, C)
    n_norm = C - C % G
    gs = n_norm // G
    gs_p = 1
    while gs_p < gs:
        gs_p *= 2
    assert gs_p <= 32, "GroupNorm group size > 32 not supported by the epilogue"
    idx = np.empty(C, np.int64)
    for c in range(C):
        idx[c] = (c // gs) * gs_p + c % gs if c < n_norm else G * gs_p + (c - n_norm)
    return GnLayout(idx, int(G * gs_p + (C - n_norm)), int(G * gs_p), int(gs_p), int(gs))


# the tuples a segment dict (DenoiserEngine._gemm) carries, by name.  Callers may pass plain tuples: _segment coerces them once
class AddVec(NamedTuple):
    """per-sample vector added after the activation: row (sample, or idx[0] of a per-timestep table) of `vec`, from column `off`"""
    vec: torch.Tensor
    off: int
    bs: int                      # per-sample stride
    idx: torch.Tensor = None     # device-side row index (None: the sample's own row)
    idx_stride: int = 0          # stride of the rows `idx` selects


class PreAdd(NamedTuple):
    """pre-activation add of a per-point table: row (output row >> shift), or shift < 0: row of the NEIGHBOUR point (K = 2^-shift)"""
    table: torch.Tensor
    shift: int
    coff: int = 0


class ResPair(NamedTuple):
    """PAIR residual: residual(p, j) = ta[q] + tb[p] (+ d2 vd + w vw): ta, tb tables, first column, vv = vd | vw fp32 [2][Opad] for
    the 8-neighbour samples or None"""
    ta: torch.Tensor
    tb: torch.Tensor
    coff: int
    vv: torch.Tensor


class Stats(NamedTuple):
    """per-sample channel sums / sums of squares of a STATS segment, from column `coff`, scaled by `scale`"""
    sum: torch.Tensor
    sq: torch.Tensor
    coff: int
    scale: float


class Gather(NamedTuple):
    """the leading `chunks` 32-column chunks of X are gathered from the neighbours' rows of `table`"""
    table: torch.Tensor
    nbr: torch.Tensor
    K: int
    chunks: int


class InAffine(NamedTuple):
    """per-sample input affine x * scale + shift, from column `off`, per-sample stride `bs`"""
    scale: torch.Tensor
    shift: torch.Tensor
    off: int
    bs: int


class GxArgs(NamedTuple):
    """the generated input of a SLIDE_OP_GEMM_GX launch (_emit_gx): columns [coff, coff + k_pad) of the pair tables, never stored"""
    ta: torch.Tensor          # tables [B*16][t_ld]: fp16, split plans float
    tb: torch.Tensor
    coff: int
    k_pad: int
    rows: int
    mode: int                 # 0: a first Mlp layer's output (+ add), 1: the keys under the joint GroupNorm (in_affine)
    add: AddVec = None
    vv: torch.Tensor = None   # per-sample (vd | vw) fp32 [B][2][t_ld] of the 8-neighbour samples


class PairTables(NamedTuple):
    """what _pair_first leaves for the consumers (generated-X GEMMs, PAIR residuals): the tables and their geometry"""
    ta: torch.Tensor
    tb: torch.Tensor
    ldy: int
    offs: list                # first table column of every segment
    rows: int                 # K-expanded rows
    vv: torch.Tensor          # per-sample (vd | vw) [B][2][ldy], 8-neighbour samples (else None)
    vv_in: np.ndarray         # their coefficient rows [2][ldy] on the host
    tabs: tuple               # (neighbour, d2, w) tables of the 8-neighbour samples (else None)

    def __getitem__(self, k):  # (fields by name as well, as callers read the dict this record replaced)
        return getattr(self, k) if isinstance(k, str) else tuple.__getitem__(self, k)


class PairFused(NamedTuple):
    """what SLIDE_OP_PAIR_FIRST takes beside its per-point GEMM (_emit_pair_first): the table pass of _pair_first"""
    cob0: int                 # 32-channel blocks of the leading (non-pair) segments
    K: int
    wa: torch.Tensor          # coordinate weights [ldy][4] of the a / b tables; vv_in [2][ldy]: 8-neighbour samples (else None)
    wb: torch.Tensor
    vv_in: torch.Tensor
    t: PairTables             # what the pass writes


class BlockPair(NamedTuple):
    """an SA / FP block's view of its pair tables: [first_mlp | res_connect | keys] at columns off1 / offr / offk"""
    t: PairTables
    off1: int
    offr: int
    offk: int
    lay1: GnLayout            # first_mlp's output layout
    add1: AddVec              # its t-embedding rows, added by the consumers (or None)
    rvv: torch.Tensor         # (vd | vw) of the res_connect columns [2][rres], 8-neighbour samples (else None)


class Query(NamedTuple):
    """an attention block's per-point query branch (_attention_query): its buffers and its GEMM segment"""
    Tq: torch.Tensor
    ssum: torch.Tensor
    ssq: torch.Tensor
    qseg: dict


class AttnState(NamedTuple):
    """an attention block between its three phases (_attn_open -> _attn_scores -> _attn_finish)"""
    apfx: str
    npx_log2: int
    C1: int                   # query channels; C1p / C2p: padded query / key channels, ldT = C1p + C2p
    C1p: int
    C2p: int
    ldT: int
    cout: int
    Tq: torch.Tensor          # per-point queries; their statistics and the keys' are in `fin`
    Tk: torch.Tensor          # stored keys (None: generated from the pair tables)
    scale: torch.Tensor       # joint GroupNorm of [q | k] as a per-sample affine ...
    shift: torch.Tensor
    fin: SlideGnFin           # ... and what finalises it (host copy: statistics, group tables, gamma / beta, scale / shift)
    pair_fin: bool            # the pair-table pass finalised it
    pair: BlockPair           # (None: stored first-layer outputs)
    mo: torch.Tensor          # the values' input, written between scores and finish
    end: str                  # "body" (SLIDE_OP_BLOCK_BODY takes over after P) | "fused" (one tail launch) | "combine"
    P: torch.Tensor = None    # from _attn_scores: per-point query half of weight_conv.2, u and its layout, scores (end == "combine")
    u: torch.Tensor = None
    lay: GnLayout = None
    S: torch.Tensor = None


class ChainFront(NamedTuple):
    """the last FP block's second Mlp as _point_chain may chain it to the head"""
    launches: list
    Z: torch.Tensor
    zin: int
    m2: str
    n1: int
    n2: int


def _rec(T, v):
    """a plain tuple, or a dict of its fields, (or None) as the record T"""
    return None if v is None else T(**v) if isinstance(v, dict) else T(*v)


_SEG_RECORDS = dict(layout=GnLayout, addvec=AddVec, pre_add=PreAdd, res_pair=ResPair, stats=Stats)


def _segment(sg):
    """a copy of a segment dict with its tuples as records and its layout filled in (no layout: the channels where they are)"""
    sg = dict(sg)
    for k, T in _SEG_RECORDS.items():
        sg[k] = _rec(T, sg.get(k))
    if sg["layout"] is None:
        sg["layout"] = GnLayout.plain(sg["w"].shape[0])
    return sg


def seg_offsets(segs):
    """(first physical column of every segment, total width) of segments stored side by side, each padded to 32 channels"""
    offs, off = [], 0
    for sg in segs:
        offs.append(off)
        lay = _rec(GnLayout, sg.get("layout"))
        off += ru(sg["w"].shape[0] if lay is None else lay.width)
    return offs, off


def chunk_major(w):
    """weights [n][k] -> [k / 32][n][32]"""
    return np.ascontiguousarray(w.reshape(w.shape[0], -1, 32).transpose(1, 0, 2))


def epi_vectors(lay, n, bias=None, gn=None):
    """[bias | gamma | beta] as float rows [3][n], in the physical channel order of `lay`"""
    v = np.zeros((3, n), np.float32)
    if bias is not None:
        v[0, lay.index] = bias
    if gn is not None:
        gam, bet = gn
        v[1, lay.index[:gam.shape[0]]] = gam
        v[2, lay.index[:bet.shape[0]]] = bet
    return v


class _Layer(NamedTuple):
    """a layer as _gemm packs it, before an emitter makes a launch of it"""
    segs: list           # the segments (_segment)
    widths: list         # padded physical width of every segment
    W: np.ndarray        # float weights [n_cob * 32][ld], row-major
    Wd: torch.Tensor     # the same on the device, in the layer's storage type and order
    w_cm: bool           # Wd is chunk-major
    epi: torch.Tensor    # descriptor array (+ packed vectors)
    epi_ptr: int         # its address as the ops carry it (bit 0: SLIDE_EPI_PACKED_VECS)
    n_cob: int
    ld: int
    rows: int
    flops: int

    def written(self):
        """bytes the layer's outputs take"""
        return sum(self.rows * n * sg["out"].element_size() for sg, n in zip(self.segs, self.widths) if sg["out"] is not None)


class _Arena:
    """keeps device tensors alive and hands out raw pointers"""

    def __init__(self, device):
        self.device = device
        self.keep = []

    def zeros(self, *shape, dtype=torch.float32):
        t = torch.zeros(*shape, device=self.device, dtype=dtype)
        self.keep.append(t)
        return t

    def put(self, arr, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(arr))
        if dtype is not None:
            t = t.to(dtype)
        t = t.to(self.device)
        self.keep.append(t)
        return t


def _dp(t):
    """data_ptr() of a tensor as make_op takes it (None stays None: a NULL pointer)"""
    return None if t is None else t.data_ptr()


class Launch:
    """one launch of a plan with what the host knows about it: the op, its accounting -- FLOPs, algorithmic HBM bytes (read, written),
    rocprofv3 kernel name (bench.py's roofline attribution); None where nothing was recorded -- and its roles.  A role says what the
    rest of the host code wants this launch for: "prep" (point preparation), "eps_copy" (compaction of the prediction), "xyz_copy"
    (reads nothing but the coordinates), "head0" / "head1" (output head layers), "pc0" .. "pc3" (layers of the point chain).  The merge
    passes carry all of it along (`merged`); positions in the plan are derived once, at the end (`plan_tables`).
    body: the BodyArgs of a SLIDE_OP_BLOCK_BODY launch; w16: the float weights of a per-point layer _merge_pp may fold."""
    __slots__ = ("op", "flops", "nbytes", "name", "roles", "body", "w16")

    def __init__(self, op, flops=None, nbytes=None, name=None, roles=(), body=None, w16=None):
        self.op, self.flops, self.nbytes, self.name, self.roles, self.body, self.w16 = op, flops, nbytes, name, set(roles), body, w16


def merged(op, name, parts):
    """the launch that stands for `parts`: their summed FLOPs and bytes, the union of their roles"""
    return Launch(op, sum(p.flops or 0 for p in parts), tuple(sum((p.nbytes or (0, 0))[z] for p in parts) for z in (0, 1)), name,
                  set().union(*(p.roles for p in parts)))


def rewrite(plan, match):
    """one peephole pass.  match(plan, i) -> None (the launch stays) or (n, out): the n launches from i are replaced by `out`, whose
    items are launches of the plan (kept as they are) or the arguments of `merged`"""
    new, i = [], 0
    while i < len(plan):
        m = match(plan, i)
        n, out = (1, [plan[i]]) if m is None else m
        new += [r if isinstance(r, Launch) else merged(*r) for r in out]
        i += n
    return new


def accounting(plan):
    """(gemm_flops, gemm_bytes, kernel_names) of a launch list, keyed by position"""
    return tuple({k: getattr(e, f) for k, e in enumerate(plan) if getattr(e, f) is not None} for f in ("flops", "nbytes", "name"))


def plan_tables(plan):
    """everything that is read by position in a finished launch list.  head / point_chain: the positions of the two / four launches
    with those roles, None unless they are distinct launches (the point chain's: consecutive ones) -- a merge pass took them"""
    at = lambda *roles: [k for r in roles for k, e in enumerate(plan) if r in e.roles]
    flops, nbytes, names = accounting(plan)
    head, pc = at("head0", "head1"), at("pc0", "pc1", "pc2", "pc3")
    return dict(ops=[e.op for e in plan], gemm_flops=flops, gemm_bytes=nbytes, kernel_names=names, xyz_copy_idx=sorted(at("xyz_copy")),
                eps_copy_idx=(at("eps_copy") or [None])[0], prep_idx=(at("prep") or [None])[0],
                head=head if len(head) == 2 and head[0] != head[1] else None,
                point_chain=pc if len(pc) == 4 and pc == list(range(pc[0], pc[0] + 4)) else None)


class DenoiserEngine:
    NP = 16  # latent points per sample
    # chunk-major storage (see _buf): off unless __init__ enables it (bare plan builders in tests / tools stay row-major)
    use_cm = False
    use_gx = False
    use_gxs = False
    _cm = frozenset()
    _fm = frozenset()
    _cm_copy = {}

    def __init__(self, hp, state_dict, batch, device, prec="fp32", per_sample_t=True, t_table=0):
        """per_sample_t=True : `forward(x, ts, label)` API, the t-embedding MLP runs every call (one workgroup / sample).
        per_sample_t=False: sampler mode -- the whole batch shares the device-side timestep t_dev[0]; the t-embedding
        path is evaluated ONCE for all t in [0, t_table) into a table that the GEMM epilogues index with t_dev[0]."""
        lib()  # fail loudly if the HIP library is missing
        # a plan may be BUILT on the CPU device (structure / FLOP checks in the CPU tests); it can only RUN on a GPU
        self._plan_state(batch, device, prec)
        self.hp = hp
        self.per_sample_t = per_sample_t
        self.t_table = int(t_table)
        assert per_sample_t or t_table > 0
        self.use_glds = self.knobs.SLIDE_GLDS  # LDS-DMA GEMM variant for fp16 GEMMs
        self.glds_nst = self.knobs.SLIDE_GLDS_WIDE  # 1: 64-deep K chunks (full cache lines)
        self.sd = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float32)
                   for k, v in state_dict.items()}
        arch = hp["architecture"]
        assert not hp.get("include_local_feature", True) and not hp.get("include_global_feature", False)
        assert arch["neighbor_definition"] == "nn" and arch.get("use_knn_FP", False) and not arch.get("include_grouper", False)
        assert hp["attach_position_to_input_feature"] and hp["include_abs_coordinate"] and hp.get("include_center_coordinate", False)
        assert hp["bias"] and hp["res_connect"] and not hp["bn_first"] and hp.get("bn", True)
        assert all(n >= self.NP for n in arch["npoint"]), "engine is specialised to N == npoint == 16 (no FPS)"
        assert all(ns >= self.NP for ns in arch["nsample"]) and arch["K"] == 8
        self.cx = 3 + hp["in_fea_dim"]
        self.out_dim = hp["out_dim"]
        self.t_dim = hp["t_dim"]
        # chunk-major activations / weights for the 128- and 256-row ring kernels (SLIDE_CM=0: row-major everywhere, A/B)
        self.use_cm = (self.prec == 1 and self.use_glds and self.glds_nst != 1 and self.knobs.SLIDE_CM
                       and not self.knobs.SLIDE_XS)
        # pair decomposition of the blocks' first layers + generated-X GEMMs (csrc/gemm_gx.hip; SLIDE_GX=0: the round-2 plan)
        self.use_gx = self.use_cm and self.knobs.SLIDE_GX
        # round 5: the pair decomposition in the SPLIT arithmetic (csrc/gemm_gxs.hip): float pair tables, generated-X split GEMMs,
        # PAIR residuals on float rows, the split attention tail -- the K-expanded first-layer outputs, scores and values of a block
        # never reach memory (SLIDE_GXS=0: the fp32-structured plan of round 4)
        self.use_gxs = self.prec == 2 and self.knobs.SLIDE_GXS
        if self.use_gxs:
            # its kernels run the split products on ONE accumulator set with the weight's high term scaled by 2^11 in fp16 (DESIGN.md
            # section 5): exact while |w| < 32.  A checkpoint with a larger convolution weight takes the fp32-structured split plan.
            wmax = max([float(np.abs(v).max()) for k, v in self.sd.items() if k.endswith(".weight") and v.ndim >= 3 and v.size] + [0.0])
            if wmax >= 31.0:
                import warnings
                warnings.warn("a convolution weight of magnitude %.1f >= 31: the split plan falls back to its fp32-structured form "
                              "(SLIDE_GXS=0 behaviour)" % wmax)
                self.use_gxs = False
        self._cm = set()
        self._fm = set()  # chunk-major buffers whose 32-row groups are fragment-major (_tail_fm)
        self._cm_copy = {}  # per-point table (data_ptr) -> its chunk-major copy, written by the table's producer as well
        self.two_lanes = self.knobs.SLIDE_TWO_LANES  # measured: no gain at batch 256
        self._tvec = []   # (name, width) of every Mlp .fc           -> offsets into the t vector
        self._cvec = []   # (name, width) of every Mlp .fc_condition -> offsets into the condition vector
        self._build()

    def _plan_state(self, batch, device, prec):
        """the state the emitters below read and write while a plan is built; bare builders (one-op tests and tools) call this in
        place of __init__.  Resolves every plan knob from the environment, once, into `self.knobs` (knobs.snapshot): nothing in this
        module reads the environment after that, so the emitters of a bare builder see SLIDE_GX_N64 and the like as they are now.
        Pins the derived attributes `use_glds`, `glds_nst`, `persistent` and `two_lanes` at their defaults, whatever the snapshot
        says: __init__ / _build set them from it (and `use_cm`, `use_gx`, `use_gxs`, `fold_copies`), bare builders assign them."""
        self.knobs = knobs.snapshot()
        self.B, self.device, self.prec = int(batch), device, PREC[prec]
        self.adt = torch.float16 if self.prec == 1 else torch.float32  # activation storage type
        self.A = _Arena(device)
        self.plan, self.flops = [], 0  # the launches (Launch), in order; total FLOPs
        self.per_sample_t = True
        self._lane, self.two_lanes = 0, False
        self.use_glds, self.glds_nst, self.persistent = True, 0, 0

    # ------------------------------------------------------------------ small helpers
    def _w(self, name):
        w = self.sd[name]
        return w.reshape(w.shape[0], -1)

    def _buf(self, rows, ch, dtype=None, cm=False, fm=False):
        """activation matrix [rows][ld].  cm=True (fp16 LDS-DMA plans): CHUNK-MAJOR storage [ld / 32][rows][32] -- the same
        bytes, but the 64-byte piece a ring kernel's DMA lane group fetches for row r + 1 follows the one of row r, so one
        LDS-DMA instruction reads 1 KB of consecutive memory (2.2x the L2 -> LDS rate, tools/lds_fill.hip) and one epilogue
        store instruction writes 2 KB of it.  Only for buffers whose every producer is a GEMM epilogue and every consumer a
        ring-kernel loader / epilogue (pointer + leading dimension per 32-channel block express the layout: ld == 32)."""
        t = self.A.zeros(rows, ru(ch), dtype=self.adt if dtype is None else dtype)
        if cm and self.use_cm:
            self._cm.add(t.data_ptr())
            if fm:
                assert t.dtype == torch.float16 and rows % 32 == 0
                self._fm.add(t.data_ptr())
        return t

    def _is_cm(self, t):
        return t.data_ptr() in self._cm

    def _is_fm(self, t):
        return t.data_ptr() in self._fm

    def _tail_fm(self, mpfx, apfx, npx_log2, n_mo):
        """round 6: are the K-expanded inputs u / mo of this attention block's fused tail stored FRAGMENT-major (SLIDE_F_OUT_FM,
        include/slide_engine.h: a chunk-major slab whose 32-row groups are ordered as the MFMA fragments the register-X tail
        kernel loads -- 1 KB of consecutive memory per wave load)?  Exactly when run_attn_tail (csrc/attn_tail.hip) picks
        attn_tail_rx_kernel for it: fp16 pair-decomposition plan (its generated-X kernels and the SA chain are the producers that
        can store the layout), fused tail, values' chunk count a multiple of 4, none
        of the opt-in tail forms.  SLIDE_FM=0: chunk-major u / mo (A/B)."""
        k = self.knobs
        cout = self.sd[apfx + ".weight_conv.5.weight"].shape[0]
        # mo's producer must be one that stores the layout: the generated-X GEMM of a two-layer Mlp, or the SA chain -- a rest_mlp
        # outside the chain is a ring GEMM over a stored h2 (gemm_ring.hip: its epilogue instantiations do not carry the layout)
        if (mpfx + ".rest_mlp.0.weight") in self.sd and not self._sa_chain_shapes(mpfx, npx_log2):
            return False
        return bool(self.use_cm and self.use_gx and self.prec == 1 and self.use_glds and k.SLIDE_FM
                    and k.SLIDE_ATTN_TAIL and k.SLIDE_TAIL_RX and not k.SLIDE_TAIL8
                    and not k.SLIDE_TAIL_OCC3 and k.SLIDE_TAIL_WIDE is None and k.SLIDE_BODY == "0"
                    and npx_log2 in (7, 8) and (ru(n_mo) // 32) % 4 == 0 and gn_layout(cout).unpermuted)

    def _ldp(self, t):
        """leading dimension as the kernels see it"""
        return 32 if self._is_cm(t) else t.shape[1]

    def _colptr(self, t, col):
        """address of channel `col` of row 0"""
        if self._is_cm(t):
            return t.data_ptr() + t.element_size() * ((col // 32) * t.shape[0] * 32 + col % 32)
        return t.data_ptr() + t.element_size() * col

    @property
    def ops(self):
        """the plan's ops, in order.  Assigning a list of bare ops starts a plan of them (no accounting, no roles)"""
        return [e.op for e in self.plan]

    @ops.setter
    def ops(self, ops):
        self.plan = [Launch(o) for o in ops]

    def _emit(self, op, flops=None, nbytes=None, name=None, role=None, **kw):
        """appends a launch to the plan with its accounting and role (Launch); returns the entry"""
        op.i[10] = self._lane if self.two_lanes else 0
        self.plan.append(Launch(op, flops, nbytes, name, () if role is None else (role,), **kw))
        return self.plan[-1]

    def _sync(self, frm, to):
        if self.two_lanes:
            self.plan.append(Launch(make_op(OP_SYNC, i=(frm, to))))

    def _sched(self):
        """tile counters of one persistent GEMM launch (9 ints, zero; the kernel re-arms them itself)"""
        return self.A.put(np.zeros(16, np.int32))

    def _tvec_off(self, prefix, width):
        off = sum(w for _, w in self._tvec)
        self._tvec.append((prefix, width))
        return off

    def _cvec_off(self, prefix, width):
        off = sum(w for _, w in self._cvec)
        self._cvec.append((prefix, width))
        return off

    def _pack_epi(self, segs, npx, rows=None, npx_log2=None, chain=None, pair_tabs=None, pre_gather=None, bare=False):
        """the SlideEpi descriptors of a layer's segments (_segment), one per 32 physical channels, and their packed vectors, in one
        walk -> (descriptor bytes, [bias | gamma | beta] of every block [n_cob][3][32]).  bare: no weights, no outputs, no bias --
        only what SLIDE_OP_PAIR_NORM reads: mode, flags, GroupNorm layout / parameters, statistics pointers"""
        n_cob = sum(ru(sg["layout"].width) for sg in segs) // 32
        epis, pv = (SlideEpi * n_cob)(), np.zeros((n_cob, 3, 32), np.float32)
        blk = 0
        for sg in segs:
            lay = sg["layout"]
            Opad = ru(lay.width)
            vec = epi_vectors(lay, Opad, None if bare else sg.get("bias"), sg.get("gn"))
            vd = self.A.put(vec[1:] if bare else vec)
            gamma = vd.data_ptr() + 4 * (0 if bare else Opad)
            out = sg["out"]
            coff = sg.get("out_coff", 0)
            flags = sg.get("flags", 0)
            if out is None:  # (the layer's output stays in the chaining kernel's registers)
                assert bare or (chain is not None and len(segs) == 1)
            else:
                assert out.shape[1] >= coff + Opad and coff % (32 if self._is_cm(out) else 8) == 0, (out.shape, coff, Opad)
                assert out.shape[0] == rows, (out.shape, rows)
                if out.dtype == torch.float32 and self.prec == 1:
                    flags |= F_OUT_F32
                else:
                    assert out.dtype == self.adt
                if self._is_fm(out):
                    assert self.prec == 1 and npx_log2 >= 7 and out.dtype == torch.float16
                    flags |= F_OUT_FM
            for j in range(Opad // 32):
                e = epis[blk]
                pv[blk] = vec[:, 32 * j:32 * j + 32]
                e.mode = sg.get("mode", EPI_RAW)
                e.flags = flags
                e.gs = lay.gs
                e.n_norm = int(min(32, max(0, lay.n_norm - 32 * j)))
                e.inv_count = 1.0 / (lay.gs_logical * sg.get("npx", npx))  # (npx: a pair segment's GroupNorm runs over the K-expanded rows)
                e.out_ld = 0 if out is None else self._ldp(out)
                e.bias = None if bare else vd.data_ptr() + 4 * (32 * j)
                e.gamma = gamma + 4 * (32 * j)
                e.beta = gamma + 4 * (Opad + 32 * j)
                e.out = None if out is None else self._colptr(out, coff + 32 * j)
                add = sg["addvec"]
                if add is not None:
                    assert add.off % 4 == 0 and add.bs % 4 == 0 and add.idx_stride % 4 == 0
                    e.addvec = add.vec.data_ptr() + 4 * (add.off + 32 * j)
                    e.addvec_bs = add.bs
                    if add.idx is not None:
                        e.addvec_idx = add.idx.data_ptr()
                        e.addvec_idx_stride = add.idx_stride
                rp = sg["res_pair"]
                if rp is not None:
                    assert rp.ta.dtype == (torch.float16 if self.prec == 1 else torch.float32) and rp.ta.shape == rp.tb.shape
                    assert rp.ta.shape[0] == self.B * 16 and (rp.coff + 32 * j) % 8 == 0 and rp.ta.shape[1] >= rp.coff + Opad
                    e.residual = rp.ta.data_ptr() + rp.ta.element_size() * (rp.coff + 32 * j)
                    e.res_b = rp.tb.data_ptr() + rp.ta.element_size() * (rp.coff + 32 * j)
                    e.res_ld = rp.ta.shape[1]
                    if rp.vv is None:
                        assert npx_log2 == 8
                        e.flags |= F_RES_PAIR
                    else:
                        assert npx_log2 == 7 and pair_tabs is not None
                        e.flags |= F_RES_PAIR_NBR
                        e.res_vd = rp.vv.data_ptr() + 4 * (32 * j)
                        e.res_vw = rp.vv.data_ptr() + 4 * (Opad + 32 * j)
                if sg.get("residual") is not None:
                    r = sg["residual"]
                    assert r.shape[0] == rows and r.shape[1] >= Opad and r.dtype == self.adt
                    e.residual = self._colptr(r, 32 * j)
                    e.res_ld = self._ldp(r)
                pa = sg["pre_add"]
                if pa is not None:
                    # shift < 0: row of the NEIGHBOUR point (K = 2^-shift), through the table passed as pre_gather
                    assert pa.table.shape[0] == self._pre_add_rows(pa, rows, npx_log2), (pa.table.shape, rows, pa.shift)
                    assert (pa.shift >= 0 or pre_gather is not None) and pa.table.shape[1] >= pa.coff + Opad and pa.table.dtype == self.adt
                    assert not self._is_cm(pa.table)
                    e.pre_add = pa.table.data_ptr() + pa.table.element_size() * (pa.coff + 32 * j)
                    e.pre_add_ld = pa.table.shape[1]
                    e.pre_add_shift = pa.shift
                st = sg["stats"]
                if st is not None:
                    e.stats_sum = st.sum.data_ptr() + 4 * (st.coff + 32 * j)
                    e.stats_sq = st.sq.data_ptr() + 4 * (st.coff + 32 * j)
                    e.stats_bs = st.sum.shape[1]
                    e.stats_scale = st.scale
                blk += 1
        assert blk == n_cob
        return np.frombuffer(bytes(epis), dtype=np.uint8), pv

    @staticmethod
    def _pre_add_rows(pa, rows, npx_log2):
        """rows of the per-point table a pre_add reads (unique rows)"""
        return rows >> pa.shift if pa.shift >= 0 else rows >> npx_log2 << 4

    def _epi_only(self, segs, npx):
        """device array of SlideEpi descriptors (one per 32 physical channels) carrying only what SLIDE_OP_PAIR_NORM reads:
        mode, flags, GroupNorm layout / parameters, statistics pointers"""
        return self.A.put(self._pack_epi([_segment(sg) for sg in segs], npx, bare=True)[0].copy())

    def _pack_layer(self, segs, npx_log2, rows, ld, in_cols, w_cm, **epi_kw):
        """weights and epilogue of a layer on the device (_Layer): the segments' weights stacked in their physical channel order,
        input channels at `in_cols`; descriptors and packed vectors in one block"""
        segs = [_segment(sg) for sg in segs]
        widths = [ru(sg["layout"].width) for sg in segs]
        wrows = []
        for sg, Opad in zip(segs, widths):
            w = sg["w"]
            wp = np.zeros((Opad, ld), np.float32)
            wp[np.ix_(sg["layout"].index, np.arange(w.shape[1]) if in_cols is None else in_cols)] = w
            wrows.append(wp)
        W = np.concatenate(wrows, axis=0)
        Wd = self.A.put(chunk_major(W) if w_cm else W, torch.float16 if self.prec == 1 else torch.float32)
        # PACKED VECTORS (SLIDE_EPI_PACKED_VECS, include/slide_engine.h): the blocks' [bias | gamma | beta] values behind the descriptor
        # array, bit 0 of the pointer the ops carry says so -- the kernels stage both by LDS-DMA instead of chasing the three pointers
        # of every block in every workgroup's prologue (SLIDE_PACKED_VECS=0: plain pointer, A/B)
        epis, pv = self._pack_epi(segs, 1 << npx_log2, rows, npx_log2, **epi_kw)
        ed = self.A.put(np.concatenate([epis, pv.reshape(-1).view(np.uint8)]))
        edp = ed.data_ptr() | (1 if self.knobs.SLIDE_PACKED_VECS else 0)
        return _Layer(segs, widths, W, Wd, w_cm, ed, edp, W.shape[0] // 32, ld, rows, 2 * rows * sum(int(sg["w"].size) for sg in segs))

    def _gemm(self, X, npx_log2, segs, in_cols=None, in_affine=None, gather=None, gn_fin=None,
              pre_gather=None, gx=None, pair_tabs=None, pair_fused=None, chain=None):
        """X: input buffer [rows][ld].  segs: list of dicts describing consecutive output segments:
             w (O,I) bias (O) | out (tensor) out_coff | mode flags | gn=(gamma,beta) for NORM | layout (gn_layout) |
             addvec (AddVec) | residual tensor | res_pair (ResPair) | pre_add (PreAdd) | stats (Stats)
           in_cols: physical column index of every logical input channel (None = identity).
           in_affine (InAffine), gather (Gather): X holds the columns that are not gathered.
           gx (GxArgs), pair_fused (PairFused), chain (_chained_layer): the launch's other forms."""
        in_affine, gather, gx = _rec(InAffine, in_affine), _rec(Gather, gather), _rec(GxArgs, gx)
        if gx is not None:  # generated-X GEMM of the pair decomposition (SLIDE_OP_GEMM_GX): X is never stored
            rows, ld = gx.rows, gx.k_pad
            assert X is None and gather is None and gn_fin is None and npx_log2 in (7, 8) and (self.use_cm or self.use_gxs)
        else:
            rows, ld = X.shape
            assert not self._is_cm(X) or (npx_log2 >= 7 and gather is None)
            assert not self._is_fm(X), "fragment-major buffers are read by the register-X attention tail only"
        if gather is not None:
            ld = gather.chunks * 32 + ld
        # chunk-major weights [k / 32][n][32] for the ring kernels of the 128- / 256-row samples (the 16-row launches run the
        # split-K small-launch kernel, which reads row-major weights)
        w_cm = bool(self.use_cm and npx_log2 >= 7) or (gx is not None and self.prec == 1)
        L = self._pack_layer(segs, npx_log2, rows, ld, in_cols, w_cm, chain=chain, pair_tabs=pair_tabs, pre_gather=pre_gather)
        if gx is not None:
            return self._emit_gx(L, gx, npx_log2, in_affine, pair_tabs, chain)
        if pair_fused is not None:
            assert in_affine is None and gather is None and gn_fin is None
            return self._emit_pair_first(L, X, npx_log2, pair_fused)
        return self._emit_plain(L, X, npx_log2, in_affine, gather, gn_fin, pre_gather, pair_tabs)

    def _chained_layer(self, seg, npx_log2, rows, k_pad, pair_tabs=None):
        """a layer CHAINED onto a split generated-X GEMM (csrc/gemm_gxs.hip): packed (_Layer), not launched -- _gemm(chain=) takes it"""
        assert self.use_gxs
        return self._pack_layer([seg], npx_log2, rows, k_pad, None, bool(self.use_cm and npx_log2 >= 7), pair_tabs=pair_tabs)

    def _emit_pair_first(self, L, X, npx_log2, pf):
        """SLIDE_OP_PAIR_FIRST: per-point GEMM + pair-table pass in one launch (_pair_first)"""
        rows, ld, t = L.rows, L.ld, pf.t
        assert npx_log2 == 4 and self.prec == 1 and not L.w_cm
        assert X.dtype == self.adt and not self._is_cm(X)
        self.flops += L.flops
        return self._emit(make_op(OP_PAIR_FIRST, i=(rows, self._ldp(X), ld, L.n_cob, pf.cob0, t.ldy, pf.K),
                                  p=(X.data_ptr(), L.Wd.data_ptr(), L.epi_ptr, self.xyz.data_ptr(), pf.wa.data_ptr(), pf.wb.data_ptr(),
                                     t.ta.data_ptr(), t.tb.data_ptr(), *map(_dp, t.tabs or (None,) * 3), _dp(pf.vv_in), _dp(t.vv))),
                          flops=L.flops, nbytes=(rows * ld * 2 + L.W.size * 2, 2 * rows * t.ldy * 2 + rows * 32 * pf.cob0 * 2),
                          name="pair_first_kernel<%s>" % ("true" if pf.K == 8 else "false"))

    def _emit_plain(self, L, X, npx_log2, in_affine, gather, gn_fin, pre_gather, pair_tabs):
        """SLIDE_OP_GEMM over a stored X (csrc/gemm_ring.hip run_gemm)"""
        rows, ld, n_cob, Wd, w_cm = L.rows, L.ld, L.n_cob, L.Wd, L.w_cm
        sc = None if in_affine is None else in_affine.scale
        assert X.dtype == self.adt
        # wide (128-channel) tiles only when the grid still covers the 256 CUs at least twice
        ntr = (rows + 255) // 256
        cbw = 4 if (self.prec == 1 and n_cob >= 4 and ntr * ((n_cob + 3) // 4) >= self.knobs.SLIDE_CBW4_TILES) else 2
        # narrow launches: 32-channel tiles double the workgroups and halve each wave's epilogue while they still fit one round
        if self.prec == 1 and self.use_glds and sc is None and npx_log2 >= 7 and ntr * n_cob <= self.knobs.SLIDE_CBW1_TILES:
            cbw = 1
        esz = X.element_size()
        rd = rows * ld * esz + L.W.size * esz + sum(rows * n * esz for sg, n in zip(L.segs, L.widths) if sg.get("residual") is not None)
        rd += sum(self._pre_add_rows(sg["pre_add"], rows, npx_log2) * n * esz
                  for sg, n in zip(L.segs, L.widths) if sg["pre_add"] is not None)  # per-point tables (unique rows)
        wr = L.written()
        glds = int(self.use_glds and self.prec == 1 and (sc is None or npx_log2 >= 7))
        # X-stationary kernel (csrc/gemm_xs.hip: a workgroup keeps its input resident in LDS -- for the GATHERED first layers
        # of the SA / FP blocks only the 16-row point table + the coordinate chunk, 24 KB instead of a 144 KB X tile -- and
        # computes several column tiles of a row tile from it, weights through a small LDS-DMA ring; bit-identical to the ring
        # kernels, tests/test_hip_engine.py).  OPT-IN.  Measured at batch 256 (round 2): alone on the GPU
        # the gathered layers gain (SA1 101 -> 85 us, FP1 87 -> 72 us; one feature chain 0.94 -> 0.91 ms/step), but in bench.py's
        # arrangement (three feature sub-batches + the position chain in flight) every variant LOSES to the ring kernels:
        # 252 / 270 / 253 shapes/s ("auto" at <= 3 / 2 / 1 workgroups per CU) vs 286 -- the ring tiles' three small
        # workgroups per CU interleave with the other chains' kernels, these larger-footprint workgroups do not.
        # SLIDE_XS = "" (default: off) | "auto" (gathered layers + plain layers with >= 8 column tiles per workgroup) |
        # "7,8" (every eligible layer of those sample sizes).
        wfrag = None
        xs_mode = self.knobs.SLIDE_XS
        xs_levels = {7, 8} if xs_mode == "auto" else {int(v) for v in xs_mode.split(",") if v}
        xs_lds = ((ld - (gather.chunks * 32 if gather is not None else 0)) // 32) * 16384  # resident X rows (gathered chunks: 1 KB each)
        if (glds and npx_log2 in xs_levels and gn_fin is None and not (gather is not None and sc is not None)
                and xs_lds + 20 * 1024 <= 160 * 1024):
            if xs_mode != "auto" or gather is not None or (npx_log2 == 8 and sc is None and n_cob >= 16 and xs_lds > 96 * 1024):
                wfrag = Wd  # (selects the kernel; it reads the same row-major weights)
                cbw = 4 if n_cob >= 4 and self.knobs.SLIDE_XS_CBW == "4" else 2
        gtab = None if gather is None else self._cm_copy.get(gather.table.data_ptr(), gather.table)  # chunk-major copy: g_ldf == 32
        assert wfrag is None or gtab is None or gtab is gather.table
        gf = (0.0, 0.0, 0.0) if gather is None else (float(gather.chunks), float(32 if gtab is not gather.table else gather.table.shape[1]),
                                                     float({8: 3, 16: 4}[gather.K]))
        knob = self.glds_nst
        assert wfrag is None or not (w_cm or self._is_cm(X))
        if wfrag is not None and self.knobs.SLIDE_XS_OCC:
            knob = 10 + int(self.knobs.SLIDE_XS_OCC)  # cap the workgroups per CU of the X-stationary kernel (A/B timing)
        has_pair = any(sg["res_pair"] is not None for sg in L.segs)  # -> the kernels compiled with the PAIR residual
        # (a per-point layer of a split plan: _merge_pp may fold it into a SLIDE_OP_PP_STAGE launch, from its float weights)
        pp = (self.use_gxs and npx_log2 == 4 and gather is None and gn_fin is None and pre_gather is None and wfrag is None and
              not any(sg["pre_add"] is not None for sg in L.segs))
        nbr, d2, wts = pair_tabs or (None, None, None)  # PAIR_NBR residual: p[9] = neighbour table, p[12] / p[13] = squared distances / weights
        assert pair_tabs is None or (gather is None and pre_gather is None)
        self.flops += L.flops
        return self._emit(make_op(OP_GEMM, i=(rows, self._ldp(X), ld, n_cob, npx_log2, 0 if in_affine is None else in_affine.bs, self.prec, cbw,
                                              glds | (2 if w_cm else 0) | (4 if has_pair else 0), knob),
                                  f=(-1.0 if self.persistent == 2 else self.knobs.SLIDE_STAGGER_US,) + gf,
                                  p=self._affine_ptrs(X.data_ptr(), Wd.data_ptr(), L.epi_ptr, in_affine) + (None, _dp(gn_fin),
                                     self._sched().data_ptr() if self.persistent else None, _dp(gtab),
                                     _dp(gather.nbr if gather is not None else pre_gather if pair_tabs is None else nbr),
                                     _dp(wfrag), None, _dp(d2), _dp(wts))),
                          flops=L.flops, nbytes=(rd, wr), w16=L.W if pp else None)  # nbytes: algorithmic HBM bytes (read, written)

    @staticmethod
    def _affine_ptrs(x, w, epi, in_affine):
        """p[0..4] of the GEMM ops: input, weights, descriptors, the input affine's scale and shift rows"""
        if in_affine is None:
            return (x, w, epi, None, None)
        return (x, w, epi, in_affine.scale.data_ptr() + 4 * in_affine.off, in_affine.shift.data_ptr() + 4 * in_affine.off)

    @staticmethod
    def _split1_ok(*ws):
        """the single-accumulator split kernels (csrc/gemm_gxs.hip) scale the weight's high term by 2^11 in fp16: |w| < 32"""
        return all(float(np.abs(w).max()) < 31.0 for w in ws if w.size)

    def _emit_gx(self, L, gx, npx_log2, in_affine, pair_tabs, chain=None):
        """SLIDE_OP_GEMM_GX (include/slide_engine.h) of the input `gx` (GxArgs); pair_tabs = (neighbour, d2, w tables) of the 8-neighbour
        samples; chain: the layer that consumes this one's output in the same launch (_chained_layer)"""
        rows, ld, n_cob = L.rows, L.ld, L.n_cob
        ta, tb, coff, add, vv = gx.ta, gx.tb, gx.coff, _rec(AddVec, gx.add), gx.vv
        tes = ta.element_size()
        assert ta.dtype == (torch.float16 if self.prec == 1 else torch.float32) and ta.shape == tb.shape and coff % 8 == 0
        assert ta.shape[1] >= coff + ld
        fl, rd, wr = L.flops, 2 * (rows >> npx_log2) * 16 * ld * tes + L.W.size * tes, L.written()
        if chain is not None:  # the chained layer's work rides on this launch
            fl += chain.flops; rd += chain.W.size * 4; wr += chain.written()
        assert (npx_log2 == 7) == (pair_tabs is not None)
        # (the launcher's choice, csrc/gemm_gx.hip: mode-1 layers run 256 x 64 tiles when three workgroups fit a CU's LDS)
        nsamp, nvec = 256 >> npx_log2, (2 if gx.mode else 1) + (2 if npx_log2 == 7 else 0)
        # (LDS of the 64-channel form: ring stages of 8 KB of weights + 4 KB of streamed table images per sample, epilogue
        #  descriptors, per-sample vectors; three stages, else two)
        shm64 = lambda nst: nst * (8192 + 4096 * nsamp) + (2 * 40 + 2 * 96) * 4 + nsamp * nvec * ld * 2 + 16
        knob = self.knobs.SLIDE_GX_N64
        n64, nst = 0, 3
        if knob != "0" and gx.mode == 1 and shm64(3) <= 53 * 1024:
            n64 = 1
        elif knob != "0" and self.knobs.SLIDE_GX_N64W and (
                n_cob <= 2 or ((rows + 255) // 256) * ((n_cob + 3) // 4) <= 256):
            # (n_cob <= 2 -- the position net's 32- / 64-channel layers: a 128-channel tile would be half empty)
            # where the 128-channel grid would leave CUs empty -- the FP blocks at 88 samples: 96 workgroups -- 64-channel tiles at
            # two workgroups per CU, either mode (SLIDE_GX_N64W=0: 128-channel tiles).  Neutral while the staged tables pinned
            # these launches to one workgroup per CU (385.4 vs 386.6); with the tables streamed through the ring 394.3 vs 390.2
            n64 = 2
        if n64 == 0:  # 128-channel tiles: two workgroups per CU (80 KB each)
            shm128 = lambda k_: k_ * (16384 + 4096 * nsamp) + (4 * 40 + 4 * 96) * 4 + nsamp * nvec * ld * 2 + 16
            nst = 3 if shm128(3) <= 80 * 1024 else 2
        name = "gemm_gx_%skernel<%d, %d, %d>" % (("", "n64_", "n64w_")[n64], npx_log2, nst, gx.mode)
        if self.prec == 2:  # split arithmetic on float tables: csrc/gemm_gxs.hip (256 x 64 tiles)
            if not self._split1_ok(L.W):
                raise SlideHipError("a weight of magnitude >= 31 in a generated-X layer: the split pair-decomposition kernels scale the "
                                    "weights' high terms by 2^11 in fp16 -- build this plan with SLIDE_GXS=0")
            n64 = 3
            name = ("gemm_gxs_chain_kernel<%d>" % npx_log2) if chain is not None else \
                "gemm_gxs_kernel<%d, %d>" % (npx_log2, gx.mode)
            assert chain is None or (npx_log2 == 8 and gx.mode == 0 and n_cob <= 2 and chain.ld == n_cob * 32)
        self.flops += fl
        return self._emit(make_op(OP_GEMM_GX,
                                  i=(rows, ta.shape[1], ld, n_cob, npx_log2, 0 if in_affine is None else in_affine.bs, gx.mode,
                                     0 if add is None else add.bs, 0 if add is None else add.idx_stride, 0 if vv is None else 2 * vv.shape[2]),
                                  f=(float(n64),) + ((float(chain.n_cob), float(chain.ld)) if chain is not None else ()),
                                  p=self._affine_ptrs(ta.data_ptr() + tes * coff, L.Wd.data_ptr(), L.epi_ptr, in_affine) +
                                    (tb.data_ptr() + tes * coff,
                                     None if add is None else add.vec.data_ptr() + 4 * add.off,
                                     None if add is None else _dp(add.idx)) + tuple(_dp(t) for t in pair_tabs or (None,) * 3) +
                                    (None if vv is None else vv.data_ptr() + 4 * coff,
                                     None if chain is None else chain.Wd.data_ptr(), None if chain is None else chain.epi_ptr)),
                          flops=fl, nbytes=(rd, wr), name=name)

    # ------------------------------------------------------------------ blocks
    def _conv_gn_relu(self, conv, gn, **kw):
        """segment of a convolution + GroupNorm + ReLU (state-dict prefixes of the two modules); kw: further keys of the segment"""
        sd = self.sd
        return dict(w=self._w(conv + ".weight"), bias=sd[conv + ".bias"], mode=EPI_NORM, flags=F_POST_RELU,
                    layout=gn_layout(sd[conv + ".weight"].shape[0]), gn=(sd[gn + ".weight"], sd[gn + ".bias"]), **kw)

    def _mlp_segments(self, pfx, tvec, out1, res_out):
        """first_mlp + res_connect segments of Mlp_plus_t_emb (pointnet2_modules.py:119-176) sharing one input"""
        sd = self.sd
        c1 = sd[pfx + ".first_mlp.0.weight"].shape[0]
        first = self._conv_gn_relu(pfx + ".first_mlp.0", pfx + ".first_mlp.1.group_norm", out=out1)
        if (pfx + ".fc.weight") in sd:
            first["addvec"] = AddVec(tvec, self._tvec_off(pfx + ".fc", c1), self._t_bs,
                                     None if self.per_sample_t else self.t_dev, self._n_fc)
        assert (pfx + ".res_connect.weight") in sd, "identity res_connect (mlp_spec[0]==mlp_spec[-1]) not planned"
        res = dict(w=self._w(pfx + ".res_connect.weight"), bias=sd[pfx + ".res_connect.bias"], mode=EPI_RAW, out=res_out)
        return first, res

    def _mlp_tail(self, pfx, npx_log2, h1, cvec, r, final_out, final_coff=0, pair=None):
        """second_mlp (+fc_condition) [+ rest_mlp] + residual, writing the module output.
        pair (BlockPair, the block's pair decomposition): h1 and r are not buffers -- the first GEMM generates its input
        from the pair tables (SLIDE_OP_GEMM_GX mode 0) and the residual enters as a PAIR residual"""
        sd = self.sd
        t, rows = (None, h1.shape[0]) if pair is None else (pair.t, pair.t.rows)

        def first_gemm(seg_, **kw):
            if pair is None:
                return self._gemm(h1, npx_log2, [seg_])
            self._gemm(None, npx_log2, [seg_], in_cols=pair.lay1.index, pair_tabs=t.tabs, **kw,
                       gx=GxArgs(t.ta, t.tb, pair.off1, ru(pair.lay1.width), rows, 0, pair.add1, t.vv))

        # the module's last layer writes the output and adds the residual
        last = dict(out=final_out, out_coff=final_coff, **(dict(residual=r) if pair is None else
                                                           dict(res_pair=ResPair(t.ta, t.tb, pair.offr, pair.rvv))))
        c2 = sd[pfx + ".second_mlp.0.weight"].shape[0]
        seg = self._conv_gn_relu(pfx + ".second_mlp.0", pfx + ".second_mlp.1.group_norm")
        if (pfx + ".fc_condition.weight") in sd:
            seg["addvec"] = AddVec(cvec, self._cvec_off(pfx + ".fc_condition", c2), self._c_bs)
        if (pfx + ".rest_mlp.0.weight") not in sd:
            return first_gemm(dict(seg, **last))
        if pair is not None and self._sa_chain(pfx, npx_log2, pair, seg, final_out, final_coff):
            return
        assert gn_layout(c2).unpermuted, "second_mlp width with padded GroupNorm groups"
        seg3 = self._conv_gn_relu(pfx + ".rest_mlp.0", pfx + ".rest_mlp.1.group_norm", **last)
        if (pair is not None and self.use_gxs and npx_log2 == 8 and ru(gn_layout(c2).width) <= 64 and self.knobs.SLIDE_GXS_CHAIN
                and self._split1_ok(seg3["w"])):
            # split plans (round 5): second_mlp -> rest_mlp of an SA block in ONE launch -- h2 stays in the generated-X kernel's
            # accumulators and feeds rest_mlp's contraction from there (csrc/gemm_gxs.hip, CHAIN); needs every channel of h2 in
            # one 64-channel tile.  SLIDE_GXS_CHAIN=0: two launches and an h2 round trip
            return first_gemm(dict(seg, out=None), chain=self._chained_layer(seg3, npx_log2, rows, ru(c2), t.tabs))
        h2 = self._buf(rows, c2, cm=npx_log2 >= 7)
        first_gemm(dict(seg, out=h2))
        self._gemm(h2, npx_log2, [seg3], pair_tabs=None if pair is None else t.tabs)

    def _sa_chain_shapes(self, pfx, npx_log2):
        """does SLIDE_OP_SA_CHAIN cover this Mlp's second_mlp -> rest_mlp (widths, identity GroupNorm layouts, group sizes)?"""
        sd = self.sd
        if (npx_log2 != 8 or not self.knobs.SLIDE_SA_CHAIN or self.prec != 1 or not self.use_gx
                or (pfx + ".rest_mlp.0.weight") not in sd):
            return False
        c1 = sd[pfx + ".first_mlp.0.weight"].shape[0]
        c2 = sd[pfx + ".second_mlp.0.weight"].shape[0]
        c3 = sd[pfx + ".rest_mlp.0.weight"].shape[0]
        l1, l2, l3 = gn_layout(c1), gn_layout(c2), gn_layout(c3)
        return bool(c2 in (128, 256) and c3 % 256 == 0 and c1 % 64 == 0 and l1.identity and l2.identity and l3.identity
                    and l2.gs in (4, 8, 16) and l3.gs in (4, 8, 16))

    def _sa_chain(self, pfx, npx_log2, pair, seg, final_out, final_coff):
        """second_mlp -> rest_mlp of an SA block (pair: its BlockPair) as ONE launch (SLIDE_OP_SA_CHAIN, csrc/sa_chain.hip: h2 stays in
        registers).  Returns False when the shapes are outside what the kernel covers (the two-launch path then runs)."""
        sd, B = self.sd, self.B
        if pair.t.vv is not None or not self._sa_chain_shapes(pfx, npx_log2):
            return False
        w1, w2 = self._w(pfx + ".second_mlp.0.weight"), self._w(pfx + ".rest_mlp.0.weight")
        (c2, c1), c3 = w1.shape, w2.shape[0]
        lay1, l2, l3 = pair.lay1, gn_layout(c2), gn_layout(c3)
        assert lay1.unpermuted and len(lay1.index) == c1 and lay1.width == c1
        if not (self._is_cm(final_out) and final_coff == 0 and final_out.shape[1] == c3):
            return False
        # (the kernel takes every channel where it logically is)
        d = [self.A.put(chunk_major(w1), torch.float16), self.A.put(chunk_major(w2), torch.float16),
             self.A.put(epi_vectors(GnLayout.plain(c2), c2, sd[pfx + ".second_mlp.0.bias"], seg["gn"])),
             self.A.put(epi_vectors(GnLayout.plain(c3), c3, sd[pfx + ".rest_mlp.0.bias"],
                                    (sd[pfx + ".rest_mlp.1.group_norm.weight"], sd[pfx + ".rest_mlp.1.group_norm.bias"])))]
        add0, add1, ta, tb = pair.add1, _rec(AddVec, seg.get("addvec")), pair.t.ta, pair.t.tb
        rows, fl = B * 256, 2 * B * 256 * (w1.size + w2.size)
        self.flops += fl
        self._emit(make_op(OP_SA_CHAIN,
                           i=(B, ta.shape[1], c1, c2, c3, l2.gs, l3.gs, 0 if add0 is None else add0.idx_stride,
                              0 if add0 is None else add0.bs, 0 if add1 is None else add1.bs),
                           f=(1.0 / (l2.gs_logical * 256), 1.0 / (l3.gs_logical * 256), 1.0 if self._is_fm(final_out) else 0.0),
                           p=(ta.data_ptr() + 2 * pair.off1, tb.data_ptr() + 2 * pair.off1,
                              ta.data_ptr() + 2 * pair.offr, tb.data_ptr() + 2 * pair.offr,
                              d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                              *((None, None) if add0 is None else (add0.vec.data_ptr() + 4 * add0.off, _dp(add0.idx))),
                              None if add1 is None else add1.vec.data_ptr() + 4 * add1.off, final_out.data_ptr())),
                   flops=fl, nbytes=(2 * B * 16 * (c1 + c3) * 2 + (w1.size + w2.size) * 2, rows * c3 * 2),
                   name="sa_chain_kernel<%d>" % (c2 // 32))
        return True

    def _attention_query(self, apfx, K):
        """buffers + GEMM segment of an attention block's per-point query branch (feat_conv): it depends on the block's input
        table only, so the query GEMMs of two blocks that read the same table (an SA block and the FP block that takes the
        same features as its skip input) are issued as ONE launch by whichever block comes first"""
        sd, B = self.sd, self.B
        C1p = ru(sd[apfx + ".feat_conv.weight"].shape[0])
        ldT = C1p + ru(sd[apfx + ".grouped_feat_conv.weight"].shape[0])
        Tq = self.A.zeros(B * 16, C1p, dtype=self.adt)
        ssum, ssq = self.A.zeros(B, ldT), self.A.zeros(B, ldT)
        qseg = dict(w=self._w(apfx + ".feat_conv.weight"), bias=sd[apfx + ".feat_conv.bias"], mode=EPI_STATS,
                    flags=F_PRE_RELU, out=Tq, stats=Stats(ssum, ssq, 0, float(K)))
        return Query(Tq, ssum, ssq, qseg)

    def _pair_first(self, npx_log2, K, feat_in, C, segs, coords, fin=None, lead_segs=()):
        """PAIR DECOMPOSITION of a block's shared first layer (csrc/gemm_gx.hip): the 1x1 convolutions over the grouped input
        [neighbour features (C) | coordinate channels] are linear, so their output for row (point p, slot j) is a[q] + b[p]
        (+ d2 vd + w vw), q the slot's neighbour.  Emits the 16-row GEMM y = Wf . feat + bias (1/K of the MACs) and
        SLIDE_OP_PAIR_NORM (tables a, b in fp16 with the GroupNorm of NORM segments folded in, sums of STATS segments);
        the K-expanded outputs are never stored.  segs: the segment dicts of the old shared GEMM (w over all grouped
        channels); coords: dict(rel, abs, ctr = first column of each 3-channel coordinate group, d2 / w = column or None).
        Returns the PairTables the consumers (generated-X GEMMs, PAIR residuals) take."""
        B = self.B
        ysegs = []
        offs, ldy = seg_offsets(segs)
        # SLIDE_PAIR_FUSED (default on): the per-point GEMM and the pair-table pass as ONE launch (SLIDE_OP_PAIR_FIRST,
        # csrc/gemm_ring.hip pair_first_kernel) -- y never goes through memory; bit-identical to the two-launch form
        fused = fin is None and self.prec == 1 and self.use_glds and self.knobs.SLIDE_PAIR_FUSED
        Y = None if fused else self.A.zeros(B * 16, ldy)  # fp32
        wa, wb, vv_in = np.zeros((ldy, 4), np.float32), np.zeros((ldy, 4), np.float32), np.zeros((2, ldy), np.float32)
        psegs = []
        for sg, o_ in zip(segs, offs):
            lay = _rec(GnLayout, sg.get("layout"))
            w = sg["w"]
            oidx = (np.arange(w.shape[0]) if lay is None else lay.index) + o_
            ysegs.append(dict(w=w[:, :C], bias=sg.get("bias"), mode=EPI_RAW, out=Y, out_coff=o_,
                              layout=None if lay is None else lay.raw()))
            rel, ab, ctr = (w[:, coords[k_]:coords[k_] + 3] for k_ in ("rel", "abs", "ctr"))
            wa[oidx, :3] = rel + ab
            wb[oidx, :3] = ctr - rel
            if coords.get("d2") is not None:
                vv_in[0, oidx] = w[:, coords["d2"]]
                vv_in[1, oidx] = w[:, coords["w"]]
            # descriptors only: mode / flags / GroupNorm parameters / statistics
            psegs.append(dict({k_: sg[k_] for k_ in ("mode", "flags", "layout", "gn", "stats") if k_ in sg}, w=w[:, :0], out=None))
        assert sum(3 for _ in ("rel", "abs", "ctr")) + (2 if coords.get("d2") is not None else 0) + C == segs[0]["w"].shape[1]
        tdt = torch.float16 if self.prec == 1 else torch.float32  # (split plans: float tables)
        ta, tb = self.A.zeros(B * 16, ldy, dtype=tdt), self.A.zeros(B * 16, ldy, dtype=tdt)
        fp = K == 8
        wa_d, wb_d = self.A.put(wa), self.A.put(wb)
        tabs = vv_d = vv = None
        if fp:
            tabs, vv_d, vv = (self.kidx, self.kd2, self.kw), self.A.put(vv_in), self.A.zeros(B, 2, ldy)
        t = PairTables(ta, tb, ldy, offs, B * 16 * K, vv, vv_in, tabs)
        if fused:
            fsegs = []
            for sg, o_ in zip(segs, offs):
                fs = dict(sg)
                fs.update(w=sg["w"][:, :C], out=ta, out_coff=o_, npx=1 << npx_log2)
                for k_ in ("addvec", "residual", "res_pair", "pre_add"):
                    assert fs.get(k_) is None or k_ == "addvec"
                fs.pop("addvec", None)  # (first_mlp's t-embedding rows are added by the consumers, after the ReLU)
                fsegs.append(fs)
            self._gemm(feat_in, 4, list(lead_segs) + fsegs, pair_fused=PairFused(seg_offsets(lead_segs)[1] // 32, K, wa_d, wb_d, vv_d, t))
        else:
            # (lead_segs: other per-point GEMM segments over the same table -- the attention queries -- ride on this launch)
            self._gemm(feat_in, 4, list(lead_segs) + ysegs)
            ed = self._epi_only(psegs, 1 << npx_log2)
            # loop-invariant when the coordinates are a fixed condition?  No: y changes every step.
            v2 = ldy <= 2048 and (self.knobs.SLIDE_PAIR_NORM_V2 or self.prec != 1)
            assert (fin is None or v2) and (self.prec == 1 or v2)
            self._emit(make_op(OP_PAIR_NORM, i=(B, ldy, K, 2 if v2 else 1, int(self.prec != 1)),
                               p=(Y.data_ptr(), self.xyz.data_ptr(), wa_d.data_ptr(), wb_d.data_ptr(), ed.data_ptr(), ta.data_ptr(),
                                  tb.data_ptr(), *map(_dp, tabs or (None,) * 3), _dp(vv_d), _dp(vv), _dp(fin))),
                       name="pair_norm2_kernel<%s, %s>" % ("true" if fp else "false", "_Float16" if self.prec == 1 else "float"))
        return t

    def _body_shape(self, mpfx, apfx, npx_log2):
        """(rest, nb1, nbm, nbu) if SLIDE_OP_BLOCK_BODY has an instantiation for this block's widths, else None"""
        sd = self.sd
        # OPT-IN since round 5 (SLIDE_BODY=1, experiments build): with the split position plan beside the feature chains the one-launch
        # body of the FP0-sized blocks LOSES 0.9 % to its three separate launches (378.5 vs 382.0 shapes/s, four alternating pairs) --
        # one workgroup per CU at 0.024 MFMA-busy holds a CU for 31 us where the ring kernels' small workgroups interleave
        if not self.use_gx or self.knobs.SLIDE_BODY == "0":
            return None
        rest = (mpfx + ".rest_mlp.0.weight") in sd
        c1 = sd[mpfx + ".first_mlp.0.weight"].shape[0]
        c2 = sd[mpfx + ".second_mlp.0.weight"].shape[0]
        n_mo = sd[mpfx + ".rest_mlp.0.weight"].shape[0] if rest else c2
        inter = sd[apfx + ".weight_conv.2.weight"].shape[0]
        cout = sd[apfx + ".weight_conv.5.weight"].shape[0]
        lay_u = gn_layout(inter)
        n_u = ru(lay_u.width)
        ident = lambda c: gn_layout(c).identity
        okgs = lambda c: gn_layout(c).gs in (4, 8, 16)
        if not (ident(c1) and ident(c2) and ident(n_mo) and ident(cout) and okgs(c2) and okgs(n_mo) and lay_u.gs in (4, 8, 16)
                and c1 % 32 == 0 and n_mo % 32 == 0 and cout % 64 == 0 and gn_layout(cout).gs <= 32):
            return None
        shape = (npx_log2, rest, (c2 // 32) if rest else 0, n_mo // 32, n_u // 32)
        # ((7, False, 0, 8, 8) -- FP1 -- was built and measured slower than its three separate launches: one wave per SIMD)
        # ((8, True, 4, 8, 5) -- SA0 -- spills under its 256-register budget: opt-in with SLIDE_BODY=2)
        if shape not in (((7, False, 0, 4, 4), (8, True, 4, 8, 5)) if self.knobs.SLIDE_BODY == "2" else ((7, False, 0, 4, 4),)):
            return None
        return shape

    def _emit_block_body(self, st, mpfx, out, cvec):
        """SLIDE_OP_BLOCK_BODY (csrc/block_body.hip): Mlp tail -> mo, keys -> u, attention tail, one workgroup per sample,
        mo / u in registers.  st: the block's AttnState after _attn_scores (end == "body": P, joint GroupNorm rows, pair tables)"""
        sd, B = self.sd, self.B
        ctx, apfx, npx_log2 = st.pair, st.apfx, st.npx_log2
        assert st.end == "body"
        npx, K = 1 << npx_log2, 1 << (npx_log2 - 4)
        rest = (mpfx + ".rest_mlp.0.weight") in sd
        vec3 = lambda n, lay, conv, gn: epi_vectors(lay, n, sd[conv + ".bias"], (sd[gn + ".weight"], sd[gn + ".bias"]))
        a, keep, slots = BodyArgs(), [], []
        put16 = lambda w: (lambda t: (keep.append(t), t)[1])(self.A.put(chunk_major(w), torch.float16))
        putf = lambda v: (lambda t: (keep.append(t), t)[1])(self.A.put(np.ascontiguousarray(v, np.float32)))

        # slot geometry (csrc/block_body.hip): eight-wave form (16 x 16-row samples) 128-row slabs / 64-channel column blocks,
        # four-wave form everything at once: 256-row images, one 32-deep chunk per slot
        srows, trows = (128, 64) if npx_log2 == 8 else (256, 128)

        def slab_slots(Wt, n, k):  # D[channel][row] stage
            cps = 256 // srows
            for r0 in range(0, n, srows):
                for kc in range(0, k // 32, cps):
                    slots.append((Wt.data_ptr() + 2 * ((kc * n + r0) * 32), n * 32, min(srows, n - r0), 0, min(cps, k // 32 - kc)))

        c1 = sd[mpfx + ".first_mlp.0.weight"].shape[0]
        w_sec = self._w(mpfx + ".second_mlp.0.weight")
        c2 = w_sec.shape[0]
        lay2 = gn_layout(c2)
        fl = 0
        if rest:
            W1 = put16(w_sec)
            slab_slots(W1, c2, c1)
            a.vec1 = putf(vec3(c2, lay2, mpfx + ".second_mlp.0", mpfx + ".second_mlp.1.group_norm")).data_ptr()
            a.n1, a.gs1, a.inv1 = c2, lay2.gs, 1.0 / (lay2.gs_logical * npx)
            if (mpfx + ".fc_condition.weight") in sd:
                a.add1 = cvec.data_ptr() + 4 * self._cvec_off(mpfx + ".fc_condition", c2)
                a.add1_bs = self._c_bs
            w_m = self._w(mpfx + ".rest_mlp.0.weight")
            n_mo = w_m.shape[0]
            laym = gn_layout(n_mo)
            Wm = put16(w_m)
            slab_slots(Wm, n_mo, c2)
            a.vecm = putf(vec3(n_mo, laym, mpfx + ".rest_mlp.0", mpfx + ".rest_mlp.1.group_norm")).data_ptr()
            fl += w_sec.size + w_m.size
        else:
            n_mo, laym = c2, lay2
            Wm = put16(w_sec)
            slab_slots(Wm, n_mo, c1)
            a.vecm = putf(vec3(n_mo, laym, mpfx + ".second_mlp.0", mpfx + ".second_mlp.1.group_norm")).data_ptr()
            if (mpfx + ".fc_condition.weight") in sd:
                a.addm = cvec.data_ptr() + 4 * self._cvec_off(mpfx + ".fc_condition", c2)
                a.addm_bs = self._c_bs
            fl += w_sec.size
        a.n_mo, a.gsm, a.invm = n_mo, laym.gs, 1.0 / (laym.gs_logical * npx)
        # keys -> u
        lay_u, C2p = st.lay, st.C2p
        n_u = ru(lay_u.width)
        w2k = self._w(apfx + ".weight_conv.2.weight")[:, st.C1:]
        wk = np.zeros((n_u, C2p), np.float32)
        wk[lay_u.index, :w2k.shape[1]] = w2k
        Wu = put16(wk)
        slab_slots(Wu, n_u, C2p)
        a.vecu = putf(vec3(n_u, lay_u, apfx + ".weight_conv.2", apfx + ".weight_conv.4.group_norm")).data_ptr()
        a.n_u, a.gsu, a.nnu, a.invu = n_u, lay_u.gs, lay_u.n_norm, 1.0 / (lay_u.gs_logical * npx)
        fl += w2k.size
        # tail
        cout = st.cout
        vlay = gn_layout(cout)
        w5 = np.zeros((cout, n_u), np.float32)
        w5[:, lay_u.index] = self._w(apfx + ".weight_conv.5.weight")
        wv = self._w(apfx + ".feat_out_conv.0.weight")
        W5, Wv = put16(w5), put16(wv)
        assert cout % trows == 0 or npx_log2 == 8
        for cbk in range((cout + trows - 1) // trows):
            for Wt, k in ((W5, n_u), (Wv, n_mo)):
                cps = 256 // trows
                for kc in range(0, k // 32, cps):
                    slots.append((Wt.data_ptr() + 2 * ((kc * cout + cbk * trows) * 32), cout * 32, min(trows, cout - cbk * trows), 1,
                                  min(cps, k // 32 - kc)))
        a.vect = putf(self._tail_vectors(apfx, cout)).data_ptr()
        a.n_out, a.gsv, a.nnv, a.invv = cout, vlay.gs, vlay.n_norm, 1.0 / (vlay.gs_logical * npx)
        fl += self._w(apfx + ".weight_conv.5.weight").size + wv.size
        # tables and vectors
        ta, tb, vv = ctx.t.ta, ctx.t.tb, ctx.t.vv
        a.ta, a.tb, a.t_ld = ta.data_ptr(), tb.data_ptr(), ta.shape[1]
        a.off1, a.k1, a.offr, a.offk, a.kk = ctx.off1, c1, ctx.offr, ctx.offk, C2p
        if K == 8:
            a.vv, a.vbs, a.rv = vv.data_ptr(), 2 * vv.shape[2], ctx.rvv.data_ptr()
            a.nbr, a.d2, a.w = self.kidx.data_ptr(), self.kd2.data_ptr(), self.kw.data_ptr()
            assert ctx.rvv.shape[1] == n_mo
        add0 = ctx.add1
        if add0 is not None:
            a.add0, a.add0_idx = add0.vec.data_ptr() + 4 * add0.off, _dp(add0.idx)
            a.add0_bs, a.add0_stride = add0.bs, add0.idx_stride
        a.sc, a.sh, a.aff_bs = st.scale.data_ptr() + 4 * st.C1p, st.shift.data_ptr() + 4 * st.C1p, st.ldT
        a.P, a.p_ld = st.P.data_ptr(), st.P.shape[1]
        assert st.P.shape[1] >= n_u and out.dtype == torch.float16 and not self._is_cm(out)
        a.out, a.out_ld = out.data_ptr(), out.shape[1]
        a.B = B
        sl = (BodySlot * len(slots))()
        for i, (src, cs, nr, kind, nv) in enumerate(slots):
            sl[i].src, sl[i].chunk_stride, sl[i].nrows, sl[i].kind, sl[i].nvalid = src, cs, nr, kind, nv
        sd_ = self.A.put(np.frombuffer(bytes(sl), dtype=np.uint8).copy())
        a.slots, a.n_slots = sd_.data_ptr(), len(slots)
        self.A.keep.append((a, keep))  # the op carries a HOST pointer to the argument block
        rows = B * 16 * K
        self.flops += 2 * rows * fl
        self._tail_of[out.data_ptr()] = self._emit(
            make_op(OP_BLOCK_BODY, i=(npx_log2, int(rest)), p=(ctypes.addressof(a),)), body=a,
            flops=2 * rows * fl, nbytes=(2 * B * 16 * ta.shape[1] * 2, B * 16 * cout * 2),
            name="block_body_kernel<%d, %s, %d, %d, %d>" % (npx_log2, "true" if rest else "false", (c2 // 32) if rest else 0,
                                                            n_mo // 32, n_u // 32))

    def _tail_vectors(self, apfx, n):
        """[scores bias | values bias | values gamma | values beta] of an attention tail, float rows [4][n]"""
        sd = self.sd
        cout = sd[apfx + ".weight_conv.5.weight"].shape[0]
        gam = sd[apfx + ".feat_out_conv.1.group_norm.weight"]
        vec = np.zeros((4, n), np.float32)
        vec[0, :cout] = sd[apfx + ".weight_conv.5.bias"]
        vec[1, :cout] = sd[apfx + ".feat_out_conv.0.bias"]
        vec[2, :gam.shape[0]] = gam
        vec[3, :gam.shape[0]] = sd[apfx + ".feat_out_conv.1.group_norm.bias"]
        return vec

    def _attn_open(self, apfx, npx_log2, q_in, mo, mlp_first, mlp_res, grouped=None, pair=None, qctx=None, extra_q=(), body=False):
        """AttentionModule (attention.py:35-96), first of three phases: the query GEMM, the shared first layer [first_mlp | res_connect |
        grouped_feat_conv] and the two syncs.  q_in: query features [B*16][ld]; grouped = (g, gather) of _grouped_input, or pair =
        (feature table, its channels, coords) for the pair decomposition; mo: the Mlp output buffer (values input), which the caller
        produces between _attn_scores and _attn_finish; body: the block ends in SLIDE_OP_BLOCK_BODY (_body_shape).
        total_feat = [feat_conv(query) broadcast over the K neighbours | grouped_feat_conv(g)] is never materialised:
        the query half is kept per point ([B*16][C1]); its GroupNorm statistics are its per-point sums x K; and
        because weight_conv.2 is linear, its query half is evaluated once per POINT (a 16-row GEMM) and enters the
        per-neighbour GEMM as a pre-activation add -- 1/K of the reference's MACs for that half.
        Returns the AttnState the other two phases take."""
        sd, B = self.sd, self.B
        K, rows = 1 << (npx_log2 - 4), B << npx_log2
        assert (grouped is None) != (pair is None)
        g, gather = grouped or (None, None)
        C1, C2, cout = (sd[apfx + k_].shape[0] for k_ in (".feat_conv.weight", ".grouped_feat_conv.weight", ".weight_conv.5.weight"))
        C1p, C2p = ru(C1), ru(C2)
        ldT = C1p + C2p                      # physical channel space of the (virtual) concatenation
        issued = qctx is not None  # the query GEMM rode on an earlier block's launch (same input table)
        if qctx is None:
            qctx = self._attention_query(apfx, K)
        Tq, ssum, ssq, qsegs = qctx.Tq, qctx.ssum, qctx.ssq, [qctx.qseg] + [e.qseg for e in extra_q]
        Tk = None if pair is not None else self._buf(rows, C2p, cm=True)
        kseg = dict(w=self._w(apfx + ".grouped_feat_conv.weight"), bias=sd[apfx + ".grouped_feat_conv.bias"],
                    mode=EPI_STATS, flags=F_PRE_RELU, out=Tk, stats=Stats(ssum, ssq, C1p, 1.0))
        # GroupNorm over the concatenation [q | k] (weight_conv.1): groups may straddle the two producers
        Ct, G = C1 + C2, min(32, C1 + C2)
        n_norm, gs = Ct - Ct % G, Ct // G
        phys = np.array([c if c < C1 else C1p + (c - C1) for c in range(Ct)], np.int64)
        gid = np.full(ldT, -1, np.int32)
        gam, bet = np.zeros(ldT, np.float32), np.zeros(ldT, np.float32)
        gid[phys[:n_norm]] = np.arange(n_norm) // gs
        gam[phys[:n_norm]] = sd[apfx + ".weight_conv.1.group_norm.weight"]
        bet[phys[:n_norm]] = sd[apfx + ".weight_conv.1.group_norm.bias"]
        gstart = np.array([phys[gq * gs] for gq in range(G)], np.int32)
        gend = np.array([phys[(gq + 1) * gs - 1] + 1 for gq in range(G)], np.int32)
        scale, shift = self.A.zeros(B, ldT), self.A.zeros(B, ldT)
        fin = SlideGnFin(*(t_.data_ptr() for t_ in [ssum, ssq] + [self.A.put(a) for a in (gid, gstart, gend, gam, bet)] + [scale, shift]),
                         inv_count=1.0 / (gs << npx_log2), C=ldT, bs=ldT, G=G)  # (the pointers in the structure's field order)
        # lane 1 (query / score branch) forks here: it only needs the module inputs
        self._sync(0, 1)
        q_rides = pair is not None and not issued and q_in is pair[0] and not self.two_lanes
        if not issued and not q_rides:
            self._lane = 1
            self._gemm(q_in, 4, qsegs)
            self._lane = 0
        pair_fin, bp = False, None
        # shared-input GEMM: [first_mlp | res_connect | grouped_feat_conv]
        if pair is not None:
            feat_tab, Cf, coords = pair
            # the per-sample table pass also finalises the joint GroupNorm (SLIDE_OP_PAIR_NORM version 2)
            # (SLIDE_PAIR_NORM_V2=1, opt-in: one 1024-thread workgroup per sample that also finalises the joint GroupNorm -- 3 %
            #  faster for a single chain, 5 % slower with four chains in flight: sixteen waves must find room on ONE CU)
            pair_fin = ldT <= 2048 and (self.knobs.SLIDE_PAIR_NORM_V2 or self.use_gxs)
            fin_d = self.A.put(np.frombuffer(bytes(fin), dtype=np.uint8).copy()) if pair_fin else None
            t = self._pair_first(npx_log2, K, feat_tab, Cf, [mlp_first, mlp_res, kseg], coords, fin=fin_d, lead_segs=qsegs if q_rides else ())
            offr, rres = t.offs[1], ru(mlp_res["w"].shape[0])
            # (rvv, K == 8: coefficient vectors of the two per-slot scalars for the res_connect channels -- RAW segment: unscaled)
            bp = BlockPair(t, *t.offs, mlp_first["layout"], _rec(AddVec, mlp_first.get("addvec")),
                           self.A.put(np.ascontiguousarray(t.vv_in[:, offr:offr + rres])) if K == 8 else None)
        elif gather is not None and gather.chunks * 32 >= self.knobs.SLIDE_SPLIT_FIRST:
            # (opt-in, SLIDE_SPLIT_FIRST=<min feature channels>: measured neutral to -1.5 % on the feature plan -- the
            # 256-row launch is bound by its epilogue, not by its K loop, and the per-point GEMM is one more launch)
            # The layer is linear in its input and the leading Cf input channels of row (point, neighbour) are the
            # NEIGHBOUR's feature row, the same for every query point: their products are evaluated once per point
            # (a 16-row GEMM over the feature table, 1/K of the MACs) and enter the per-neighbour GEMM -- now over the
            # coordinate channels only -- as a gathered pre-activation term.
            Cf = gather.chunks * 32
            segs = (mlp_first, mlp_res, kseg)
            offs, ldy = seg_offsets(segs)
            Y = self._buf(B * 16, ldy)
            self._gemm(gather.table, 4, [dict(w=sg["w"][:, :Cf], mode=EPI_RAW, out=Y, out_coff=o_,
                                              layout=None if sg.get("layout") is None else sg["layout"].raw())
                                         for sg, o_ in zip(segs, offs)])
            self._gemm(g, npx_log2, [dict(sg, w=sg["w"][:, Cf:], pre_add=PreAdd(Y, 4 - npx_log2, o_)) for sg, o_ in zip(segs, offs)],
                       pre_gather=gather.nbr)
        else:
            self._gemm(g, npx_log2, [mlp_first, mlp_res, kseg], gather=gather)
        self._sync(0, 1)  # the key statistics are ready
        # how the block ends.  "fused": scores GEMM + values GEMM + softmax-weighted sum in one launch -- csrc/attn_tail.hip, or (round 5)
        # the same tail in the split arithmetic on float rows (csrc/attn_tail_split.hip attn_tail_split_kernel; SLIDE_TAIL_SPLIT=0:
        # scores GEMM + values GEMM + combine launch), whose single-accumulator split needs |w| < 32
        fused = gn_layout(cout).unpermuted and (
            (self.prec == 1 and self.use_glds and self.knobs.SLIDE_ATTN_TAIL) or
            (self.use_gxs and self.knobs.SLIDE_TAIL_SPLIT
             and self._split1_ok(self._w(apfx + ".weight_conv.5.weight"), self._w(apfx + ".feat_out_conv.0.weight"))))
        return AttnState(apfx, npx_log2, C1, C1p, C2p, ldT, cout, Tq, Tk, scale, shift, fin, pair_fin, bp, mo,
                         "body" if body else "fused" if fused else "combine")

    def _attn_scores(self, st):
        """second phase, the score lane (lane 1): the joint GroupNorm of [q | k] -- finalised by the pair-table pass, inside the
        per-point query GEMM (its small-launch kernel) or by its own launch --, P, keys -> u, and the scores GEMM unless the tail
        computes them.  Returns the state with P, u, lay (and S) filled in"""
        sd, B, apfx, npx_log2, fin, rows = self.sd, self.B, st.apfx, st.npx_log2, st.fin, self.B << st.npx_log2
        self._lane = 1
        lay = gn_layout(sd[apfx + ".weight_conv.2.weight"].shape[0])
        # (only the small-launch kernel finalises: same grid bound as run_gemm's dispatch)
        fuse_fin = (self.prec == 1 and self.use_glds and self.knobs.SLIDE_FUSE_FIN and
                    ((B * 16 + 63) // 64) * ((ru(lay.width) // 32 + 1) // 2) <= 1024)
        gn_fin = None
        if fuse_fin and not st.pair_fin:  # finalised inside the per-point query GEMM below (its small-launch kernel), one launch less
            gn_fin = self.A.put(np.frombuffer(bytes(fin), dtype=np.uint8).copy())
        elif not st.pair_fin:
            self._emit(make_op(OP_FINALIZE_GN, i=(B, st.ldT, st.ldT), f=(fin.inv_count,),
                               p=(fin.sum, fin.sq, fin.gid, fin.gstart, fin.gend, fin.gamma, fin.beta, fin.scale, fin.shift)))
        w2 = self._w(apfx + ".weight_conv.2.weight")
        aff = lambda off: InAffine(st.scale, st.shift, off, st.ldT)
        # query half, once per point: P = W2[:, :C1] . GN(relu(q))      (no bias, raw)
        P = self.A.zeros(B * 16, ru(lay.width), dtype=self.adt)
        self._gemm(st.Tq, 4, [dict(w=w2[:, :st.C1], mode=EPI_RAW, layout=lay.raw(), out=P)], in_affine=aff(0), gn_fin=gn_fin)
        u = S = None
        if st.end != "body":  # (the block body kernel, SLIDE_OP_BLOCK_BODY, takes it from P)
            # neighbour half: u = GN4(relu(W2[:, C1:] . GN(relu(k)) + bias + P[point]))
            u = self._buf(rows, ru(lay.width), cm=True, fm=self._is_fm(st.mo))
            useg = dict(w=w2[:, st.C1:], bias=sd[apfx + ".weight_conv.2.bias"], mode=EPI_NORM,
                        flags=F_PRE_RELU, layout=lay, out=u, pre_add=PreAdd(P, npx_log2 - 4),
                        gn=(sd[apfx + ".weight_conv.4.group_norm.weight"], sd[apfx + ".weight_conv.4.group_norm.bias"]))
            if st.pair is not None:  # the keys max(a[q] + b[p], 0) * scale + shift are generated from the pair tables
                t = st.pair.t
                self._gemm(None, npx_log2, [useg], in_affine=aff(st.C1p), pair_tabs=t.tabs,
                           gx=GxArgs(t.ta, t.tb, st.pair.offk, st.C2p, rows, 1, vv=t.vv))
            else:
                self._gemm(st.Tk, npx_log2, [useg], in_affine=aff(st.C1p))
        if st.end == "combine":
            S = self._buf(rows, st.cout)
            self._gemm(u, npx_log2, [dict(w=self._w(apfx + ".weight_conv.5.weight"), bias=sd[apfx + ".weight_conv.5.bias"],
                                          mode=EPI_RAW, out=S)], in_cols=lay.index)
        self._lane = 0
        return st._replace(P=P, u=u, lay=lay, S=S)

    def _attn_finish(self, st, out):
        """third phase, after the caller's Mlp tail wrote st.mo: the fused tail, or the values GEMM + join + combine"""
        if st.end == "fused":
            return self._attn_tail(st.apfx, st.npx_log2, st.u, st.lay, st.mo, out)
        assert st.end == "combine"
        return self._attn_combine(st.apfx, st.npx_log2, st.S, st.mo, out)

    def _attn_tail(self, apfx, npx_log2, u, lay, mo, out):
        """the fused end of an AttentionModule as ONE launch (SLIDE_OP_ATTN_TAIL: csrc/attn_tail.hip in fp16, csrc/attn_tail_split.hip in the
        split arithmetic): scores W5 . u + b5 (u: the intermediate layer's output in its PADDED GroupNorm layout `lay`), values
        relu(GN(Wv . mo + bv)), out[point] = sum_k softmax_k(scores) * values.  Returns the launch"""
        cout = self.sd[apfx + ".weight_conv.5.weight"].shape[0]
        rows, npx = self.B * 16 << (npx_log2 - 4), 1 << npx_log2
        vlay = gn_layout(cout)
        Cp = ru(cout)
        w5 = np.zeros((Cp, u.shape[1]), np.float32)
        w5[np.ix_(np.arange(cout), lay.index)] = self._w(apfx + ".weight_conv.5.weight")
        wv_l = self._w(apfx + ".feat_out_conv.0.weight")
        wv = np.zeros((Cp, mo.shape[1]), np.float32)
        wv[:cout, :wv_l.shape[1]] = wv_l
        cmw = chunk_major if self.use_cm else (lambda w: w)
        wdt = torch.float16 if self.prec == 1 else torch.float32  # (split tail: float row-major weights)
        d = [self.A.put(cmw(w5), wdt), self.A.put(cmw(wv), wdt), self.A.put(self._tail_vectors(apfx, Cp))]
        assert out.dtype == self.adt and u.dtype == self.adt and mo.dtype == self.adt and not self._is_cm(out)
        assert self._is_fm(u) == self._is_fm(mo)
        self._sync(1, 0)
        self.flops += 2 * rows * (w5.size + wv.size)
        wide_from = 1000 if self.knobs.SLIDE_TAIL_WIDE is None else int(self.knobs.SLIDE_TAIL_WIDE)  # (channel blocks; unset: no layer)
        out_cm = None
        if self.use_cm and self.knobs.SLIDE_CM_TABLES and npx_log2 == 8:  # (SA outputs feed gathers)
            out_cm = self._cm_copy[out.data_ptr()] = self.A.zeros(out.shape[0], out.shape[1], dtype=self.adt)
        self._tail_of[out.data_ptr()] = self._emit(make_op(OP_ATTN_TAIL, i=(rows, self._ldp(u), u.shape[1], self._ldp(mo), mo.shape[1], Cp // 32, npx_log2,
                                            vlay.gs, vlay.n_norm, out.shape[1]),
                                # f[1]: 1 = chunk-major operands, + 2 = two-stage ring at three workgroups per CU (opt-in,
                                # SLIDE_TAIL_OCC3=1: measured neutral, 373.0 vs 372.3 shapes/s)
                                f=(1.0 / (vlay.gs_logical * npx), (1.0 if self.use_cm else 0.0) + (8.0 if self.prec != 1 else 0.0) +
                                   (2.0 if self.knobs.SLIDE_TAIL_OCC3 else 0.0) +
                                   (4.0 if (Cp // 32) % 4 == 0 and Cp // 32 >= wide_from else 0.0) +
                                   (16.0 if self._is_fm(mo) else 0.0)),  # bit 4: u / mo fragment-major
                                p=(u.data_ptr(), d[0].data_ptr(), mo.data_ptr(), d[1].data_ptr(), out.data_ptr(),
                                   d[2].data_ptr(), _dp(out_cm))),
            flops=2 * rows * cout * (len(lay.index) + wv_l.shape[1]),  # logical channels
            name=None if self.prec == 1 else "attn_tail_split_kernel<%d>" % npx_log2)
        return self._tail_of[out.data_ptr()]

    def _attn_combine(self, apfx, npx_log2, S, mo, out):
        """the three-launch end of an AttentionModule, after the scores GEMM that wrote S: the values GEMM (lane 0), the join, and the
        softmax-weighted sum over a point's K rows (SLIDE_OP_ATTN_COMBINE).  Returns the combine launch"""
        cout = self.sd[apfx + ".weight_conv.5.weight"].shape[0]
        K = 1 << (npx_log2 - 4)
        rows = self.B * 16 * K
        V = self._buf(rows, cout)
        self._gemm(mo, npx_log2, [self._conv_gn_relu(apfx + ".feat_out_conv.0", apfx + ".feat_out_conv.1.group_norm", out=V)])
        assert out.dtype == self.adt
        self._sync(1, 0)
        return self._emit(make_op(OP_ATTN_COMBINE, i=(rows // K, cout, S.shape[1], V.shape[1], out.shape[1], K, self.prec),
                                  p=(S.data_ptr(), V.data_ptr(), out.data_ptr())))

    def _grouped_input(self, kind, feat_in, C, Cg, K):
        """the grouped input of an SA / FP block.  fp16 LDS-DMA path: only the last chunks (left-over feature columns +
        coordinate channels) are assembled; the GEMM gathers the leading 32-column chunks from the neighbours' rows of
        `feat_in` itself (returns (tail buffer, gather tuple)).  Otherwise the whole [rows][Cg] matrix is assembled."""
        B, rows, ldg = self.B, self.B * 16 * K, ru(Cg)
        nsplit = (C // 8) * 8 // 32 if self.prec == 1 and self.use_glds and self.knobs.SLIDE_GATHER else 0
        c_begin = nsplit * 32
        g = self.A.zeros(rows, ldg - c_begin, dtype=self.adt)
        ptrs = (self.xyz.data_ptr(), feat_in.data_ptr(), self.kidx.data_ptr())
        if kind == OP_ASSEMBLE_FP:
            ptrs += (self.kd2.data_ptr(),)
        # only coordinate channels left: loop-invariant when the coordinates are a fixed condition
        self._emit(make_op(kind, i=(B, C, feat_in.shape[1], ldg, K, self.prec, c_begin, ldg - c_begin), p=ptrs + (g.data_ptr(),)),
                   role="xyz_copy" if nsplit and c_begin == C else None)
        return g, (Gather(feat_in, self.kidx, K, nsplit) if nsplit else None)

    def _sa_module(self, i, feat_in, C, extra_q=()):
        sd, B = self.sd, self.B
        pfx = "SA_modules.%d" % i
        mp, ap = pfx + ".mlps.0", pfx + ".attention_modules.0"
        K, rows, Cg = 16, B * 256, C + 9
        c1, c_last = sd[mp + ".first_mlp.0.weight"].shape[0], sd[mp + ".res_connect.weight"].shape[0]
        assert sd[mp + ".first_mlp.0.weight"].shape[1] == Cg
        mo = self._buf(rows, c_last, cm=True, fm=self._tail_fm(mp, ap, 8, c_last))
        out = self._buf(B * 16, c_last)
        pair = grouped = h1 = r = None
        if self.use_gx or self.use_gxs:
            # pair decomposition (csrc/gemm_gx.hip): no grouped input, no h1 / r / key buffers; rows in natural neighbour order
            pair = (feat_in, C, dict(rel=C, abs=C + 3, ctr=C + 6))
        else:
            grouped = self._grouped_input(OP_ASSEMBLE_SA, feat_in, C, Cg, K)
            h1, r = self._buf(rows, c1, cm=True), self._buf(rows, c_last, cm=True)
        first, res = self._mlp_segments(mp, self.tvec, h1, r)
        st = self._attn_open(ap, 8, feat_in, mo, first, res, grouped, pair, extra_q=extra_q, body=self._body_shape(mp, ap, 8) is not None)
        st = self._attn_scores(st)                                     # lane 1: finalize, P, weight_conv.2, weight_conv.5
        if st.end == "body":
            self._emit_block_body(st, mp, out, self.cvec)
        else:
            self._mlp_tail(mp, 8, h1, self.cvec, r, mo, pair=st.pair)  # lane 0: second / rest mlp
            self._attn_finish(st, out)                                 # lane 0: values; join; softmax-combine
        return out, st.cout

    def _fp_module(self, j, U, CU, Kf, C2, out_buf=None, qctx=None):
        """PointnetKnnFPModule.forward (pointnet2_modules.py:771-873).  U: unknown (skip) features, Kf: known features."""
        sd, B = self.sd, self.B
        pfx = "FP_modules.%d" % j
        m1, m2, ap = pfx + ".mlp1", pfx + ".mlp2", pfx + ".attention_module"
        K, rows, Cg = 8, B * 128, C2 + 11
        c1, c_last = sd[m1 + ".first_mlp.0.weight"].shape[0], sd[m1 + ".res_connect.weight"].shape[0]
        assert sd[m1 + ".first_mlp.0.weight"].shape[1] == Cg
        mo = self._buf(rows, c_last, cm=True, fm=self._tail_fm(m1, ap, 7, c_last))
        pair = grouped = h1 = r = None
        if self.use_gx or self.use_gxs:  # pair decomposition: group_knn's channels are [feats | d2 | w | abs | rel | centre]
            pair = (Kf, C2, dict(d2=C2, w=C2 + 1, abs=C2 + 2, rel=C2 + 5, ctr=C2 + 8))
        else:
            grouped = self._grouped_input(OP_ASSEMBLE_FP, Kf, C2, Cg, K)
            h1, r = self._buf(rows, c1, cm=True), self._buf(rows, c_last, cm=True)
        first, res = self._mlp_segments(m1, self.tvec, h1, r)
        # mlp2 input: [interpolated (c_last) | unknown feats (CU) | xyz (3)]  (pointnet2_modules.py:842-855)
        zin = c_last + CU + 3
        assert sd[m2 + ".first_mlp.0.weight"].shape[1] == zin
        Z = self._buf(B * 16, zin)
        st = self._attn_scores(self._attn_open(ap, 7, U, mo, first, res, grouped, pair, qctx=qctx, body=self._body_shape(m1, ap, 7) is not None))
        # skip features and coordinates: columns of Z the attention output does not touch -- on the score lane, beside
        # the value branch (joined by finish)
        es = Z.element_size()
        self._lane = 1
        # skip-feature columns: written by the producer of U itself where it can (the point preparation for the input
        # features, the fused attention tail of the SA block that made U) -- a COPY launch otherwise
        tail = self._tail_of.get(U.data_ptr())  # the launch that wrote U, if it is a fused tail / block body
        if self.fold_copies and U is self.feat0:
            self._prep_copies.append((Z.data_ptr() + es * c_last, Z.shape[1], 0, CU))
        elif self.fold_copies and tail is not None and tail.body is not None:
            ba = tail.body
            ba.out2, ba.out2_ld, ba.out2_n = Z.data_ptr() + es * c_last, Z.shape[1], CU
        elif self.fold_copies and tail is not None:
            t_op = tail.op
            t_op.p[7], t_op.f[2], t_op.f[3] = Z.data_ptr() + es * c_last, float(Z.shape[1]), float(CU)
        else:
            self._emit(make_op(OP_COPY_COLS, i=(B * 16, CU, U.shape[1], Z.shape[1], int(self.prec == 1), int(self.prec == 1)),
                                    p=(U.data_ptr(), Z.data_ptr() + es * c_last)))
        if self.fold_copies:
            self._prep_copies.append((Z.data_ptr() + es * (c_last + CU), Z.shape[1], 1, 3))
        else:
            self._emit(make_op(OP_COPY_COLS, i=(B * 16, 3, 3, Z.shape[1], 0, int(self.prec == 1)),
                               p=(self.xyz.data_ptr(), Z.data_ptr() + es * (c_last + CU))),
                       role="xyz_copy")  # loop-invariant when the coordinates are a fixed condition
        self._lane = 0
        if st.end == "body":
            self._emit_block_body(st, m1, Z, self.cvec)
        else:
            self._mlp_tail(m1, 7, h1, self.cvec, r, mo, pair=st.pair)
            self._attn_finish(st, Z)
        n1, n2 = sd[m2 + ".first_mlp.0.weight"].shape[0], sd[m2 + ".res_connect.weight"].shape[0]
        hz, rz = self._buf(B * 16, n1), self._buf(B * 16, n2)
        f2, r2 = self._mlp_segments(m2, self.tvec, hz, rz)
        i0 = len(self.plan)
        self._gemm(Z, 4, [f2, r2])
        out = out_buf if out_buf is not None else self._buf(B * 16, n2)
        self._mlp_tail(m2, 4, hz, self.cvec, rz, out)
        if out_buf is not None:  # the last FP block: its second Mlp may join the output head in one launch (_point_chain)
            self._chain_front = ChainFront(self.plan[i0:], Z, zin, m2, n1, n2)
        return out, n2

    def _head_arrays(self, k0):
        """the output head fc_lyaer packed on the host for the kernels that run it whole: (W0, W1, b1, v0, n1c) (k0: padded input
        columns), or None when its shapes are outside what they cover.  Every user uploads its own device copies"""
        sd, w0, w1 = self.sd, self._w("fc_lyaer.0.weight"), self._w("fc_lyaer.3.weight")
        lay0, n1c = gn_layout(w0.shape[0]), ru(self.out_dim) // 32
        if not (self.prec == 1 and w0.shape[0] == 128 and lay0.identity and lay0.gs == 4 and k0 <= 160 and w1.shape[1] == 128
                and self.out_dim <= 64 and sd["fc_lyaer.1.weight"].shape[0] == 128):
            return None
        W0 = np.zeros((128, k0), np.float32); W0[:, :w0.shape[1]] = w0
        W1 = np.zeros((n1c * 32, 128), np.float32); W1[:w1.shape[0]] = w1
        b1 = np.zeros(n1c * 32, np.float32); b1[:w1.shape[0]] = sd["fc_lyaer.3.bias"]
        return W0, W1, b1, epi_vectors(lay0, 128, sd["fc_lyaer.0.bias"], (sd["fc_lyaer.1.weight"], sd["fc_lyaer.1.bias"])), n1c

    def _point_chain(self, dec0, head):
        """round 5: the last FP block's second Mlp + the output head as ONE launch (SLIDE_OP_POINT_CHAIN, csrc/point_chain.hip) -- what
        the kernel needs, or None when the shapes are outside what it covers (fp16 plans; every width 128 with identity GroupNorm layout;
        per-timestep t-embedding table).  The samplers swap it in for the four per-point GEMM launches (diffusion.py); the plan itself
        keeps them (forward() of the engine, parity tests of the layers)."""
        sd, fr = self.sd, getattr(self, "_chain_front", None)
        hd = self._head_arrays(dec0.shape[1])  # (arrays of its own: on the CPU device an upload is the array itself)
        if fr is None or hd is None or not self.knobs.SLIDE_POINT_CHAIN:
            return None
        m2, lay = fr.m2, gn_layout(128)
        c2 = sd[m2 + ".second_mlp.0.weight"].shape[0]
        has_t, has_c = (m2 + ".fc.weight") in sd, (m2 + ".fc_condition.weight") in sd
        if not (fr.n1 == 128 and fr.n2 == 128 and c2 == 128 and (m2 + ".rest_mlp.0.weight") not in sd and lay.identity and lay.gs == 4
                and len(fr.launches) == 2 and self.plan[-4:] == fr.launches + head and fr.Z.shape[1] <= 192 and 128 < dec0.shape[1]):
            return None
        A, kz, zin = self.A, fr.Z.shape[1], fr.zin
        Wz = np.zeros((256, kz), np.float32)
        Wz[:128, :zin] = self._w(m2 + ".first_mlp.0.weight")
        Wz[128:, :zin] = self._w(m2 + ".res_connect.weight")
        vz = np.stack([sd[m2 + ".first_mlp.0.bias"], sd[m2 + ".first_mlp.1.group_norm.weight"], sd[m2 + ".first_mlp.1.group_norm.bias"],
                       sd[m2 + ".res_connect.bias"]]).astype(np.float32)
        v2 = epi_vectors(lay, 128, sd[m2 + ".second_mlp.0.bias"], (sd[m2 + ".second_mlp.1.group_norm.weight"],
                                                                   sd[m2 + ".second_mlp.1.group_norm.bias"]))
        (W0, W1, b1, v0, n1c), W2 = hd, self._w(m2 + ".second_mlp.0.weight")
        off = lambda lst, pfx: sum(w for _, w in lst[:[p_ for p_, _ in lst].index(pfx)])
        for role, e in zip(("pc0", "pc1", "pc2", "pc3"), self.plan[-4:]):
            e.roles.add(role)
        d = dict(Z=fr.Z, kz=kz, X=dec0, k0=dec0.shape[1], n1c=n1c,
                 Wz=A.put(Wz, torch.float16), W2=A.put(W2, torch.float16),
                 W0=A.put(W0, torch.float16), W1=A.put(W1, torch.float16), vz=A.put(vz), v2=A.put(v2), v0=A.put(v0), b1=A.put(b1),
                 t_off=off(self._tvec, m2 + ".fc") if has_t else None,
                 c_off=off(self._cvec, m2 + ".fc_condition") if has_c else None)
        # round 6: the chain in the SPLIT arithmetic -- low fragments lo' = fp16((w - fp16(w)) 2^11) of the four
        # weight matrices.  These layers are the end of the network: their operand rounding reaches the prediction unattenuated
        # (tools/prec_select_feat.py), at 0.3 % of the FLOPs.  SLIDE_POINT_CHAIN_WIDE=0: fp16 operands as in round 5.
        if self.knobs.SLIDE_POINT_CHAIN_WIDE:
            def lo(w):
                w = np.asarray(w, np.float32)
                return ((w - w.astype(np.float16).astype(np.float32)) * np.float32(2048.0)).astype(np.float32)
            los = [lo(w) for w in (Wz, W2, W0, W1)]
            d.update(Wz_lo=A.put(los[0], torch.float16), W2_lo=A.put(los[1], torch.float16), W0_lo=A.put(los[2], torch.float16),
                     W1_lo=A.put(los[3], torch.float16))
        else:
            los = None
        # the same fp16 values once more as ONE buffer of MFMA fragments in the order the kernel consumes them (chain_pack.py): the
        # launch then reads 1 KB of consecutive memory per load instruction.  The weights are fixed for the life of the engine, so
        # this is plan-time work.  SLIDE_POINT_CHAIN_PACKED=0: the row-major launch (A/B).
        if self.knobs.SLIDE_POINT_CHAIN_PACKED:
            d["Wpk"] = A.put(chain_pack.pack(Wz, W2, W0, W1, los))
        return d

    def point_chain_args(self, eps_out=None):
        """SlidePointChainArgs of this plan's point chain (None when the plan has none): the caller keeps the returned block alive and
        puts its address into a SLIDE_OP_POINT_CHAIN op in place of the four launches `self.point_chain["idx"]`."""
        pch = getattr(self, "point_chain", None)
        if pch is None:
            return None
        c = SlidePointChainArgs()
        packed = "Wpk" in pch  # (then Wz is the packed buffer and the other seven weight pointers stay NULL)
        for k_ in ("Z", "vz", "v2", "v0", "b1", "X") + (() if packed else ("Wz", "W2", "W0", "W1", "Wz_lo", "W2_lo", "W0_lo", "W1_lo")):
            if k_ in pch:
                setattr(c, k_, pch[k_].data_ptr())
        if packed:
            c.Wz, c.wpk_bytes = pch["Wpk"].data_ptr(), pch["Wpk"].numel() * 2
        c.eps = (eps_out if eps_out is not None else self.eps_pad).data_ptr()
        c.rows, c.z_ld, c.kz, c.x_ld, c.k0, c.n1c = self.B * 16, pch["Z"].shape[1], pch["kz"], pch["X"].shape[1], pch["k0"], pch["n1c"]
        c.eps_ld = self.eps_pad.shape[1]
        if pch["t_off"] is not None:
            c.tvec = self.tvec.data_ptr() + 4 * pch["t_off"]
            if self.per_sample_t:  # forward(): every sample's own t-embedding row
                c.t_idx, c.t_stride, c.t_bs = None, 0, self._t_bs
            else:                  # samplers: row t of the per-timestep table (the engine's t_dev[0])
                c.t_idx, c.t_stride, c.t_bs = self.t_dev.data_ptr(), self._n_fc, 0
        if pch["c_off"] is not None:
            c.cvec, c.c_bs = self.cvec.data_ptr() + 4 * pch["c_off"], self._c_bs
        return c

    # ------------------------------------------------------------------ whole network
    def _build(self):
        hp, sd, B, A = self.hp, self.sd, self.B, self.A
        arch = hp["architecture"]
        self.persistent = self.knobs.SLIDE_PERSISTENT  # 1: tile counter per XCD, 2: static tile lists
        # persistent I/O + per-step state
        self.x = A.zeros(B, 16, self.cx)
        self.ts = A.zeros(B)
        self.label = A.zeros(B, dtype=torch.int64)
        self.t_dev = A.zeros(8, dtype=torch.int32)  # [t, step counter, blocks-done counter of the update kernel, chain nonce, global index of the chain's first sample, -, -, -]
        self.xyz = A.zeros(B * 16, 3)
        C0 = self.cx  # in_fea_dim + 3 (position attached as feature)
        self.feat0 = self._buf(B * 16, C0)  # activation storage type
        self.kidx = A.zeros(B * 16, 16, dtype=torch.int32)
        self.kd2 = A.zeros(B * 16, 16)
        self.kw = A.zeros(B * 16, 16)  # group_knn's interpolation weights of the 8 nearest (pair decomposition)
        # t / condition vectors: widths are only known after the walk, so allocate generously and fix up below
        n_fc = sum(v.shape[0] for k, v in sd.items() if k.endswith(".fc.weight"))
        n_fcc = sum(v.shape[0] for k, v in sd.items() if k.endswith(".fc_condition.weight"))
        self._n_fc = n_fc
        self._t_bs = n_fc if self.per_sample_t else 0
        self._c_bs = n_fcc
        self.tvec = A.zeros(B if self.per_sample_t else self.t_table, n_fc)
        self.cvec = A.zeros(B, n_fcc)
        temb_slot = None
        if self.per_sample_t:
            temb_slot = Launch(None)  # TEMB placeholder (needs the .fc order of the walk)
            self.plan.append(temb_slot)
        # (opt-in, SLIDE_CM_TABLES=1: chunk-major second copies of the per-point tables the first layers gather from, written
        # by prep_points / the attention tails -- measured neutral, 298-301 shapes/s either way: the gathers hit the vector cache)
        feat0_cm = None
        if self.use_cm and self.knobs.SLIDE_CM_TABLES:
            feat0_cm = self._cm_copy[self.feat0.data_ptr()] = self._buf(B * 16, C0)
        # COPY launches folded into the producers of their sources (SLIDE_FOLD_COPIES=0: separate launches)
        self.fold_copies = self.knobs.SLIDE_FOLD_COPIES
        self._prep_copies, self._tail_of = [], {}  # _tail_of: output table (data_ptr) -> the fused tail / block body that writes it
        prep = self._emit(make_op(OP_PREP_POINTS, i=(B, self.cx, self.feat0.shape[1], self.prec),
                                  p=(self.x.data_ptr(), self.xyz.data_ptr(), self.feat0.data_ptr(), self.kidx.data_ptr(),
                                     self.kd2.data_ptr(), _dp(feat0_cm), None, self.kw.data_ptr())), role="prep").op
        feats, chans = [self.feat0], [C0]
        nsa, nfp = len(arch["npoint"]), len(arch["decoder_feature_dim"]) - 1
        # FP block j takes feats[nsa + j - nfp] as its skip / query input -- the table SA block nsa + j - nfp reads as well:
        # its query GEMM rides on that SA block's (SLIDE_MERGE_Q=0: one launch each)
        fp_q = {}
        for i in range(nsa):
            j = i + nfp - nsa
            extra = ()
            if 0 <= j < nfp and self.knobs.SLIDE_MERGE_Q:
                fp_q[j] = self._attention_query("FP_modules.%d.attention_module" % j, 8)
                extra = (fp_q[j],)
            o, c = self._sa_module(i, feats[i], chans[i], extra_q=extra)
            feats.append(o); chans.append(c)
        # per-level per-point outputs [B*16][ld] (diagnostics: tools/prec_probe.py compares them between precisions)
        self.levels = {"sa%d" % i: (feats[i + 1], chans[i + 1]) for i in range(nsa)}
        dec0 = None
        for i in range(-1, -(nfp + 1), -1):
            j = nfp + i
            out_buf = None
            if j == 0:  # the last FP module writes straight into the head's input [features | xyz]
                n2 = sd["FP_modules.0.mlp2.res_connect.weight"].shape[0]
                dec0 = self._buf(B * 16, n2 + 3)
                out_buf = dec0
            o, c = self._fp_module(j, feats[i - 1], chans[i - 1], feats[i], chans[i], out_buf, qctx=fp_q.get(j))
            feats[i - 1], chans[i - 1] = o, c
            self.levels["fp%d" % j] = (o, c)
        # output head fc_lyaer (pointnet2_with_pcld_condition.py:480-483): conv -> GN(32,128) -> ReLU -> conv
        c = chans[0]
        if self.fold_copies:
            self._prep_copies.append((dec0.data_ptr() + dec0.element_size() * c, dec0.shape[1], 1, 3))
        else:
            self._emit(make_op(OP_COPY_COLS, i=(B * 16, 3, 3, dec0.shape[1], 0, int(self.prec == 1)),
                               p=(self.xyz.data_ptr(), dec0.data_ptr() + dec0.element_size() * c)), role="xyz_copy")
        hh = self._buf(B * 16, sd["fc_lyaer.0.weight"].shape[0])
        assert sd["fc_lyaer.0.weight"].shape[1] == c + 3
        head = [None, None]
        head[0] = self._gemm(dec0, 4, [self._conv_gn_relu("fc_lyaer.0", "fc_lyaer.1", out=hh)])
        self.eps_pad = self._buf(B * 16, self.out_dim, dtype=torch.float32)
        head[1] = self._gemm(hh, 4, [dict(w=self._w("fc_lyaer.3.weight"), bias=sd["fc_lyaer.3.bias"], mode=EPI_RAW, out=self.eps_pad)])
        # what SLIDE_OP_HEAD_UPDATE needs (the samplers replace the two head GEMMs + their update launch by it, diffusion.py)
        self.head, hd = None, self._head_arrays(dec0.shape[1])
        if hd is not None:
            W0, W1, b1, v0, n1c = hd
            head[0].roles.add("head0"); head[1].roles.add("head1")
            self.head = dict(X=dec0, k0=dec0.shape[1], n1c=n1c, W0=A.put(W0, torch.float16), W1=A.put(W1, torch.float16), v0=A.put(v0), b1=A.put(b1))
        self.point_chain = self._point_chain(dec0, head)
        self.eps = A.zeros(B, 16, self.out_dim)
        self._emit(make_op(OP_COPY_COLS, i=(B * 16, self.out_dim, self.eps_pad.shape[1], self.out_dim, 0, 0),
                           p=(self.eps_pad.data_ptr(), self.eps.data_ptr())), role="eps_copy")  # samplers read eps_pad and drop this op
        # t-embedding MLP + all .fc layers, class embedding + all .fc_condition layers (input-major weights)
        assert sum(w for _, w in self._tvec) == n_fc and sum(w for _, w in self._cvec) == n_fcc
        half = self.t_dim // 2
        cfreq = np.float32(np.log(10000) / (half - 1))
        freq = np.exp(np.arange(half, dtype=np.float32) * -cfreq).astype(np.float32)
        wfc = np.concatenate([sd[p + ".weight"] for p, _ in self._tvec], axis=0)      # (n_fc, 4*t_dim)
        bfc = np.concatenate([sd[p + ".bias"] for p, _ in self._tvec], axis=0)
        d = [A.put(a) for a in (sd["fc_t1.weight"].T, sd["fc_t1.bias"], sd["fc_t2.weight"].T, sd["fc_t2.bias"], wfc.T,
                                bfc, freq)]
        if self.per_sample_t:
            ts_src, nsamp = self.ts, B
        else:  # one-off table over every timestep (run once by `prepare()`), indexed by t_dev[0] in the epilogues
            ts_src, nsamp = A.put(np.arange(self.t_table, dtype=np.float32)), self.t_table
        temb = make_op(OP_TEMB, i=(nsamp, self.t_dim, n_fc),
                       p=(ts_src.data_ptr(), self.t_dev.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                          d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), self.tvec.data_ptr(), d[6].data_ptr()))
        self.table_ops = None
        if self.per_sample_t:
            temb_slot.op = temb
        else:
            self.table_ops = (SlideOp * 1)(temb)
        wc = np.concatenate([sd[p + ".weight"] for p, _ in self._cvec], axis=0)
        bc = np.concatenate([sd[p + ".bias"] for p, _ in self._cvec], axis=0)
        dc = [A.put(a) for a in (sd["class_emb.weight"], wc.T, bc)]
        self.cond_op = make_op(OP_COND, i=(B, sd["class_emb.weight"].shape[1], n_fcc),
                               p=(self.label.data_ptr(), dc[0].data_ptr(), dc[1].data_ptr(), dc[2].data_ptr(),
                                  self.cvec.data_ptr()))
        if self._prep_copies:
            tab = (SlidePrepCopy * len(self._prep_copies))()
            for q, (dst, ld_, kind, n_) in enumerate(self._prep_copies):
                tab[q].dst, tab[q].ld, tab[q].kind, tab[q].n = dst, ld_, kind, n_
            self._prep_tab = A.put(np.frombuffer(bytes(tab), dtype=np.uint8).copy())
            prep.p[6], prep.i[4] = self._prep_tab.data_ptr(), len(self._prep_copies)
        # (the host blocks the merged ops point to are kept alive here)
        self._chain_keep, self._dual_keep, self._chain_p_keep, self._pp_keep = [], [], [], []
        for merge in (self._merge_chains, self._merge_gx_pairs, self._merge_chain_query, self._merge_pp):
            self.plan = rewrite(self.plan, merge())
        self._derive_tables()
        # forward() runs the point chain too (round 6): what the samplers' step plans launch is what the golden forwards measure
        self.layer_ops = list(self.ops)  # (the four per-point GEMMs as launches of their own: parity tests of the layers)
        ops = self.layer_ops
        self._fwd_chain_args = self.point_chain_args()
        if self._fwd_chain_args is not None and all(self.ops[i].kind == OP_GEMM for i in self.point_chain["idx"]):
            idx = self.point_chain["idx"]
            ops = [o if i != idx[0] else make_op(OP_POINT_CHAIN, p=(ctypes.addressof(self._fwd_chain_args),))
                   for i, o in enumerate(self.ops) if i not in idx[1:]]
        self.step_ops = (SlideOp * len(ops))(*ops)
        self.cond_ops = (SlideOp * 1)(self.cond_op)

    def _derive_tables(self):
        """the finished plan as the rest of the code reads it, by position (plan_tables)"""
        t = plan_tables(self.plan)
        for k_ in ("gemm_flops", "gemm_bytes", "kernel_names", "xyz_copy_idx", "eps_copy_idx"):
            setattr(self, k_, t[k_])
        self._prep_idx = t["prep_idx"]
        for e in self.plan:
            e.w16 = None
        for k_ in ("head", "point_chain"):  # (None where a merge pass took their launches)
            if getattr(self, k_) is not None:
                setattr(self, k_, None if t[k_] is None else dict(getattr(self, k_), idx=t[k_]))

    # ------------------------------------------------------------------ merge passes: matchers for `rewrite`, in the order _build runs them
    @staticmethod
    def _host_op(kind, i, block, keep, lane=0):
        """an op whose p[0] is a HOST block (ctypes array or int64 record), which `keep` holds alive"""
        keep.append(block)
        op = make_op(kind, i=i, p=(block.ctypes.data if isinstance(block, np.ndarray) else ctypes.addressof(block),))
        op.i[10] = lane
        return op

    def _merge_chains(self):
        """runs of consecutive per-point GEMM launches (16 rows per sample, fp16, plain input) become ONE SLIDE_OP_GEMM_CHAIN
        launch each (csrc/gemm_chain.hip): the FP blocks' second Mlp_plus_t_emb, the output head.  SLIDE_GEMM_CHAIN=0 keeps the
        launches apart."""
        # SLIDE_GEMM_CHAIN = largest chain in KB of weights (default 0: none).  OPT-IN -- measured in bench.py's arrangement (three
        # feature sub-batches + the position chain): 92 launches per step instead of 108, but 366 shapes/s with every chain
        # merged and 371 with the chains of <= 256 KB of weights against 374 without: a chain's 20-odd workgroups each stream
        # ALL its weights (660 KB for the feature net's FP1.mlp2) and pay every layer's descriptor -> operands -> epilogue ->
        # store round trips in sequence, where the wide-grid launches of the other chains fill the same CUs meanwhile
        max_kb = self.knobs.SLIDE_GEMM_CHAIN
        if self.prec != 1 or not self.use_glds or max_kb <= 0:
            return lambda plan, i: None

        def eligible(o):
            return (o.kind == OP_GEMM and o.i[4] == 4 and o.i[6] == 1 and o.i[8] == 1 and o.i[9] != 3
                    and not any(o.p[k] for k in (3, 4, 6, 7, 8, 9, 10, 11, 12, 13)) and o.i[2] <= 1024)

        def match(plan, i):
            o0, j = plan[i].op, i
            while j < len(plan) and j - i < 6 and eligible(plan[j].op) and plan[j].op.i[0] == o0.i[0] and plan[j].op.i[10] == o0.i[10]:
                j += 1
            while j - i >= 2 and sum(e.op.i[2] * e.op.i[3] * 64 for e in plan[i:j]) > max_kb * 1024:
                j -= 1  # (drop layers from the end until the chain's weights fit)
            if j - i < 2:
                return None
            tab = (SlideChainLayer * (j - i))()
            for q, e in enumerate(plan[i:j]):
                o = e.op
                tab[q].X, tab[q].W, tab[q].epi = o.p[0], o.p[1], o.p[2] & ~1  # (strip SLIDE_EPI_PACKED_VECS: this kernel reads the descriptors' pointers)
                tab[q].x_ld, tab[q].k_pad, tab[q].n_cob = o.i[1], o.i[2], o.i[3]
            return j - i, [(self._host_op(OP_GEMM_CHAIN, (o0.i[0], j - i), tab, self._chain_keep, o0.i[10]), "gemm_chain_kernel", plan[i:j])]
        return match

    def _merge_gx_pairs(self):
        """the mode-1 (keys -> u) and mode-0 (first Mlp layer) generated-X GEMMs of an FP block are independent and adjacent in
        the plan: where both run 64-channel tiles at two workgroups per CU they become ONE SLIDE_OP_GEMM_GX_DUAL launch
        (SLIDE_GX_DUAL=0: two launches)."""
        if not self.knobs.SLIDE_GX_DUAL:
            return lambda plan, i: None

        def match(plan, i):
            if i + 1 >= len(plan):
                return None
            a_, b_ = plan[i].op, plan[i + 1].op
            if not (a_.kind == OP_GEMM_GX and b_.kind == OP_GEMM_GX and a_.i[6] == 1 and b_.i[6] == 0
                    and ((a_.f[0] in (1.0, 2.0) and b_.f[0] == 2.0) or (a_.f[0] == 3.0 and b_.f[0] == 3.0))
                    and a_.i[0] == b_.i[0] and a_.i[4] == b_.i[4] and a_.i[10] == b_.i[10]):
                return None
            pair = (SlideOp * 2)(SlideOp.from_buffer_copy(bytes(a_)), SlideOp.from_buffer_copy(bytes(b_)))
            return 2, [(self._host_op(OP_GEMM_GX_DUAL, (a_.i[0],), pair, self._dual_keep, a_.i[10]),
                        ("gemm_gxs_dual_kernel<%d>" if a_.f[0] == 3.0 else "gemm_gx_dual_kernel<%d>") % a_.i[4], plan[i:i + 2])]
        return match

    def _merge_chain_query(self):
        """SA blocks: [per-point query GEMM P | keys -> u GEMM (needs P) | fused Mlp chain (needs neither)] becomes
        [chain + query GEMM in ONE launch (SLIDE_OP_SA_CHAIN_P) | keys -> u GEMM]: the query GEMM's launch and gap disappear under
        the chain (SLIDE_CHAIN_P=0: three launches)."""
        if not self.knobs.SLIDE_CHAIN_P:
            return lambda plan, i: None
        is_p = lambda o: (o.kind == OP_GEMM and o.i[4] == 4 and o.i[6] == 1 and not (o.i[8] & 6) and o.i[9] != 3 and o.p[3] and o.p[6]
                          and not any(o.p[k] for k in (8, 9, 10, 11, 12, 13)))

        def match(plan, i):
            if i + 2 >= len(plan):
                return None
            o0, o1, o2 = (e.op for e in plan[i:i + 3])
            if not (is_p(o0) and o1.kind == OP_GEMM_GX and o1.i[6] == 1 and o2.kind == OP_SA_CHAIN
                    and o0.i[0] == o2.i[0] * 16 and o0.i[10] == o1.i[10] == o2.i[10]):
                return None
            pair = (SlideOp * 2)(SlideOp.from_buffer_copy(bytes(o2)), SlideOp.from_buffer_copy(bytes(o0)))
            return 3, [(self._host_op(OP_SA_CHAIN_P, (o2.i[0],), pair, self._chain_p_keep, o0.i[10]),
                        "sa_chain_p_kernel<%d>" % (o2.i[3] // 32), [plan[i], plan[i + 2]]), plan[i + 1]]
        return match

    def _merge_pp(self):
        """split plans (round 5): runs of consecutive per-point launches -- 16-row SLIDE_OP_GEMM in the split arithmetic and the float
        pair-table pass -- become ONE SLIDE_OP_PP_STAGE launch each (csrc/experiments/pp_stage.hip: one workgroup per sample walks the steps, the
        dense layers as exact fp32 FMA chains; 30 -> 17 launches per position step).  SLIDE_PP=0 keeps the launches apart."""
        # OPT-IN (SLIDE_PP=1): measured SLOWER -- one workgroup per sample re-reads every layer's weights per sample and its K loop is a
        # chain of dependent L2 round trips on four waves: 55 - 131 us per stage launch against 27 - 45 us for the launches it replaces
        # (position chain alone 365 -> 652 us per step, bench 379 -> 227 shapes/s)
        if not self.use_gxs or not self.knobs.SLIDE_PP:
            return lambda plan, i: None
        B = self.B

        def step_kind(e):  # 0: dense layer, 1: pair-table pass, None: not a step
            o = e.op
            if o.kind == OP_GEMM and e.w16 is not None and o.i[0] == B * 16 and o.i[2] <= 192 and not o.i[10]:
                return 0
            if o.kind == OP_PAIR_NORM and o.i[3] == 2 and o.i[4] == 1 and o.i[0] == B and not o.i[10]:
                return 1
            return None

        def step(e):
            o = e.op
            if step_kind(e) == 1:
                return [1] + [o.p[k] or 0 for k in range(13)] + [o.i[1], o.i[2]]
            wt = self.A.put(np.ascontiguousarray(e.w16.T), torch.float32)  # K-major [k_pad][n_cob*32] (only for layers that are merged)
            return [0, o.p[0], wt.data_ptr(), o.p[2] & ~1, o.p[3] or 0, o.p[4] or 0, o.i[1], o.i[2], o.i[3], o.i[5]] + [0] * 6

        def match(plan, i):
            kinds, j = [], i
            while j < len(plan) and len(kinds) < 8 and step_kind(plan[j]) is not None and (step_kind(plan[j]) == 0 or sum(kinds) < 2):
                kinds.append(step_kind(plan[j]))
                j += 1
            if j - i < 2:
                return None
            rec = np.array([j - i, B] + [v for e in plan[i:j] for v in step(e)], np.int64)
            return j - i, [(self._host_op(OP_PP_STAGE, (B, j - i), rec, self._pp_keep), "pp_stage_kernel", plan[i:j])]
        return match

    # ------------------------------------------------------------------ execution
    def run(self, ops_array, n=None):
        if self.x.device.type != "cuda":
            raise SlideHipError("DenoiserEngine plans only run on a GPU; there is no CPU fallback")
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.x.device)
        check(lib().slide_run_ops2(ops_array, len(ops_array) if n is None else n, stream_of(),
                                   self._side.cuda_stream), "slide_run_ops2")

    def prepare(self):
        """sampler mode: fill the per-timestep t-embedding table (once)"""
        if self.table_ops is not None:
            self.run(self.table_ops)
            self.table_ops = None

    def set_label(self, label):
        self.label.copy_(torch.as_tensor(label).to(self.device, torch.int64).reshape(self.B))
        self.run(self.cond_ops)

    def forward(self, x, ts, label):
        """PointNet2CloudCondition.forward(pointcloud=x, ts=ts, label=label) -> (B,16,out_dim)."""
        assert self.per_sample_t, "engine was built for a shared device-side timestep"
        self.x.copy_(torch.as_tensor(x).to(self.device, torch.float32).reshape(self.x.shape))
        self.ts.copy_(torch.as_tensor(ts).to(self.device, torch.float32).reshape(self.B))
        self.set_label(label)
        self.run(self.step_ops)
        return self.eps.clone()
