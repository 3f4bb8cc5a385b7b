"""Differentiable row-major layers: forward = the module path's HIP kernels, backward = csrc/train_ops.hip + the forward GEMM on the
transposed weights.  Activations are fp32 CUDA tensors [rows, ld], ld a multiple of 32, pad columns ZERO (every Function keeps
them zero).  The GEMMs run in the split mode (fp32 storage, contractions as two-term fp16 operand splits: fp32-grade results on
the fp16 matrix pipe, include/slide_engine.h SLIDE_PREC_SPLIT)."""
import ctypes
import weakref

import numpy as np
import torch

from torch.autograd.function import once_differentiable

from .. import _ext
from .._lib import check, lib
from ..abi import (EPI_RAW, GN_POST_RELU, GN_PRE_RELU, GROUP_ABS, GROUP_CENTER, GROUP_FP, GROUP_IDX32, GROUP_NO_XYZ, OP_GEMM,
                   OP_ROWS_ATTN, OP_ROWS_CONCAT_QK, OP_ROWS_GN, OP_ROWS_GROUP, PREC_SPLIT, SlideEpi, make_op, ptr, ru, stream_of)
from ..rows import _rop, _run


def _chk(x):
    if not x.is_cuda:
        raise RuntimeError("CPU not supported: the training layers launch HIP kernels")
    assert x.dim() == 2 and x.dtype == torch.float32 and x.shape[1] % 32 == 0 and x.is_contiguous(), (x.shape, x.dtype)


def pad_cols(x, ld=None):
    """[rows, C] -> [rows, ld] (zero pad columns); differentiable (torch ops)"""
    ld = ru(x.shape[1]) if ld is None else ld
    if x.shape[1] == ld:
        return x.contiguous()
    return torch.nn.functional.pad(x, (0, ld - x.shape[1])).contiguous()


_EPI_CACHE = {}   # (bias-vector address, blocks, out_ld) -> (device epilogue-table template, mask of its `out` words): a step's table is
                  # template + mask * output address, one small device add -- an upload would be a blocking host -> device copy
_PACK_CACHE = {}  # id(parameter) -> persistent packed buffers (refilled in place every call: the weights change every step)


def _packs(weight, kp, op_):
    # (the shape is part of the key: a new parameter can inherit the id of a collected one, and the buffers' pad regions must stay zero)
    key = (id(weight), tuple(weight.shape), kp, op_, weight.device.index)
    c = _PACK_CACHE.get(key)
    if c is None:
        if len(_PACK_CACHE) > 4096:
            # (never evict a LIVE parameter's buffers: their addresses are baked into captured step graphs -- ADVICE r4; a model has a
            #  few hundred entries, and entries die with their parameter, below)
            raise RuntimeError("slide_amd.train: more than 4096 packed weight buffers alive -- parameters are being re-created every step")
        dev = weight.device
        c = {"W": torch.zeros(op_, kp, device=dev), "Wt": torch.zeros(kp, op_, device=dev), "vec": torch.zeros(op_, device=dev),
             "zero": torch.zeros(kp, device=dev)}
        _PACK_CACHE[key] = c
        # the entry lives exactly as long as its parameter: a collected parameter's buffers and epilogue tables are released,
        # and a recycled id() can never pick up buffers whose addresses an older captured graph holds
        weakref.finalize(weight, _drop_pack, key)
    return c


def _drop_pack(key):
    c = _PACK_CACHE.pop(key, None)
    if c is not None:
        addr = c["vec"].data_ptr()
        for k in [k for k in _EPI_CACHE if k[0] == addr]:
            _EPI_CACHE.pop(k, None)


def _gemm(x, w_packed, bias_vec, n_out_pad):
    """y [rows, n_out_pad] = x [rows, kp] @ w_packed[n_out_pad, kp]^T + bias_vec (split-precision MFMA GEMM, RAW epilogue)"""
    rows, kp = x.shape
    out = torch.empty(rows, n_out_pad, device=x.device, dtype=torch.float32)
    if rows == 0:
        return out
    n_cob = n_out_pad // 32
    key = (bias_vec.data_ptr(), n_cob, n_out_pad, x.device.index)
    c = _EPI_CACHE.get(key)
    if c is None:
        if len(_EPI_CACHE) > 8192:
            raise RuntimeError("slide_amd.train: more than 8192 epilogue tables alive (their addresses are baked into captured graphs)")
        tab = (SlideEpi * n_cob)()
        for j in range(n_cob):
            t = tab[j]
            t.mode = EPI_RAW
            t.out_ld = n_out_pad
            t.bias = bias_vec.data_ptr() + 4 * 32 * j
            t.out = 4 * 32 * j
        words = ctypes.sizeof(SlideEpi) // 8
        mask = np.zeros((n_cob, words), np.int64)
        mask[:, SlideEpi.out.offset // 8] = 1
        c = (torch.from_numpy(np.frombuffer(bytes(tab), dtype=np.int64).reshape(n_cob, words).copy()).to(x.device),
             torch.from_numpy(mask).to(x.device))
        _EPI_CACHE[key] = c
    epi = torch.add(c[0], c[1], alpha=out.data_ptr())
    # small launches (fewer than 256 of the 256-row tiles): the 64-row-tile kernel (the RAW epilogue does not look at samples, so the
    # "16 rows per sample" form that selects it is only a tile-shape request)
    npx = 4 if ((rows + 255) // 256) * ((n_cob + 1) // 2) < 256 else 8  # (measured: 0 / 256 / 1024 / always -- 256 is best at batch 32 and 256)
    _run(make_op(OP_GEMM, i=(rows, kp, kp, n_cob, npx, 0, PREC_SPLIT, 2, 0, 0),
                 p=(x.data_ptr(), w_packed.data_ptr(), epi.data_ptr())))
    return out


def col_sums(x):
    """sum over the rows of x [rows, ld] -> [ld] (csrc/train_ops.hip col_sums_kernel: coalesced row chunks, then the same kernel over
    the partial rows).  torch's dim-0 reduction of a 65536 x 128 matrix runs at 4 % of the HBM rate, and its multi-block reductions
    (semaphore + staging buffer) returned garbage inside replayed HIP graphs (tools/debug_train_nan4.py)."""
    rows, ld = x.shape
    buf = torch.empty(1025 if rows >= 128 else 1, ld, device=x.device, dtype=torch.float32)
    check(lib().slide_col_sums(rows, ld, ptr(x), ptr(buf), buf.data_ptr() + 4 * ld if rows >= 128 else None, stream_of()),
          "slide_col_sums")
    return buf[0]


def col_sums_seg(x, B, S):
    """per-sample column sums of x [B * S, ld] -> [B, ld] (csrc/train_ops.hip col_sums_seg_kernel, include/slide_train.h
    slide_col_sums_seg): the reduction col_sums does over all rows, over the S rows of each sample -- torch's x.view(B, S, ld).sum(1)
    is the reduction shape col_sums' docstring rules out on the training path"""
    _chk(x)
    ld = x.shape[1]
    assert x.shape[0] == B * S
    out = torch.empty(B, ld, device=x.device, dtype=torch.float32)
    scratch = torch.empty(B * min(256, S // 64) * ld, device=x.device, dtype=torch.float32) if S >= 128 else None
    check(lib().slide_col_sums_seg(B, S, ld, ptr(x), ptr(out), ptr(scratch), stream_of()), "slide_col_sums_seg")
    return out


class AddVecRows(torch.autograd.Function):
    """x[(b, s)][c] += vec[b][c] on rows [B * S, ld], vec [B, C <= ld] (the class- / t-embedding term of Mlp_plus_t_emb,
    pointnet2_modules.py:150-166).  The forward is an elementwise broadcast add (torch); the backward's dvec is the per-sample
    column sum of dy over the S rows of a sample: slide_col_sums_seg."""

    @staticmethod
    def forward(ctx, x, vec, B, S):
        _chk(x)
        assert x.shape[0] == B * S and vec.shape[0] == B and vec.shape[1] <= x.shape[1], (x.shape, vec.shape, B, S)
        ctx.cfg = (B, S, vec.shape[1])
        return (x.view(B, S, -1) + pad_cols(vec, x.shape[1])[:, None, :]).reshape(B * S, -1)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        B, S, C = ctx.cfg
        dvec = col_sums_seg(dy.contiguous(), B, S)[:, :C] if ctx.needs_input_grad[1] else None
        return dy if ctx.needs_input_grad[0] else None, dvec, None, None


def _weight_grad(dy, x):
    """dW (padded) [op_, kp] = dy^T x over the rows: a library GEMM (hipBLASLt through torch) whose contraction is the LONG dimension
    (up to 65536 rows against 32..512 outputs), so it is split into row slabs -- a batched GEMM that fills the chip -- and the
    slab results are added."""
    rows = dy.shape[0]
    slabs = 1
    while slabs < 64 and rows % (slabs * 2) == 0 and rows // (slabs * 2) >= 256:
        slabs *= 2
    if slabs == 1:
        return dy.t() @ x
    return torch.bmm(dy.view(slabs, rows // slabs, -1).transpose(1, 2), x.view(slabs, rows // slabs, -1)).sum(dim=0)


class ConvRows(torch.autograd.Function):
    """nn.Conv2d(1x1) / nn.Conv1d(1) / nn.Linear on rows: y[:, :O] = x[:, :I] @ W^T + b, pad columns zero"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _chk(x)
        O, I = weight.shape[0], int(np.prod(weight.shape[1:]))
        kp, op_ = x.shape[1], ru(O)
        assert kp == ru(I), (kp, I)
        c = _packs(weight, kp, op_)
        c["W"][:O, :I].copy_(weight.detach().reshape(O, I))
        if bias is not None:
            c["vec"][:O].copy_(bias.detach())
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return _gemm(x, c["W"], c["vec"], op_)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        O, I = weight.shape[0], int(np.prod(weight.shape[1:]))
        kp, op_ = x.shape[1], dy.shape[1]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:  # dx = dy @ W: the forward GEMM on the transposed weights
            c = _packs(weight, kp, op_)
            c["Wt"][:I, :O].copy_(weight.detach().reshape(O, I).t())
            dx = _gemm(dy, c["Wt"], c["zero"], kp)
        if ctx.needs_input_grad[1]:
            dw = _weight_grad(dy, x)[:O, :I].reshape(weight.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = col_sums(dy)[:O]
        return dx, dw, db


class GroupNormRows(torch.autograd.Function):
    """post_relu?(MyGroupNorm(pre_relu?(x))) over the S rows of each of the B samples: G groups over the first len(gamma) channels,
    the rest pass through (pointnet2_modules.py:24-42).  gamma None: ReLUs only."""

    @staticmethod
    def forward(ctx, x, gamma, beta, B, S, G, pre_relu, post_relu):
        _chk(x)
        assert x.shape[0] == B * S
        ld = x.shape[1]
        n_norm = 0 if gamma is None else gamma.shape[0]
        G = G if n_norm else 0
        flags = (GN_PRE_RELU if pre_relu else 0) | (GN_POST_RELU if post_relu else 0)
        out = torch.empty_like(x)
        gam = bet = part = mr = None
        if n_norm:
            gam, bet = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
            part = torch.empty(B * 64 * ld * 2 + B * 2 * ld, device=x.device, dtype=torch.float32)
            mr = torch.empty(B, 64, 2, device=x.device, dtype=torch.float32)  # the statistics, for the backward
        if x.shape[0]:
            _run(_rop(OP_ROWS_GN, False, (B, S, ld, G, n_norm, flags, 0, 0, 0), (x, gam, bet, None, None, part, out, None, None, None, mr)))
        ctx.save_for_backward(x, gam, bet, mr)
        ctx.cfg = (B, S, G, n_norm, flags)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, gam, bet, mr = ctx.saved_tensors
        B, S, G, n_norm, flags = ctx.cfg
        ld = x.shape[1]
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg = db = scratch = None
        if n_norm:
            dg, db = torch.empty(B, ld, device=x.device), torch.empty(B, ld, device=x.device)
            scratch = torch.empty(B * (64 * ld * 2 + 128), device=x.device, dtype=torch.float32)
        if x.shape[0]:
            check(lib().slide_gn_rows_bwd(B, S, ld, G, n_norm, flags, ptr(x), ptr(gam), ptr(bet), ptr(mr), ptr(dy), ptr(dx), ptr(dg), ptr(db),
                                          ptr(scratch), stream_of()), "slide_gn_rows_bwd")
        elif n_norm:
            dg.zero_(), db.zero_()
        return (dx, None if dg is None else col_sums(dg)[:n_norm], None if db is None else col_sums(db)[:n_norm], None, None, None, None, None)


class GroupRows(torch.autograd.Function):
    """grouped input of an SA block (QueryAndGroup: [feat | rel | abs | centre]) or of a kNN feature-propagation block
    (group_knn: [feat | d2 | w | abs | rel | centre]) as rows [(b, p, k)] (pointnet2_utils.py:383-430, :497-524); differentiable in the
    features and -- for given neighbours -- in both coordinate tensors (csrc/group_coord_bwd.hip; d2 is differentiated as the squared
    distance of the pair).  feat None: C = 0.  idx int64 (knn_points) or int32 (ball_query); counts (B, np) int32 or None: a centre
    with count 0 is its own neighbour, with zero features.  With coordinates that do not require grad nothing is saved for them and
    the coordinate kernel is not launched."""

    @staticmethod
    def forward(ctx, feat, xyz, new_xyz, idx, d2, flags, C, counts=None):
        if feat is not None:
            _chk(feat)
        elif not xyz.is_cuda:
            raise RuntimeError("CPU not supported: the training layers launch HIP kernels")
        B, N = xyz.shape[:2]
        npnt, K = idx.shape[1:]
        flags = (flags & ~GROUP_IDX32) | (GROUP_IDX32 if idx.dtype == torch.int32 else 0)
        ncoord = 11 if flags & GROUP_FP else 0 if flags & GROUP_NO_XYZ else 3 + (3 if flags & GROUP_ABS else 0) + (3 if flags & GROUP_CENTER else 0)
        ldf = 0 if feat is None else feat.shape[1]
        # (GROUP_NO_XYZ keeps the width it always had here: room for the rel columns, left zero)
        out = torch.empty(B * npnt * K, ru(C + max(ncoord, 3)), device=xyz.device, dtype=torch.float32)
        idx = idx.contiguous()
        assert idx.dtype in (torch.int64, torch.int32) and (feat is None or feat.shape[0] == B * N) and (feat is not None or C == 0)
        assert counts is None or (counts.dtype == torch.int32 and counts.shape == (B, npnt))
        need_coord = ncoord > 0 and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        if need_coord and (xyz.dtype != torch.float32 or new_xyz.dtype != torch.float32):
            raise RuntimeError("the coordinate gradient of the grouping layer takes float32 coordinates")
        xyz_c, new_c = xyz.contiguous().float(), new_xyz.contiguous().float()
        d2 = None if d2 is None else d2.contiguous()
        counts = None if counts is None else counts.contiguous()
        _run(_rop(OP_ROWS_GROUP, False, (B, N, npnt, K, C, ldf, out.shape[1], flags), (xyz_c, new_c, feat, idx, d2, out, counts)))
        # (slide_group_rows_bwd reads int64 indices)
        idx64 = idx.long() if feat is not None and idx.dtype == torch.int32 and ctx.needs_input_grad[0] else None
        if need_coord:
            ctx.save_for_backward(idx, idx64, counts, xyz_c, new_c, d2)
        else:
            ctx.save_for_backward(idx, idx64, counts)
        ctx.cfg = (B, N, npnt, K, C, ldf, out.shape[1], flags, need_coord)
        return out

    @staticmethod
    def backward(ctx, dout):
        idx, idx64, counts = ctx.saved_tensors[:3]
        B, N, npnt, K, C, ldf, ldg, flags, need_coord = ctx.cfg
        dout = dout.contiguous()
        dfeat = dxyz = dnew = None
        if ldf and ctx.needs_input_grad[0]:
            dfeat = torch.zeros(B * N, ldf, device=dout.device, dtype=torch.float32)
            check(lib().slide_group_rows_bwd(B, N, npnt, K, C, ldf, ldg, ptr(idx if idx64 is None else idx64), ptr(counts), ptr(dout), ptr(dfeat),
                                             stream_of()), "slide_group_rows_bwd")
        if need_coord:
            xyz, new_xyz, d2 = ctx.saved_tensors[3:]
            if ctx.needs_input_grad[1]:
                dxyz = torch.zeros(B, N, 3, device=dout.device, dtype=torch.float32)  # (accumulated with atomics)
            if ctx.needs_input_grad[2]:
                dnew = torch.empty(B, npnt, 3, device=dout.device, dtype=torch.float32)  # (written in full)
            check(lib().slide_group_rows_coord_bwd(B, N, npnt, K, C, ldg, flags, ptr(xyz), ptr(new_xyz), ptr(idx), ptr(d2), ptr(counts), ptr(dout),
                                                   ptr(dxyz), ptr(dnew), stream_of()), "slide_group_rows_coord_bwd")
        return dfeat, dxyz, dnew, None, None, None, None, None


class ConcatQK(torch.autograd.Function):
    """relu([q(point) broadcast over the K neighbours | k(point, neighbour)])  (attention.py:78-88)"""

    @staticmethod
    def forward(ctx, q, k, K, C1, C2):
        _chk(q), _chk(k)
        assert k.shape[0] == q.shape[0] * K
        out = torch.empty(k.shape[0], ru(C1 + C2), device=k.device, dtype=torch.float32)
        if k.shape[0]:
            _run(_rop(OP_ROWS_CONCAT_QK, False, (k.shape[0], K, C1, q.shape[1], C2, k.shape[1], out.shape[1]), (q, k, out)))
        ctx.save_for_backward(out)
        ctx.cfg = (K, C1, q.shape[1], C2, k.shape[1])
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        K, C1, ldq, C2, ldk = ctx.cfg
        dout = dout.contiguous()
        pts = out.shape[0] // K
        dq = torch.zeros(pts, ldq, device=out.device, dtype=torch.float32)
        dk = torch.zeros(out.shape[0], ldk, device=out.device, dtype=torch.float32)
        check(lib().slide_concat_qk_bwd(pts, K, C1, ldq, C2, ldk, out.shape[1], ptr(out), ptr(dout), ptr(dq), ptr(dk), stream_of()),
              "slide_concat_qk_bwd")
        return dq, dk, None, None, None


class AttendRows(torch.autograd.Function):
    """softmax over the K neighbour rows of each point, weighted sum of the values (attention.py:89-95; 'nn' grouping: all K count)"""

    @staticmethod
    def forward(ctx, scores, values, K, C):
        _chk(scores), _chk(values)
        assert scores.shape[0] == values.shape[0]
        pts = scores.shape[0] // K
        out = torch.empty(pts, ru(C), device=scores.device, dtype=torch.float32)
        if pts:
            _run(_rop(OP_ROWS_ATTN, False, (pts, K, C, scores.shape[1], values.shape[1], out.shape[1], 1, 0), (scores, values, out, None, None)))
        ctx.save_for_backward(scores, values)
        ctx.cfg = (K, C, out.shape[1])
        return out

    @staticmethod
    def backward(ctx, dout):
        scores, values = ctx.saved_tensors
        K, C, ldo = ctx.cfg
        dout = dout.contiguous()
        pts = scores.shape[0] // K
        ds, dv = torch.zeros_like(scores), torch.zeros_like(values)
        check(lib().slide_attn_rows_bwd(pts, K, C, scores.shape[1], values.shape[1], ldo, ptr(scores), ptr(values), None,
                                        ptr(dout), ptr(ds), ptr(dv), stream_of()), "slide_attn_rows_bwd")
        return ds, dv, None, None


class ChamferCD(torch.autograd.Function):
    """per-cloud Chamfer sums of (output, gt) -> red (B, 2, 5), direction 0 = gt -> output: chamfer_nn + chamfer_reduce exactly as
    metrics_point_cloud.chamfer_and_f1.calc_cd_reduced calls them (feature term `mse` when C > 3), bit-equal to it.  Backward: one
    launch of csrc/chamfer_bwd.hip (include/slide_train.h slide_chamfer_cd_bwd) on the saved neighbours; no double backward.  Where a
    distance or a feature term is 0 its square root contributes the subgradient 0 (torch's autograd: NaN)."""

    @staticmethod
    def forward(ctx, output, gt, f1_threshold):
        gt = gt.detach().contiguous()
        output = output.detach().contiguous()
        d1, i1, d2, i2 = _ext.chamfer_nn(gt, output)
        if gt.shape[2] > 3:
            red = _ext.chamfer_reduce(d1, i1, d2, i2, threshold=f1_threshold, fx=gt[:, :, 3:], fy=output[:, :, 3:], term="mse")
        else:
            red = _ext.chamfer_reduce(d1, None, d2, None, threshold=f1_threshold)
        ctx.save_for_backward(gt, output, d1, i1, d2, i2)
        return red

    @staticmethod
    @once_differentiable
    def backward(ctx, dred):
        gt, output, d1, i1, d2, i2 = ctx.saved_tensors
        dgt, dout = _ext.chamfer_cd_bwd(gt, output, d1, i1, d2, i2, dred.contiguous(), need_dx=ctx.needs_input_grad[1],
                                        need_dy=ctx.needs_input_grad[0])
        return dout, dgt, None


def chamfer_cd(output, gt, f1_threshold=1e-4):
    """differentiable counterpart of calc_cd_reduced(output, gt, f1_threshold, 'mse')[0]: output (B, P_out, C), gt (B, P_gt, C) fp32
    CUDA tensors, C = 3 + F (F <= 16 feature channels) -> red (B, 2, 5) = [pair][direction] (sum d, sum sqrt d, count d < threshold,
    sum t, sum sqrt t), direction 0 over gt's points; differentiable in both clouds (the count has no gradient)."""
    if not (torch.is_tensor(output) and torch.is_tensor(gt)) or output.ndim != 3 or gt.ndim != 3:
        raise ValueError("Expected points to be of shape (N, P, D)")
    if output.shape[0] != gt.shape[0] or output.shape[2] != gt.shape[2]:
        raise ValueError("y does not have the correct shape.")
    if gt.shape[1] < 1 or output.shape[1] < 1 or gt.shape[2] < 3:
        raise ValueError("point clouds must hold at least one point of at least three channels")
    if gt.shape[2] > 3 + 16:
        raise ValueError("at most 16 feature channels are supported")
    for t in (output, gt):
        if not t.is_cuda:
            raise RuntimeError("CPU not supported: the Chamfer loss launches HIP kernels")
        if t.dtype != torch.float32:
            raise RuntimeError("the Chamfer loss takes float32 tensors")
    return ChamferCD.apply(output, gt, float(f1_threshold))


class DpsrGrid(torch.autograd.Function):
    """DPSR.forward (pointnet2/dpsr_utils/dpsr.py): V, N (B, n, 3) and the filter G -> phi (B, r, r, r), bit-equal to _ext.dpsr_grid.
    Saves V, N, phi and the per-sample (offset, |fv0|) only (G is the module's buffer, held by reference); backward: csrc/dpsr_bwd.hip (include/slide_hip.h slide_dpsr_grid_bwd) on the
    same chunks.  G gets no gradient; no double backward."""

    @staticmethod
    def forward(ctx, V, N, G, shift, scale, chunk):
        V, N, G = V.detach().contiguous(), N.detach().contiguous(), G.detach()
        phi, coef = _ext.dpsr_grid(V, N, G, shift=shift, scale=scale, chunk=chunk, return_coef=True)
        ctx.save_for_backward(V, N, G, phi, coef)
        ctx.flags = (bool(shift), bool(scale), chunk)
        return phi

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():  # (create_graph=True: the engine runs backward functions with grad mode on)
            raise RuntimeError("DpsrGrid: double backward is not supported (the backward kernels are not differentiable)")
        V, N, G, phi, coef = ctx.saved_tensors
        shift, scale, chunk = ctx.flags
        # (contiguous(): the gradient of a sum or a mean arrives as an expanded scalar)
        dV, dN = _ext.dpsr_grid_backward(V, N, G, phi, coef, g.contiguous(), shift=shift, scale=scale, need_v=ctx.needs_input_grad[0],
                                         need_n=ctx.needs_input_grad[1], chunk=chunk)
        return dV, dN, None, None, None, None


def dpsr_grid(V, N, G, shift=True, scale=True, chunk=None):
    """differentiable DPSR: V (B, n, 3) coordinates in [0, 1), N (B, n, 3) normals, fp32 CUDA tensors, G the module's Gaussian filter
    (r, r, r/2 + 1, ...) -> phi (B, r, r, r); differentiable in V and N, once."""
    for t in (V, N):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("CPU not supported: DPSR launches HIP kernels")
        if t.dtype != torch.float32:
            raise RuntimeError("DPSR takes float32 tensors")
    if V.shape != N.shape:
        raise ValueError("V and N must have the same shape, got %s and %s" % (tuple(V.shape), tuple(N.shape)))
    return DpsrGrid.apply(V, N, G, bool(shift), bool(scale), chunk)


class ColMaxSeg(torch.autograd.Function):
    """max over the S rows of each sample of x [B * S, ld] -> [B, ld] (columns >= C zero): the point-wise maxima of Pnet2Stage
    (pointnet2/models/pnet.py:32-40).  One launch forward (slide_col_max_seg: the value and the first row that attains it), one
    backward (slide_col_max_seg_bwd: a gather that writes dx in full) -- torch composes amax + argmax + a zero fill + a scatter."""

    @staticmethod
    def forward(ctx, x, B, S, C):
        _chk(x)
        assert x.shape[0] == B * S and 0 <= C <= x.shape[1], (x.shape, B, S, C)
        ld = x.shape[1]
        out = torch.empty(B, ld, device=x.device, dtype=torch.float32)
        arg = torch.empty(B, ld, device=x.device, dtype=torch.int32)
        check(lib().slide_col_max_seg(B, S, C, ld, ptr(x), ptr(out), ptr(arg), stream_of()), "slide_col_max_seg")
        ctx.save_for_backward(arg)
        ctx.cfg = (B, S)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, _darg):
        (arg,) = ctx.saved_tensors
        B, S = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty(B * S, arg.shape[1], device=dy.device, dtype=torch.float32)
        check(lib().slide_col_max_seg_bwd(B, S, arg.shape[1], ptr(arg), ptr(dy), ptr(dx), stream_of()), "slide_col_max_seg_bwd")
        return dx, None, None, None


class GaussPosterior(torch.autograd.Function):
    """DiagonalGaussianDistribution (pointnet2/data_utils/distributions.py:4-43) on rows: params [B * S, ldp] = [mean (C) | logvar (C)]
    -> (z [B * S, ru(C)], kl [B]); z = mean + exp(0.5 clamp(logvar, -30, 20)) * eps, or the mode with eps None; kl = 0.5 * the sum over
    the sample of mean^2 + var - 1 - clamp(logvar).  Differentiable in params; eps is a plain tensor [B * S, ru(C)] the caller draws
    (the kernels never draw numbers: a captured step refills a static eps between replays)."""

    @staticmethod
    def forward(ctx, params, eps, B, S, C):
        _chk(params)
        assert params.shape[0] == B * S and 2 * C <= params.shape[1], (params.shape, B, S, C)
        ldz = ru(C)
        if eps is not None:
            _chk(eps)
            assert eps.shape == (B * S, ldz), (eps.shape, B, S, C)
        z = torch.empty(B * S, ldz, device=params.device, dtype=torch.float32)
        kl = torch.empty(B, device=params.device, dtype=torch.float32)
        check(lib().slide_gauss_posterior_fwd(B, S, C, params.shape[1], ldz, ptr(params), ptr(eps), ptr(z), ptr(kl), stream_of()),
              "slide_gauss_posterior_fwd")
        ctx.save_for_backward(params, eps)
        ctx.cfg = (B, S, C, ldz)
        ctx.set_materialize_grads(False)  # an output nobody differentiates arrives as None: the kernel's NULL (that term is 0)
        return z, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, dkl):
        params, eps = ctx.saved_tensors
        B, S, C, ldz = ctx.cfg
        dz = None if dz is None else dz.contiguous()
        dkl = None if dkl is None else dkl.contiguous()
        dparams = torch.empty_like(params)
        check(lib().slide_gauss_posterior_bwd(B, S, C, params.shape[1], ldz, ptr(params), ptr(eps), ptr(dz), ptr(dkl), ptr(dparams),
                                              stream_of()), "slide_gauss_posterior_bwd")
        return dparams, None, None, None, None


def col_max_seg(x, B, S, C):
    """-> (max [B, ld], arg [B, ld] int32: the first row of the sample that attains it; -1 in the pad columns)"""
    return ColMaxSeg.apply(x, B, S, C)


def gauss_posterior(params, eps, B, S, C):
    return GaussPosterior.apply(params, eps, B, S, C)


def conv_rows(x, weight, bias=None):
    return ConvRows.apply(x, weight, bias)


def gn_rows(x, gamma, beta, B, S, G, pre_relu=False, post_relu=False):
    return GroupNormRows.apply(x, gamma, beta, B, S, G, pre_relu, post_relu)


def group_rows(feat, xyz, new_xyz, idx, d2, flags, C, counts=None):
    return GroupRows.apply(feat, xyz, new_xyz, idx, d2, flags, C, counts)


def add_vec_rows(x, vec, B, S):
    return AddVecRows.apply(x, vec, B, S)


def concat_qk(q, k, K, C1, C2):
    return ConcatQK.apply(q, k, K, C1, C2)


def attend_rows(scores, values, K, C):
    return AttendRows.apply(scores, values, K, C)
