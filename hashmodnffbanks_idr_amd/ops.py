"""Thin Python operators over the C ABI (include/hashmod.h) + the autograd glue.

Every function here launches hand-written HIP kernels from libhashmod.so on torch's current
stream; torch supplies device memory only.  CPU tensors raise (no fallback).
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check, dptr, lib, require_gpu, stream_ptr

FRAC_MODES = {"reference": 0, "trilinear": 1}
# sdf_fwd / sdf_fwd_emb tile_points: the 64-point launch with quarter tiles enabled (hashmod.h: HM_SDF_TILE64_QUARTER)
TILE64_QUARTER = 1664


# =========================================================================================
# deterministic mode (DESIGN.md "Deterministic mode")
# =========================================================================================
_DETERMINISTIC = []     # stack of the active deterministic(...) contexts' settings (module-wide, not thread-local:
                        # autograd runs the backward nodes on a thread of its own)


class deterministic:
    """``with ops.deterministic():`` - every reduction of the library runs without fp32 atomics, in an order that
    depends on shapes and indices only, so that a training step is bitwise reproducible: gemm / gemm_group_tn split K
    through k-part workspaces, the column sums through slab workspaces, encode_bwd_table sorts its contributions.
    Nestable; ``deterministic(False)`` switches the mode off inside an outer context.  Outside every context the mode
    follows ``torch.are_deterministic_algorithms_enabled()``."""

    def __init__(self, enabled=True):
        self.enabled = bool(enabled)

    def __enter__(self):
        _DETERMINISTIC.append(self.enabled)
        return self

    def __exit__(self, *exc):
        _DETERMINISTIC.pop()


def is_deterministic():
    """the innermost deterministic(...) setting, else torch's deterministic-algorithms flag"""
    return _DETERMINISTIC[-1] if _DETERMINISTIC else torch.are_deterministic_algorithms_enabled()


# library scratch memory, one owner per purpose (DESIGN.md "Scratch memory under graph capture")
_DET_WS = _lib.Workspace("deterministic mode")      # shared by the deterministic reductions: one stream orders their use
_ENC_WS = _lib.Workspace("encode_fwd")              # the z-ordered encode's point permutation
_ENC_BWD_WS = _lib.Workspace("encode_bwd_table")    # the z-ordered table backward
_SORT_WS = _lib.Workspace("sort_pairs")


def _det_workspace(device, need):
    """(pointer, bytes) of the deterministic reductions' workspace"""
    ws = _DET_WS.get(device, need)
    return dptr(ws), 0 if ws is None else ws.numel()


def level_table(n_levels, log2_hashmap_size, base_resolution, desired_resolution, in_dim=3):
    """res[l], rows[l] in host double precision, the arithmetic of
    reference model/embeddings/hashGridEmbedding.py:126-132 (Python ``math``, not fp32)."""
    beta_growth = math.exp((math.log(desired_resolution) - math.log(base_resolution)) / (n_levels - 1))
    res, rows = [], []
    for level_idx in range(n_levels):
        resolution = math.floor(base_resolution * (beta_growth ** level_idx))
        res.append(resolution)
        rows.append(min(resolution ** in_dim, 2 ** log2_hashmap_size))
    return res, rows


class GridDesc:
    """Owns an hm_grid_desc (host-side level table handed to kernels by value)."""

    def __init__(self, res, rows, n_features=2):
        self.L = len(res)
        self.F = int(n_features)
        self.res = np.asarray(res, np.int32)
        self.rows = np.asarray(rows, np.uint32)
        self.row_off = np.concatenate([[0], np.cumsum(self.rows.astype(np.uint64))]).astype(np.uint64)
        self.total_rows = int(self.row_off[-1])
        self.E = 3 + 2 * self.L + self.L * self.F
        self._h = C.c_void_p(0)
        check(lib().hm_grid_desc_create(self.L, self.F, self.res.ctypes.data_as(C.c_void_p),
                                        self.rows.ctypes.data_as(C.c_void_p),
                                        self.row_off.ctypes.data_as(C.c_void_p), C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def __reduce__(self):  # copy.deepcopy / pickle: rebuild the native descriptor from the host arrays
        return (GridDesc, (self.res.tolist(), self.rows.tolist(), self.F))

    def __del__(self):
        try:
            if self._h:
                lib().hm_grid_desc_destroy(self._h)
                self._h = C.c_void_p(0)
        except Exception:
            pass


def _prep_x(x):
    if x.dtype != torch.float32:
        x = x.float()
    return x.reshape(-1, 3).contiguous()


def corner_ids(desc, level, x):
    """xi [N,3] int32 and the 8 corner row ids [N,8] (as int64) of one level - bit-exact with
    reference hash_func (hashGridEmbedding.py:32-40,84-98)."""
    x = _prep_x(x)
    require_gpu(x)
    n = x.shape[0]
    xi = torch.empty((n, 3), dtype=torch.int32, device=x.device)
    ids = torch.empty((n, 8), dtype=torch.int32, device=x.device)
    check(lib().hm_corner_ids(desc.handle, int(level), dptr(x), n, dptr(xi), dptr(ids), stream_ptr(x)))
    return xi, ids.long() & 0xFFFFFFFF


def encode_fwd(desc, x, table, B, frac_mode=0, hash_only=False):
    """[N,E] embedding (or [N,L*F] hash features when hash_only) - no autograd."""
    x = _prep_x(x)
    require_gpu(x, table, B)
    assert table.is_contiguous() and table.dtype == torch.float32 and table.shape == (desc.total_rows, desc.F)
    n = x.shape[0]
    width = desc.L * desc.F if hash_only else desc.E
    Bp = None if hash_only else B.contiguous()
    if n >= 131072:     # big launches: z-ordered gather (needs scratch for the point permutation)
        # rows padded to a multiple of 4 floats (268 -> 272 bytes at E = 67): every row then starts on a 16-byte boundary
        # and leaves the kernel as ONE dwordx4 store instruction; the caller gets the [n, width] view of the buffer
        stride = (width + 3) & ~3
        buf = torch.empty((n, stride), dtype=torch.float32, device=x.device)
        out = buf[:, :width] if stride != width else buf
        ws = _ENC_WS.get(x.device, check(lib().hm_encode_workspace_bytes(desc.handle, n)))
        check(lib().hm_encode_fwd_ws(desc.handle, dptr(x), n, dptr(table), dptr(Bp), dptr(buf), stride, int(frac_mode),
                                     dptr(ws), ws.numel(), stream_ptr(x)))
    else:
        out = torch.empty((n, width), dtype=torch.float32, device=x.device)
        check(lib().hm_encode_fwd(desc.handle, dptr(x), n, dptr(table), dptr(Bp), dptr(out), width, int(frac_mode),
                                  stream_ptr(x)))
    return out


def encode_bwd_table(desc, x, d_feat, frac_mode=0, out=None, deterministic=None):
    """Scatter-add of the hash-feature gradient d_feat [N,L*F] into a [rows,F] table gradient.
    deterministic: sort the contributions by destination row (sort_pairs: the library's stable radix sort) and sum each row's run in one thread
    (hm_encode_rows + hm_encode_bwd_table_sorted) instead of fp32 atomics - bitwise reproducible.  None follows
    is_deterministic()."""
    if deterministic is None:
        deterministic = is_deterministic()
    x = _prep_x(x)
    require_gpu(x, d_feat)
    n = x.shape[0]
    assert d_feat.shape == (n, desc.L * desc.F) and d_feat.dtype == torch.float32
    if d_feat.stride(1) != 1:
        d_feat = d_feat.contiguous()
    if out is None:
        out = torch.zeros((desc.total_rows, desc.F), dtype=torch.float32, device=x.device)
    if deterministic and n > 0:
        corners, skeys, perm, wts = sorted_rows(desc, x, frac_mode)
        check(lib().hm_encode_bwd_table_sorted(desc.handle, dptr(skeys), dptr(perm), skeys.numel(), corners, dptr(d_feat),
                                               d_feat.stride(0), dptr(wts), dptr(out), stream_ptr(x)))
        return out
    if n >= 131072 and desc.F == 2:     # big launches: z-ordered, LDS-privatised scatter (needs scratch)
        ws = _ENC_BWD_WS.get(x.device, check(lib().hm_encode_bwd_workspace_bytes(desc.handle, n)))
        check(lib().hm_encode_bwd_table_ws(desc.handle, dptr(x), n, dptr(d_feat), d_feat.stride(0), dptr(out),
                                           int(frac_mode), dptr(ws), ws.numel(), stream_ptr(x)))
        return out
    check(lib().hm_encode_bwd_table(desc.handle, dptr(x), n, dptr(d_feat), d_feat.stride(0), dptr(out),
                                    int(frac_mode), stream_ptr(x)))
    return out


def sorted_rows(desc, x, frac_mode=0):
    """(corners, destination rows sorted, permutation, corner weights or None) of the table-gradient contributions of
    the points x: hm_encode_rows + sort_pairs, the first half of the deterministic scatter"""
    n = x.shape[0]
    corners = 1 if int(frac_mode) == 0 else 8
    keys = torch.empty(n * desc.L * corners, dtype=torch.int32, device=x.device)
    wts = torch.empty(n * desc.L * corners, dtype=torch.float32, device=x.device) if corners == 8 else None
    check(lib().hm_encode_rows(desc.handle, dptr(x), n, int(frac_mode), dptr(keys), dptr(wts), stream_ptr(x)))
    skeys, perm = sort_pairs(keys, max(int(desc.total_rows - 1).bit_length(), 1))
    return corners, skeys, perm, wts


def sort_pairs(keys, key_bits=31):
    """(sorted keys, permutation as int64) of non-negative int32 keys < 2^key_bits: the library's stable LSD radix sort
    (hm_sort_pairs_i32), the sort behind encode_bwd_table(deterministic=True)."""
    require_gpu(keys)
    if keys.dtype != torch.int32 or keys.dim() != 1 or not keys.is_contiguous():
        raise ValueError("hashmod sort_pairs: contiguous 1-D int32 keys expected")
    n = keys.numel()
    out = torch.empty_like(keys)
    perm = torch.empty(n, dtype=torch.int64, device=keys.device)
    if n == 0:
        return out, perm
    ws = _SORT_WS.get(keys.device, check(lib().hm_sort_workspace_bytes(n)))
    check(lib().hm_sort_pairs_i32(dptr(keys), n, int(key_bits), dptr(out), dptr(perm), dptr(ws), ws.numel(),
                                  stream_ptr(keys)))
    return out, perm


class _HashFeatures(torch.autograd.Function):
    """Encoder output as an autograd node: hash features [N,L*F] (B is None) or the full
    [N,E] row [x|sin|cos|features] (B given; only the feature columns carry gradient).
    Differentiable to any order w.r.t. the table (the op is linear in it).  In reference frac mode
    d/dx of the hash features is identically zero, exactly as in the reference where
    xf = x - x.float() kills the interpolation weights (hashGridEmbedding.py:86); in trilinear mode
    d/dx is the node _HashInputGrad (differentiable once more)."""

    @staticmethod
    def forward(ctx, x, table, B, desc, frac_mode, collector=None):
        ctx.desc, ctx.frac_mode, ctx.collector = desc, frac_mode, collector
        ctx.hoff = 0 if B is None else 3 + 2 * desc.L
        ctx.save_for_backward(x)
        ctx.table = table if (frac_mode != 0 and ctx.needs_input_grad[0]) else None   # d/dx gathers the table again
        return encode_fwd(desc, x, table, B, frac_mode, hash_only=B is None)

    @staticmethod
    def backward(ctx, d_out):
        (x,) = ctx.saved_tensors
        d_table = d_x = None
        if ctx.needs_input_grad[1]:
            d_feat = d_out[:, ctx.hoff:] if ctx.hoff else d_out
            if ctx.collector is not None and ctx.collector.active:
                # data-parallel static step (parallel.TouchedRowExchange): the collector scatters into ITS static dense
                # gradient (bound as table.grad) and lists the touched rows for the exchange; autograd gets nothing
                ctx.collector.add(x, d_feat)
                d_table = None
            else:
                d_table = _HashScatter.apply(x, d_feat, ctx.desc, ctx.frac_mode)
        if ctx.needs_input_grad[0]:
            if ctx.hoff:
                raise RuntimeError("internal: full-row encode node must not be used when x requires grad")
            if ctx.frac_mode != 0:
                d_x = _HashInputGrad.apply(x, ctx.table, d_out, ctx.desc)
        return d_x, d_table, None, None, None, None


class _HashInputGrad(torch.autograd.Function):
    """gx = J(x)^T d_feat of the trilinear encoder (J = d features / d x) as a node of its own, so that
    ImplicitNetwork.gradient(create_graph=True) can be differentiated once more: the eikonal / normal terms' backward
    arrives here as gg_x and leaves towards d_feat (J gg_x), the table and x (csrc/hm_encode_dx.hip)."""

    @staticmethod
    def forward(ctx, x, table, d_feat, desc):
        ctx.desc = desc
        d_feat = _rowmajor(d_feat)
        ctx.save_for_backward(x, table, d_feat)
        gx = torch.empty_like(x)
        check(lib().hm_encode_bwd_input(desc.handle, dptr(x), x.shape[0], dptr(table), dptr(d_feat), _ld(d_feat),
                                        None, dptr(gx), stream_ptr(x)))
        return gx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gg_x):
        x, table, d_feat = ctx.saved_tensors
        desc, n = ctx.desc, x.shape[0]
        gg_x = gg_x.contiguous()
        d_x = d_table = d_dfeat = None
        if ctx.needs_input_grad[0]:
            d_x = torch.empty_like(x)
            check(lib().hm_encode_bwd_input(desc.handle, dptr(x), n, dptr(table), dptr(d_feat), _ld(d_feat),
                                            dptr(gg_x), dptr(d_x), stream_ptr(x)))
        if ctx.needs_input_grad[1]:
            if is_deterministic():
                raise NotImplementedError("hashmod deterministic mode: the trilinear encoder's second-order table term "
                                          "(hm_encode_bwd_table_jvp) scatters with atomics; use frac_mode='reference'")
            d_table = torch.zeros_like(table)
            check(lib().hm_encode_bwd_table_jvp(desc.handle, dptr(x), n, dptr(gg_x), dptr(d_feat), _ld(d_feat),
                                                dptr(d_table), stream_ptr(x)))
        if ctx.needs_input_grad[2]:
            d_dfeat = torch.empty((n, desc.L * desc.F), dtype=torch.float32, device=x.device)
            check(lib().hm_encode_jvp(desc.handle, dptr(x), n, dptr(table), dptr(gg_x), dptr(d_dfeat),
                                      d_dfeat.stride(0), stream_ptr(x)))
        return d_x, d_table, d_dfeat, None


class _HashScatter(torch.autograd.Function):
    """d_table = scatter_add(d_feat at x); its own backward is the gather again."""

    @staticmethod
    def forward(ctx, x, d_feat, desc, frac_mode):
        ctx.desc, ctx.frac_mode = desc, frac_mode
        ctx.save_for_backward(x)
        return encode_bwd_table(desc, x, d_feat, frac_mode)

    @staticmethod
    def backward(ctx, gg_table):
        (x,) = ctx.saved_tensors
        gg = None
        if ctx.needs_input_grad[1]:
            gg = _HashFeatures.apply(x, gg_table.contiguous(), None, ctx.desc, ctx.frac_mode, None)
        return None, gg, None, None


class _AttachInputGrad(torch.autograd.Function):
    """Puts the full embedding row [x | sin | cos | hash features] (already computed by ONE encoder launch as a
    table-gradient-only node, encode_table_grad) onto the graph of the points x: the row is returned as it is
    (mark_dirty, no copy); backward hands d_row on to the table node and produces d_x = _RowInputGrad.  Two nodes, so
    that autograd.grad(e, x, create_graph=True) (ImplicitNetwork.gradient) does not run the table backward at all:
    the engine only visits producers of the inputs that were asked for.  Reference frac mode only (the hash features
    do not depend on x there, hashGridEmbedding.py:86)."""

    @staticmethod
    def forward(ctx, row, x, B):
        ctx.save_for_backward(x, B)
        ctx.mark_dirty(row)
        return row

    @staticmethod
    def backward(ctx, d_row):
        x, B = ctx.saved_tensors
        d_x = _RowInputGrad.apply(x, B, d_row) if ctx.needs_input_grad[1] else None
        return (d_row if ctx.needs_input_grad[0] else None), d_x, None


class _RowInputGrad(torch.autograd.Function):
    """gx = d_row[:, :3] + (d Fourier columns / d x)^T d_row as ONE kernel, differentiable once more: the eikonal /
    normal terms' backward arrives as gg and leaves towards d_row and x in one kernel too (csrc/hm_encode_dx.hip).
    The torch expression of the same thing is ~10 elementwise kernels and a K = 3 vendor matmul per pass."""

    @staticmethod
    def forward(ctx, x, B, d_row):
        d_row = _rowmajor(d_row)
        ctx.save_for_backward(x, B, d_row)
        gx = torch.empty_like(x)
        check(lib().hm_fourier_bwd_input(dptr(x), x.shape[0], dptr(B), B.shape[1], dptr(d_row), _ld(d_row), dptr(gx),
                                         stream_ptr(x)))
        return gx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gg):
        x, B, d_row = ctx.saved_tensors
        n, width = d_row.shape
        gg = gg.contiguous()
        d_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dd = torch.empty((n, width), dtype=torch.float32, device=x.device) if ctx.needs_input_grad[2] else None
        if d_x is not None or dd is not None:
            check(lib().hm_fourier_bwd_input_bwd(dptr(x), n, dptr(B), B.shape[1], dptr(d_row), _ld(d_row), dptr(gg),
                                                 dptr(d_x), dptr(dd), width, width, stream_ptr(x)))
        return d_x, None, dd


def embed_row_input_grad(x, table, B, desc, collector=None):
    """[N,E] embedding row in ONE kernel, differentiable w.r.t. the table (any order) and w.r.t. x (twice) -
    reference frac mode."""
    x = _prep_x(x)
    row = _HashFeatures.apply(x.detach(), table, B, desc, 0, collector)
    return _AttachInputGrad.apply(row, x, B)


def hash_features(x, table, desc, frac_mode=0, collector=None):
    """[N,L*F] hash features with autograd (table grads of any order)."""
    return _HashFeatures.apply(_prep_x(x), table, None, desc, frac_mode, collector)


def encode_table_grad(x, table, B, desc, frac_mode=0, collector=None):
    """Full [N,E] embedding in ONE kernel, differentiable w.r.t. the table only (x is a constant)."""
    return _HashFeatures.apply(_prep_x(x).detach(), table, B, desc, frac_mode, collector)


# =========================================================================================
# exact-fp32 MFMA GEMM (csrc/hm_gemm.hip) as an any-order differentiable torch op
# =========================================================================================
def _check_gemm_out(buf, M, cols, dev, what):
    """a caller-owned GEMM destination: fp32 [M, cols] on `dev`, unit column stride, any row stride"""
    if buf.dtype != torch.float32 or tuple(buf.shape) != (M, cols) or buf.device != dev or \
            (cols > 1 and buf.stride(1) != 1):
        raise ValueError(f"hashmod {what}: bad output buffer (need fp32 [{M}, {cols}] with unit column stride on {dev}; "
                         f"got {buf.dtype} {tuple(buf.shape)} strides {tuple(buf.stride())} on {buf.device})")


def _check_gemm_bias(bias, N, dev, what):
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N or bias.device != dev):
        raise ValueError(f"hashmod {what}: bias must be fp32 with N = {N} elements on {dev}")


def gemm(a, b, bias=None, trans_a=False, trans_b=False, out=None, accumulate=False):
    """C = op(a) @ op(b) (+ bias) on the HIP kernel; no autograd.  out: optional caller-owned fp32 [M, N] destination
    with unit column stride (a row-strided view is fine); accumulate=True adds into it (and needs it)."""
    require_gpu(a, b, bias, out)
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError("hashmod gemm: fp32 only")
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    Kb, N = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if K != Kb:
        raise ValueError(f"hashmod gemm: inner dimensions differ ({K} vs {Kb})")
    _check_gemm_bias(bias, N, a.device, "gemm")
    if out is not None:
        _check_gemm_out(out, M, N, a.device, "gemm")
    elif accumulate:
        raise ValueError("hashmod gemm: accumulate=True adds into out, which is missing")
    if a.stride(-1) != 1:
        a = a.contiguous()
    if b.stride(-1) != 1:
        b = b.contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if bias is not None:
        bias = bias.contiguous()
    if is_deterministic():
        need = check(lib().hm_gemm_f32_det_workspace_bytes(int(trans_a), int(trans_b), M, N, K, _ld(a), _ld(b)))
        ws, nb = _det_workspace(a.device, need)
        check(lib().hm_gemm_f32_det(int(trans_a), int(trans_b), M, N, K, dptr(a), _ld(a), dptr(b), _ld(b), dptr(bias),
                                    dptr(out), _ld(out), int(accumulate), ws, nb, stream_ptr(a)))
        return out
    check(lib().hm_gemm_f32(int(trans_a), int(trans_b), M, N, K, dptr(a), _ld(a), dptr(b), _ld(b), dptr(bias),
                            dptr(out), _ld(out), int(accumulate), stream_ptr(a)))
    return out


def gemm_group_tn(problems):
    """C += A^T @ B for every (A [K, M], B [K, N], C [M, N]) of `problems` in ONE launch (hm_gemm_f32_group_tn): the
    weight gradients of one backward pass.  Row-major fp32 views with arbitrary row strides; C is accumulated into."""
    if not problems:
        return
    items = (_lib.GemmGroupItem * len(problems))()
    keep = []
    for i, (a, b, c) in enumerate(problems):
        require_gpu(a, b, c)
        a, b = _rowmajor(a), _rowmajor(b)
        if c.stride(-1) != 1 or a.dtype != torch.float32 or b.dtype != torch.float32 or c.dtype != torch.float32:
            raise ValueError("hashmod gemm_group_tn: fp32 row-major operands expected")
        K, M = a.shape
        Kb, N = b.shape
        if K != Kb or tuple(c.shape) != (M, N):
            raise ValueError(f"hashmod gemm_group_tn: shapes {tuple(a.shape)}^T @ {tuple(b.shape)} -> {tuple(c.shape)}")
        keep += [a, b]
        items[i] = _lib.GemmGroupItem(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, _ld(a), _ld(b), _ld(c))
    if is_deterministic():
        need = check(lib().hm_gemm_f32_group_tn_det_workspace_bytes(C.cast(items, C.c_void_p), len(problems)))
        ws, nb = _det_workspace(problems[0][0].device, need)
        check(lib().hm_gemm_f32_group_tn_det(C.cast(items, C.c_void_p), len(problems), ws, nb,
                                             stream_ptr(problems[0][0])))
        return
    check(lib().hm_gemm_f32_group_tn(C.cast(items, C.c_void_p), len(problems), stream_ptr(problems[0][0])))


def _group_tn_takes(K, lda, ldb):
    """does the grouped kernel take a problem (else hm_gemm_f32 runs it)?  The rule of group_tn in csrc/hm_gemm.hip,
    pinned to the library by tests/test_gemm_group_add_cpu.py."""
    return K % 128 == 0 and 4 * lda * K < 2 ** 31 and 4 * ldb * K < 2 ** 31


def gemm_group_tn_add(problems):
    """gemm_group_tn over operands with ADDENDS: every problem is (A [K, M], B [K, N], C [M, N], a_add, b_add) with
    a_add = None or (A2 [rows, M], k0): rows [k0, k0 + rows) of A are used as A[k] + A2[k - k0] (one fp32 add per
    element); b_add likewise for B.  The sum is formed where the grouped kernel stages its operands
    (hm_gemm_f32_group_tn_add), so the products of two autograd nodes over the same saved rows cost one.  An addend the
    kernel does not take - a range that is no multiple of 4, a non-unit column stride, a problem that runs on the plain
    GEMM (K no multiple of 128, operands of 2 GB) - is added to a copy of its operand beforehand: the same values (and,
    in deterministic mode, the same bits) from the existing paths."""
    if not problems:
        return
    items = (_lib.GemmGroupAddItem * len(problems))()
    keep = []
    for i, (a, b, c, a_add, b_add) in enumerate(problems):
        require_gpu(a, b, c)
        a, b = _rowmajor(a), _rowmajor(b)
        if c.stride(-1) != 1 or a.dtype != torch.float32 or b.dtype != torch.float32 or c.dtype != torch.float32:
            raise ValueError("hashmod gemm_group_tn_add: fp32 row-major operands expected")
        K, M = a.shape
        Kb, N = b.shape
        if K != Kb or tuple(c.shape) != (M, N):
            raise ValueError(f"hashmod gemm_group_tn_add: shapes {tuple(a.shape)}^T @ {tuple(b.shape)} -> {tuple(c.shape)}")
        grouped = _group_tn_takes(K, _ld(a), _ld(b))

        def addend(x, add):
            """(operand, addend or None, ld2, k0, k1): the addend as the kernel takes it, or added beforehand"""
            if add is None or add[0].shape[0] == 0:
                return x, None, 0, 0, 0
            x2, k0 = add
            require_gpu(x2)
            k0, rows = int(k0), x2.shape[0]
            if x2.dtype != torch.float32 or x2.dim() != 2 or x2.shape[1] != x.shape[1] or k0 < 0 or k0 + rows > K:
                raise ValueError(f"hashmod gemm_group_tn_add: addend {tuple(x2.shape)} at row {k0} of {tuple(x.shape)}")
            if grouped and k0 % 4 == 0 and rows % 4 == 0 and x2.stride(1) == 1 and 4 * _ld(x2) * K < 2 ** 31:
                return x, x2, _ld(x2), k0, k0 + rows
            x = x.clone()
            x[k0:k0 + rows] += x2
            return x, None, 0, 0, 0

        a, a2, lda2, a_k0, a_k1 = addend(a, a_add)
        b, b2, ldb2, b_k0, b_k1 = addend(b, b_add)
        keep += [a, b, a2, b2]
        items[i] = _lib.GemmGroupAddItem(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, _ld(a), _ld(b), _ld(c),
                                         dptr(a2), dptr(b2), lda2, ldb2, a_k0, a_k1, b_k0, b_k1)
    dev = problems[0][0]
    if is_deterministic():
        need = check(lib().hm_gemm_f32_group_tn_add_det_workspace_bytes(C.cast(items, C.c_void_p), len(problems)))
        ws, nb = _det_workspace(dev.device, need)
        check(lib().hm_gemm_f32_group_tn_add_det(C.cast(items, C.c_void_p), len(problems), ws, nb, stream_ptr(dev)))
        return
    check(lib().hm_gemm_f32_group_tn_add(C.cast(items, C.c_void_p), len(problems), stream_ptr(dev)))


EPI_SOFTPLUS, EPI_S1MUL, EPI_ADJOINT, EPI_RELU, EPI_RELUMASK = 1, 2, 3, 4, 5


def _rowmajor(t):
    return t if t.stride(-1) == 1 else t.contiguous()


def _ld(t):
    """row stride in elements; torch reports arbitrary strides for size-1 dimensions"""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1], 1)


def gemm_ep(a, b, bias, trans_a, trans_b, mode, beta, thr, scale=1.0, z=None, g=None, nz=None, want_c=True,
            want_out3=False, out1=None, out3=None):
    """GEMM with a fused Softplus epilogue (hm_gemm_f32_ep; include/hashmod.h).  v = (op(a) @ op(b) + bias) * scale.
      EPI_SOFTPLUS -> (v, softplus(v))
      EPI_S1MUL    -> (v or None, v[:, :nz] * s1(z) (+ g))
      EPI_ADJOINT  -> (v * s1(z), v * g * s2(z), g * s1(z) or None)
      EPI_RELU     -> (v or None, max(v, 0));   EPI_RELUMASK -> (v or None, where(z > 0, v, 0)[:, :nz] (+ g))
    Row-major 2-D operands with arbitrary row strides (views of wider tensors are fine); no autograd.
    out1 / out3: optional caller-owned destinations (row slices of larger buffers) for the first / third output."""
    require_gpu(a, b, bias, z, g)
    a, b = _rowmajor(a), _rowmajor(b)
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    Kb, N = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if K != Kb:
        raise ValueError(f"hashmod gemm: inner dimensions differ ({K} vs {Kb})")
    dev = a.device
    _check_gemm_bias(bias, N, dev, "gemm_ep")
    new = lambda cols: torch.empty((M, cols), dtype=torch.float32, device=dev)  # noqa: E731
    ep = _lib.GemmEpilogue()
    ep.mode, ep.scale, ep.beta, ep.threshold = mode, float(scale), float(beta), float(thr)
    c = new(N) if (want_c or mode == EPI_SOFTPLUS) else None
    masked = mode in (EPI_S1MUL, EPI_RELUMASK)
    outs = ()
    def dest(buf, cols):
        if buf is None:
            return new(cols)
        _check_gemm_out(buf, M, cols, dev, "gemm_ep")
        return buf

    if mode in (EPI_SOFTPLUS, EPI_RELU):
        o1 = dest(out1, N)
        outs = (c, o1)
    else:
        z = _rowmajor(z)
        g = _rowmajor(g) if g is not None else None
        ncol = (z.shape[1] if nz is None else nz) if masked else N
        if z.shape[0] != M or z.shape[1] < ncol or (g is not None and (g.shape[0] != M or g.shape[1] < ncol)):
            raise ValueError("hashmod gemm_ep: epilogue operand shape")
        ep.nz = ncol
        ep.z, ep.ldz = z.data_ptr(), _ld(z)
        if g is not None:
            ep.g, ep.ldg = g.data_ptr(), _ld(g)
        o1 = dest(out1, ncol)
        if masked:
            outs = (c, o1)
        else:
            o2 = new(N)
            o3 = dest(out3, N) if (want_out3 or out3 is not None) else None
            ep.out2, ep.ld2 = o2.data_ptr(), _ld(o2)
            if o3 is not None:
                ep.out3, ep.ld3 = o3.data_ptr(), _ld(o3)
            outs = (o1, o2, o3)
    ep.out1, ep.ld1 = o1.data_ptr(), _ld(o1)
    if bias is not None:
        bias = bias.contiguous()
    check(lib().hm_gemm_f32_ep(int(trans_a), int(trans_b), M, N, K, dptr(a), _ld(a), dptr(b), _ld(b), dptr(bias),
                               dptr(c), _ld(c) if c is not None else N, C.byref(ep), stream_ptr(a)))
    return outs


_INPUT_GRAD_ONLY = [False]


class input_grad_only:
    """`with ops.input_grad_only(): torch.autograd.grad(e, x, ..., create_graph=True)` - the caller asks for the gradient
    w.r.t. the POINTS only.  A custom Function cannot see which of its inputs were asked for (needs_input_grad only says
    which require grad), so without this hint every Linear of an embedder also forms its weight / bias gradient in that
    pass (a split-K GEMM, its zeroing launch and a column sum each) just to have it thrown away."""

    def __enter__(self):
        self.prev = _INPUT_GRAD_ONLY[0]
        _INPUT_GRAD_ONLY[0] = True

    def __exit__(self, *exc):
        _INPUT_GRAD_ONLY[0] = self.prev


class _MatMul(torch.autograd.Function):
    """C = op(A) @ op(B) + bias.  backward is expressed with the same op, so autograd can
    differentiate it again (ImplicitNetwork.gradient uses create_graph=True)."""

    @staticmethod
    def forward(ctx, a, b, bias, trans_a, trans_b):
        ctx.ta, ctx.tb = trans_a, trans_b
        ctx.save_for_backward(a, b)
        ctx.has_bias = bias is not None
        ctx.is_param = tuple(isinstance(t, torch.nn.Parameter) for t in (a, b, bias))
        return gemm(a, b, bias, trans_a, trans_b)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        ta, tb = ctx.ta, ctx.tb
        da = db = dbias = None
        # (parameters are leaves: they cannot lie on a path to the points)
        skip = ctx.is_param if (_INPUT_GRAD_ONLY[0] and torch.is_grad_enabled()) else (False, False, False)
        if ctx.needs_input_grad[0] and not skip[0]:
            # dA' = dC B'^T ; stored layout follows ta
            da = matmul(b, dc, None, tb, True) if ta else matmul(dc, b, None, False, not tb)
        if ctx.needs_input_grad[1] and not skip[1]:
            db = matmul(dc, a, None, True, ta) if tb else matmul(a, dc, None, not ta, False)
        if ctx.has_bias and ctx.needs_input_grad[2] and not skip[2]:
            dbias = colsum(dc)
        return da, db, dbias, None, None


def matmul(a, b, bias=None, trans_a=False, trans_b=False):
    return _MatMul.apply(a, b, bias, trans_a, trans_b)


def linear(x, weight, bias=None):
    """x [N,in] @ weight[out,in]^T + bias - nn.Linear on the HIP GEMM, differentiable to any order."""
    return _MatMul.apply(x, weight, bias, False, True)


# =========================================================================================
# fused no-grad SDF forward (csrc/hm_sdf.hip)
# =========================================================================================
def pack_mlp_layer(W, segs, kblock=8):
    """Packed MFMA operand image of one folded layer (layout contract: include/hashmod.h).

    W [out, sum(real segment widths)];  segs = [(src, real_width), ...] with src 1 = embedding,
    0 = previous layer output.  kblock 8: image for the 64-point kernel (32-row tiles, octets);
    kblock 16: image for the 16-point kernel (16-row tiles, 16-wide k blocks).
    Returns (w_packed, n_tiles, seg_blocks, seg_src)."""
    out_dim = W.shape[0]
    n_tiles = (out_dim + 31) // 32
    cols, c0, octs, srcs = [], 0, [], []
    for src, width in segs:
        pad = (-width) % kblock
        blk = W[:, c0:c0 + width]
        if pad:
            blk = torch.nn.functional.pad(blk, (0, pad))
        cols.append(blk)
        octs.append((width + pad) // kblock)
        srcs.append(src)
        c0 += width
    assert c0 == W.shape[1]
    Wp = torch.cat(cols, 1)
    Wp = torch.nn.functional.pad(Wp, (0, 0, 0, n_tiles * 32 - out_dim))
    G = Wp.shape[1] // kblock
    if kblock == 8:   # [u][g][h][i][s]  <- W[32u+i][8g+4h+s]
        Wp = Wp.view(n_tiles, 32, G, 2, 4).permute(0, 2, 3, 1, 4).contiguous()
    else:             # [u][t][q][i][e]  <- W[16u+i][16t+4q+e]
        Wp = Wp.view(n_tiles * 2, 16, G, 4, 4).permute(0, 2, 3, 1, 4).contiguous()
    while len(octs) < 2:
        octs.append(0)
        srcs.append(0)
    return Wp, n_tiles, octs, srcs


SDF_FP32, SDF_BF16, SDF_SPLIT = 0, 1, 2     # kernel families of hm_sdf_net_fits (HM_SDF_*)


class PackedSdf:
    """Device-resident packed weights + the [host] hm_mlp_desc for hm_sdf_fwd.

    The image buffers are allocated once (stable pointers, so the descriptor stays valid across
    optimizer steps and inside captured graphs); update() re-packs them with one launch per image family."""

    def __init__(self, weights, biases, E, skip_in, beta, with_bf16=False, split=None):
        n = len(weights)
        self.has_bf16 = bool(with_bf16)
        self.bf16 = []
        if split not in (None, "bf16x2", "f16x2"):
            raise ValueError("hashmod PackedSdf: split must be None, 'bf16x2' or 'f16x2'")
        self.split = split                  # kind of the (hi, lo) operand images for hm_sdf_fwd_split, or None
        self.split_imgs, self.split_scales = [], []
        self.desc = _lib.MlpDesc()
        self.desc.split_kind = {None: -1, "bf16x2": 0, "f16x2": 1}[split]
        self.desc.n_layers = n
        self.keep, self.segs, self.bufs = [], [], []
        dev = weights[0].device
        prev_out = None
        for l in range(n):
            out_dim = weights[l].shape[0]
            if l == 0:
                w0, w1, srcs = E, 0, (1, 0)
            elif l in skip_in:
                w0, w1, srcs = prev_out, E, (0, 1)
            else:
                w0, w1, srcs = prev_out, 0, (0, 0)
            assert weights[l].shape[1] == w0 + w1
            n_tiles = (out_dim + 31) // 32
            oct0, oct1 = (w0 + 7) // 8, (w1 + 7) // 8
            b0, b1 = (w0 + 15) // 16, (w1 + 15) // 16
            img8 = torch.empty(n_tiles * (oct0 + oct1) * 256, dtype=torch.float32, device=dev)
            img16 = torch.empty(2 * n_tiles * (b0 + b1) * 256, dtype=torch.float32, device=dev)
            bpad = torch.empty(n_tiles * 32, dtype=torch.float32, device=dev)
            self.bufs.append((img8, img16, bpad))
            self.segs.append((out_dim, w0, w1))
            ly = self.desc.layer[l]
            ly.w_packed, ly.bias, ly.w_packed_m16 = img8.data_ptr(), bpad.data_ptr(), img16.data_ptr()
            if with_bf16:    # operand image of hm_sdf_fwd_bf16 (2-byte elements; torch.bfloat16 as the container)
                ib = torch.empty(n_tiles * (b0 + b1) * 512, dtype=torch.bfloat16, device=dev)
                self.bf16.append(ib)
                ly.w_packed_bf16 = ib.data_ptr()
            else:
                ly.w_packed_bf16 = None
            if split is not None:  # [tile][16-block][hi | lo][64 lanes][8] 2-byte elements (int16 as the container)
                isp = torch.empty(n_tiles * (b0 + b1) * 1024, dtype=torch.int16, device=dev)
                self.split_imgs.append(isp)
                ly.w_packed_split = isp.data_ptr()
                # the skip layer consumes cat[x, emb]/sqrt(2): x is divided by the previous layer's epilogue, the
                # embedding segment carries the factor in its weights
                self.split_scales.append((1.0, 1.0 / math.sqrt(2.0)) if l in skip_in else (1.0, 1.0))
            else:
                ly.w_packed_split = None
            ly.out_dim, ly.n_tiles = out_dim, n_tiles
            ly.seg_octets[0], ly.seg_octets[1] = oct0, oct1
            ly.seg_blocks16[0], ly.seg_blocks16[1] = b0, b1
            ly.seg_src[0], ly.seg_src[1] = srcs
            ly.activation = 1 if l < n - 1 else 0
            ly.post_div_sqrt2 = 1 if (l + 1) in skip_in else 0
            prev_out = out_dim
        self.out_dim = prev_out
        self.E = E
        self._fits = {}
        self.update(weights, biases, beta)

    def fits(self, family):
        """whether the fused kernels of `family` (SDF_FP32 / SDF_BF16 / SDF_SPLIT) accept this network: the host-side
        checks of their launches (hm_sdf_net_fits), asked once per family - update() never changes a layer's shape"""
        r = self._fits.get(family)
        if r is None:
            r = self._fits[family] = check(lib().hm_sdf_net_fits(C.byref(self.desc), int(self.E), int(family))) == 1
        return r

    def update(self, weights, biases, beta):
        self.desc.beta = float(beta)
        items = (_lib.PackItem * len(self.bufs))()
        split_items = (_lib.PackSplitItem * len(self.bufs))()
        self.keep = []
        for l, (img8, img16, bpad) in enumerate(self.bufs):
            out_dim, w0, w1 = self.segs[l]
            W = weights[l].detach()
            b = biases[l].detach()
            if W.dtype != torch.float32 or W.stride(-1) != 1:
                W = W.float().contiguous()
            if b.dtype != torch.float32 or not b.is_contiguous():
                b = b.float().contiguous()
            require_gpu(W, b)
            self.keep += [W, b]
            items[l] = _lib.PackItem(W.data_ptr(), b.data_ptr(), img8.data_ptr(), img16.data_ptr(), bpad.data_ptr(),
                                     W.stride(0), out_dim, w0, w1, 0)
            if self.has_bf16:
                check(lib().hm_pack_mlp_layer_bf16(dptr(W), W.stride(0), out_dim, w0, w1, dptr(self.bf16[l]),
                                                   stream_ptr(W)))
            if self.split is not None:
                s0, s1 = self.split_scales[l]
                split_items[l] = _lib.PackSplitItem(W.data_ptr(), self.split_imgs[l].data_ptr(), W.stride(0), out_dim, w0,
                                                    w1, s0, s1, 0)
        # all split images in ONE launch; all fp32 operand images (8-k, 16-k) and padded biases in another
        if self.split is not None:
            check(lib().hm_pack_mlp_layers_split(C.cast(split_items, C.c_void_p), len(self.bufs), self.desc.split_kind,
                                                 stream_ptr(self.bufs[0][0])))
        check(lib().hm_pack_mlp_layers(C.cast(items, C.c_void_p), len(self.bufs), stream_ptr(self.bufs[0][0])))


def sdf_fwd(desc, packed, x, table, B, frac_mode=0, sdf_only=False, max_workgroups=0, tile_points=0, n_dev=None):
    """Fused encode + MLP + clamp.  Returns [N] (sdf_only) or [N, out_dim].
    tile_points 0 = auto (16-point tiles for small batches, 64 otherwise); n_dev = optional device
    int32 tensor holding the live point count (the call is then sync-free for device-compacted work)."""
    x = _prep_x(x)
    require_gpu(x, table, B)
    n = x.shape[0]
    cols = 1 if sdf_only else packed.out_dim
    out = torch.empty((n, cols), dtype=torch.float32, device=x.device)
    check(lib().hm_sdf_fwd(desc.handle, C.byref(packed.desc), dptr(x), n, dptr(table), dptr(B.contiguous()),
                           dptr(out), cols, cols, int(frac_mode), int(tile_points), dptr(n_dev),
                           int(max_workgroups), stream_ptr(x)))
    return out[:, 0] if sdf_only else out


def _sdf_fwd_coarse(name, kind, packed, x, n_dev, run_min, grid=None):
    """sdf-only values [N] from the 16-bit coarse-search kernels (kind "bf16": hm_sdf_fwd_bf16, "split":
    hm_sdf_fwd_split; packed.split names the split kind) on points x with grid = (desc, table, B, frac_mode), or on
    precomputed embedding rows x when grid is None (the _emb_ entry points)"""
    if grid is None:
        require_gpu(x)
        if x.stride(-1) != 1:
            x = x.contiguous()
        n, width = x.shape
    else:
        desc, table, B, frac_mode = grid
        x = _prep_x(x)
        require_gpu(x, table, B)
        n = x.shape[0]
    if not (packed.has_bf16 if kind == "bf16" else packed.split is not None):
        raise ValueError(f"hashmod {name}: the packed weights carry no {kind} image")
    out = torch.empty((n, 1), dtype=torch.float32, device=x.device)
    if grid is None:
        fn = lib().hm_sdf_fwd_emb_bf16 if kind == "bf16" else lib().hm_sdf_fwd_emb_split
        check(fn(C.byref(packed.desc), dptr(x), x.stride(0), width, n, dptr(out), 1, dptr(n_dev), int(run_min),
                 stream_ptr(x)))
    else:
        fn = lib().hm_sdf_fwd_bf16 if kind == "bf16" else lib().hm_sdf_fwd_split
        check(fn(desc.handle, C.byref(packed.desc), dptr(x), n, dptr(table), dptr(B.contiguous()), dptr(out), 1,
                 int(frac_mode), dptr(n_dev), int(run_min), stream_ptr(x)))
    return out[:, 0]


def sdf_fwd_bf16(desc, packed, x, table, B, frac_mode=0, n_dev=None, run_min=0):
    """sdf-only values [N] from the bf16 variant of the fused kernel (hm_sdf_fwd_bf16; coarse-search precision)."""
    return _sdf_fwd_coarse("sdf_fwd_bf16", "bf16", packed, x, n_dev, run_min, (desc, table, B, frac_mode))


def sdf_fwd_split(desc, packed, x, table, B, frac_mode=0, n_dev=None, run_min=0):
    """sdf-only values [N] from the split-operand kernel (hm_sdf_fwd_split; kind = packed.split)."""
    return _sdf_fwd_coarse("sdf_fwd_split", "split", packed, x, n_dev, run_min, (desc, table, B, frac_mode))


def sdf_fwd_emb_split(packed, emb, n_dev=None, run_min=0):
    """the same on precomputed embedding rows (hm_sdf_fwd_emb_split)"""
    return _sdf_fwd_coarse("sdf_fwd_emb_split", "split", packed, emb, n_dev, run_min)


def sdf_fwd_emb_bf16(packed, emb, n_dev=None, run_min=0):
    """sdf_fwd_bf16 on precomputed embedding rows (hm_sdf_fwd_emb_bf16)"""
    return _sdf_fwd_coarse("sdf_fwd_emb_bf16", "bf16", packed, emb, n_dev, run_min)


def sdf_fwd_emb(packed, emb, sdf_only=False, tile_points=0, n_dev=None, max_workgroups=0):
    """The fused MLP + clamp on PRECOMPUTED embedding rows (hm_sdf_fwd_emb): SDF networks whose embedder is not
    the plain hash grid (FourierFilterBanks via nffb_fwd)."""
    require_gpu(emb)
    if emb.stride(-1) != 1:
        emb = emb.contiguous()
    n, width = emb.shape
    cols = 1 if sdf_only else packed.out_dim
    out = torch.empty((n, cols), dtype=torch.float32, device=emb.device)
    check(lib().hm_sdf_fwd_emb(C.byref(packed.desc), dptr(emb), emb.stride(0), width, n, dptr(out), cols, cols,
                               int(tile_points), dptr(n_dev), int(max_workgroups), stream_ptr(emb)))
    return out[:, 0] if sdf_only else out


# =========================================================================================
# fused Fourier-filter-bank embedder forward (csrc/hm_nffb.hip)
# =========================================================================================
class NffbPacked:
    """[host] hm_nffb_desc over the live parameters of a FourierFilterBanks module (no copies: the kernel reads the
    nn.Linear weights in place, so optimizer updates are seen without re-packing)."""

    def __init__(self, mod):
        self.desc = _lib.NffbDesc()
        self.refresh(mod)

    def refresh(self, mod):
        d = self.desc
        L = mod.n_levels
        d.n_levels, d.bound, d.w0, d.style_eps = int(L), float(mod.bound), float(mod.sin_w0), 1e-5
        keep = []
        for l in range(L - 1):
            lin = getattr(mod, "ff_lin" + str(l))
            w, b = lin.weight.detach(), lin.bias.detach()
            require_gpu(w, b)
            if not (w.is_contiguous() and b.is_contiguous() and w.dtype == torch.float32):
                raise ValueError("hashmod nffb: contiguous fp32 parameters expected")
            d.trunk_w[l], d.trunk_b[l] = w.data_ptr(), b.data_ptr()
            keep += [w, b]
        d.out_w, d.out_b = mod.out_layer.weight.data_ptr(), mod.out_layer.bias.data_ptr()
        if mod.modulationApplied:
            lt = mod.StyleAttentionBlock.linear_transform
            d.style_w, d.style_b = lt.weight.data_ptr(), lt.bias.data_ptr()
            d.style_eps = float(mod.StyleAttentionBlock.eps)
        else:
            d.style_w, d.style_b = None, None
        self.key = tuple(t.data_ptr() for t in keep)


def nffb_packed(mod):
    """the module's hm_nffb_desc, pointers refreshed (parameters may have been moved / re-bound since the last call)"""
    pk = mod.__dict__.get("_nffb_packed")
    if pk is None:
        pk = mod.__dict__["_nffb_packed"] = NffbPacked(mod)
    else:
        pk.refresh(mod)
    return pk


def nffb_fwd(mod, x, n_dev=None, out=None):
    """[N, 3 + 8 + 8L] embedding of a FourierFilterBanks module in one kernel (no autograd)."""
    x = _prep_x(x)
    grid = mod.grid_enc
    n = x.shape[0]
    width = mod.embeddings_dim
    # the kernel writes n rows of `width` fp32 values through raw pointers and reads one int32 count: whatever it cannot
    # address as such is rejected here, before anything is enqueued
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.dim() == 2):
            raise ValueError("hashmod nffb_fwd: out must be a 2-D float32 tensor")
        if out.shape[0] < n or out.shape[1] < width:
            raise ValueError(f"hashmod nffb_fwd: out {tuple(out.shape)} is smaller than [{n}, {width}]")
        if out.stride(1) != 1 or out.stride(0) < width:
            raise ValueError(f"hashmod nffb_fwd: out needs unit column stride and a row stride of at least {width}, "
                             f"got strides {tuple(out.stride())}")
        if out.device != x.device:
            raise ValueError(f"hashmod nffb_fwd: out is on {out.device}, the points on {x.device}")
    if n_dev is not None:
        if not (isinstance(n_dev, torch.Tensor) and n_dev.dtype == torch.int32 and n_dev.numel() >= 1):
            raise ValueError("hashmod nffb_fwd: n_dev must be an int32 tensor holding the live point count")
        if n_dev.device != x.device:
            raise ValueError(f"hashmod nffb_fwd: n_dev is on {n_dev.device}, the points on {x.device}")
    require_gpu(x, grid.table)
    if out is None:
        out = torch.empty((n, width), dtype=torch.float32, device=x.device)
    pk = nffb_packed(mod)
    check(lib().hm_nffb_fwd(grid.desc.handle, C.byref(pk.desc), dptr(x), n, dptr(grid.table.detach()),
                            dptr(grid.freq_encoding.B), dptr(out), out.stride(0), FRAC_MODES[grid.frac_mode],
                            dptr(n_dev), stream_ptr(x)))
    return out


# =========================================================================================
# sync-free ray tracer (csrc/hm_trace.hip)
# =========================================================================================
def trace_workspace_bytes(n_rays, cfg, nffb_levels=0):
    if nffb_levels:
        return check(lib().hm_trace_workspace_bytes_nffb(int(n_rays), C.byref(cfg), int(nffb_levels)))
    return check(lib().hm_trace_workspace_bytes(int(n_rays), C.byref(cfg)))


def trace_guard_clear(workspace):
    """zeroes the tracer workspace's persistent header: the sticky word of the guarded coarse scans (no host sync)"""
    require_gpu(workspace)
    check(lib().hm_trace_guard_clear(dptr(workspace), workspace.numel(), stream_ptr(workspace)))


def trace_guard_tolerances():
    """(tau, tau_trip) of the guarded coarse scans (csrc/hm_trace_dev.h: kGuardTau, kGuardTrip)"""
    tau, trip = C.c_float(), C.c_float()
    check(lib().hm_trace_guard_tolerances(C.byref(tau), C.byref(trip)))
    return tau.value, trip.value


TRACE_GUARD_TRIPPED = 0x47554152    # the sticky word's value once the guard's monitor has tripped (kGuardTripped)


def camera_rays(uv, pose, intrinsics, radius):
    """(ray_dirs [B,N,3], cam_loc [B,3], t_sphere [B,N,2], hit [B,N] bool) of fixed 4x4 cameras in one launch
    (hm_camera_rays: rend_util.get_camera_params + get_sphere_intersection; no gradient)."""
    require_gpu(uv, pose, intrinsics)
    Bn, N = int(uv.shape[0]), int(uv.shape[1])
    if tuple(pose.shape[1:]) != (4, 4) or tuple(intrinsics.shape[1:]) != (4, 4):
        raise ValueError("hashmod camera_rays: pose and intrinsics must be [B,4,4]")
    uv_c, pose_c, k_c = uv.detach().float().contiguous(), pose.detach().float().contiguous(), intrinsics.detach().float().contiguous()
    dev = uv.device
    dirs = torch.empty((Bn, N, 3), dtype=torch.float32, device=dev)
    cam = torch.empty((Bn, 3), dtype=torch.float32, device=dev)
    t = torch.empty((Bn, N, 2), dtype=torch.float32, device=dev)
    hit = torch.empty((Bn, N), dtype=torch.uint8, device=dev)
    check(lib().hm_camera_rays(dptr(uv_c), dptr(pose_c), dptr(k_c), Bn, N, float(radius), dptr(dirs), dptr(cam), dptr(t),
                               dptr(hit), stream_ptr(uv_c)))
    return dirs, cam, t, hit.bool()


def trace_forward(desc, packed, table, B, frac_mode, tile_points, cfg, cam_loc, ray_dirs, object_mask, t_sphere,
                  hit_mask, rays_per_image, sampler_fracs, steps_u, workspace, stats=None, nffb=None):
    """Enqueues the whole intersection search (no host sync).  Returns (points, net_mask_u8, dists).
    nffb: NffbPacked of a FourierFilterBanks embedder (desc / table / B are then its hash grid's)."""
    require_gpu(cam_loc, ray_dirs, object_mask, t_sphere, hit_mask, sampler_fracs, workspace)
    n = ray_dirs.shape[0]
    dev = ray_dirs.device
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((n,), dtype=torch.uint8, device=dev)
    dists = torch.empty((n,), dtype=torch.float32, device=dev)
    tail = (dptr(table), dptr(B), int(frac_mode), int(tile_points), C.byref(cfg), dptr(cam_loc), dptr(ray_dirs),
            dptr(object_mask), dptr(t_sphere), dptr(hit_mask), n, int(rays_per_image), dptr(sampler_fracs),
            dptr(steps_u), dptr(pts), dptr(mask), dptr(dists), dptr(workspace), workspace.numel(), dptr(stats),
            stream_ptr(ray_dirs))
    if nffb is not None:
        check(lib().hm_trace_forward_nffb(desc.handle, C.byref(nffb.desc), C.byref(packed.desc), *tail))
    else:
        check(lib().hm_trace_forward(desc.handle, C.byref(packed.desc), *tail))
    return pts, mask, dists


# =========================================================================================
# fused elementwise passes (csrc/hm_elem.hip)
# =========================================================================================
class _ColSum(torch.autograd.Function):
    """sum over rows (bias gradient) in one pass; its backward is a broadcast."""

    @staticmethod
    def forward(ctx, x):
        ctx.rows = x.shape[0]
        if x.stride(-1) != 1:
            x = x.contiguous()
        out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
        if is_deterministic():
            ws, nb = _det_workspace(x.device, check(lib().hm_colsum_det_workspace_bytes(x.shape[0], x.shape[1])))
            check(lib().hm_colsum_det(dptr(x), x.shape[0], x.shape[1], max(x.stride(0), 1), dptr(out), ws, nb,
                                      stream_ptr(x)))
            return out
        check(lib().hm_colsum(dptr(x), x.shape[0], x.shape[1], max(x.stride(0), 1), dptr(out), stream_ptr(x)))
        return out

    @staticmethod
    def backward(ctx, g):
        return g.unsqueeze(0).expand(ctx.rows, -1)


def colsum(x):
    require_gpu(x)
    return _ColSum.apply(x)


def sdf_head_fwd(zl, beta_rho):
    """(out, sdf, c, denom) of the soft SDF clamp (hm_sdf_head; no autograd)."""
    require_gpu(zl)
    zl = zl.contiguous()
    n, cols = zl.shape
    out = torch.empty_like(zl)
    sdf, c, denom = (torch.empty(n, dtype=torch.float32, device=zl.device) for _ in range(3))
    check(lib().hm_sdf_head(0, dptr(zl), n, cols, float(beta_rho), dptr(out), dptr(sdf), dptr(c), dptr(denom),
                            None, stream_ptr(zl)))
    return out, sdf, c, denom


def sdf_head_bwd(d_out, sdf, c, denom, cb=None):
    """z-bar of the last layer from d_out (and the gradient sweep's c-bar, if any)."""
    require_gpu(d_out, cb)
    d_out = d_out.contiguous()
    n, cols = d_out.shape
    zb = torch.empty_like(d_out)
    cbp = cb.contiguous() if cb is not None else None
    check(lib().hm_sdf_head(1, dptr(d_out), n, cols, 1.0, dptr(zb), dptr(sdf), dptr(c), dptr(denom), dptr(cbp),
                            stream_ptr(d_out)))
    return zb


def dcopy_(dst, src):
    """dst.copy_(src) for 2-D (or 1-D) fp32 row-major tensors as a KERNEL launch (hm_copy2d_f32).  torch copies
    contiguous tensors with hipMemcpyAsync, which a graph capture records as a MEMCPY node."""
    require_gpu(dst, src)
    if dst.shape != src.shape or dst.dtype != torch.float32 or src.dtype != torch.float32:
        raise ValueError("hashmod dcopy_: shape / dtype mismatch")
    d2 = dst if dst.dim() == 2 else dst.reshape(1, -1) if dst.is_contiguous() else None
    s2 = src if src.dim() == 2 else src.reshape(1, -1) if src.is_contiguous() else None
    if d2 is None or s2 is None or d2.stride(-1) != 1 or s2.stride(-1) != 1:
        raise ValueError("hashmod dcopy_: row-major 2-D (or contiguous) tensors only")
    rows, cols = d2.shape
    check(lib().hm_copy2d_f32(dptr(d2), _ld(d2), dptr(s2), _ld(s2), rows, cols, stream_ptr(dst)))
    return dst


class _TakeBlock(torch.autograd.Function):
    """y = x[r0:r0+nr, c0:c0+nc] as a fresh contiguous tensor.  Plain slicing is a view whose autograd backward
    (SliceBackward: zeros + narrow().copy_()) copies contiguous rows with hipMemcpyAsync, i.e. a MEMCPY node in a
    captured graph; here both directions are kernel copies (hm_copy2d_f32).  Differentiable to any order."""

    @staticmethod
    def forward(ctx, x, r0, nr, c0, nc):
        ctx.box = (x.shape, r0, nr, c0, nc)
        y = torch.empty((nr, nc), dtype=torch.float32, device=x.device)
        return dcopy_(y, x[r0:r0 + nr, c0:c0 + nc])

    @staticmethod
    def backward(ctx, dy):
        shape, r0, nr, c0, nc = ctx.box
        return _PutBlock.apply(dy, shape, r0, nr, c0, nc), None, None, None, None


class _PutBlock(torch.autograd.Function):
    """zeros(shape) with dy written at [r0:r0+nr, c0:c0+nc] (the adjoint of _TakeBlock)."""

    @staticmethod
    def forward(ctx, dy, shape, r0, nr, c0, nc):
        ctx.box = (r0, nr, c0, nc)
        dx = torch.zeros(shape, dtype=torch.float32, device=dy.device)      # fill kernel
        dcopy_(dx[r0:r0 + nr, c0:c0 + nc], dy if dy.stride(-1) == 1 else dy.contiguous())
        return dx

    @staticmethod
    def backward(ctx, ddx):
        r0, nr, c0, nc = ctx.box
        return _TakeBlock.apply(ddx, r0, nr, c0, nc), None, None, None, None, None


def take_block(x, r0, nr, c0=0, nc=None):
    """x[r0:r0+nr, c0:c0+nc] of a 2-D fp32 tensor as a new tensor, with kernel copies in forward and backward."""
    require_gpu(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("hashmod take_block: 2-D fp32 tensor expected")
    if x.stride(-1) != 1:
        x = x.contiguous()
    nc = x.shape[1] - c0 if nc is None else nc
    return _TakeBlock.apply(x, int(r0), int(nr), int(c0), int(nc))


def cat_rows_(dst, parts, dim):
    """torch.cat(parts, dim, out=dst) for 2-D fp32 tensors through dcopy_ (no MEMCPY graph nodes)."""
    o = 0
    for t in parts:
        n = t.shape[dim]
        dcopy_(dst.narrow(dim, o, n), t if t.stride(-1) == 1 else t.contiguous())
        o += n
    return dst


def colsum_into(x, out):
    """out += column sums of x (no autograd; `out` zeroed by the caller)."""
    require_gpu(x, out)
    x = _rowmajor(x)
    if is_deterministic():
        ws, nb = _det_workspace(x.device, check(lib().hm_colsum_det_workspace_bytes(x.shape[0], x.shape[1])))
        check(lib().hm_colsum_acc_det(dptr(x), x.shape[0], x.shape[1], _ld(x), dptr(out), ws, nb, stream_ptr(x)))
        return out
    check(lib().hm_colsum_acc(dptr(x), x.shape[0], x.shape[1], _ld(x), dptr(out), stream_ptr(x)))
    return out


def colsum_into_multi(pairs):
    """out += column sums of x for every (x, out) of `pairs` in ONE launch (hm_colsum_acc_multi)."""
    if not pairs:
        return
    items = (_lib.ColsumItem * len(pairs))()
    keep = []
    for i, (x, out) in enumerate(pairs):
        require_gpu(x, out)
        x = _rowmajor(x)
        keep.append(x)
        items[i] = _lib.ColsumItem(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _ld(x))
    if is_deterministic():
        need = check(lib().hm_colsum_acc_multi_det_workspace_bytes(C.cast(items, C.c_void_p), len(pairs)))
        ws, nb = _det_workspace(pairs[0][0].device, need)
        check(lib().hm_colsum_acc_multi_det(C.cast(items, C.c_void_p), len(pairs), ws, nb, stream_ptr(pairs[0][0])))
        return
    check(lib().hm_colsum_acc_multi(C.cast(items, C.c_void_p), len(pairs), stream_ptr(pairs[0][0])))


def _twice_differentiable(name, call, prep, doc):
    """The autograd node of y = f(x; *params), differentiable twice, over ONE kernel entry call(order, x, gy, gg, *params)
    -> (out0, out1): order 0 gives y, order 1 gx = J(x)^T gy, order 2 (d_gy, d_x) of gx for its cotangent gg.  prep puts
    x and gy into the layout the kernel reads.  Returns the forward node; its backward is the node `name`Bwd."""

    def bwd_forward(ctx, x, gy, *params):
        gy = prep(gy)
        ctx.params = params
        ctx.save_for_backward(x, gy)
        return call(1, x, gy, None, *params)[0]

    @torch.autograd.function.once_differentiable
    def bwd_backward(ctx, gg):
        x, gy = ctx.saved_tensors
        d_gy, d_x = call(2, x, gy, gg.contiguous(), *ctx.params)
        return (d_x, d_gy) + (None,) * len(ctx.params)

    bwd = type(name + "Bwd", (torch.autograd.Function,),
               {"forward": staticmethod(bwd_forward), "backward": staticmethod(bwd_backward)})

    def forward(ctx, x, *params):
        x = prep(x)
        ctx.params = params
        ctx.save_for_backward(x)
        return call(0, x, None, None, *params)[0]

    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return (bwd.apply(x, gy, *ctx.params),) + (None,) * len(ctx.params)

    return type(name, (torch.autograd.Function,),
                {"__doc__": doc, "forward": staticmethod(forward), "backward": staticmethod(backward)})


def _softplus_call(order, z, gy, gg, beta, thr):
    n = z.numel()
    out0 = torch.empty_like(z)
    out1 = torch.empty_like(z) if order == 2 else None
    check(lib().hm_softplus(order, dptr(z), dptr(gy), dptr(gg), dptr(out0), dptr(out1), n, float(beta), float(thr),
                            stream_ptr(z)))
    return out0, out1


_Softplus = _twice_differentiable(
    "_Softplus", _softplus_call, torch.Tensor.contiguous,
    "nn.Softplus(beta, threshold); gz = gy * s1(z) is differentiable once more (d/dgy and d/dz in one fused pass).")


def _sine_call(order, x, gy, gg, w0):
    out0 = torch.empty_like(x)
    out1 = torch.empty_like(x) if order == 2 else None
    check(lib().hm_sine(order, dptr(x), dptr(gy), dptr(gg), dptr(out0), dptr(out1), x.numel(), float(w0), stream_ptr(x)))
    return out0, out1


_Sine = _twice_differentiable(
    "_Sine", _sine_call, torch.Tensor.contiguous,
    "sin(w0 x) (SIREN activation) with one-kernel backward and double backward (csrc/hm_elem.hip).")


def sine(x, w0):
    """sin(w0 * x), differentiable twice (third order is not provided)."""
    require_gpu(x)
    return _Sine.apply(x, float(w0))


class _WeightNormFold(torch.autograd.Function):
    """W_l = g_l * v_l / ||v_l||_row for a LIST of weight-normed layers: one launch forward, one backward
    (torch._weight_norm is one launch per layer and pass)."""

    @staticmethod
    def forward(ctx, *vg):
        L = len(vg) // 2
        vs = [t.contiguous() for t in vg[:L]]
        gs = [t.contiguous() for t in vg[L:]]
        ws = [torch.empty_like(v) for v in vs]
        norms = [torch.empty(v.shape[0], dtype=torch.float32, device=v.device) for v in vs]
        tab = (_lib.WnLayer * L)()
        for i in range(L):
            tab[i].v, tab[i].g, tab[i].w, tab[i].norm = vs[i].data_ptr(), gs[i].data_ptr(), ws[i].data_ptr(), norms[i].data_ptr()
            tab[i].rows, tab[i].cols = vs[i].shape[0], vs[i].shape[1]
        check(lib().hm_weight_norm_multi(0, L, C.cast(tab, C.c_void_p), stream_ptr(vs[0])))
        ctx.L = L
        ctx.save_for_backward(*vs, *gs, *norms)
        return tuple(ws)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gws):
        L = ctx.L
        sv = ctx.saved_tensors
        vs, gs, norms = sv[:L], sv[L:2 * L], sv[2 * L:]
        idx = [i for i in range(L) if gws[i] is not None]
        gv = [None] * L
        gg = [None] * L
        if idx:
            keep = []
            tab = (_lib.WnLayer * len(idx))()
            for k, i in enumerate(idx):
                gw = gws[i].contiguous()
                keep.append(gw)
                gv[i] = torch.empty_like(vs[i])
                gg[i] = torch.empty_like(gs[i])
                tab[k].v, tab[k].g, tab[k].norm = vs[i].data_ptr(), gs[i].data_ptr(), norms[i].data_ptr()
                tab[k].grad_w, tab[k].grad_v, tab[k].grad_g = gw.data_ptr(), gv[i].data_ptr(), gg[i].data_ptr()
                tab[k].rows, tab[k].cols = vs[i].shape[0], vs[i].shape[1]
            check(lib().hm_weight_norm_multi(1, len(idx), C.cast(tab, C.c_void_p), stream_ptr(vs[0])))
        return (*gv, *gg)


def weight_norm_fold(vs, gs):
    """[g * v / ||v||_row for (v, g) in zip(vs, gs)] (g of shape [rows, 1] or [rows]) - differentiable once."""
    require_gpu(*vs)
    return list(_WeightNormFold.apply(*vs, *[g.reshape(-1) for g in gs]))


def _rownorm_call(order, y, g, gg, eps):
    out0 = torch.empty_like(y)
    out1 = torch.empty_like(y) if order == 2 else None
    check(lib().hm_rownorm(order, dptr(y), dptr(g), dptr(gg), dptr(out0), dptr(out1), y.shape[0], y.shape[1], float(eps),
                           stream_ptr(y)))
    return out0, out1


_RowNorm = _twice_differentiable(
    "_RowNorm", _rownorm_call, torch.Tensor.contiguous,
    "(y - mean) / sqrt(var + eps) per row with one-kernel backward and double backward (csrc/hm_elem.hip).")


def rownorm(y, eps=1e-5):
    """per-row normalisation of a [N, W] tensor (biased variance), differentiable twice."""
    require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("hashmod rownorm: [N, W] fp32 input")
    return _RowNorm.apply(y, float(eps))


def _posenc_call(order, c, g, gg, freqs):
    n, D = c.shape
    W = 2 * D + 2 * len(freqs) * D
    fa = (C.c_float * len(freqs))(*freqs)
    out0 = torch.empty((n, D if order == 1 else W), dtype=torch.float32, device=c.device)
    out1 = torch.empty((n, D), dtype=torch.float32, device=c.device) if order == 2 else None
    check(lib().hm_posenc(order, C.cast(fa, C.c_void_p), len(freqs), D, dptr(c), _ld(c), dptr(g),
                          _ld(g) if g is not None else 0, dptr(gg), dptr(out0), out0.stride(0), dptr(out1), n,
                          stream_ptr(c)))
    return out0, out1


_PosEnc = _twice_differentiable(
    "_PosEnc", _posenc_call, _rowmajor,
    "[c | c | sin(f0 c) | cos(f0 c) | ...] (NeRF positional encoding as the reference builds it with include_input) "
    "with one-kernel backward and double backward (csrc/hm_elem.hip).")


def posenc(c, freqs):
    """NeRF positional encoding rows (include_input form of the reference), differentiable twice."""
    require_gpu(c)
    if c.dim() != 2 or c.dtype != torch.float32:
        raise ValueError("hashmod posenc: [N, D] fp32 input")
    return _PosEnc.apply(c, tuple(float(f) for f in freqs))


def softplus(z, beta=100.0, threshold=20.0):
    """nn.Softplus(beta, threshold) with fused backward and double backward (third order is not provided)."""
    require_gpu(z)
    return _Softplus.apply(z, float(beta), float(threshold))


# =========================================================================================
# mesh extraction (csrc/hm_mesh.hip)
# =========================================================================================
def marching_cubes(volume, level=0.0, spacing=(1.0, 1.0, 1.0)):
    """(verts [V,3] fp32, faces [F,3] int32, normals [V,3] fp32) of the `level` isosurface of a device fp32 volume
    [nx, ny, nz] - skimage.measure.marching_cubes(volume, level, spacing) as plots.py:122-128 calls it, with the
    normals pointing toward increasing values (the reference's -normals) and the triangulation of the generated case
    table (csrc/hm_mc_table.h).  Any element strides (the transposed meshgrid view of sdf_volume needs no copy).
    One host read of the counts between the two phases; not graph-capturable.  Empty outputs when nothing crosses."""
    require_gpu(volume)
    if volume.dtype != torch.float32 or volume.dim() != 3:
        raise ValueError("hashmod marching_cubes: a 3-D fp32 volume expected")
    nx, ny, nz = (int(s) for s in volume.shape)
    sx, sy, sz = (int(s) for s in volume.stride())
    dev = volume.device
    L = lib()
    ws = torch.empty(check(L.hm_mc_workspace_bytes(nx, ny, nz)), dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    st = stream_ptr(volume)
    args = (dptr(volume), nx, ny, nz, sx, sy, sz, float(level))
    check(L.hm_mc_count(*args, dptr(ws), ws.numel(), dptr(counts), st))
    n_verts, n_faces, has_nan = counts.tolist()
    if has_nan:
        raise _lib.HashmodError("hashmod marching_cubes: the volume contains NaN")
    verts = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    if n_verts > 0:
        sp = (C.c_float * 3)(*(float(s) for s in spacing))
        check(L.hm_mc_emit(*args, sp, dptr(ws), ws.numel(), n_verts, n_faces, dptr(verts), dptr(normals), dptr(faces),
                           st))
    return verts, faces, normals


# =========================================================================================
# brick-sparse mesh extraction (csrc/hm_mesh_sparse.hip)
# =========================================================================================
_BRICK = 8
_BRICK_POINTS = _BRICK ** 3
_MCS_MAX_LIST = 1 << 22


def _lattice_args(axes, rot, shift):
    """(device fp32 axis tensors, their lengths, the [host] transform of hm_mcs_points_* or None)"""
    dev = next((a.device for a in axes if torch.is_tensor(a) and a.is_cuda), torch.device("cuda"))
    ax = [torch.as_tensor(a, dtype=torch.float32, device=dev).reshape(-1).contiguous() for a in axes]
    if len(ax) != 3:
        raise ValueError("hashmod lattice: three coordinate arrays expected")
    xform = None
    if rot is not None or shift is not None:
        r = torch.eye(3) if rot is None else torch.as_tensor(rot).detach().reshape(3, 3)
        s = torch.zeros(3) if shift is None else torch.as_tensor(shift).detach().reshape(3)
        xform = (C.c_float * 12)(*torch.cat([r.reshape(9).float().cpu(), s.float().cpu()]).tolist())
    return ax, tuple(int(a.numel()) for a in ax), xform


def lattice_points(axes, q, rot=None, shift=None):
    """Coordinates [n, 3] fp32 of the lattice points with linear indices q (int64, (i*ny + j)*nz + k) of the lattice
    axes[0] x axes[1] x axes[2], taken to p @ rot + shift when either is given.  The generator of
    marching_cubes_sparse: one fixed fp32 expression per point, so a point's coordinates depend on its index alone."""
    ax, (nx, ny, nz), xform = _lattice_args(axes, rot, shift)
    q = torch.as_tensor(q, dtype=torch.int64, device=ax[0].device).reshape(-1).contiguous()
    out = torch.empty((q.numel(), 3), dtype=torch.float32, device=q.device)
    check(lib().hm_mcs_points_index(dptr(q), q.numel(), dptr(ax[0]), dptr(ax[1]), dptr(ax[2]), nx, ny, nz, xform,
                                    dptr(out), stream_ptr(out)))
    return out


def _grow(grid, below, above):
    """the bool brick grid OR-ed with itself moved one brick down (below) / up (above) along every axis in turn"""
    for a in range(3):
        n = grid.shape[a]
        out = grid.clone()
        if below and n > 1:
            out.narrow(a, 0, n - 1).logical_or_(grid.narrow(a, 1, n - 1))
        if above and n > 1:
            out.narrow(a, 1, n - 1).logical_or_(grid.narrow(a, 0, n - 1))
        grid = out
    return grid


def _listed(grid, count):
    """the int32 ids of the `count` set bricks of a bool brick grid, ascending (count was read by the caller)"""
    return torch.nonzero_static(grid.reshape(-1), size=count).reshape(-1).to(torch.int32)


@torch.no_grad()
def marching_cubes_sparse(sdf, axes, spacing, seeds, level=0.0, rot=None, shift=None, chunk=1 << 22,
                          return_stats=False):
    """ops.marching_cubes of the volume sdf(lattice_points(axes, every index, rot, shift)) without evaluating that
    volume: (verts, faces, normals[, stats]), bit for bit the dense call's outputs if every component of the level set
    meets a brick that holds a seed, or one of its 26 neighbours.  A component that is not reached is absent as a whole.

    The lattice is split into 8^3-point bricks (csrc/hm_mesh_sparse.hip).  From the seed bricks, a brick whose cell
    block has values on both sides of `level` is a surface brick, and every block face of it with both signs makes the
    brick across it a candidate of the next round; a round evaluates what its candidates' cell blocks need and costs
    one host read.  Then the 27-neighbourhoods of the surface bricks are evaluated (cell corners and the +-1 points of
    the normals) and the marching-cubes kernels run over the surface bricks.  No bound on the SDF's slope is assumed.

    sdf: callable [n, 3] -> [n] fp32 whose value at a point does not depend on the batch it arrives in (for
    ImplicitNetwork.sdf: a fixed tile_points); axes: three ascending coordinate arrays; seeds: [S, 3] in the frame of
    the axes (before rot / shift), those outside the lattice are ignored; new bricks go to sdf in batches of at most
    `chunk` points.  NaN in an evaluated value raises HashmodError.  stats: bricks_evaluated, surface_bricks, points
    (handed to sdf), rounds, sdf_calls, lattice_points."""
    L = lib()
    ax, (nx, ny, nz), xform = _lattice_args(axes, rot, shift)
    dev = ax[0].device
    bdim = tuple(-(-n // _BRICK) for n in (nx, ny, nz))
    n_bricks = bdim[0] * bdim[1] * bdim[2]
    if min(nx, ny, nz) < 2:
        raise ValueError("hashmod marching_cubes_sparse: every lattice dimension must be >= 2")
    if n_bricks >= 1 << 31:
        raise ValueError("hashmod marching_cubes_sparse: the brick map must have fewer than 2^31 entries")
    st = stream_ptr(ax[0])
    level = float(level)
    map_g = torch.full(bdim, -1, dtype=torch.int32, device=dev)
    decided = torch.zeros(n_bricks, dtype=torch.bool, device=dev)
    surface = torch.zeros(n_bricks, dtype=torch.bool, device=dev)
    bad = torch.zeros(2, dtype=torch.bool, device=dev)          # a NaN / an undecidable status seen so far
    state = {"pool": torch.empty((256, _BRICK_POINTS), dtype=torch.float32, device=dev), "slots": 0, "points": 0,
             "calls": 0}

    def lattice():
        return C.byref(_lib.McsLattice(nx, ny, nz, state["slots"], map_g.data_ptr(), state["pool"].data_ptr()))

    def evaluate(ids):
        n, pool, first = ids.numel(), state["pool"], state["slots"]
        if first + n > pool.shape[0]:
            pool = torch.empty((max(2 * pool.shape[0], first + n), _BRICK_POINTS), dtype=torch.float32, device=dev)
            pool[:first] = state["pool"][:first]
            state["pool"] = pool
        per = min(max(1, int(chunk) // _BRICK_POINTS), _MCS_MAX_LIST)
        for s in range(0, n, per):
            part = ids[s:s + per]
            pts = torch.empty((part.numel() * _BRICK_POINTS, 3), dtype=torch.float32, device=dev)
            check(L.hm_mcs_points_bricks(dptr(part), part.numel(), dptr(ax[0]), dptr(ax[1]), dptr(ax[2]), nx, ny, nz,
                                         xform, dptr(pts), st))
            pool[first + s:first + s + part.numel()].view(-1).copy_(sdf(pts).reshape(-1))
            state["points"] += pts.shape[0]
            state["calls"] += 1
        map_g.view(-1)[ids.long()] = torch.arange(first, first + n, dtype=torch.int32, device=dev)
        state["slots"] = first + n

    def status_of(ids):
        out = torch.empty(ids.numel(), dtype=torch.int32, device=dev)
        for s in range(0, ids.numel(), _MCS_MAX_LIST):
            part = ids[s:s + _MCS_MAX_LIST]
            check(L.hm_mcs_status(dptr(part), part.numel(), lattice(), level, dptr(out[s:]), st))
        return out

    def check_bad(nan, undecided):
        if nan:
            raise _lib.HashmodError("hashmod marching_cubes_sparse: the SDF returned NaN")
        if undecided:
            raise _lib.HashmodError("hashmod marching_cubes_sparse: a candidate brick's cell block was not evaluated")

    # seed bricks and their 26 neighbours
    pts = torch.as_tensor(seeds, dtype=torch.float32, device=dev).reshape(-1, 3)
    inside = torch.ones(pts.shape[0], dtype=torch.bool, device=dev)
    brick = torch.zeros(pts.shape[0], dtype=torch.int64, device=dev)
    for a, n in enumerate((nx, ny, nz)):
        c = pts[:, a].contiguous()
        inside &= (c >= ax[a][0]) & (c <= ax[a][-1])
        brick = brick * bdim[a] + (torch.searchsorted(ax[a], c, right=True) - 1).clamp_(0, n - 1) // _BRICK
    seeded = torch.zeros(n_bricks + 1, dtype=torch.bool, device=dev)
    seeded[torch.where(inside, brick, n_bricks)] = True
    cand = _grow(seeded[:n_bricks].view(bdim), 1, 1)

    rounds = n_decided = 0
    strides = (bdim[1] * bdim[2], bdim[2], 1)
    while True:
        want = _grow(cand, 0, 1) & (map_g < 0)               # the candidates' cell blocks: they and their upper neighbours
        n_c, n_w, nan, und = torch.stack([cand.sum(), want.sum(), *bad.long()]).tolist()    # the round's host read
        check_bad(nan, und)
        if n_c == 0:
            break
        rounds += 1
        n_decided += n_c
        ids = _listed(cand, n_c)
        if n_w:
            evaluate(_listed(want, n_w))
        status = status_of(ids)
        idl = ids.long()
        decided[idl] = True
        surface[idl] = (status & 1) != 0
        bad |= torch.stack([(status & 128).any(), (status & 256).any()])
        nxt = torch.zeros(n_bricks, dtype=torch.bool, device=dev)
        for f in range(6):
            step = strides[f // 2] * (1 if f & 1 else -1)
            nxt[idl + step * ((status & (2 << f)) != 0)] = True     # no such face: the brick itself, which is decided
        cand = (nxt & ~decided).view(bdim)

    # halo: the 27-neighbourhood of every surface brick
    halo = _grow(surface.view(bdim), 1, 1) & (map_g < 0)
    n_h, n_s = torch.stack([halo.sum(), surface.sum()]).tolist()
    if n_h:
        evaluate(_listed(halo, n_h))
    n_rest = state["slots"] - n_decided                          # evaluated, never a candidate: only their NaN bit
    if n_rest:
        bad[0] |= (status_of(_listed((map_g.view(-1) >= 0) & ~decided, n_rest)) & 128).any()
    stats = {"bricks_evaluated": state["slots"], "surface_bricks": n_s, "points": state["points"], "rounds": rounds,
             "sdf_calls": state["calls"], "lattice_points": nx * ny * nz}
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    if n_s:
        ids = _listed(surface, n_s)
        list_pos = torch.full((n_bricks,), -1, dtype=torch.int32, device=dev)
        list_pos[ids.long()] = torch.arange(n_s, dtype=torch.int32, device=dev)
        ws = torch.empty(check(L.hm_mcs_workspace_bytes(n_s)), dtype=torch.uint8, device=dev)
        check(L.hm_mcs_count(dptr(ids), n_s, lattice(), level, dptr(ws), ws.numel(), dptr(counts), st))
    n_verts, n_faces, has_nan, rest_nan, n_mapped = torch.cat([counts, bad[:1].long(),
                                                               (map_g >= 0).sum().reshape(1)]).tolist()
    check_bad(has_nan or rest_nan, False)
    if n_mapped != state["slots"]:
        raise _lib.HashmodError("hashmod marching_cubes_sparse: a brick was evaluated twice")
    verts = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    if n_verts > 0:
        vkeys = torch.empty(n_verts, dtype=torch.int64, device=dev)
        fkeys = torch.empty(n_faces, dtype=torch.int64, device=dev)
        sp = (C.c_float * 3)(*(float(s) for s in spacing))
        check(L.hm_mcs_emit(dptr(ids), n_s, lattice(), dptr(list_pos), level, sp, dptr(ws), ws.numel(), n_verts,
                            n_faces, dptr(verts), dptr(normals), dptr(faces), dptr(vkeys), dptr(fkeys), st))
        if n_faces and int(faces.min()) < 0:
            raise _lib.HashmodError("hashmod marching_cubes_sparse: a face refers to a brick that was not reached")
        # the dense kernel's order: vertices by (owning point, axis), faces by (cell, table order)
        order = torch.sort(vkeys)[1]
        verts, normals = verts[order], normals[order]
        new_id = torch.empty(n_verts, dtype=torch.int32, device=dev)
        new_id[order] = torch.arange(n_verts, dtype=torch.int32, device=dev)
        faces = new_id[faces.long()][torch.sort(fkeys)[1]]
    return (verts, faces, normals, stats) if return_stats else (verts, faces, normals)


# =========================================================================================
# mesh cleanup: components, areas, moments, largest component (csrc/hm_mesh_cc.hip)
# =========================================================================================
def _check_mesh(what, faces, n_verts=None, verts=None, normals=None, label=None, gpu_first=True):
    """the checks the mesh ops share; returns (F, V).  A CPU tensor raises HashmodError before its dtype and shape are
    looked at, or after them with gpu_first=False"""
    if gpu_first:
        require_gpu(faces, verts, normals, label)
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or not faces.is_contiguous():
        raise ValueError(f"hashmod {what}: contiguous int32 faces [F, 3] expected")
    if verts is not None:
        if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3 or not verts.is_contiguous():
            raise ValueError(f"hashmod {what}: contiguous fp32 verts [V, 3] expected")
        n_verts = verts.shape[0]
    n_verts, n_faces = int(n_verts), int(faces.shape[0])
    if n_verts < 0 or n_verts >= 1 << 31 or n_faces >= 1 << 31:
        raise ValueError(f"hashmod {what}: the numbers of vertices and faces must be below 2^31")
    if normals is not None and (normals.dtype != torch.float32 or normals.shape != verts.shape
                                or not normals.is_contiguous()):
        raise ValueError(f"hashmod {what}: contiguous fp32 normals [V, 3] expected")
    if label is not None and (label.dtype != torch.int32 or label.shape != (n_verts,) or not label.is_contiguous()):
        raise ValueError(f"hashmod {what}: contiguous int32 label [V] expected")
    for t in (verts, normals, label):
        if t is not None and t.device != faces.device:
            raise ValueError(f"hashmod {what}: the tensors are on different devices")
    require_gpu(faces, verts, normals, label)
    return n_faces, n_verts


def _check_mesh_status(what, status):
    if int(status.item()):
        raise _lib.HashmodError(f"hashmod {what}: a face index lies outside [0, n_verts) (or the label does not belong "
                                "to this mesh)")


def mesh_components(faces, n_verts):
    """label [V] int32 of the mesh with faces [F,3] int32 (as marching_cubes returns them) over `n_verts` vertices:
    label[v] is the smallest vertex id of v's connected component - eval.py's mesh.split(only_watertight=False) as a
    labelling, in TriMesh.split's order (components by their lowest vertex).  Vertices are connected when a face holds
    both; a vertex of no face labels itself.  Lock-free union-find in one pass over the faces plus a flatten launch.
    A face index outside [0, n_verts) raises HashmodError (it is reported by the kernel, never dereferenced).
    V and F < 2^31; one host read of the status word, so not graph-capturable."""
    n_faces, n_verts = _check_mesh("mesh_components", faces, n_verts)
    dev = faces.device
    label = torch.empty(n_verts, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().hm_mesh_cc_labels(dptr(faces), n_faces, n_verts, dptr(label), dptr(status), stream_ptr(faces)))
    _check_mesh_status("mesh_components", status)
    return label


def mesh_component_areas(verts, faces, label):
    """(ids [C] int32 ascending, area [C] float64, n_faces [C] int64) of the components of mesh_components' `label`
    that own at least one face - eval.py's areas = [c.area for c in components], in the same order.  Face areas are
    0.5 |(v1 - v0) x (v2 - v0)| of the fp32 vertices cast to fp64 (TriMesh.area_faces); each component's faces are
    brought together by the library's stable sort and summed in a fixed order without atomics, so two calls give the
    same bits.  V and F < 2^31; host reads of C and the status word, so not graph-capturable."""
    n_faces, n_verts = _check_mesh("mesh_component_areas", faces, verts=verts, label=label)
    dev = faces.device
    L = lib()
    st = stream_ptr(faces)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    used = torch.zeros(n_verts, dtype=torch.int32, device=dev)
    face_area = torch.empty(n_faces, dtype=torch.float64, device=dev)
    check(L.hm_mesh_cc_face_stats(dptr(verts), dptr(faces), n_faces, n_verts, dptr(face_area), dptr(used), dptr(status),
                                  st))
    # bookkeeping between the launches: the roots that own faces, ranked in ascending order
    root = (label == torch.arange(n_verts, dtype=torch.int32, device=dev)) & (used != 0)
    incl = torch.cumsum(root, 0, dtype=torch.int32)
    rank = incl - root.to(torch.int32)
    ids = torch.nonzero(root).reshape(-1).to(torch.int32)
    n_comp = int(ids.shape[0])
    area = torch.empty(n_comp, dtype=torch.float64, device=dev)
    count = torch.empty(n_comp, dtype=torch.int64, device=dev)
    if n_comp:
        ws = torch.empty(check(L.hm_mesh_cc_sums_workspace_bytes(n_faces)), dtype=torch.uint8, device=dev)
        check(L.hm_mesh_cc_sums(dptr(faces), n_faces, n_verts, dptr(label), dptr(rank), dptr(face_area), n_comp,
                                dptr(area), dptr(count), dptr(ws), ws.numel(), dptr(status), st))
    _check_mesh_status("mesh_component_areas", status)
    return ids, area, count


def mesh_select(verts, faces, normals, label, component_id):
    """(verts, faces, normals or None) of the component `component_id` (a value of mesh_components' `label`): its used
    vertices in ascending original order, its faces in original order and renumbered, the normals gathered like the
    vertices - the element of TriMesh.split() with that lowest vertex, bit for bit (np.unique(faces,
    return_inverse=True)).  A component without faces gives empty outputs.  V and F < 2^31; one host read of the two
    counts between marking and emitting, so not graph-capturable."""
    n_faces, n_verts = _check_mesh("mesh_select", faces, verts=verts, normals=normals, label=label)
    dev = faces.device
    L = lib()
    st = stream_ptr(faces)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    vflag = torch.zeros(n_verts, dtype=torch.int32, device=dev)
    fflag = torch.empty(n_faces, dtype=torch.int32, device=dev)
    component_id = int(component_id)
    if not -(1 << 31) <= component_id < 1 << 31:
        raise ValueError("hashmod mesh_select: component_id does not fit int32")
    check(L.hm_mesh_select_mark(dptr(faces), n_faces, n_verts, dptr(label), component_id, dptr(vflag), dptr(fflag),
                                dptr(status), st))
    return _mesh_emit_flagged("mesh_select", verts, faces, normals, vflag, fflag, status)


def _mesh_emit_flagged(what, verts, faces, normals, vflag, fflag, status):
    """the tail mesh_select and mesh_keep_vertices share: prefix sums of the int32 flags a mark kernel wrote, one host
    read of the two counts and the status word, hm_mesh_select_emit"""
    n_faces, n_verts = int(faces.shape[0]), int(verts.shape[0])
    dev = faces.device
    L = lib()
    st = stream_ptr(faces)
    vincl = torch.cumsum(vflag, 0, dtype=torch.int32)
    fincl = torch.cumsum(fflag, 0, dtype=torch.int32)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    nv, nf, bad = torch.cat([vincl[-1:] if n_verts else zero, fincl[-1:] if n_faces else zero, status]).tolist()
    if bad:
        _check_mesh_status(what, status)
    vpre, fpre = vincl - vflag, fincl - fflag
    verts_out = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces_out = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    normals_out = None if normals is None else torch.empty((nv, 3), dtype=torch.float32, device=dev)
    if nv:
        check(L.hm_mesh_select_emit(dptr(verts), dptr(normals), dptr(faces), n_faces, n_verts, dptr(vflag), dptr(vpre),
                                    dptr(fflag), dptr(fpre), nv, nf, dptr(verts_out), dptr(normals_out),
                                    dptr(faces_out), st))
    return verts_out, faces_out, normals_out


def mesh_largest_component(verts, faces, normals=None):
    """(verts, faces, normals) of the component with the largest area - eval.py's components[areas.argmax()] after
    mesh.split(only_watertight=False), on the device: mesh_components, mesh_component_areas, the first maximum (equal
    areas go to the lower id, as numpy's argmax over split()'s order), mesh_select.  A mesh without faces comes back
    unchanged.  Host reads in every step; not graph-capturable."""
    n_faces, n_verts = _check_mesh("mesh_largest_component", faces, verts=verts, normals=normals)
    if n_faces == 0:
        return verts, faces, normals
    label = mesh_components(faces, n_verts)
    ids, area, _ = mesh_component_areas(verts, faces, label)
    return mesh_select(verts, faces, normals, label, int(ids[torch.argmax(area)].item()))


def mesh_surface_moments(verts, faces):
    """(area [] , mean [3], cov [3,3]) float64 of the uniform distribution on the mesh surface, exact from its
    triangles: the formula of utils/plots._surface_moments in fp64 on the fp32 vertices, as a fixed-order two-level
    reduction (two calls give the same bits).  NaN mean and covariance for a mesh without area.  V and F < 2^31; one
    host read of the status word, so not graph-capturable."""
    n_faces, n_verts = _check_mesh("mesh_surface_moments", faces, verts=verts)
    dev = faces.device
    L = lib()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(13, dtype=torch.float64, device=dev)
    ws = torch.empty(check(L.hm_mesh_moments_workspace_bytes(n_faces)), dtype=torch.uint8, device=dev)
    check(L.hm_mesh_moments(dptr(verts), dptr(faces), n_faces, n_verts, dptr(out), dptr(ws), ws.numel(), dptr(status),
                            stream_ptr(faces)))
    _check_mesh_status("mesh_surface_moments", status)
    return out[0], out[1:4], out[4:13].view(3, 3)


# =========================================================================================
# mesh simplification: vertex clustering (csrc/hm_mesh_simplify.hip, DESIGN.md "Mesh simplification")
# =========================================================================================
def _simplify_grid(lo, hi, cell):
    """(h as fp32, g[3]) of the clustering grid over the box [lo, hi] (float lists), g as _nn_grid computes it; a grid
    beyond nn_grid()'s limits (hm_nn_dev.h) raises ValueError"""
    h = float(np.float32(cell))
    if not (h > 0.0 and math.isfinite(h)):
        raise ValueError("hashmod mesh_simplify: cell must be positive and finite in fp32")
    g = []
    for a, b in zip(lo, hi):
        q = max(float(b) - float(a), 0.0) / h
        g.append(int(math.floor(q)) + 1 if math.isfinite(q) else 1 << 62)
    if max(g) > 1 << 30 or g[0] * g[1] * g[2] >= 1 << 31:
        raise ValueError(f"hashmod mesh_simplify: cell={cell} gives a grid of {g[0]}x{g[1]}x{g[2]} cells; a dimension "
                         "may be at most 2^30 and the grid must have fewer than 2^31 cells")
    return h, g


def mesh_simplify(verts, faces, normals=None, cell=None, placement="quadric", reg=0.05):
    """(verts_out [C,3] fp32, faces_out [G,3] int32, normals_out [C,3] fp32 or None, vertex_map [V] int32): the mesh
    decimated by vertex clustering on a uniform grid of edge `cell` (DESIGN.md "Mesh simplification").

    Grid: h = fp32(cell) over the box of ALL rows of verts (aminmax, read by the host), nn_index's cell function; more
    than 2^30 cells on an axis or 2^31 in all raise ValueError, a non-finite coordinate HashmodError.  The vertices
    that some face uses and that share a cell form a cluster; clusters are numbered by ascending cell key.  Its
    representative, in fp64 from the fp32 inputs and rounded once: placement="mean", the members' mean m;
    placement="quadric" (needs normals), the minimiser m + A^-1 b of the members' point-normal quadric regularised
    towards m (A = sum n n^T + reg k I over the k unit normals, b = sum n (n . (p - m))), clamped per axis to the
    cell's box widened to hold m.  Its normal is the normalised sum of the members' unit normals (0 when they cancel;
    a zero or non-finite normal adds nothing); None without normals.  Faces: mapped to clusters, dropped when two
    corners share one, rotated to smallest-id-first, and of equal triples only the first survives ((a,b,c) and (a,c,b)
    differ); the survivors keep their order.  Clusters of no surviving face are dropped and the rest renumbered in
    ascending order; vertex_map[v] is the output row of v's cluster, -1 for a vertex of no face or a dropped cluster.
    V == 0 or F == 0 gives empty outputs.  Every sum has a fixed order and no atomics: two calls give the same bits.

    Clustering does not preserve manifoldness: a cell that holds two sheets of the surface welds them, and an edge
    may end up with more than two faces.  A face index outside [0, V) raises HashmodError (reported by the kernel,
    never dereferenced).  Host reads of the box and of the counts between the launches, so not graph-capturable."""
    n_faces, n_verts = _check_mesh("mesh_simplify", faces, verts=verts, normals=normals)
    if not (isinstance(cell, (int, float)) and math.isfinite(cell) and cell > 0):
        raise ValueError("hashmod mesh_simplify: cell must be a positive finite number")
    if placement not in ("quadric", "mean"):
        raise ValueError('hashmod mesh_simplify: placement must be "quadric" or "mean"')
    if placement == "quadric" and normals is None:
        raise ValueError('hashmod mesh_simplify: placement="quadric" needs normals')
    if not (isinstance(reg, (int, float)) and math.isfinite(reg) and reg > 0):
        raise ValueError("hashmod mesh_simplify: reg must be a positive finite number")
    dev = faces.device

    i32 = dict(dtype=torch.int32, device=dev)

    def result(nv, nf):
        """uninitialised outputs of nv vertices and nf faces; the map all -1"""
        return (torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nf, 3), **i32),
                None if normals is None else torch.empty((nv, 3), dtype=torch.float32, device=dev),
                torch.full((n_verts,), -1, **i32))

    if n_verts == 0 or n_faces == 0:
        return result(0, 0)
    lo, hi = torch.aminmax(verts, dim=0)
    box = torch.stack([lo, hi]).tolist()
    if not all(math.isfinite(v) for v in box[0] + box[1]):
        raise _lib.HashmodError("hashmod mesh_simplify: a vertex has a non-finite coordinate")
    h, g = _simplify_grid(box[0], box[1], cell)
    lo_c, g_c = (C.c_float * 3)(*box[0]), (C.c_int32 * 3)(*g)
    L = lib()
    st = stream_ptr(faces)

    # clusters: the sorted keys' runs
    status = torch.zeros(1, **i32)
    used = torch.zeros(n_verts, **i32)
    keys_sorted, head = torch.empty(n_verts, **i32), torch.empty(n_verts, **i32)
    perm = torch.empty(n_verts, dtype=torch.int64, device=dev)
    ws = torch.empty(check(L.hm_mesh_simplify_keys_workspace_bytes(n_verts)), dtype=torch.uint8, device=dev)
    check(L.hm_mesh_simplify_keys(dptr(verts), dptr(faces), n_faces, n_verts, lo_c, h, g_c, dptr(used), dptr(keys_sorted),
                                  dptr(perm), dptr(head), dptr(ws), ws.numel(), dptr(status), st))
    start = torch.nonzero(head).reshape(-1)      # a host read of the number of clusters
    n_clusters = int(start.shape[0])
    _check_mesh_status("mesh_simplify", status)
    start = torch.cat([start, used.sum(dtype=torch.int64).reshape(1)])
    rep = torch.empty((n_clusters, 3), dtype=torch.float32, device=dev)
    rep_normals = None if normals is None else torch.empty((n_clusters, 3), dtype=torch.float32, device=dev)
    cluster_of = torch.full((n_verts,), -1, **i32)
    check(L.hm_mesh_simplify_clusters(dptr(verts), dptr(normals), n_verts, dptr(keys_sorted), dptr(perm), dptr(start),
                                      n_clusters, lo_c, h, g_c, int(placement == "quadric"), float(reg), dptr(rep),
                                      dptr(rep_normals), dptr(cluster_of), st))

    # faces: drop the collapsed ones, then the repeats
    fkeep = torch.empty(n_faces, **i32)
    check(L.hm_mesh_simplify_face_flags(dptr(faces), n_faces, n_verts, dptr(cluster_of), n_clusters, dptr(fkeep), st))
    fincl = torch.cumsum(fkeep, 0, dtype=torch.int32)
    n_tri = int(fincl[-1].item())
    if n_tri == 0:
        return result(0, 0)
    fpre = fincl - fkeep
    tri = torch.empty((3, n_tri), **i32)
    tkeep = torch.empty(n_tri, **i32)
    cused = torch.zeros(n_clusters, **i32)
    ws = torch.empty(check(L.hm_mesh_simplify_dedupe_workspace_bytes(n_tri)), dtype=torch.uint8, device=dev)
    check(L.hm_mesh_simplify_dedupe(dptr(faces), n_faces, n_verts, dptr(cluster_of), n_clusters, dptr(fkeep), dptr(fpre),
                                    n_tri, dptr(tri), dptr(tkeep), dptr(cused), dptr(ws), ws.numel(), st))

    # compaction: the clusters some surviving face uses, renumbered in ascending order
    cincl = torch.cumsum(cused, 0, dtype=torch.int32)
    tincl = torch.cumsum(tkeep, 0, dtype=torch.int32)
    nv, nf = torch.cat([cincl[-1:], tincl[-1:]]).tolist()
    cpre, tpre = cincl - cused, tincl - tkeep
    verts_out, faces_out, normals_out, vertex_map = result(nv, nf)
    check(L.hm_mesh_simplify_emit(dptr(rep), dptr(rep_normals), n_clusters, dptr(cused), dptr(cpre), nv, dptr(tri), n_tri,
                                  dptr(tkeep), dptr(tpre), nf, dptr(cluster_of), n_verts, dptr(verts_out),
                                  dptr(normals_out), dptr(faces_out), dptr(vertex_map), st))
    return verts_out, faces_out, normals_out, vertex_map


# =========================================================================================
# Chamfer evaluation: nearest neighbours, triangle upsampling, the metric (csrc/hm_nn.hip, csrc/hm_mesh_sample.hip)
# =========================================================================================
NN_MAX_CELLS = 1 << 26      # cap of the dense cell_start table (256 MiB of int32)
_NN_PER_CELL = 4.0          # points per occupied cell the default cell edge aims at
_NN_WS = _lib.Workspace("nearest_neighbors")


def _check_cloud(what, name, t, like=None):
    """contiguous fp32 [., 3]; on `like`'s device; a GPU tensor"""
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3
            or not t.is_contiguous()):
        raise ValueError(f"hashmod {what}: contiguous fp32 {name} [., 3] expected")
    if t.shape[0] >= 1 << 31:
        raise ValueError(f"hashmod {what}: {name} must have fewer than 2^31 rows")
    if like is not None and t.device != like.device:
        raise ValueError(f"hashmod {what}: the tensors are on different devices")


def _nn_grid(lo, hi, n, cell, what="nn_index", per_cell=_NN_PER_CELL):
    """(h as fp32, g[3]) of the grid over the box [lo, hi] (float lists): the cell edge a surface-like cloud of n points
    needs for per_cell = _NN_PER_CELL points per occupied cell - its area taken as half the box's - unless `cell` gives
    it, grown until the grid has at most NN_MAX_CELLS cells; a zero extent gives one cell on that axis.  `what` names
    the caller in the error messages"""
    ext = [max(float(b) - float(a), 0.0) for a, b in zip(lo, hi)]
    if cell is None:
        area = ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]
        if area > 0.0:
            h = math.sqrt(per_cell * area / n)
        elif max(ext) > 0.0:
            h = per_cell * max(ext) / n
        else:
            h = 1.0
        h = max(h, max(ext) * 2.0 ** -20)
    else:
        h = float(cell)
    while True:
        h = float(np.float32(h))
        if not (h > 0.0 and math.isfinite(h)):
            raise ValueError(f"hashmod {what}: the cell edge must be positive and finite in fp32")
        g = [int(math.floor(e / h)) + 1 for e in ext]
        if max(g) <= 1 << 30 and g[0] * g[1] * g[2] <= NN_MAX_CELLS:
            return h, g
        if cell is not None:
            raise ValueError(f"hashmod {what}: cell={cell} gives a grid of {g[0]}x{g[1]}x{g[2]} cells, more than "
                             f"NN_MAX_CELLS = {NN_MAX_CELLS}")
        h *= 1.125


class NNIndex:
    """The uniform grid over a point cloud that ops.nn_index builds: the points ordered by cell as 16-byte records and
    the dense cell_start table.  query() answers nearest-neighbour queries against it."""

    def __init__(self, points, cell=None):
        _check_cloud("nn_index", "points", points)
        if cell is not None and not (isinstance(cell, (int, float)) and math.isfinite(cell) and cell > 0):
            raise ValueError("hashmod nn_index: cell must be a positive finite number")
        n = int(points.shape[0])
        if n < 1:
            raise ValueError("hashmod nn_index: at least one point is needed")
        require_gpu(points)
        dev = points.device
        lo, hi = torch.aminmax(points, dim=0)
        box = torch.stack([lo, hi]).tolist()
        if not all(math.isfinite(v) for v in box[0] + box[1]):
            raise _lib.HashmodError("hashmod nn_index: a point has a non-finite coordinate")
        self.h, self.g = _nn_grid(box[0], box[1], n, cell)
        self.lo = box[0]
        self.n = n
        self.device = dev
        cells = self.g[0] * self.g[1] * self.g[2]
        self.cell_start = torch.empty(cells + 1, dtype=torch.int32, device=dev)
        self.records = torch.empty((n, 4), dtype=torch.float32, device=dev)
        L = lib()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _NN_WS.get(dev, check(L.hm_nn_workspace_bytes(n)))
        check(L.hm_nn_build(dptr(points), n, self._lo(), self.h, self._g(), dptr(self.cell_start), dptr(self.records),
                            dptr(ws), ws.numel(), dptr(status), stream_ptr(points)))
        if int(status.item()):
            raise _lib.HashmodError("hashmod nn_index: a point has a non-finite coordinate")

    def _lo(self):
        return (C.c_float * 3)(*self.lo)

    def _g(self):
        return (C.c_int32 * 3)(*self.g)

    def _query(self, query, max_dist2, stats=None):
        """stats: a dict that receives "candidate_tests", the launch's number of distance evaluations (one more host
        read; for scripts/chamfer_time.py)"""
        _check_cloud("nearest_neighbors", "query", query, self.records)
        m = int(query.shape[0])
        dev = self.device
        d2 = torch.empty(m, dtype=torch.float32, device=dev)
        index = torch.empty(m, dtype=torch.int32, device=dev)
        if m == 0:
            return d2, index
        L = lib()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _NN_WS.get(dev, check(L.hm_nn_workspace_bytes(m)))
        tests = None if stats is None else torch.zeros(1, dtype=torch.int64, device=dev)
        check(L.hm_nn_query(dptr(query), m, dptr(self.records), self.n, dptr(self.cell_start), self._lo(), self.h,
                            self._g(), max_dist2, dptr(d2), dptr(index), dptr(ws), ws.numel(), dptr(status),
                            dptr(tests), stream_ptr(query)))
        if stats is not None:
            stats["candidate_tests"] = int(tests.item())
        if int(status.item()):
            raise _lib.HashmodError("hashmod nearest_neighbors: a query has a non-finite coordinate")
        return d2, index

    def query(self, query, max_dist=None):
        """(d2 [m] fp32, index [m] int32) of the nearest point of every row of query [m,3]: see nearest_neighbors"""
        return self._query(query, _max_dist2("nearest_neighbors", max_dist))


def _max_dist2(what, max_dist):
    """max_dist as the kernel's fp32 bound on d2: fp32(max_dist) squared in fp32; inf for None"""
    if max_dist is None:
        return math.inf
    if not (isinstance(max_dist, (int, float)) and max_dist >= 0):      # NaN fails
        raise ValueError(f"hashmod {what}: max_dist must be a number >= 0 (or None)")
    md = np.float32(max_dist)
    with np.errstate(over="ignore"):
        return float(md * md)


def nn_index(points, cell=None):
    """The search structure of nearest_neighbors over points [n,3] fp32 (n >= 1), to be queried many times: a uniform
    grid of cell edge `cell` over the points' bounding box (read by the host through aminmax).  Without `cell` the
    edge is chosen from n and the box so that an occupied cell of a surface-like cloud holds a handful of points; the
    dense cell table is capped at NN_MAX_CELLS = 2^26 cells (the edge grows to fit; an explicit `cell` that does not
    fit raises ValueError).  A zero extent on an axis gives one cell on that axis.  The points are ordered by cell with
    the library's stable radix sort.  A non-finite coordinate raises HashmodError.  The grid changes the speed of a
    query, never its result.  Host reads of the box and the status word, so not graph-capturable."""
    return NNIndex(points, cell)


def nearest_neighbors(query, points, max_dist=None, cell=None):
    """(d2 [m] fp32, index [m] int32): for every row of query [m,3] the row of points [n,3] that minimises the fp32
    value d2 = (dx*dx + dy*dy) + dz*dz, dx = q.x - p.x and so on, each operation rounded once; among equal d2 the
    lowest index.  That is a brute-force fp32 argmin over all points, bit for bit: exact, and independent of the grid,
    of m and of the thread order.  With max_dist, a query whose d2 exceeds fp32(max_dist)^2 (squared in fp32) gets
    index -1 and d2 = inf; d2 equal to the bound is reported.  m = 0 gives empty outputs; n >= 1, contiguous fp32
    tensors on one GPU (else ValueError); a non-finite coordinate raises HashmodError.  nn_index(points, cell).query(
    query, max_dist) is the same in two steps.  Host reads of the box and the status words, so not
    graph-capturable."""
    _check_cloud("nearest_neighbors", "query", query)
    _check_cloud("nearest_neighbors", "points", points, query)
    md2 = _max_dist2("nearest_neighbors", max_dist)
    return NNIndex(points, cell)._query(query, md2)


def mesh_sample_surface(verts, faces, density, return_face=False):
    """samples [S,3] fp32 (and face_of [S] int32 with return_face): every triangle upsampled to one point per
    density^2 of area by the rule of the DTU evaluation, in fp64 on the fp32 vertices - include/hashmod.h states it;
    tests/nn_cases.sample_ref is its numpy restatement and gives the same points bit for bit.  Faces ascending, then
    the rule's own order; faces without area or smaller than the density give nothing, a mesh without faces [0,3].
    density > 0 and finite (else ValueError); a face index outside [0, V) raises HashmodError (reported by the kernel,
    never dereferenced); S < 2^31.  Host reads of the total and the status word, so not graph-capturable."""
    if not (isinstance(density, (int, float)) and math.isfinite(density) and density > 0):
        raise ValueError("hashmod mesh_sample_surface: density must be a positive finite number")
    n_faces, n_verts = _check_mesh("mesh_sample_surface", faces, verts=verts, gpu_first=False)
    dev = faces.device
    samples = torch.empty((0, 3), dtype=torch.float32, device=dev)
    face_of = torch.empty(0, dtype=torch.int32, device=dev)
    if n_faces:
        L = lib()
        st = stream_ptr(faces)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        count = torch.empty(n_faces, dtype=torch.int64, device=dev)
        rows = torch.empty(n_faces, dtype=torch.int32, device=dev)
        check(L.hm_mesh_sample_count(dptr(verts), dptr(faces), n_faces, n_verts, float(density), dptr(count),
                                     dptr(rows), dptr(status), st))
        # bookkeeping between the launches: positions from the counts, the totals to the host
        incl = torch.cumsum(count, 0)
        total, max_rows, bad = torch.stack([incl[-1], rows.max().to(torch.int64), status[0].to(torch.int64)]).tolist()
        if bad:
            _check_mesh_status("mesh_sample_surface", status)
        if total >= 1 << 31:
            raise ValueError(f"hashmod mesh_sample_surface: density={density} gives 2^31 samples or more")
        if total:
            samples = torch.empty((total, 3), dtype=torch.float32, device=dev)
            face_of = torch.empty(total, dtype=torch.int32, device=dev)
            prefix = incl - count
            check(L.hm_mesh_sample_emit(dptr(verts), dptr(faces), n_faces, n_verts, float(density), dptr(prefix),
                                        total, max_rows, dptr(samples), dptr(face_of), st))
    return (samples, face_of) if return_face else samples


class ChamferResult(tuple):
    """mean_a2b, mean_b2a, overall = (mean_a2b + mean_b2a)/2 and the numbers of distances n_a2b, n_b2a that entered
    the two means, as host scalars; mesh_chamfer adds n_cloud"""
    _fields = ("mean_a2b", "mean_b2a", "overall", "n_a2b", "n_b2a", "n_cloud")

    def __new__(cls, mean_a2b, mean_b2a, n_a2b, n_b2a, n_cloud=None):
        return super().__new__(cls, (mean_a2b, mean_b2a, 0.5 * (mean_a2b + mean_b2a), n_a2b, n_b2a, n_cloud))

    def __getattr__(self, name):
        try:
            return self[self._fields.index(name)]
        except ValueError:
            raise AttributeError(name) from None

    def __repr__(self):
        return "ChamferResult(" + ", ".join(f"{k}={v!r}" for k, v in zip(self._fields, self)) + ")"


def _one_sided(src, index, max_dist, md2):
    """(sum, count) as one fp64 [2] device tensor of the distances src -> the index's cloud below max_dist"""
    d2, _ = index._query(src, md2)
    d = torch.sqrt(d2.to(torch.float64))
    keep = d < max_dist if max_dist is not None else torch.ones_like(d, dtype=torch.bool)
    zero = torch.zeros((), dtype=torch.float64, device=d.device)
    return torch.stack([torch.where(keep, d, zero).sum(), keep.sum().to(torch.float64)])


def chamfer_distance(a, b, max_dist=None):
    """ChamferResult of the clouds a [na,3] and b [nb,3] (fp32, both non-empty): the DTU evaluation's accuracy and
    completeness.  mean_a2b is the mean over the points of a of the distance to their nearest point of b, taken over
    the distances < max_dist (strict, the DTU rule; all of them for None), mean_b2a the same the other way, overall
    their mean; n_a2b, n_b2a count the distances that entered.  A mean over no distance is nan with count 0.  The
    distances are the fp64 square roots of nearest_neighbors' exact fp32 d2; the sums are fixed-order fp64 device
    reductions, so two calls give the same bits.  Only the four scalars come to the host.  Not graph-capturable."""
    _check_cloud("chamfer_distance", "a", a)
    _check_cloud("chamfer_distance", "b", b, a)
    if max_dist is not None and not (isinstance(max_dist, (int, float)) and max_dist > 0):
        raise ValueError("hashmod chamfer_distance: max_dist must be a positive number (or None)")
    if a.shape[0] < 1 or b.shape[0] < 1:
        raise ValueError("hashmod chamfer_distance: both clouds need at least one point")
    md2 = _search_bound2(max_dist)
    sa, ca, sb, cb = torch.cat([_one_sided(a, NNIndex(b), max_dist, md2),
                                _one_sided(b, NNIndex(a), max_dist, md2)]).tolist()
    return ChamferResult(sa / ca if ca else math.nan, sb / cb if cb else math.nan, int(ca), int(cb))


def _search_bound2(max_dist):
    """the kernel may stop searching beyond a bound safely above max_dist; the strict fp64 rule is applied afterwards"""
    return math.inf if max_dist is None else float(np.nextafter(np.float32(min(float(max_dist) ** 2 * (1.0 + 1e-6),
                                                                              3.0e38)), np.float32(np.inf)))


def one_sided_distance(src, dst, max_dist=None, cell=None):
    """(mean, count): one direction of chamfer_distance for two different sets - the mean over the rows of src [m,3]
    of the distance to their nearest row of dst [n,3], over the distances < max_dist (strict; all for None), and how
    many entered.  The same distances, rule and fixed-order fp64 reduction as chamfer_distance's mean_a2b, which it
    equals bit for bit for (a, b).  An empty src or dst, or no distance below max_dist, gives (nan, 0).  `cell` is
    nn_index's.  Host scalars; not graph-capturable."""
    _check_cloud("one_sided_distance", "src", src)
    _check_cloud("one_sided_distance", "dst", dst, src)
    if max_dist is not None and not (isinstance(max_dist, (int, float)) and max_dist > 0):
        raise ValueError("hashmod one_sided_distance: max_dist must be a positive number (or None)")
    if src.shape[0] < 1 or dst.shape[0] < 1:
        return math.nan, 0
    s, c = _one_sided(src, NNIndex(dst, cell), max_dist, _search_bound2(max_dist)).tolist()
    return (s / c if c else math.nan), int(c)


# =========================================================================================
# Point-to-mesh distance: the triangle grid and the exact closest point (csrc/hm_mesh_dist.hip)
# =========================================================================================
MESH_DIST_BIG_FACE = 64     # cells of a face's cell box above which the face goes to the list every wave tests in full
_MD_PER_CELL = 32.0         # mean face areas per cell face the default cell edge aims at
_MD_WS = _lib.Workspace("mesh_closest_point")
_MR_PER_CELL = 24.0         # the aim of mesh_ray_cast's default cell edge, about 2.75 lattice spacings of a marching-
                            # cubes mesh: scripts/mesh_ray_time.py's sweep is fastest between 2 and 3


def _check_on_gpu(what, *tensors):
    """the mesh-distance ops reject a CPU tensor as an argument error (a ValueError and a HashmodError) before the
    library is touched"""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.HashmodArgumentError(f"hashmod {what}: the tensors must be on a GPU; there is no CPU path")


class MeshIndex:
    """The uniform grid over a triangle mesh that ops.mesh_index builds: every face listed in the cells of its
    bounding box - grown by `pad` on every side - as 48-byte records ordered by cell (ascending face inside a cell), the
    big faces as a run of records behind them, and the dense cell_start table.  query() answers closest-point queries
    against it, ray_cast() first-hit queries."""

    def __init__(self, verts, faces, cell=None, big_face=MESH_DIST_BIG_FACE, pad=0.0, _per_cell=_MD_PER_CELL,
                 _auto_pad=False):
        if cell is not None and not (isinstance(cell, (int, float)) and not isinstance(cell, bool)
                                     and math.isfinite(cell) and cell > 0):
            raise ValueError("hashmod mesh_index: cell must be a positive finite number")
        if not (isinstance(big_face, int) and not isinstance(big_face, bool) and 1 <= big_face < 1 << 62):
            raise ValueError("hashmod mesh_index: big_face must be an integer >= 1")
        self.pad = None if _auto_pad and pad is None else _ray_pad("mesh_index", pad)
        if not isinstance(verts, torch.Tensor) or not isinstance(faces, torch.Tensor):
            raise ValueError("hashmod mesh_index: verts and faces must be tensors")
        if faces.dim() == 2 and faces.shape[0] < 1:
            raise ValueError("hashmod mesh_index: at least one face is needed")
        _check_on_gpu("mesh_index", verts, faces)
        n_faces, n_verts = _check_mesh("mesh_index", faces, verts=verts, gpu_first=False)
        dev = faces.device
        if n_verts < 1:
            raise _lib.HashmodError("hashmod mesh_index: a face index lies outside [0, n_verts)")
        lo, hi = torch.aminmax(verts, dim=0)
        box = torch.stack([lo, hi]).tolist()
        if not all(math.isfinite(v) for v in box[0] + box[1]):
            raise _lib.HashmodError("hashmod mesh_index: a vertex has a non-finite coordinate")
        self.h, self.g = _nn_grid(box[0], box[1], n_faces, cell, "mesh_index", _per_cell)
        self.lo = box[0]
        if self.pad is None:                # mesh_ray_cast's default, from the box already read: mesh_ray_pad's value
            self.pad = _default_ray_pad(box)
        self.n_faces, self.n_verts = n_faces, n_verts
        self.big_face = big_face
        self.device = dev
        cells = self.g[0] * self.g[1] * self.g[2]
        L = lib()
        st = stream_ptr(faces)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        count = torch.empty(n_faces, dtype=torch.int32, device=dev)
        big = torch.empty(n_faces, dtype=torch.int32, device=dev)
        check(L.hm_mesh_index_count(dptr(verts), dptr(faces), n_faces, n_verts, self._lo(), self.h, self._g(), self.pad,
                                    big_face, dptr(count), dptr(big), dptr(status), st))
        # bookkeeping between the launches: positions from the counts, the totals and the status word to the host
        cincl = torch.cumsum(count, 0, dtype=torch.int64)
        bincl = torch.cumsum(big, 0, dtype=torch.int64)
        n_pairs, n_big, bad = torch.stack([cincl[-1], bincl[-1], status[0].to(torch.int64)]).tolist()
        if bad & 1:
            _check_mesh_status("mesh_index", status)
        if bad:
            raise _lib.HashmodError("hashmod mesh_index: a vertex of a face has a non-finite coordinate")
        if n_pairs + n_big >= 1 << 31:
            raise ValueError(f"hashmod mesh_index: the faces fill {n_pairs} cells of the grid, 2^31 or more; use a "
                             "larger cell or a smaller big_face")
        self.n_pairs, self.n_big = n_pairs, n_big
        prefix = (cincl - count).to(torch.int32)
        big_prefix = (bincl - big).to(torch.int32)
        self.cell_start = torch.empty(cells + 1, dtype=torch.int32, device=dev)
        self.records = torch.empty((n_pairs + n_big, 12), dtype=torch.float32, device=dev)
        ws = _MD_WS.get(dev, check(L.hm_mesh_dist_workspace_bytes(n_pairs)))
        check(L.hm_mesh_index_build(dptr(verts), dptr(faces), n_faces, n_verts, self._lo(), self.h, self._g(), self.pad,
                                    dptr(count), dptr(big), dptr(prefix), n_pairs, dptr(big_prefix), n_big,
                                    dptr(self.cell_start), dptr(self.records), dptr(ws), ws.numel(), st))

    def _lo(self):
        return (C.c_float * 3)(*self.lo)

    def _g(self):
        return (C.c_int32 * 3)(*self.g)

    def _query(self, query, max_dist2, return_point=True, return_feature=False, stats=None):
        """(d2, face, point or None, feature or None); stats: a dict that receives "candidate_tests", the launch's
        number of (query, face) tests (one more host read; for scripts/mesh_distance_time.py)"""
        _check_cloud("mesh_closest_point", "query", query, self.records)
        _check_on_gpu("mesh_closest_point", query)
        m = int(query.shape[0])
        dev = self.device
        d2 = torch.empty(m, dtype=torch.float32, device=dev)
        face = torch.empty(m, dtype=torch.int32, device=dev)
        point = torch.empty((m, 3), dtype=torch.float32, device=dev) if return_point else None
        feature = torch.empty(m, dtype=torch.int32, device=dev) if return_feature else None
        if m == 0:
            return d2, face, point, feature
        L = lib()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _MD_WS.get(dev, check(L.hm_mesh_dist_workspace_bytes(m)))
        tests = None if stats is None else torch.zeros(1, dtype=torch.int64, device=dev)
        check(L.hm_mesh_dist_query(dptr(query), m, dptr(self.records), self.n_pairs, self.n_big, dptr(self.cell_start),
                                   self._lo(), self.h, self._g(), max_dist2, dptr(d2), dptr(face), dptr(point),
                                   dptr(feature), dptr(ws), ws.numel(), dptr(status), dptr(tests), stream_ptr(query)))
        if stats is not None:
            stats["candidate_tests"] = int(tests.item())
        if int(status.item()):
            raise _lib.HashmodError("hashmod mesh_closest_point: a query has a non-finite coordinate")
        return d2, face, point, feature

    def query(self, query, max_dist=None, return_point=True, return_feature=False):
        """mesh_closest_point's outputs for the rows of query [m,3] against this mesh"""
        _check_flags("mesh_closest_point", return_point=return_point, return_feature=return_feature)
        out = self._query(query, _max_dist2("mesh_closest_point", max_dist), return_point, return_feature)
        return tuple(t for t in out if t is not None)

    def ray_cast(self, origins, dirs, t_min=0.0, t_max=math.inf, return_uv=True, return_point=False, stats=None):
        """mesh_ray_cast's outputs for the rays (origins, dirs) [m,3] against this mesh, with the index's own pad;
        stats: a dict that receives "face_tests", the launch's number of (ray, face) tests (one more host read; for
        scripts/mesh_ray_time.py)"""
        what = "mesh_ray_cast"
        _check_cloud(what, "origins", origins)
        _check_cloud(what, "dirs", dirs, origins)
        m = int(origins.shape[0])
        if int(dirs.shape[0]) != m:
            raise ValueError(f"hashmod {what}: origins and dirs must have the same number of rows")
        _check_flags(what, return_uv=return_uv, return_point=return_point)
        if stats is not None and not isinstance(stats, dict):
            raise ValueError(f"hashmod {what}: stats must be a dict (or None)")
        bounds = [_ray_bound(what, "t_min", t_min, 0.0, m, origins),
                  _ray_bound(what, "t_max", t_max, math.inf, m, origins)]
        _check_on_gpu(what, origins, dirs)
        if origins.device != self.device:
            raise ValueError(f"hashmod {what}: the tensors are on different devices")
        dev = self.device
        t = torch.empty(m, dtype=torch.float32, device=dev)
        face = torch.empty(m, dtype=torch.int32, device=dev)
        uv = torch.empty((m, 2), dtype=torch.float32, device=dev) if return_uv else None
        point = torch.empty((m, 3), dtype=torch.float32, device=dev) if return_point else None
        out = tuple(x for x in (t, face, uv, point) if x is not None)
        if stats is not None:
            stats["face_tests"] = 0
        if m == 0:
            return out
        for k, b in enumerate(bounds):      # a number other than the default becomes a filled tensor
            if isinstance(b, float):
                bounds[k] = torch.full((m,), b, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        tests = None if stats is None else torch.zeros(1, dtype=torch.int64, device=dev)
        check(lib().hm_mesh_ray_cast(dptr(origins), dptr(dirs), dptr(bounds[0]), dptr(bounds[1]), m, dptr(self.records),
                                     self.n_pairs, self.n_big, dptr(self.cell_start), self._lo(), self.h, self._g(),
                                     self.pad, dptr(t), dptr(face), dptr(uv), dptr(point), dptr(status), dptr(tests),
                                     stream_ptr(origins)))
        if stats is not None:
            stats["face_tests"] = int(tests.item())
        if int(status.item()):
            raise _lib.HashmodError(f"hashmod {what}: a ray has a non-finite origin, direction or t_min, or a NaN "
                                    "t_max")
        return out

    def signed_distance(self, query, topology, max_dist=None, return_sign=False, return_face=False,
                        return_point=False):
        """mesh_signed_distance's outputs for the rows of query [m,3] against this mesh; `topology` is
        ops.mesh_topology(verts, faces) of the same mesh (its n_faces, n_verts and device must be the index's, else
        ValueError)"""
        what = "mesh_signed_distance"
        _check_flags(what, return_sign=return_sign, return_face=return_face, return_point=return_point)
        sd, sign, _, face, point = _mesh_sign(self, topology, query, _max_dist2(what, max_dist), return_sign)
        out = tuple(t for t, wanted in ((sd, True), (sign, return_sign), (face, return_face), (point, return_point))
                    if wanted)
        return out if len(out) > 1 else sd


def _default_ray_pad(box):
    ext = max(np.float32(b) - np.float32(a) for a, b in zip(box[0], box[1]))
    return float(np.float32(2.0 ** -12) * ext)


def _ray_pad(what, pad):
    """pad as the fp32 value the kernels use"""
    if not (isinstance(pad, (int, float)) and not isinstance(pad, bool) and math.isfinite(pad) and pad >= 0):
        raise ValueError(f"hashmod {what}: pad must be a finite number >= 0")
    with np.errstate(over="ignore"):
        pad = float(np.float32(pad))
    if not math.isfinite(pad):
        raise ValueError(f"hashmod {what}: pad must be finite in fp32")
    return pad


def _ray_bound(what, name, value, default, m, like):
    """a range end of the rays: None for the default (the kernel's NULL), a float to be filled in, or the [m] fp32
    tensor itself"""
    if isinstance(value, torch.Tensor):
        if value.dtype != torch.float32 or value.dim() != 1 or not value.is_contiguous():
            raise ValueError(f"hashmod {what}: {name} must be a number or a contiguous fp32 tensor [m]")
        if int(value.shape[0]) != m:
            raise ValueError(f"hashmod {what}: {name} must have one entry per ray")
        if value.device != like.device:
            raise ValueError(f"hashmod {what}: the tensors are on different devices")
        return value
    if not isinstance(value, (int, float)) or isinstance(value, bool):
        raise ValueError(f"hashmod {what}: {name} must be a number or a contiguous fp32 tensor [m]")
    value = float(value)
    if value != value or (name == "t_min" and math.isinf(value)):
        raise ValueError(f"hashmod {what}: {name} must not be NaN" + (" or infinite" if name == "t_min" else ""))
    return None if value == default else value


def _check_flags(what, **flags):
    for name, value in flags.items():
        if not isinstance(value, bool):
            raise ValueError(f"hashmod {what}: {name} must be a bool")


def mesh_index(verts, faces, cell=None, big_face=MESH_DIST_BIG_FACE, pad=0.0):
    """The search structure of mesh_closest_point (and, with a pad, of ray casting) over the mesh verts [V,3] fp32,
    faces [F,3] int32 (F >= 1), to be queried many times: a uniform grid of cell edge `cell` over the vertices' bounding box (read by the host through
    aminmax), every face listed in all cells of its own bounding box.  Without `cell` the edge is sqrt(32 A / F) with A
    half the box's surface area - a cell face with the area of 32 mean faces of a surface-like mesh, about three
    bounding-box edges of a marching-cubes face: small cells list a face many times and make far queries walk many
    rings, large cells make near queries test many faces, and scripts/mesh_distance_time.py's mesh and cloud put the
    best compromise between two and four lattice spacings (DESIGN.md has the sweep); the dense cell table is capped
    at NN_MAX_CELLS = 2^26 cells (the edge grows to fit; an explicit `cell` that does not fit raises ValueError).  A
    face whose cell box has more than `big_face` cells (default MESH_DIST_BIG_FACE = 64: a face more than about three
    cells across on every axis) is not listed in the grid but in a separate run that every query wave tests in full,
    so that one large face among many small ones does not fill the table.  The pairs are ordered by cell with the
    library's stable radix sort.  A non-finite vertex or a face index outside [0, V) raises HashmodError (reported by
    the kernel's status word, never dereferenced).  The grid changes the speed of a query, never its result.  `pad`
    (a finite number >= 0, kept as index.pad in fp32) lists every face over its bounding box grown by pad on every
    side: index.ray_cast needs it (mesh_ray_pad gives the usual value) and its result depends on it, the closest-point
    query stays exact on a padded index, and pad = 0 is the index without one, tensor for tensor.  Host reads of the
    box, the totals and the status word, so not graph-capturable."""
    return MeshIndex(verts, faces, cell, big_face, pad)


def mesh_ray_pad(verts):
    """The default pad of ray casting: fp32(2^-12 * the largest bounding-box extent of verts [V,3]) - far above fp32
    rounding, a few percent of a default cell.  One host read."""
    if (not isinstance(verts, torch.Tensor) or verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3
            or verts.shape[0] < 1 or not verts.is_contiguous()):
        raise ValueError("hashmod mesh_ray_pad: contiguous fp32 verts [V,3] with V >= 1 expected")
    box = torch.stack(torch.aminmax(verts, dim=0)).tolist()
    if not all(math.isfinite(v) for v in box[0] + box[1]):
        raise _lib.HashmodError("hashmod mesh_ray_pad: a vertex has a non-finite coordinate")
    return _default_ray_pad(box)


def mesh_ray_index(verts, faces, cell=None, big_face=MESH_DIST_BIG_FACE, pad=None):
    """The MeshIndex that mesh_ray_cast builds, to be cast at many times: mesh_index with the defaults of ray casting -
    pad = mesh_ray_pad(verts) for None (taken from the box the build reads anyway), and without `cell` the edge
    sqrt(24 A / F), about 2.75 bounding-box edges of a marching-cubes face, where scripts/mesh_ray_time.py's sweep is
    fastest.  Neither changes a result for a given pad."""
    return MeshIndex(verts, faces, cell, big_face, pad, _per_cell=_MR_PER_CELL, _auto_pad=True)


def mesh_ray_cast(origins, dirs, verts, faces, t_min=0.0, t_max=math.inf, pad=None, cell=None,
                  big_face=MESH_DIST_BIG_FACE, return_uv=True, return_point=False):
    """(t [m] fp32, face [m] int32, then uv [m,2] fp32 with return_uv, then point [m,3] fp32 with return_point): for
    every ray origins[i] + t * dirs[i], t_min <= t <= t_max (numbers or [m] fp32 tensors, both ends inclusive, t_max
    may be inf), the first face of the triangle mesh it meets: the ray parameter t (the Euclidean distance for a unit
    direction), the face, its barycentric (u, v) (the hit is (1-u-v) a + u b + v c) and the point o + t d.  The result
    is the brute-force fp32 argmin of the per-face value that include/hashmod.h defines (tests/mesh_ray_cases.ray_ref
    is its numpy restatement): the smallest t, the lowest face index among equal t, bit for bit, independent of the
    grid, of big_face, of m and of the ray and thread order.  Both windings hit; a miss (a zero direction included)
    gives t = inf, face -1, NaN uv and point.  `pad` is part of the definition (a hit point must lie in its face's
    bounding box grown by pad): None takes mesh_ray_pad(verts).  No claim of watertightness.  m = 0 gives empty
    outputs; contiguous fp32 tensors on one GPU (else ValueError); a non-finite origin, direction or t_min, or a NaN
    t_max, raises HashmodError.  mesh_ray_index(verts, faces, cell, big_face, pad).ray_cast(origins, dirs, ...) is the
    same in two steps.  Not graph-capturable."""
    _check_cloud("mesh_ray_cast", "origins", origins)
    _check_cloud("mesh_ray_cast", "dirs", dirs, origins)
    _check_flags("mesh_ray_cast", return_uv=return_uv, return_point=return_point)
    if pad is not None:
        pad = _ray_pad("mesh_ray_cast", pad)
    if origins.shape[0] != dirs.shape[0]:
        raise ValueError("hashmod mesh_ray_cast: origins and dirs must have the same number of rows")
    for name, value, default in (("t_min", t_min, 0.0), ("t_max", t_max, math.inf)):
        _ray_bound("mesh_ray_cast", name, value, default, int(origins.shape[0]), origins)
    index = mesh_ray_index(verts, faces, cell, big_face, pad)
    return index.ray_cast(origins, dirs, t_min, t_max, return_uv, return_point)


def mesh_closest_point(query, verts, faces, max_dist=None, cell=None, big_face=MESH_DIST_BIG_FACE, return_point=True,
                       return_feature=False):
    """(d2 [m] fp32, face [m] int32, then point [m,3] fp32 with return_point, then feature [m] int32 with
    return_feature): for every row of query [m,3] the exact closest point of the triangle mesh, the face it lies on,
    that face's feature (0 the interior, 1, 2, 3 the edges (a,b), (b,c), (c,a) with their end points) and the squared
    distance.  The result is the brute-force fp32 argmin of the per-face value that include/hashmod.h defines
    (tests/mesh_dist_cases.closest_ref is its numpy restatement), the lowest face index among equal d2, bit for bit:
    independent of the grid, of big_face, of m and of the thread order.  With max_dist, a query whose d2 exceeds
    fp32(max_dist)^2 (squared in fp32) gets d2 = inf, face -1, a NaN point and feature -1; d2 equal to the bound is
    reported (nearest_neighbors' rule).  m = 0 gives empty outputs; F >= 1; contiguous tensors on one GPU (else
    ValueError); a non-finite coordinate or a face index outside [0, V) raises HashmodError.  mesh_index(verts, faces,
    cell, big_face).query(query, max_dist, ...) is the same in two steps.  Not graph-capturable."""
    _check_cloud("mesh_closest_point", "query", query)
    _check_flags("mesh_closest_point", return_point=return_point, return_feature=return_feature)
    md2 = _max_dist2("mesh_closest_point", max_dist)
    index = MeshIndex(verts, faces, cell, big_face)
    if query.device != index.device:
        raise ValueError("hashmod mesh_closest_point: the tensors are on different devices")
    return tuple(t for t in index._query(query, md2, return_point, return_feature) if t is not None)


def _point_mesh_sums(src, index, max_dist):
    """(sum, count, max) as one fp64 [3] device tensor of the distances src -> the index's mesh below max_dist, and
    d2; the rule and the reduction of _one_sided"""
    d2 = index._query(src, _search_bound2(max_dist), return_point=False)[0]
    d = torch.sqrt(d2.to(torch.float64))
    keep = d < max_dist if max_dist is not None else torch.ones_like(d, dtype=torch.bool)
    zero = torch.zeros((), dtype=torch.float64, device=d.device)
    kept = torch.where(keep, d, zero)
    return torch.stack([kept.sum(), keep.sum().to(torch.float64), kept.max()]), d2


def point_mesh_distance(src, mesh_or_index, max_dist=None):
    """(mean, count): the mean over the rows of src [m,3] of the exact distance to the mesh - a MeshIndex or a
    (verts, faces) pair - over the distances < max_dist (strict; all for None), and how many entered: what
    one_sided_distance is against a cloud, against the triangles themselves, so that it can stand in the same
    formulas.  The distances are the fp64 square roots of mesh_closest_point's exact fp32 d2, summed by the same
    fixed-order fp64 device reduction.  An empty src, or no distance below max_dist, gives (nan, 0).  Host scalars;
    not graph-capturable."""
    _check_cloud("point_mesh_distance", "src", src)
    if max_dist is not None and not (isinstance(max_dist, (int, float)) and max_dist > 0):
        raise ValueError("hashmod point_mesh_distance: max_dist must be a positive number (or None)")
    index = _as_mesh_index("point_mesh_distance", mesh_or_index)
    if src.shape[0] < 1:
        return math.nan, 0
    s, c, _ = _point_mesh_sums(src, index, max_dist)[0].tolist()
    return (s / c if c else math.nan), int(c)


def _as_mesh_index(what, mesh_or_index):
    if isinstance(mesh_or_index, MeshIndex):
        return mesh_or_index
    if isinstance(mesh_or_index, (tuple, list)) and len(mesh_or_index) == 2:
        return MeshIndex(mesh_or_index[0], mesh_or_index[1])
    raise ValueError(f"hashmod {what}: the mesh must be a MeshIndex or a (verts, faces) pair")


# =========================================================================================
# Signed distance to the mesh: pseudo-normal tables and the sign of a closest-point result (csrc/hm_mesh_topo.hip)
# =========================================================================================
_MT_WS = _lib.Workspace("mesh_topology")
_MT_MAX_FACES = ((1 << 31) - 1) // 3


class MeshTopology:
    """The two pseudo-normal tables of a triangle mesh that ops.mesh_topology builds - vertex_normals [V,3] fp64 (the
    angle-weighted sum of the unit normals of a vertex's faces, zero for a vertex no face names) and edge_normals
    [F,3,3] fp64 (per half-edge, the sum of the unit normals of ALL faces on its edge) - and what the half-edges say
    about the mesh: boundary_edges (edges of one face), nonmanifold_edges (of more than two), flipped_edges (of two
    faces that traverse it in the same direction), and closed, true when all three are 0.  It keeps verts and faces
    (not copies): MeshIndex.signed_distance reads the winning face's vertices from them."""

    def __init__(self, verts, faces):
        what = "mesh_topology"
        if not isinstance(verts, torch.Tensor) or not isinstance(faces, torch.Tensor):
            raise ValueError(f"hashmod {what}: verts and faces must be tensors")
        if faces.dim() == 2 and faces.shape[0] < 1:
            raise ValueError(f"hashmod {what}: at least one face is needed")
        if faces.dim() == 2 and faces.shape[0] > _MT_MAX_FACES:
            raise ValueError(f"hashmod {what}: 3 F must be below 2^31")
        _check_on_gpu(what, verts, faces)
        n_faces, n_verts = _check_mesh(what, faces, verts=verts, gpu_first=False)
        dev = faces.device
        if n_verts < 1:
            raise _lib.HashmodError(f"hashmod {what}: a face index lies outside [0, n_verts)")
        self.verts, self.faces = verts, faces
        self.n_faces, self.n_verts = n_faces, n_verts
        self.device = dev
        self.vertex_normals = torch.empty((n_verts, 3), dtype=torch.float64, device=dev)
        self.edge_normals = torch.empty((n_faces, 3, 3), dtype=torch.float64, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        L = lib()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _MT_WS.get(dev, check(L.hm_mesh_topology_workspace_bytes(n_faces)))
        check(L.hm_mesh_topology_build(dptr(verts), dptr(faces), n_faces, n_verts, dptr(self.vertex_normals),
                                       dptr(self.edge_normals), dptr(counts), dptr(ws), ws.numel(), dptr(status),
                                       stream_ptr(faces)))
        # one host read: the three counts and the status word
        b, n, f, bad = torch.cat([counts, status.to(torch.int64)]).tolist()
        if bad & 1:
            _check_mesh_status(what, status)
        if bad:
            raise _lib.HashmodError(f"hashmod {what}: a vertex of a face has a non-finite coordinate")
        self.boundary_edges, self.nonmanifold_edges, self.flipped_edges = b, n, f
        self.closed = b == 0 and n == 0 and f == 0

    def __repr__(self):
        return (f"MeshTopology(n_verts={self.n_verts}, n_faces={self.n_faces}, boundary_edges={self.boundary_edges}, "
                f"nonmanifold_edges={self.nonmanifold_edges}, flipped_edges={self.flipped_edges})")


def mesh_topology(verts, faces):
    """The MeshTopology of the mesh verts [V,3] fp32, faces [F,3] int32 (F >= 1, 3 F < 2^31): the angle-weighted
    pseudo-normals of Baerentzen and Aanaes as two fp64 tables and the counts of boundary, non-manifold and flipped
    edges, by the definition of include/hashmod.h (tests/mesh_sign_cases.topology_ref is its numpy restatement).  The
    corners are sorted by vertex and the half-edges by their vertex pair with the library's stable radix sort, and one
    lane sums each run in sorted order: no floating-point atomics, the same bits whatever the thread order; the edge
    table and the counts equal the restatement bit for bit, the vertex table up to the device's atan2.  Contiguous
    tensors on one GPU (else ValueError); a face index outside [0, V) or a non-finite vertex of a face raises
    HashmodError (reported by the kernel's status word, never dereferenced).  One host read, so not
    graph-capturable."""
    return MeshTopology(verts, faces)


def _mesh_sign(index, topology, query, max_dist2, want_sign):
    """(sd, sign or None, d2, face, point) of the queries: the closest-point query, then the sign kernel"""
    what = "mesh_signed_distance"
    if not isinstance(topology, MeshTopology):
        raise ValueError(f"hashmod {what}: topology must be a MeshTopology (ops.mesh_topology)")
    if (topology.n_faces != index.n_faces or topology.n_verts != index.n_verts or topology.device != index.device):
        raise ValueError(f"hashmod {what}: the topology is not of the index's mesh (n_faces, n_verts and device must "
                         "agree)")
    d2, face, point, feature = index._query(query, max_dist2, True, True)
    m = int(query.shape[0])
    dev = index.device
    sd = torch.empty(m, dtype=torch.float32, device=dev)
    sign = torch.empty(m, dtype=torch.int32, device=dev) if want_sign else None
    if m:
        check(lib().hm_mesh_sign(dptr(query), m, dptr(face), dptr(feature), dptr(point), dptr(d2),
                                 dptr(topology.verts), dptr(topology.faces), topology.n_faces, topology.n_verts,
                                 dptr(topology.vertex_normals), dptr(topology.edge_normals), dptr(sd), dptr(sign),
                                 stream_ptr(query)))
    return sd, sign, d2, face, point


def mesh_signed_distance(query, verts, faces, max_dist=None, cell=None, big_face=MESH_DIST_BIG_FACE, return_sign=False,
                         return_face=False, return_point=False):
    """sd [m] fp32 (then sign [m] int32 with return_sign, face [m] int32 with return_face, point [m,3] fp32 with
    return_point; a tuple when more than sd is asked for): for every row of query [m,3] the signed distance to the
    triangle mesh, negative inside.  |sd| is the fp32 square root of mesh_closest_point's exact d2; the sign is the
    sign of dot(q - closest point, N), N the angle-weighted pseudo-normal of the feature the closest point lies on -
    the face's normal, its edge's, or its vertex's (Baerentzen and Aanaes) - by the definition of include/hashmod.h
    (tests/mesh_sign_cases.sign_ref is its numpy restatement): a function of the closest-point result and
    mesh_topology's two tables and of nothing else, so independent of the grid, of big_face, of m and of the thread
    order.  It is the inside/outside of a closed, consistently wound mesh (MeshTopology.closed); elsewhere it is
    still defined - above an open sheet is +, below it -.  A zero dot product is outside (+1): a query on the surface,
    a zero pseudo-normal.  A query cut by max_dist gets sd = +inf, sign 0.  m = 0 gives empty outputs.  mesh_index(...)
    .signed_distance(query, mesh_topology(verts, faces), ...) is the same in two steps.  Not graph-capturable."""
    _check_cloud("mesh_signed_distance", "query", query)
    _check_flags("mesh_signed_distance", return_sign=return_sign, return_face=return_face, return_point=return_point)
    _max_dist2("mesh_signed_distance", max_dist)
    index = MeshIndex(verts, faces, cell, big_face)
    if query.device != index.device:
        raise ValueError("hashmod mesh_signed_distance: the tensors are on different devices")
    return index.signed_distance(query, MeshTopology(verts, faces), max_dist, return_sign, return_face, return_point)


def _as_signed_mesh(what, mesh):
    """(MeshIndex, MeshTopology) of a (MeshIndex, MeshTopology) or a (verts, faces) pair"""
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        if isinstance(mesh[0], MeshIndex) and isinstance(mesh[1], MeshTopology):
            return mesh[0], mesh[1]
        if isinstance(mesh[0], torch.Tensor) and isinstance(mesh[1], torch.Tensor):
            return MeshIndex(mesh[0], mesh[1]), MeshTopology(mesh[0], mesh[1])
    raise ValueError(f"hashmod {what}: the mesh must be a (MeshIndex, MeshTopology) or a (verts, faces) pair")


def mesh_contains(query, mesh):
    """inside [m] bool: mesh_signed_distance's sign < 0 for the rows of query [m,3]; `mesh` is a (MeshIndex,
    MeshTopology) pair of one mesh or a (verts, faces) pair.  A query on the surface is outside.  Meaningful for a
    closed mesh (MeshTopology.closed).  An index built with a pad gives the same result: the closest-point query is
    exact on it."""
    _check_cloud("mesh_contains", "query", query)
    index, topology = _as_signed_mesh("mesh_contains", mesh)
    return _mesh_sign(index, topology, query, math.inf, True)[1] < 0


# =========================================================================================
# The rest of the DTU evaluation: greedy radius down-sampling, mask and plane filters (csrc/hm_nn_radius.hip,
# csrc/hm_dtu_filter.hip)
# =========================================================================================
_NR_WS = _lib.Workspace("radius_downsample")
_NR_BATCH = 4               # rounds launched between two host reads of the remaining count
_NR_TAIL = 1024             # hm_nn_radius_rounds finishes a list this short in one workgroup


def radius_downsample(points, radius, cell=None, stats=None):
    """keep [n] bool: DTU's greedy down-sampling of points [n,3] fp32 -
        mask = ones; for i in range(n): if mask[i]: mask[neighbours of i within radius] = 0; mask[i] = 1
    - on the device.  Index order is the greedy order (shuffle beforehand, as DTU does).  j is a neighbour of i when the
    fp32 value d2 = (dx*dx + dy*dy) + dz*dz of nearest_neighbors is <= fp32(radius)^2 (squared in fp32); equality
    counts, as in sklearn's radius_neighbors.  A point is kept exactly when none of its lower-index neighbours is kept,
    which csrc/hm_nn_radius.hip finds in rounds on nn_index's grid; the result is the sequential loop's, bit for bit,
    whatever the grid (`cell`, nn_index's argument, changes the speed only) and the thread order.  Shuffled clouds take
    a handful of rounds, an ordered one up to n.  The loop below ends when the device reports no undecided point and
    has no other exit.  stats: a dict that receives "rounds".  radius > 0 and finite, also as fp32 (else ValueError);
    n = 0 gives an empty mask; a non-finite coordinate raises HashmodError.  Host reads of the count between batches of
    rounds, so not graph-capturable."""
    _check_cloud("radius_downsample", "points", points)
    if not (isinstance(radius, (int, float)) and math.isfinite(radius) and radius > 0):
        raise ValueError("hashmod radius_downsample: radius must be a positive finite number")
    r32 = np.float32(radius)
    if not (r32 > 0 and np.isfinite(r32)):
        raise ValueError("hashmod radius_downsample: radius must be positive and finite in fp32")
    radius2 = _max_dist2("radius_downsample", float(radius))
    # an outward estimate of the largest per-axis offset inside the radius; the kernel checks and widens it per point
    bound = float(min(np.nextafter(np.float32(max(math.sqrt(min(radius2, 3.0e38)), float(r32)) * (1.0 + 2.0 ** -20)),
                                   np.float32(np.inf)), np.float32(3.0e38)))
    n = int(points.shape[0])
    if stats is not None:
        stats["rounds"] = 0
    if n == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device)
    index = NNIndex(points, cell)
    dev = index.device
    L = lib()
    st = stream_ptr(points)
    ws = _NR_WS.get(dev, check(L.hm_nn_radius_workspace_bytes(n)))
    info = torch.empty(4, dtype=torch.int32, device=dev)
    check(L.hm_nn_radius_begin(n, dptr(ws), ws.numel(), dptr(info), st))
    remaining, rounds = n, 0
    while remaining > 0:
        # a list of at most _NR_TAIL points is finished by one workgroup, which leaves the count in the same word
        check(L.hm_nn_radius_rounds(dptr(index.records), n, dptr(index.cell_start), index._lo(), index.h, index._g(),
                                    radius2, bound, remaining, rounds, _NR_BATCH, dptr(ws), ws.numel(), dptr(info), st))
        if remaining > _NR_TAIL:
            rounds += _NR_BATCH
        remaining = info.tolist()[rounds & 1]
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    check(L.hm_nn_radius_finish(dptr(index.records), n, dptr(ws), ws.numel(), dptr(keep), st))
    if stats is not None:
        stats["rounds"] = int(info[2].item())
    return keep.view(torch.bool)


DTU_INBOUND, DTU_IN_MASK, DTU_ABOVE_PLANE = 1, 2, 4


def _dtu_params(what, obs_mask, bb, res, patch, plane):
    """(shape (c_int64 * 3), params (c_double * 14)) of hm_dtu_point_flags from the scan's data, checked"""
    if (not isinstance(obs_mask, torch.Tensor) or obs_mask.dtype != torch.uint8 or obs_mask.dim() != 3
            or not obs_mask.is_contiguous() or obs_mask.numel() == 0):
        raise ValueError(f"hashmod {what}: obs_mask must be a non-empty contiguous uint8 [X, Y, Z] tensor")
    try:
        bb = np.asarray(bb, np.float64)
        plane = np.asarray(plane, np.float64).reshape(-1)
        res, patch = float(res), float(patch)
    except (TypeError, ValueError):
        raise ValueError(f"hashmod {what}: bb [2,3], res, patch and plane [4] must be numbers") from None
    if bb.shape != (2, 3) or plane.shape != (4,):
        raise ValueError(f"hashmod {what}: bb must be [2,3] and plane [4]")
    if not (np.isfinite(bb).all() and np.isfinite(plane).all() and math.isfinite(res) and res > 0
            and math.isfinite(patch)):
        raise ValueError(f"hashmod {what}: bb, plane and patch must be finite, res finite and positive")
    params = np.concatenate([bb[0] - patch, bb[1] + patch * 2, bb[0], [res], plane])
    return (C.c_int64 * 3)(*obs_mask.shape), (C.c_double * 14)(*params.tolist())


def dtu_point_flags(points, obs_mask, bb, res, patch, plane):
    """flags [n] uint8 of points [n,3] fp32 against a DTU scan's data (evaluation.chamfer.load_dtu_scan): bit 0
    (DTU_INBOUND) bb[0] - patch <= p < bb[1] + 2*patch on all axes; bit 1 (DTU_IN_MASK) the voxel
    k = rint((p - bb[0])/res) (half to even, np.around) lies inside obs_mask [X,Y,Z] uint8 and is set there; bit 2
    (DTU_ABOVE_PLANE) ((P0*x + P1*y) + P2*z) + P3 > 0.  fp64 on the fp32 coordinates, every operation rounded once:
    tests/dtu_cases.flags_ref gives the same bits.  A non-finite coordinate gives 0; no voxel outside the volume is
    read.  bb [2,3], res, patch and plane [4] are host values.  n = 0 gives an empty tensor.  No host read."""
    _check_cloud("dtu_point_flags", "points", points)
    shape, params = _dtu_params("dtu_point_flags", obs_mask, bb, res, patch, plane)
    if obs_mask.device != points.device:
        raise ValueError("hashmod dtu_point_flags: the tensors are on different devices")
    require_gpu(points)
    n = int(points.shape[0])
    flags = torch.empty(n, dtype=torch.uint8, device=points.device)
    if n:
        check(lib().hm_dtu_point_flags(dptr(points), n, dptr(obs_mask), shape, params, dptr(flags), stream_ptr(points)))
    return flags


# =========================================================================================
# Image metrics of rendered views: PSNR over a mask and SSIM (csrc/hm_image.hip)
# =========================================================================================
_IMG_WS = _lib.Workspace("image metrics")
SSIM_TILE = (16, 16)        # window positions (rows, columns) one workgroup of hm_image_ssim scores
SQERR_PIXELS = 1024         # pixels one workgroup of hm_image_sqerr sums
SSIM_MAX_WIN = 31


def _check_images(what, x, y):
    """(x, y) as contiguous fp32 [B, H, W, C] on one device, 1 <= C <= 4; [H, W, C] becomes B = 1"""
    for name, t in (("x", x), ("y", y)):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (3, 4)
                or not t.is_contiguous()):
            raise ValueError(f"hashmod {what}: contiguous fp32 {name} [B, H, W, C] or [H, W, C] expected")
    if x.shape != y.shape:
        raise ValueError(f"hashmod {what}: x {tuple(x.shape)} and y {tuple(y.shape)} differ in shape")
    if x.device != y.device:
        raise ValueError(f"hashmod {what}: the tensors are on different devices")
    if x.dim() == 3:
        x, y = x[None], y[None]
    B, H, W, Cn = x.shape
    if not 1 <= Cn <= 4:
        raise ValueError(f"hashmod {what}: C must be in [1, 4], got {Cn}")
    if min(B, H, W) < 1 or max(B, H, W) >= 1 << 31:
        raise ValueError(f"hashmod {what}: B, H and W must be in [1, 2^31)")
    return x, y


def _check_data_range(what, data_range):
    if not (isinstance(data_range, (int, float)) and not isinstance(data_range, bool) and math.isfinite(data_range)
            and data_range > 0):
        raise ValueError(f"hashmod {what}: data_range must be a positive finite number")
    return float(data_range)


def image_psnr(x, y, mask=None, data_range=1.0):
    """psnr [B] fp64 (device) of the images x, y [B, H, W, C] fp32, contiguous, 1 <= C <= 4 ([H, W, C]: B = 1) - the
    reference's calculate_psnr.  mask: None or [B, H, W] bool / uint8 on the same device; n_b = its set pixels of image
    b (H*W without a mask), mse_b = sum over the set pixels and their channels of (x - y)^2 / (n_b * C),
    psnr_b = 10 log10(data_range^2 / mse_b); mse_b == 0 gives +inf and n_b == 0 nan.  Pixels outside the mask are not
    read.  Differences, squares and sums are fp64; the sum is a fixed-order two-stage reduction without atomics, so two
    calls give the same bits.  A wrong dtype, shape, device, contiguity, C, data_range or mask raises ValueError before
    the GPU is touched.  No host read; the partials' buffer is a module workspace, so capture only after a warm-up."""
    x, y = _check_images("image_psnr", x, y)
    L2 = _check_data_range("image_psnr", data_range) ** 2
    B, H, W, Cn = x.shape
    if mask is not None:
        if (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8)
                or not mask.is_contiguous()):
            raise ValueError("hashmod image_psnr: mask must be a contiguous bool or uint8 tensor")
        if tuple(mask.shape) not in ((B, H, W), (H, W)) or (mask.dim() == 2 and B != 1):
            raise ValueError(f"hashmod image_psnr: mask {tuple(mask.shape)} is not [B, H, W] = {(B, H, W)}")
        if mask.device != x.device:
            raise ValueError("hashmod image_psnr: mask is on a different device than the images")
    require_gpu(x)
    lib_ = lib()
    ws = _IMG_WS.get(x.device, check(lib_.hm_image_sqerr_workspace_bytes(B, H, W)))
    out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    check(lib_.hm_image_sqerr(dptr(x), dptr(y), dptr(mask), B, H, W, Cn, dptr(ws), dptr(out), stream_ptr(x)))
    return 10.0 * torch.log10(L2 / (out[:, 0] / (out[:, 1] * Cn)))


def ssim_window(win=11, sigma=1.5):
    """the win fp64 weights g(r) ~ exp(-(r - (win-1)/2)^2 / (2 sigma^2)) normalised to sum 1 (numpy); the SSIM window
    is their outer product"""
    if not (isinstance(win, int) and not isinstance(win, bool) and 3 <= win <= SSIM_MAX_WIN and win % 2 == 1):
        raise ValueError(f"hashmod image_ssim: win must be an odd integer in [3, {SSIM_MAX_WIN}]")
    if not (isinstance(sigma, (int, float)) and math.isfinite(sigma) and sigma > 0):
        raise ValueError("hashmod image_ssim: sigma must be a positive finite number")
    r = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    g = np.exp(-(r * r) / (2.0 * float(sigma) ** 2))
    return g / g.sum()


def image_ssim(x, y, data_range=1.0, win=11, sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """ssim [B] fp64 (device) of the images x, y [B, H, W, C] fp32, contiguous, 1 <= C <= 4 ([H, W, C]: B = 1): SSIM of
    Wang et al. 2004 with the win x win Gaussian window g(i) g(j), g = ssim_window(win, sigma), C1 = (k1 data_range)^2,
    C2 = (k2 data_range)^2 - the torchmetrics defaults, skimage with gaussian_weights=True,
    use_sample_covariance=False.  For every window wholly inside the image, (H-win+1)(W-win+1) positions per channel
    and no padding (both libraries pad and crop the same border away), the weighted moments mx, my, Exx, Eyy, Exy,
    sx2 = Exx - mx^2, sy2 = Eyy - my^2, sxy = Exy - mx my and
        s = ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2));
    ssim_b is the mean of s over positions and channels.  Moments, formula and mean are fp64 from the fp32 values, the
    mean a fixed-order two-stage reduction without atomics: two calls give the same bits and image_ssim(x, x) is
    exactly 1.  return_map=True returns (ssim, map) with map [B, H-win+1, W-win+1, C] fp64 = s.  win odd in [3, 31];
    H < win or W < win, a wrong dtype, shape, device, contiguity, C, data_range, k1 or k2 raise ValueError before the
    GPU is touched.  SSIM_TILE is the block of positions one workgroup scores.  The weights are uploaded per call (a
    host-to-device copy) and the partials' buffer is a module workspace: not graph-capturable."""
    x, y = _check_images("image_ssim", x, y)
    L = _check_data_range("image_ssim", data_range)
    weights = ssim_window(win, sigma)
    for name, k in (("k1", k1), ("k2", k2)):
        if not (isinstance(k, (int, float)) and math.isfinite(k) and k > 0):
            raise ValueError(f"hashmod image_ssim: {name} must be a positive finite number")
    B, H, W, Cn = x.shape
    if H < win or W < win:
        raise ValueError(f"hashmod image_ssim: the image {H} x {W} is smaller than the {win} x {win} window")
    c1, c2 = (float(k1) * L) ** 2, (float(k2) * L) ** 2
    if not (c1 > 0 and c2 > 0 and math.isfinite(c1) and math.isfinite(c2)):
        raise ValueError("hashmod image_ssim: (k1 data_range)^2 and (k2 data_range)^2 must be positive and finite")
    require_gpu(x)
    lib_ = lib()
    dev = x.device
    ws = _IMG_WS.get(dev, check(lib_.hm_image_ssim_workspace_bytes(B, H, W, win)))
    wdev = torch.from_numpy(weights).to(dev)
    out = torch.empty(B, dtype=torch.float64, device=dev)
    smap = torch.empty((B, H - win + 1, W - win + 1, Cn), dtype=torch.float64, device=dev) if return_map else None
    check(lib_.hm_image_ssim(dptr(x), dptr(y), B, H, W, Cn, win, dptr(wdev), c1, c2, dptr(smap), dptr(ws), dptr(out),
                             stream_ptr(x)))
    return (out, smap) if return_map else out


# =========================================================================================
# Mesh culling by camera masks and visibility (csrc/hm_mesh_cull.hip, DESIGN.md "Mesh culling on the device")
# =========================================================================================
_CULL_WS = _lib.Workspace("mesh_depth_maps")
CULL_BIG_FACE = 64          # pixels of a face's clamped bounding box above which one wave draws it instead of one lane
CULL_MAX_IMAGE = 65536      # H and W; and H*W < 2^31
CULL_MAX_PAD = 64


def _check_views(what, verts, proj, H=None, W=None):
    """(V, n) after the checks the vote and raster ops share: contiguous fp32 verts [V,3]; proj float64 [n,3,4] as a
    numpy array or a tensor; the image size, when given, within the kernels' range"""
    _check_cloud(what, "verts", verts)
    if isinstance(proj, torch.Tensor):
        ok = proj.dtype == torch.float64 and proj.dim() == 3 and tuple(proj.shape[1:]) == (3, 4)
    else:
        ok = isinstance(proj, np.ndarray) and proj.dtype == np.float64 and proj.ndim == 3 and proj.shape[1:] == (3, 4)
    if not ok:
        raise ValueError(f"hashmod {what}: float64 proj [n, 3, 4] expected (evaluation.cull.view_projections)")
    if H is not None:
        if not (isinstance(H, int) and isinstance(W, int) and 1 <= H <= CULL_MAX_IMAGE and 1 <= W <= CULL_MAX_IMAGE
                and H * W < 1 << 31):
            raise ValueError(f"hashmod {what}: H and W must be integers in [1, {CULL_MAX_IMAGE}] with H*W < 2^31")
    return int(verts.shape[0]), int(proj.shape[0])


def _device_proj(proj, device):
    if not isinstance(proj, torch.Tensor):
        proj = torch.from_numpy(np.ascontiguousarray(proj))
    return proj.to(device).contiguous()


def _mask_table(masks):
    """the summed-area table [n, H+1, W+1] int32 of masks [n, H, W]: table[v, r, c] = the non-zero pixels of view v in
    rows < r and columns < c (torch plumbing: n*H*W adds, once per scan)"""
    n, H, W = masks.shape
    sat = torch.zeros((n, H + 1, W + 1), dtype=torch.int32, device=masks.device)
    sat[:, 1:, 1:] = torch.cumsum(torch.cumsum(masks != 0, 2, dtype=torch.int32), 1, dtype=torch.int32)
    return sat


def mesh_mask_votes(verts, proj, masks, dilate, table_bytes=1 << 28):
    """(n_in_image [V] int32, n_in_mask [V] int32) of verts [V,3] fp32 against the views proj [n,3,4] float64 (host or
    device) and their masks [n,H,W] bool or uint8 on the device.  A view counts in n_in_image iff the vertex is
    projectable (finite, w finite and > 0, p = P @ (x, y, z, 1) in fp64 rounded once per operation) and its pixel
    (rint(u), rint(v)), half to even, is in the image; it also counts in n_in_mask iff a mask pixel within `dilate`
    pixels (a (2 dilate + 1)^2 square, cv2.dilate with ones; zero outside the image) is non-zero.  The masks become a
    summed-area table by two torch.cumsum calls, `table_bytes` of it at a time, and one lane per vertex loops over the
    views with four table reads each; no atomics.  tests/mesh_cull_cases.mask_votes_ref gives the same bits."""
    n_verts, n_views = _check_views("mesh_mask_votes", verts, proj)
    if (not isinstance(masks, torch.Tensor) or masks.dtype not in (torch.bool, torch.uint8) or masks.dim() != 3
            or masks.shape[0] != n_views):
        raise ValueError("hashmod mesh_mask_votes: bool or uint8 masks [n, H, W] expected, one per view")
    H, W = int(masks.shape[1]), int(masks.shape[2])
    _check_views("mesh_mask_votes", verts, proj, H, W)
    if not (isinstance(dilate, int) and not isinstance(dilate, bool) and dilate >= 0):
        raise ValueError("hashmod mesh_mask_votes: dilate must be an integer >= 0")
    if masks.device != verts.device:
        raise ValueError("hashmod mesh_mask_votes: the tensors are on different devices")
    require_gpu(verts, masks)
    dev = verts.device
    proj = _device_proj(proj, dev)
    n_img = torch.zeros(n_verts, dtype=torch.int32, device=dev)
    n_msk = torch.zeros(n_verts, dtype=torch.int32, device=dev)
    per = max(1, int(table_bytes) // (4 * (H + 1) * (W + 1)))
    for v0 in range(0, n_views, per):
        sat = _mask_table(masks[v0:v0 + per])
        check(lib().hm_mesh_mask_votes(dptr(verts), n_verts, dptr(proj[v0:]), int(sat.shape[0]), dptr(sat), H, W,
                                       min(dilate, CULL_MAX_IMAGE), 1 if v0 else 0, dptr(n_img), dptr(n_msk),
                                       stream_ptr(verts)))
    return n_img, n_msk


def mesh_depth_maps(verts, faces, proj, H, W, big_face=CULL_BIG_FACE):
    """(depth [n,H,W] fp32, n_skipped [n] int32): the mesh's nearest surface per pixel of every view, +inf where nothing
    is drawn.  Per view every vertex is projected once (fixed-point X = rint(256 u), Y = rint(256 v) and 1/w); a face
    with an unprojectable corner or a position beyond |X|, |Y| < 2^24 is skipped and counted - there is NO clipping:
    the cameras are expected outside the object.  Coverage: the pixel centres (256 col, 256 row) of the face's clamped
    bounding box whose three int64 edge functions are all >= 0 or all <= 0 (both windings, inclusive edges; zero area
    draws nothing).  Depth: perspective-correct, z = 1/((b0/w0 + b1/w1) + b2/w2) in fp64 rounded once per operation,
    then to fp32, kept when finite and > 0 by an unsigned atomicMin on its bits - the result does not depend on the
    order of the faces and two calls give the same bits (tests/mesh_cull_cases.depth_map_ref gives them too).  A face
    whose clamped box exceeds `big_face` pixels is listed and drawn by one wave, any other by one lane.  A face index
    outside [0, V) raises HashmodError.  One host read of the status word; not graph-capturable."""
    n_verts, n_views = _check_views("mesh_depth_maps", verts, proj, H, W)
    if not (isinstance(big_face, int) and big_face >= 1):
        raise ValueError("hashmod mesh_depth_maps: big_face must be an integer >= 1")
    n_faces, _ = _check_mesh("mesh_depth_maps", faces, verts=verts, gpu_first=False)
    dev = verts.device
    proj = _device_proj(proj, dev)
    depth = torch.empty((n_views, H, W), dtype=torch.float32, device=dev)
    n_skipped = torch.empty(n_views, dtype=torch.int32, device=dev)
    if n_views == 0:
        return depth, n_skipped
    L = lib()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _CULL_WS.get(dev, check(L.hm_mesh_depth_workspace_bytes(n_verts, n_faces)))
    check(L.hm_mesh_depth_maps(dptr(verts), n_verts, dptr(faces), n_faces, dptr(proj), n_views, H, W, big_face,
                               dptr(depth), dptr(n_skipped), dptr(ws), ws.numel(), dptr(status), stream_ptr(verts)))
    _check_mesh_status("mesh_depth_maps", status)
    return depth, n_skipped


def mesh_visible_votes(verts, proj, depth, pad=1, tol=0.0, out=None):
    """n_visible [V] int32: the views of proj [n,3,4] in which the vertex is projectable, in the image, and
    float32(w) <= m + float32(tol), m = the maximum of depth [n,H,W] (mesh_depth_maps) over the (2 pad + 1)^2 pixels
    around the vertex' pixel, indices clamped to the image.  The neighbourhood maximum makes the rule conservative: a
    marching-cubes vertex rarely projects onto the pixel centre its own faces were sampled at, so the single-pixel rule
    (pad = 0) loses about half of the front-facing vertices, and a depth tolerance does not bring all of them back;
    with pad = 1, tol = 0 none is lost.  The price is that back-facing vertices within `pad` pixels of the silhouette
    also count as visible: for culling, keeping too much at the rim is the right direction.  `out` [V] int32, when
    given, is added to (the next chunk of views) and returned."""
    n_verts, n_views = _check_views("mesh_visible_votes", verts, proj)
    if (not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.dim() != 3
            or depth.shape[0] != n_views or not depth.is_contiguous()):
        raise ValueError("hashmod mesh_visible_votes: contiguous fp32 depth [n, H, W] expected, one map per view")
    H, W = int(depth.shape[1]), int(depth.shape[2])
    _check_views("mesh_visible_votes", verts, proj, H, W)
    if not (isinstance(pad, int) and not isinstance(pad, bool) and 0 <= pad <= CULL_MAX_PAD):
        raise ValueError(f"hashmod mesh_visible_votes: pad must be an integer in [0, {CULL_MAX_PAD}]")
    if not (isinstance(tol, (int, float)) and not math.isnan(tol)):
        raise ValueError("hashmod mesh_visible_votes: tol must be a number")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.shape != (n_verts,)
                            or not out.is_contiguous()):
        raise ValueError("hashmod mesh_visible_votes: contiguous int32 out [V] expected")
    for t in (depth, out):
        if t is not None and t.device != verts.device:
            raise ValueError("hashmod mesh_visible_votes: the tensors are on different devices")
    require_gpu(verts, depth, out)
    dev = verts.device
    proj = _device_proj(proj, dev)
    n_vis = torch.zeros(n_verts, dtype=torch.int32, device=dev) if out is None else out
    check(lib().hm_mesh_visible_votes(dptr(verts), n_verts, dptr(proj), n_views, dptr(depth), H, W, pad, float(tol),
                                      0 if out is None else 1, dptr(n_vis), stream_ptr(verts)))
    return n_vis


def mesh_keep_vertices(verts, faces, normals, keep):
    """(verts, faces, normals or None) of the faces whose three vertices have keep [V] bool set: the surviving vertices
    are those a surviving face uses, in ascending original order; the faces stay in order and are renumbered; the
    normals are gathered like the vertices - mesh_select's conventions (np.unique(faces[kept], return_inverse=True)),
    and its emit kernels.  A face index outside [0, V) raises HashmodError (reported by the kernel, never
    dereferenced).  One host read of the counts; not graph-capturable."""
    _check_cloud("mesh_keep_vertices", "verts", verts)
    if (not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.shape != (verts.shape[0],)
            or not keep.is_contiguous()):
        raise ValueError("hashmod mesh_keep_vertices: contiguous bool keep [V] expected")
    if keep.device != verts.device:
        raise ValueError("hashmod mesh_keep_vertices: the tensors are on different devices")
    n_faces, n_verts = _check_mesh("mesh_keep_vertices", faces, verts=verts, normals=normals, gpu_first=False)
    dev = faces.device
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    vflag = torch.zeros(n_verts, dtype=torch.int32, device=dev)
    fflag = torch.empty(n_faces, dtype=torch.int32, device=dev)
    check(lib().hm_mesh_keep_mark(dptr(faces), n_faces, n_verts, dptr(keep), dptr(vflag), dptr(fflag), dptr(status),
                                  stream_ptr(faces)))
    return _mesh_emit_flagged("mesh_keep_vertices", verts, faces, normals, vflag, fflag, status)


# =========================================================================================
# The mesh through a camera (csrc/hm_mesh_render.hip, DESIGN.md "Rendering the mesh")
# =========================================================================================
RENDER_MAX_ATTR = 16
MeshRender = namedtuple("MeshRender", ["face_id", "depth", "weights", "image", "n_skipped"])


def mesh_render(verts, faces, proj, H, W, attrs=None, background=0.0, big_face=CULL_BIG_FACE, return_weights=False):
    """MeshRender(face_id [n,H,W] int32, depth [n,H,W] fp32, weights [n,H,W,3] fp32 or None, image [n,H,W,C] fp32 or
    None, n_skipped [n] int32): the mesh seen by every view, with the vertex attributes attrs [V,C] fp32 (0 <= C <= 16)
    interpolated over the visible faces.

    Visibility.  The projection, the skipped and counted faces (NO clipping), the coverage of a pixel centre and the
    depth z of a covered pixel are mesh_depth_maps' - the same device functions - and so are `depth`'s bits.  A pixel
    keeps the smallest 64-bit key (float_bits(z) << 32) | face over the samples with z finite and > 0, by an unsigned
    64-bit atomicMin: the nearest sample and, among equal depths, the smallest face index, whatever the order in which
    the faces are drawn; two calls give the same bits.  A face whose clamped box exceeds `big_face` pixels is drawn by
    one wave, any other by one lane.

    Resolve (one lane per pixel, no atomics).  Nothing drawn: face_id = -1, depth = +inf, weights = 0, image =
    `background` (a float, or C floats).  Else, with b_m = E_m / area the screen-space barycentric weights of the face's
    corners and iw_m = 1 / w_m:  t_m = b_m iw_m,  s = (t_0 + t_1) + t_2,  weights[m] = float32(t_m / s),
    image[c] = float32((((t_0 a_0c) + (t_1 a_1c)) + (t_2 a_2c)) / s) - perspective-correct, every operation fp64 and
    rounded once, in this order; a NaN attribute propagates.  No anti-aliasing, no lighting.
    tests/mesh_render_cases.render_ref gives the same bits.

    A face index outside [0, V) raises HashmodError (reported by the kernel, never dereferenced).  One host read of
    the status word; not graph-capturable."""
    what = "mesh_render"
    n_verts, n_views = _check_views(what, verts, proj, H, W)
    if not (isinstance(big_face, int) and big_face >= 1):
        raise ValueError(f"hashmod {what}: big_face must be an integer >= 1")
    n_attr = 0
    if attrs is not None:
        if (not isinstance(attrs, torch.Tensor) or attrs.dtype != torch.float32 or attrs.dim() != 2
                or attrs.shape[0] != n_verts or attrs.shape[1] > RENDER_MAX_ATTR or not attrs.is_contiguous()):
            raise ValueError(f"hashmod {what}: contiguous fp32 attrs [V, C] with C <= {RENDER_MAX_ATTR} expected")
        if attrs.device != verts.device:
            raise ValueError(f"hashmod {what}: the tensors are on different devices")
        n_attr = int(attrs.shape[1])
    try:
        bg = np.asarray(background, np.float32)
        bg = np.ascontiguousarray(np.broadcast_to(bg, (n_attr,)) if bg.ndim == 0 else bg)
    except (TypeError, ValueError):
        bg = None
    if background is None or bg is None or bg.shape != (n_attr,):
        raise ValueError(f"hashmod {what}: background must be a float or a sequence of C floats")
    n_faces, _ = _check_mesh(what, faces, verts=verts, gpu_first=False)
    require_gpu(attrs)
    dev = verts.device
    proj = _device_proj(proj, dev)
    face_id = torch.empty((n_views, H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((n_views, H, W), dtype=torch.float32, device=dev)
    weights = torch.empty((n_views, H, W, 3), dtype=torch.float32, device=dev) if return_weights else None
    image = None if attrs is None else torch.empty((n_views, H, W, n_attr), dtype=torch.float32, device=dev)
    n_skipped = torch.empty(n_views, dtype=torch.int32, device=dev)
    if n_views == 0:
        return MeshRender(face_id, depth, weights, image, n_skipped)
    L = lib()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _CULL_WS.get(dev, check(L.hm_mesh_render_workspace_bytes(n_verts, n_faces, H, W)))
    given = n_attr > 0                 # C == 0: an empty tensor has no address; the kernel then has no image to write
    check(L.hm_mesh_render(dptr(verts), n_verts, dptr(faces), n_faces, dptr(proj), n_views, H, W, big_face,
                           dptr(attrs) if given else None, n_attr, bg.ctypes.data_as(C.c_void_p) if given else None,
                           dptr(face_id), dptr(depth), dptr(weights), dptr(image) if given else None,
                           dptr(n_skipped), dptr(ws), ws.numel(), dptr(status), stream_ptr(verts)))
    _check_mesh_status(what, status)
    return MeshRender(face_id, depth, weights, image, n_skipped)


# =========================================================================================
# Mesh colouring from the input views (csrc/hm_mesh_color.hip, DESIGN.md "Mesh colouring on the device")
# =========================================================================================
COLOR_MODES = {"blend": 0, "best": 1}
COLOR_MAX_POWER = 8


def _device_centers(what, centers, n_views, device):
    if isinstance(centers, torch.Tensor):
        ok = centers.dtype == torch.float64 and tuple(centers.shape) == (n_views, 3)
    else:
        ok = isinstance(centers, np.ndarray) and centers.dtype == np.float64 and centers.shape == (n_views, 3)
    if not ok:
        raise ValueError(f"hashmod {what}: float64 centers [n, 3] expected, one camera centre per view")
    if not isinstance(centers, torch.Tensor):
        centers = torch.from_numpy(np.ascontiguousarray(centers))
    return centers.to(device).contiguous()


def mesh_vertex_colors(verts, normals, proj, centers, images, depth, *, masks=None, erode=0, pad=1, tol=0.0,
                       min_cos=0.0, power=1, mode="blend", out=None):
    """(acc [V,4] float64, n_used [V] int32): the colour each vertex of verts [V,3] fp32 collects from the views
    proj [n,3,4], centers [n,3] (float64, host or device; the camera centres pose[:, :3, 3]) with images [n,H,W,3] fp32
    and the mesh's depth maps depth [n,H,W] fp32 (mesh_depth_maps), all on the device.  A view contributes iff the
    vertex is projectable with its pixel (rint(u), rint(v)) in the image; visible by mesh_visible_votes' rule with
    `pad` and `tol`; with masks [n,H,W] bool or uint8, every mask pixel of the (2 erode + 1)^2 square around its pixel
    that lies in the image is set (cv2.erode with its default border; erode >= 1 makes all four taps mask pixels); and,
    with normals [V,3] fp32, cos(normal, centre - vertex) is finite and > min_cos in [0, 1).  The weight is 1 without
    normals and cos^power (an integer in [0, 8]) with them; the sample is bilinear at (u, v), taps clamped to the image.
    mode="blend": acc[:, :3] = the sum of weight * sample, acc[:, 3] = the sum of the weights, added in view order;
    mode="best": the sample and weight of the view with the largest weight, of equals the first.  n_used counts the
    contributing views.  out = (acc, n_used), when given, is continued with these views (the next chunk) and returned:
    the bits do not depend on how the views are split.  fp64 operations rounded once, no atomics:
    tests/mesh_color_cases.vertex_colors_ref gives the same bits.  mesh_colors_finish turns acc into colours."""
    what = "mesh_vertex_colors"
    n_verts, n_views = _check_views(what, verts, proj)
    if normals is not None:
        _check_cloud(what, "normals", normals, like=verts)
        if normals.shape[0] != n_verts:
            raise ValueError(f"hashmod {what}: normals must have one row per vertex")
    if (not isinstance(images, torch.Tensor) or images.dtype != torch.float32 or images.dim() != 4
            or images.shape[0] != n_views or images.shape[3] != 3 or not images.is_contiguous()):
        raise ValueError(f"hashmod {what}: contiguous fp32 images [n, H, W, 3] expected, one per view")
    H, W = int(images.shape[1]), int(images.shape[2])
    _check_views(what, verts, proj, H, W)
    if (not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or tuple(depth.shape) != (n_views, H, W)
            or not depth.is_contiguous()):
        raise ValueError(f"hashmod {what}: contiguous fp32 depth [n, H, W] expected, one map per view")
    if masks is not None and (not isinstance(masks, torch.Tensor) or masks.dtype not in (torch.bool, torch.uint8)
                              or tuple(masks.shape) != (n_views, H, W)):
        raise ValueError(f"hashmod {what}: bool or uint8 masks [n, H, W] expected, one per view")
    if not (isinstance(erode, int) and not isinstance(erode, bool) and erode >= 0):
        raise ValueError(f"hashmod {what}: erode must be an integer >= 0")
    if not (isinstance(pad, int) and not isinstance(pad, bool) and 0 <= pad <= CULL_MAX_PAD):
        raise ValueError(f"hashmod {what}: pad must be an integer in [0, {CULL_MAX_PAD}]")
    if not (isinstance(tol, (int, float)) and not math.isnan(tol)):
        raise ValueError(f"hashmod {what}: tol must be a number")
    if not (isinstance(min_cos, (int, float)) and not isinstance(min_cos, bool) and 0.0 <= min_cos < 1.0):
        raise ValueError(f"hashmod {what}: min_cos must be a number in [0, 1)")
    if not (isinstance(power, int) and not isinstance(power, bool) and 0 <= power <= COLOR_MAX_POWER):
        raise ValueError(f"hashmod {what}: power must be an integer in [0, {COLOR_MAX_POWER}]")
    if mode not in COLOR_MODES:
        raise ValueError(f"hashmod {what}: mode must be 'blend' or 'best'")
    if out is not None:
        if (not isinstance(out, (tuple, list)) or len(out) != 2 or not all(isinstance(t, torch.Tensor) for t in out)
                or out[0].dtype != torch.float64 or tuple(out[0].shape) != (n_verts, 4) or not out[0].is_contiguous()
                or out[1].dtype != torch.int32 or tuple(out[1].shape) != (n_verts,) or not out[1].is_contiguous()):
            raise ValueError(f"hashmod {what}: out must be (contiguous float64 acc [V, 4], contiguous int32 n_used [V])")
    others = (images, depth, masks) + (tuple(out) if out is not None else ())
    for t in others:
        if t is not None and t.device != verts.device:
            raise ValueError(f"hashmod {what}: the tensors are on different devices")
    dev = verts.device
    centers = _device_centers(what, centers, n_views, dev)
    require_gpu(verts, normals, *others)
    proj = _device_proj(proj, dev)
    sat = None if masks is None else _mask_table(masks)
    if out is None:
        acc = torch.zeros((n_verts, 4), dtype=torch.float64, device=dev)
        n_used = torch.zeros(n_verts, dtype=torch.int32, device=dev)
    else:
        acc, n_used = out
    check(lib().hm_mesh_vertex_colors(dptr(verts), dptr(normals), n_verts, dptr(proj), dptr(centers), dptr(images),
                                      dptr(depth), dptr(sat), n_views, H, W, pad, float(tol),
                                      min(erode, CULL_MAX_IMAGE), float(min_cos), power, COLOR_MODES[mode],
                                      0 if out is None else 1, dptr(acc), dptr(n_used), stream_ptr(verts)))
    return acc, n_used


def mesh_colors_finish(acc, n_used, mode, fill=(0.0, 0.0, 0.0)):
    """colours [V,3] fp32 of mesh_vertex_colors' (acc, n_used): acc[:, :3] / acc[:, 3:] in float64 for mode="blend",
    acc[:, :3] for mode="best", cast to fp32; `fill` (three numbers) where no view contributed.  Torch plumbing."""
    if mode not in COLOR_MODES:
        raise ValueError("hashmod mesh_colors_finish: mode must be 'blend' or 'best'")
    if (not isinstance(acc, torch.Tensor) or acc.dtype != torch.float64 or acc.dim() != 2 or acc.shape[1] != 4
            or not isinstance(n_used, torch.Tensor) or n_used.dtype != torch.int32
            or tuple(n_used.shape) != (acc.shape[0],) or n_used.device != acc.device):
        raise ValueError("hashmod mesh_colors_finish: float64 acc [V, 4] and int32 n_used [V] on one device expected")
    try:
        fill = [float(c) for c in fill]
    except (TypeError, ValueError):
        fill = []
    if len(fill) != 3:
        raise ValueError("hashmod mesh_colors_finish: fill must be three numbers")
    rgb = acc[:, :3] / acc[:, 3:] if mode == "blend" else acc[:, :3]
    fill = torch.tensor(fill, dtype=torch.float32, device=acc.device)
    return torch.where((n_used > 0)[:, None], rgb.to(torch.float32), fill)


# =========================================================================================
# Per-face texture atlases (csrc/hm_mesh_texture.hip, DESIGN.md "Texturing the mesh")
# =========================================================================================
TEXTURE_MAX_RES = 4096
TEXTURE_MAX_TEXELS = 1 << 40


def texture_block_shape(res):
    """(Hb, Wb) = (res + 2, res + 3): the texels of a block, which holds two faces"""
    return res + 2, res + 3


def _check_texture_res(what, res, n_faces):
    if not (isinstance(res, int) and not isinstance(res, bool) and 1 <= res <= TEXTURE_MAX_RES):
        raise ValueError(f"hashmod {what}: res must be an integer in [1, {TEXTURE_MAX_RES}]")
    if not (isinstance(n_faces, int) and not isinstance(n_faces, bool) and 0 <= n_faces < 1 << 31):
        raise ValueError(f"hashmod {what}: n_faces must be an integer in [0, 2^31)")
    Hb, Wb = texture_block_shape(res)
    if (n_faces + 1) // 2 * Hb * Wb >= TEXTURE_MAX_TEXELS:
        raise ValueError(f"hashmod {what}: the atlas must have fewer than 2^40 texels (res too large for the mesh)")
    return (n_faces + 1) // 2, Hb, Wb


def mesh_texture_points(verts, faces, res, normals=None):
    """(points [T,3] fp32, normals [T,3] fp32 or None, face [T] int32): the point on its face, the interpolated vertex
    normal (not normalised) and the face of every texel of the mesh's atlas at `res` texel steps per face edge.

    The atlas (include/hashmod.h states it once): two faces per block of (res + 2) x (res + 3) texels, block b = faces
    2b and 2b + 1, T = ceil(F / 2) (res + 2) (res + 3) texels in block-major order.  A texel's barycentrics are small
    integers over 2 res - the lattice point inside the face, the nearest point of the hypotenuse on the gutter - and
    its point is float32(((b0 A) + (b1 B)) + (b2 C)) in fp64, rounded once per operation.  The texels of the absent
    upper half of the last block (odd F) have face -1 and NaN point and normal, which mesh_vertex_colors cannot
    project.  tests/mesh_texture_cases.texel_points_ref gives the same bits.  A face index outside [0, V) raises
    HashmodError (reported by the kernel, never dereferenced).  One host read of the status word."""
    what = "mesh_texture_points"
    _check_texture_res(what, res, 0)
    n_faces, n_verts = _check_mesh(what, faces, verts=verts, normals=normals, gpu_first=False)
    n_blocks, Hb, Wb = _check_texture_res(what, res, n_faces)
    dev = verts.device
    T = n_blocks * Hb * Wb
    points = torch.empty((T, 3), dtype=torch.float32, device=dev)
    tex_normals = None if normals is None else torch.empty((T, 3), dtype=torch.float32, device=dev)
    face = torch.empty(T, dtype=torch.int32, device=dev)
    if T == 0:
        return points, tex_normals, face
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().hm_mesh_texture_points(dptr(verts), dptr(normals), n_verts, dptr(faces), n_faces, res, dptr(points),
                                       dptr(tex_normals), dptr(face), dptr(status), stream_ptr(verts)))
    _check_mesh_status(what, status)
    return points, tex_normals, face


def _background3(what, background):
    try:
        bg = np.asarray(background, np.float32)
        bg = np.ascontiguousarray(np.broadcast_to(bg, (3,)) if bg.ndim == 0 else bg)
    except (TypeError, ValueError):
        bg = None
    if background is None or bg is None or bg.shape != (3,):
        raise ValueError(f"hashmod {what}: background must be a float or three floats")
    return bg


def mesh_texture_sample(texels, res, n_faces, face_id, weights, background=0.0):
    """colours [..., 3] fp32 of the samples face_id [...] int32, weights [..., 3] fp32 (mesh_render's, of any leading
    shape) in the atlas texels [n_blocks, res + 2, res + 3, 3] fp32 of a mesh of n_faces faces.

    face_id < 0 or a non-finite weight gives `background` (a float or three).  Else the position in the face's half
    block is (w1 res, w2 res), point-mirrored to (res + 2 - w1 res, res + 1 - w2 res) for an odd face, clamped to the
    block as doubles before any integer is formed; four taps, interpolated along x and then along y in fp64 with
    (a (1 - f)) + (b f), rounded once to fp32.  Weights exactly at a corner return that corner's texel.
    tests/mesh_texture_cases.texture_sample_ref gives the same bits; two calls give the same bits.  A face_id >=
    n_faces raises HashmodError (reported by the kernel, nothing is read).  One host read of the status word."""
    what = "mesh_texture_sample"
    n_blocks, Hb, Wb = _check_texture_res(what, res, n_faces)
    if (not isinstance(texels, torch.Tensor) or texels.dtype != torch.float32
            or tuple(texels.shape) != (n_blocks, Hb, Wb, 3) or not texels.is_contiguous()):
        raise ValueError(f"hashmod {what}: contiguous fp32 texels [ceil(n_faces / 2), res + 2, res + 3, 3] expected")
    if not isinstance(face_id, torch.Tensor) or face_id.dtype != torch.int32 or not face_id.is_contiguous():
        raise ValueError(f"hashmod {what}: contiguous int32 face_id [...] expected")
    if (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32
            or tuple(weights.shape) != tuple(face_id.shape) + (3,) or not weights.is_contiguous()):
        raise ValueError(f"hashmod {what}: contiguous fp32 weights [..., 3] expected, three per face_id")
    if face_id.numel() >= TEXTURE_MAX_TEXELS:
        raise ValueError(f"hashmod {what}: face_id must have fewer than 2^40 samples")
    bg = _background3(what, background)
    for t in (face_id, weights):
        if t.device != texels.device:
            raise ValueError(f"hashmod {what}: the tensors are on different devices")
    require_gpu(texels, face_id, weights)
    dev = texels.device
    out = torch.empty(tuple(face_id.shape) + (3,), dtype=torch.float32, device=dev)
    if face_id.numel() == 0:
        return out
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().hm_mesh_texture_sample(dptr(texels) if n_blocks else None, res, n_faces, dptr(face_id), dptr(weights),
                                       face_id.numel(), bg.ctypes.data_as(C.c_void_p), dptr(out), dptr(status),
                                       stream_ptr(texels)))
    if int(status.item()):
        raise _lib.HashmodError(f"hashmod {what}: a face_id lies outside [-inf, n_faces): the samples are not of this "
                                "atlas' mesh")
    return out


class TextureAtlas:
    """A baked per-face texture: res, n_faces, block_shape = (Hb, Wb), texels [n_blocks,Hb,Wb,3] fp32 (the dataset's
    [-1, 1] range when evaluation.texture.texture_mesh made them), used [n_blocks,Hb,Wb] bool (a view coloured the
    texel) and fill, the three floats of the unused rest of the 2-D image.  sample() is mesh_texture_sample over it;
    image() and face_uvs() lay the blocks out for an export (torch plumbing, no kernel)."""

    def __init__(self, res, n_faces, texels, used=None, fill=(0.0, 0.0, 0.0)):
        n_blocks, Hb, Wb = _check_texture_res("TextureAtlas", res, n_faces)
        if (not isinstance(texels, torch.Tensor) or texels.dtype != torch.float32
                or tuple(texels.shape) != (n_blocks, Hb, Wb, 3) or not texels.is_contiguous()):
            raise ValueError("hashmod TextureAtlas: contiguous fp32 texels [ceil(n_faces / 2), res + 2, res + 3, 3] "
                             "expected")
        if used is None:
            used = torch.ones((n_blocks, Hb, Wb), dtype=torch.bool, device=texels.device)
        if (not isinstance(used, torch.Tensor) or used.dtype != torch.bool or tuple(used.shape) != (n_blocks, Hb, Wb)
                or used.device != texels.device):
            raise ValueError("hashmod TextureAtlas: bool used [n_blocks, res + 2, res + 3] on the texels' device "
                             "expected")
        try:
            fill = tuple(float(c) for c in fill)
        except (TypeError, ValueError):
            fill = ()
        if len(fill) != 3:
            raise ValueError("hashmod TextureAtlas: fill must be three numbers")
        self.res, self.n_faces, self.block_shape = res, n_faces, (Hb, Wb)
        self.texels, self.used, self.fill = texels, used, fill

    @property
    def n_blocks(self):
        return int(self.texels.shape[0])

    def sample(self, face_id, weights, background=0.0):
        return mesh_texture_sample(self.texels, self.res, self.n_faces, face_id, weights, background)

    def atlas_shape(self, blocks_per_row=None):
        """(bw, Ha, Wa): bw blocks per row, Wa = bw Wb, Ha = ceil(n_blocks / bw) Hb.  The default bw is, of the
        integers within one of sqrt(n_blocks Hb / Wb), the one whose image is nearest a square"""
        Hb, Wb = self.block_shape
        nb = max(self.n_blocks, 1)
        if blocks_per_row is None:
            k = math.isqrt(nb * Hb // Wb)
            blocks_per_row = min((b for b in (k - 1, k, k + 1, k + 2) if b >= 1),
                                 key=lambda b: (abs(b * Wb - -(-nb // b) * Hb), b))
        if not (isinstance(blocks_per_row, int) and not isinstance(blocks_per_row, bool) and blocks_per_row >= 1):
            raise ValueError("hashmod TextureAtlas: blocks_per_row must be an integer >= 1")
        return blocks_per_row, -(-nb // blocks_per_row) * Hb, blocks_per_row * Wb

    def image(self, blocks_per_row=None):
        """[Ha,Wa,3] fp32 on the texels' device: block b at column (b mod bw) Wb and row (b div bw) Hb, row 0 on top;
        the unused tail of the last block row holds `fill`"""
        Hb, Wb = self.block_shape
        bw, Ha, Wa = self.atlas_shape(blocks_per_row)
        rows = Ha // Hb
        grid = torch.tensor(self.fill, dtype=torch.float32, device=self.texels.device).repeat(rows * bw, Hb, Wb, 1)
        grid[:self.n_blocks] = self.texels
        return grid.reshape(rows, bw, Hb, Wb, 3).permute(0, 2, 1, 3, 4).reshape(Ha, Wa, 3).contiguous()

    def face_uvs(self, blocks_per_row=None):
        """float64 numpy [F,3,2]: the corners' texture coordinates vt = ((x + 0.5) / Wa, 1 - (y + 0.5) / Ha) at their
        texel centres - (x0, y0), (x0 + n, y0), (x0, y0 + n) for an even face of the block at (x0, y0) and
        (x0 + n + 2, y0 + n + 1), (x0 + 2, y0 + n + 1), (x0 + n + 2, y0 + 1) for an odd one - so that a standard
        bilinear texture fetch reads the texels mesh_texture_sample reads"""
        Hb, Wb = self.block_shape
        n = self.res
        bw, Ha, Wa = self.atlas_shape(blocks_per_row)
        f = np.arange(self.n_faces, dtype=np.int64)
        origin = np.stack([((f >> 1) % bw) * Wb, ((f >> 1) // bw) * Hb], 1)[:, None, :]
        lower = np.array([[0, 0], [n, 0], [0, n]], np.int64)
        upper = np.array([[n + 2, n + 1], [2, n + 1], [n + 2, 1]], np.int64)
        xy = (origin + np.where(((f & 1) == 1)[:, None, None], upper[None], lower[None])).astype(np.float64)
        return np.stack([(xy[..., 0] + 0.5) / Wa, 1.0 - (xy[..., 1] + 0.5) / Ha], -1)
