"""Operators of the ConAN hot path on MI355X: thin torch.autograd wrappers over the C-ABI (include/conan_fgw_hip.h).

torch is used for device memory, streams and autograd bookkeeping only; every computation below is a HIP kernel of
libconan_fgw_hip.so.  All ops require CUDA(ROCm) tensors and raise otherwise.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
from torch import Tensor

from . import wgrad
from ._lib import FgwParams, call, lib, ptr, stream_ptr

f32, i32, i64 = torch.float32, torch.int32, torch.int64


def _c(t: Tensor) -> Tensor:
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------ graphs
FUSED_GRAPH_BUILD = True      # neighbour lists, pairs and transpose from conan_radius_graph_build (three launches); tools / tests switch the three
                              # separate entry points back on to compare (never read from the environment)


class RadiusGraph:
    """Device-resident neighbour lists of a batch of conformer graphs: CSR by target (+ lazily its by-source transpose).

    Counterpart of what `RadiusInteractionGraph.forward` returns in the reference (schnet_no_sum.py:160,208,342), kept in
    the layout the kernels consume.  `edge_index()` / `edge_weight()` export the reference's tensors (one host sync for E).
    """

    def __init__(self, pos: Tensor, graph_ptr: Tensor, num_graphs: int, cutoff: float, max_num_neighbors: int, loop: bool = False,
                 pairs: bool = False, transpose: bool = False):
        """`pairs` / `transpose`: hints that the caller will ask for `pairs()` / `transpose()` — the fused build (FUSED_GRAPH_BUILD) then writes them
        in the same three launches as the neighbour lists; without the hint they are built on first use by their own entry points."""
        pos = _c(pos)
        if pos.dtype != f32:
            raise RuntimeError("pos must be float32")
        n = pos.shape[0]
        dev = pos.device
        self.num_atoms, self.num_graphs, self.graph_ptr = n, num_graphs, graph_ptr
        self.cutoff, self.cap, self.loop = float(cutoff), int(max_num_neighbors), bool(loop)
        # worst case per target: cap + 1 edges without self loops (the self hit may fall outside torch-cluster's cap + 1 window)
        self.max_edges = ME = max(1, n * (self.cap if self.loop else self.cap + 1))
        self.rowptr = torch.empty(n + 1, dtype=i32, device=dev)
        self.col = torch.empty(ME, dtype=i32, device=dev)
        self.tgt = torch.empty(ME, dtype=i32, device=dev)
        self.dist = torch.empty(ME, dtype=f32, device=dev)
        self._deg = torch.empty(n + 1, dtype=i32, device=dev)
        self._t_rowptr = self._t_eid = None
        self.pid = None
        if FUSED_GRAPH_BUILD:
            ws = torch.empty(max(1, lib().conan_radius_graph_build_ws(n, num_graphs, self.cap, int(self.loop))), dtype=i32, device=dev)
            if pairs:
                self.pid = torch.empty(ME, dtype=i32, device=dev)
                self.pair_e0 = torch.empty(ME, dtype=i32, device=dev)
                self.pair_e1 = torch.empty(ME, dtype=i32, device=dev)
                self.pair_dist = torch.empty(ME, dtype=f32, device=dev)
                self.num_pairs_dev = torch.empty(1, dtype=i32, device=dev)
            if transpose:
                self._t_rowptr = torch.empty(n + 1, dtype=i32, device=dev)
                self._t_eid = torch.empty(ME, dtype=i32, device=dev)
            call("conan_radius_graph_build", ptr(pos) if n else None, ptr(graph_ptr, i32), n, num_graphs, self.cutoff, self.cap, int(self.loop), ptr(ws),
                 ptr(self.rowptr), ptr(self.col), ptr(self.tgt), ptr(self.dist),
                 ptr(self.pid), ptr(self.pair_e0 if pairs else None), ptr(self.pair_e1 if pairs else None), ptr(self.pair_dist if pairs else None),
                 ptr(self.num_pairs_dev if pairs else None), ptr(self._t_rowptr), ptr(self._t_eid), stream_ptr())
        else:
            call("conan_radius_graph_csr", ptr(pos), ptr(graph_ptr, i32), n, num_graphs, self.cutoff, self.cap, int(self.loop),
                 ptr(self._deg), ptr(self.rowptr), ptr(self.col), ptr(self.tgt), ptr(self.dist), stream_ptr())
        self.num_edges_dev = self.rowptr[n:]            # device-side edge count (1-element view)
        self._num_edges: Optional[int] = None

    @property
    def num_edges(self) -> int:
        if self._num_edges is None:
            self._num_edges = int(self.num_edges_dev.item())     # host sync
        return self._num_edges

    def transpose(self):
        if self._t_rowptr is None:
            dev = self.rowptr.device
            self._t_rowptr = torch.empty(self.num_atoms + 1, dtype=i32, device=dev)
            self._t_eid = torch.empty(self.max_edges, dtype=i32, device=dev)
            call("conan_csr_transpose", ptr(self.graph_ptr), self.num_graphs, self.num_atoms, ptr(self.rowptr), ptr(self.col),
                 ptr(self._deg), ptr(self._t_rowptr), ptr(self._t_eid), stream_ptr())
        return self._t_rowptr, self._t_eid

    def pairs(self):
        """Undirected pairs of the edge set (conan_edge_pairs): the continuous filter is evaluated once per pair.
        Returns self; fills pid [max_edges], pair_e0/pair_e1/pair_dist [max_edges] and num_pairs_dev (device int)."""
        if getattr(self, "pid", None) is None:
            dev, ME = self.rowptr.device, self.max_edges
            flag = torch.empty(ME + 1, dtype=i32, device=dev)
            pidx = torch.empty(ME + 1, dtype=i32, device=dev)
            scan_ws = torch.empty(2 * (ME // 4096 + 2), dtype=i32, device=dev)
            self.pid = torch.empty(ME, dtype=i32, device=dev)
            self.pair_e0 = torch.empty(ME, dtype=i32, device=dev)
            self.pair_e1 = torch.empty(ME, dtype=i32, device=dev)
            self.pair_dist = torch.empty(ME, dtype=f32, device=dev)
            call("conan_edge_pairs", ptr(self.rowptr), ptr(self.col), ptr(self.tgt), ptr(self.dist), ptr(self.num_edges_dev), ME, ptr(flag),
                 ptr(pidx), ptr(scan_ws), ptr(self.pid), ptr(self.pair_e0), ptr(self.pair_e1), ptr(self.pair_dist), stream_ptr())
            self.num_pairs_dev = pidx[ME:]
        return self

    def edge_index(self) -> Tensor:
        E = self.num_edges
        ei = torch.empty(2, E, dtype=i64, device=self.rowptr.device)
        call("conan_edge_index_i64", ptr(self.col), ptr(self.tgt), E, ptr(ei), stream_ptr())
        return ei

    def edge_weight(self) -> Tensor:
        return self.dist[: self.num_edges]


def empty_rows(rows: int, width: int, device, m_dev: Optional[Tensor]) -> Tensor:
    """[rows, width] fp32 buffer whose rows beyond the device-side count `m_dev` are zero (the rows below it are for the caller's
    kernel to write): a tail-only clear instead of a full memset of a worst-case-sized edge buffer."""
    t = torch.empty(rows, width, dtype=f32, device=device)
    if m_dev is not None:
        call("conan_zero_tail", ptr(t), ptr(m_dev), rows, width, stream_ptr())
    return t


# Debug switch for the "rows beyond the device-side count are never read" contract of the worst-case-sized edge buffers (unread_rows): when set,
# those buffers start as NaN instead of whatever the allocator hands out, so that a consumer that does read the tail shows up as non-finite
# results (tests/test_gpu_visnet.py runs a whole training step both ways and demands identical bits).
POISON_UNREAD_TAILS = False


def unread_rows(rows: int, width: int, device) -> Tensor:
    """[rows, width] fp32 buffer of which the caller's kernel writes the first m_dev rows and NOBODY reads the rest (every consumer walks the CSR
    or takes the same device-side count): no clear at all."""
    t = torch.empty(rows, width, dtype=f32, device=device)
    if POISON_UNREAD_TAILS:
        t.fill_(float("nan"))
    return t


def batch_hints(batch: Optional[Tensor]):
    """(num_graphs, max_nodes) that DeviceCollator attached to the node -> graph index tensor it produced (host-known from the item sizes), or
    (None, None): a caller that passes no size arguments — the reference's call shape — then needs no device -> host read to size anything."""
    h = getattr(batch, "_conan_hints", None) if batch is not None else None
    return h if h is not None else (None, None)


def graph_ptr_from_batch(batch: Tensor, num_graphs: int) -> Tensor:
    batch = _c(batch)
    out = torch.empty(num_graphs + 1, dtype=i32, device=batch.device)
    call("conan_graph_ptr_from_batch", ptr(batch, i64), batch.shape[0], num_graphs, ptr(out), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ weight gradients: wgrad.py (two API names stay here)
deferred_weight_gradients, flush_weight_gradients = wgrad.deferred, wgrad.flush


# max |g| of pair-level filter gradients: produced by conan_cfconv_bwd_w_pairs (one device float per backward of a CFConv), consumed by
# the filter network's backward, whose two MFMA kernels then run on two fp16 planes (half the matrix-pipe work).  It travels ON the
# gradient tensor (attribute _conan_gmax = (device float, tensor version at production)): a gradient that autograd copied or summed into
# a new tensor has no attribute, one it accumulated into IN PLACE has another version — both take the bf16 path, which needs no scale.
# (Round 3 kept a module-level dict keyed by data_ptr: a pointer is not an identity — stale entries, in-place sums.)
gmax_stats = {"tracked": 0, "used": 0}


def _tag_gmax(t: Tensor, gmax: Tensor):
    t._conan_gmax = (gmax, t._version)
    gmax_stats["tracked"] += 1


def _take_gmax(t: Tensor, g: Tensor):
    tag = getattr(t, "_conan_gmax", None)
    if tag is None or tag[1] != t._version or g.data_ptr() != t.data_ptr():
        return None
    gmax_stats["used"] += 1
    return tag[0]


# ------------------------------------------------------------------------------------------------ linear / activation
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, residual, act, m_dev, grad_tail_unread=False):
        x, w = _c(x), _c(w)
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, dtype=f32, device=x.device)
        call("conan_linear_fwd", ptr(x, f32), ptr(w, f32), ptr(b), ptr(_c(residual)) if residual is not None else None,
             M, K, N, 0, act, ptr(m_dev), ptr(y), stream_ptr())
        ctx.act, ctx.m_dev, ctx.has_b, ctx.has_res, ctx.grad_tail_unread = act, m_dev, b is not None, residual is not None, grad_tail_unread
        ctx.save_for_backward(x, w, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = _c(dy)
        M, K = x.shape
        N = w.shape[0]
        md = ctx.m_dev
        if ctx.act:
            if ctx.has_res:
                raise RuntimeError("act + residual backward is not defined for this op")
            g = torch.empty_like(dy)
            call("conan_ssp_bwd", ptr(dy), ptr(y), M, N, ptr(md), ptr(g), stream_ptr())
        else:
            g = dy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if ctx.grad_tail_unread:       # the caller's promise: whatever consumes dx takes md or walks the CSR (ViS_MP's s_proj: 22 us per layer for a tail nobody reads)
                dx = unread_rows(x.shape[0], x.shape[1], x.device)
            else:
                dx = empty_rows(x.shape[0], x.shape[1], x.device, md)
            call("conan_linear_fwd", ptr(g), ptr(w), None, None, M, N, K, 1, 0, ptr(md), ptr(dx), stream_ptr())
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw, db = wgrad.plain(g, x, M, K, N, md, w, ctx.has_b)
        return dx, dw, db, (dy if ctx.has_res else None), None, None, None


class _LinearTapFn(torch.autograd.Function):
    """(x W^T, x): a bias-free Linear that also hands its input through.  The second output is for a residual connection taken from the
    same x further down: its gradient then arrives HERE, together with the gradient of the product, and the backward forms
    dx = dy W + d_tap in the epilogue of the one input-gradient GEMM instead of leaving a separate add of two [M,K] tensors to autograd."""

    @staticmethod
    def forward(ctx, x, w):
        x, w = _c(x), _c(w)
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, dtype=f32, device=x.device)
        call("conan_linear_fwd", ptr(x, f32), ptr(w, f32), None, None, M, K, N, 0, 0, None, ptr(y), stream_ptr())
        ctx.save_for_backward(x, w)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dtap):
        x, w = ctx.saved_tensors
        M, K = x.shape
        N = w.shape[0]
        dx = dw = None
        if dy is None:                                             # only the tap was used downstream
            return dtap, None
        dy = _c(dy)
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, dtype=f32, device=x.device)
            call("conan_linear_fwd", ptr(dy), ptr(w), None, ptr(_c(dtap)) if dtap is not None else None, M, N, K, 1, 0, None, ptr(dx), stream_ptr())
        elif dtap is not None:
            dx = dtap
        if ctx.needs_input_grad[1]:
            dw, _ = wgrad.plain(dy, x, M, K, N, None, w, False)
        return dx, dw


def linear_tap(x: Tensor, weight: Tensor):
    """Returns (x @ weight.T, x'): x' is x, to be used for a residual connection downstream (see _LinearTapFn)."""
    return _LinearTapFn.apply(x, weight)


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, act: bool = False, residual: Optional[Tensor] = None,
           m_dev: Optional[Tensor] = None, grad_tail_unread: bool = False) -> Tensor:
    """act(x @ weight.T + bias) (+ residual) with act = shifted softplus.  `m_dev`: device int32 row count (edge-level); the rows of the input
    gradient beyond it are zero unless `grad_tail_unread` (then undefined: for callers whose consumers never read them)."""
    return _LinearFn.apply(x, weight, bias, residual, 1 if act else 0, m_dev, grad_tail_unread)


class _Mlp2Fn(torch.autograd.Function):
    """y = ssp(x w1^T + b1) w2^T + b2 (+ residual) in one launch; backward: one launch for both input-gradient GEMMs and the
    activation derivative between them, then the two weight gradients (conan_mlp2_fwd / conan_mlp2_bwd)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual):
        x, w1, w2 = _c(x), _c(w1), _c(w2)
        M, K = x.shape
        N1, N2 = w1.shape[0], w2.shape[0]
        need = any(ctx.needs_input_grad[:5])
        mid = torch.empty(M, N1, dtype=f32, device=x.device) if need else None
        y = torch.empty(M, N2, dtype=f32, device=x.device)
        call("conan_mlp2_fwd", ptr(x, f32), ptr(w1, f32), ptr(_c(b1), f32), ptr(w2, f32), ptr(_c(b2), f32),
             ptr(_c(residual)) if residual is not None else None, M, K, N1, N2, ptr(mid), ptr(y), stream_ptr())
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, w1, w2, mid)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, mid = ctx.saved_tensors
        dy = _c(dy)
        M, K = x.shape
        N1, N2 = w1.shape[0], w2.shape[0]
        dmid = torch.empty(M, N1, dtype=f32, device=x.device)
        dx = torch.empty(M, K, dtype=f32, device=x.device)
        call("conan_mlp2_bwd", ptr(dy), ptr(w2), ptr(w1), ptr(mid), M, K, N1, N2, ptr(dmid), ptr(dx), stream_ptr())
        dw2, db2 = wgrad.plain(dy, mid, M, N1, N2, None, w2, True)
        dw1, db1 = wgrad.plain(dmid, x, M, K, N1, None, w1, True)
        return dx, dw1, db1, dw2, db2, (dy if ctx.has_res else None)


def mlp2(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, residual: Optional[Tensor] = None) -> Tensor:
    """ssp(x w1^T + b1) w2^T + b2 (+ residual).  One launch where conan_mlp2_supported (node-level rows, 128-wide layers), else the two
    linear kernels."""
    if x.is_cuda and b1 is not None and b2 is not None and lib().conan_mlp2_supported(x.shape[0], x.shape[1], w1.shape[0], w2.shape[0]):
        return _Mlp2Fn.apply(x, w1, b1, w2, b2, residual)
    return linear(linear(x, w1, b1, act=True), w2, b2, residual=residual)


class _Mlp2OutActFn(torch.autograd.Function):
    """y = ssp((x w1^T + b1) w2^T + b2) in one launch; backward: dy * ssp'(y), both input-gradient GEMMs in one launch, then the two weight
    gradients (conan_mlp2_outact_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x, w1, w2 = _c(x), _c(w1), _c(w2)
        M, K = x.shape
        N1, N2 = w1.shape[0], w2.shape[0]
        need = any(ctx.needs_input_grad)
        mid = torch.empty(M, N1, dtype=f32, device=x.device) if need else None
        y = torch.empty(M, N2, dtype=f32, device=x.device)
        call("conan_mlp2_outact_fwd", ptr(x, f32), ptr(w1, f32), ptr(_c(b1), f32), ptr(w2, f32), ptr(_c(b2), f32), M, K, N1, N2, ptr(mid), ptr(y),
             stream_ptr())
        ctx.save_for_backward(x, w1, w2, mid, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, mid, y = ctx.saved_tensors
        dy = _c(dy)
        M, K = x.shape
        N1, N2 = w1.shape[0], w2.shape[0]
        dev = x.device
        g = torch.empty(M, N2, dtype=f32, device=dev)
        dmid = torch.empty(M, N1, dtype=f32, device=dev)
        dx = torch.empty(M, K, dtype=f32, device=dev)
        call("conan_mlp2_outact_bwd", ptr(dy), ptr(y), ptr(w2), ptr(w1), M, K, N1, N2, ptr(g), ptr(dmid), ptr(dx), stream_ptr())
        dw2, db2 = wgrad.plain(g, mid, M, N1, N2, None, w2, True)
        dw1, db1 = wgrad.plain(dmid, x, M, K, N1, None, w1, True)
        return dx, dw1, db1, dw2, db2


def mlp2_outact(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
    """ssp((x w1^T + b1) w2^T + b2).  One launch where conan_mlp2_outact_supported (node-level rows, 128 -> 64 -> 64), else two linear kernels."""
    if x.is_cuda and b1 is not None and b2 is not None and lib().conan_mlp2_outact_supported(x.shape[0], x.shape[1], w1.shape[0], w2.shape[0]):
        return _Mlp2OutActFn.apply(x, w1, b1, w2, b2)
    return linear(linear(x, w1, b1), w2, b2, act=True)


DUAL_HEAD = True              # both heads of the shared trunk in one launch each way (conan_mlp2_outact_dual_fwd / _bwd); tools / tests switch the two
                              # single-head functions back on to compare (never read from the environment)
DUAL_HEAD_FORWARD_FORM = 0    # how the forward launch shares the heads: 0 = a second grid dimension, 1 = every workgroup runs both on one load of its rows
                              # (not distinguishable in the captured cfg2 step: DESIGN.md §8 item 4)


class _Mlp2OutActDualFn(torch.autograd.Function):
    """(y_a, y_b) = two _Mlp2OutActFn of ONE x, one launch each way; the backward writes dx = dx_a + dx_b once, in the kernel's epilogue, instead of
    leaving the add of two [M,K] tensors to autograd.  Saves what the two functions save and queues the same four weight gradients, in the order in
    which autograd runs the two (the later head's first)."""

    @staticmethod
    def forward(ctx, x, w1a, b1a, w2a, b2a, w1b, b1b, w2b, b2b, m_dev):
        x, w1a, w2a, w1b, w2b = _c(x), _c(w1a), _c(w2a), _c(w1b), _c(w2b)
        M, K = x.shape
        N1, N2 = w1a.shape[0], w2a.shape[0]
        dev = x.device
        need = any(ctx.needs_input_grad)
        mid_a, mid_b = (torch.empty(M, N1, dtype=f32, device=dev) if need else None for _ in range(2))
        y_a, y_b = (torch.empty(M, N2, dtype=f32, device=dev) for _ in range(2))
        call("conan_mlp2_outact_dual_fwd", ptr(x, f32), ptr(w1a, f32), ptr(_c(b1a), f32), ptr(w2a, f32), ptr(_c(b2a), f32), ptr(w1b, f32),
             ptr(_c(b1b), f32), ptr(w2b, f32), ptr(_c(b2b), f32), M, K, N1, N2, ptr(m_dev), DUAL_HEAD_FORWARD_FORM, ptr(mid_a), ptr(y_a), ptr(mid_b),
             ptr(y_b), stream_ptr())
        ctx.m_dev = m_dev
        ctx.save_for_backward(x, w1a, w2a, mid_a, y_a, w1b, w2b, mid_b, y_b)
        return y_a, y_b

    @staticmethod
    def backward(ctx, dy_a, dy_b):
        x, w1a, w2a, mid_a, y_a, w1b, w2b, mid_b, y_b = ctx.saved_tensors
        M, K = x.shape
        N1, N2 = w1a.shape[0], w2a.shape[0]
        dev, md = x.device, ctx.m_dev
        dy_a, dy_b = _c(dy_a), _c(dy_b)
        g_a, g_b = (torch.empty(M, N2, dtype=f32, device=dev) for _ in range(2))
        dmid_a, dmid_b = (torch.empty(M, N1, dtype=f32, device=dev) for _ in range(2))
        dx = empty_rows(M, K, dev, md)
        call("conan_mlp2_outact_dual_bwd", ptr(dy_a), ptr(y_a), ptr(w2a), ptr(w1a), ptr(dy_b), ptr(y_b), ptr(w2b), ptr(w1b), M, K, N1, N2, ptr(md),
             ptr(g_a), ptr(dmid_a), ptr(g_b), ptr(dmid_b), ptr(dx), stream_ptr())
        dw2b, db2b = wgrad.plain(g_b, mid_b, M, N1, N2, md, w2b, True)
        dw1b, db1b = wgrad.plain(dmid_b, x, M, K, N1, md, w1b, True)
        dw2a, db2a = wgrad.plain(g_a, mid_a, M, N1, N2, md, w2a, True)
        dw1a, db1a = wgrad.plain(dmid_a, x, M, K, N1, md, w1a, True)
        return dx, dw1a, db1a, dw2a, db2a, dw1b, db1b, dw2b, db2b, None


def mlp2_outact_dual_supported(M: int, K: int, N1: int, N2: int) -> bool:
    return bool(lib().conan_mlp2_outact_supported(int(M), int(K), int(N1), int(N2)))


def mlp2_outact_dual(x: Tensor, head_a, head_b, m_dev: Optional[Tensor] = None):
    """(mlp2_outact(x, *head_a), mlp2_outact(x, *head_b)) for two weight sets (w1, b1, w2, b2) of the same widths, one launch each way where DUAL_HEAD
    and mlp2_outact_dual_supported; else the two single-head calls (`m_dev`, a device-side row count, is for the one-launch form only)."""
    (w1a, b1a, w2a, b2a), (w1b, b1b, w2b, b2b) = head_a, head_b
    if (DUAL_HEAD and x.is_cuda and all(b is not None for b in (b1a, b2a, b1b, b2b)) and w1a.shape == w1b.shape and w2a.shape == w2b.shape
            and mlp2_outact_dual_supported(x.shape[0], x.shape[1], w1a.shape[0], w2a.shape[0])):
        return _Mlp2OutActDualFn.apply(x, w1a, b1a, w2a, b2a, w1b, b1b, w2b, b2b, m_dev)
    if m_dev is not None:
        raise ValueError("mlp2_outact_dual: a device-side row count needs the one-launch form")
    return mlp2_outact(x, w1a, b1a, w2a, b2a), mlp2_outact(x, w1b, b1b, w2b, b2b)


class _Stage2HeadFn(torch.autograd.Function):
    """out = Linreg(mean_K(Lin3d(x3) + xc + aw * Linbary(xb))): one launch each way (conan_stage2_head_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x3, xc, xb, W3, b3, Wb, bb, wreg, breg, aw, K):
        x3, xc, xb = _c(x3), _c(xc), _c(xb)
        G, D = x3.shape
        if G % K != 0:
            raise ValueError(f"stage2_head: {G} conformer graphs are not a multiple of num_conformers={K}")
        B = G // K
        dev = x3.device
        out = torch.empty(B, 1, dtype=f32, device=dev)
        m3, mb, t = (torch.empty(B, D, dtype=f32, device=dev) for _ in range(3))
        call("conan_stage2_head_fwd", ptr(x3, f32), ptr(xc, f32), ptr(xb, f32), ptr(_c(W3), f32), ptr(_c(b3), f32), ptr(_c(Wb), f32), ptr(_c(bb), f32),
             ptr(_c(wreg), f32), ptr(_c(breg), f32), float(aw), B, K, D, ptr(out), ptr(m3), ptr(mb), ptr(t), stream_ptr())
        ctx.save_for_backward(W3, Wb, wreg, m3, mb, t)
        ctx.dims, ctx.aw = (B, K, D), float(aw)
        return out

    @staticmethod
    def backward(ctx, dout):
        W3, Wb, wreg, m3, mb, t = ctx.saved_tensors
        B, K, D = ctx.dims
        dev = dout.device
        dx3, dxc, dxb = (torch.empty(B * K, D, dtype=f32, device=dev) for _ in range(3))
        dW3, dWb = torch.empty(D, D, dtype=f32, device=dev), torch.empty(D, D, dtype=f32, device=dev)
        db3, dbb = torch.empty(D, dtype=f32, device=dev), torch.empty(D, dtype=f32, device=dev)
        dwreg, dbreg = torch.empty(1, D, dtype=f32, device=dev), torch.empty(1, dtype=f32, device=dev)
        call("conan_stage2_head_bwd", ptr(_c(dout)), ptr(_c(W3)), ptr(_c(Wb)), ptr(_c(wreg)), ptr(m3), ptr(mb), ptr(t), ctx.aw, B, K, D,
             ptr(dx3), ptr(dxc), ptr(dxb), ptr(dW3), ptr(db3), ptr(dWb), ptr(dbb), ptr(dwreg), ptr(dbreg), stream_ptr())
        return dx3, dxc, dxb, dW3, db3, dWb, dbb, dwreg, dbreg, None, None


def stage2_head(x3: Tensor, xc: Tensor, xb: Tensor, lin3d, linbary, linreg, agg_weight: float, K: int) -> Tensor:
    """[G,D] x 3 -> [G/K, 1]: Linreg(mean over the K conformers of (Lin3d(x3) + xc + agg_weight * Linbary(xb)))."""
    return _Stage2HeadFn.apply(x3, xc, xb, lin3d.weight, lin3d.bias, linbary.weight, linbary.bias, linreg.weight, linreg.bias, agg_weight, K)


def stage2_head_supported(D: int) -> bool:
    return bool(lib().conan_stage2_head_supported(int(D)))


HEAD_SUMS_FUSED = True        # the stage-2 head forms the per-graph sums of h_3d and the readout of Y itself (conan_stage2_head_sums_fwd / _bwd: one launch
                              # each way instead of three); tools / tests switch it off to compare (never read from the environment)


class _Stage2HeadSumsFn(torch.autograd.Function):
    """_Stage2HeadFn(segment_sum(h3, gptr), xc, fgw_readout(Y, K, 0), ...) in one launch each way: the backward writes the per-atom gradient of h3 and
    dY directly."""

    @staticmethod
    def forward(ctx, Y, h3, gptr, xc, W3, b3, Wb, bb, wreg, breg, aw, K):
        Y, h3, xc = _c(Y), _c(h3), _c(xc)
        B, N, D = Y.shape
        if gptr.numel() != B * K + 1 or xc.shape != (B * K, D) or h3.shape[1] != D:
            raise ValueError(f"stage2_head_sums: Y {tuple(Y.shape)}, h3 {tuple(h3.shape)}, xc {tuple(xc.shape)} and {gptr.numel() - 1} graphs do not "
                             f"belong to {B} molecules of {K} conformers")
        dev = Y.device
        out = torch.empty(B, 1, dtype=f32, device=dev)
        m3, mb, t = (torch.empty(B, D, dtype=f32, device=dev) for _ in range(3))
        call("conan_stage2_head_sums_fwd", ptr(Y, f32), ptr(h3, f32), ptr(gptr, i32), ptr(xc, f32), ptr(_c(W3), f32), ptr(_c(b3), f32), ptr(_c(Wb), f32),
             ptr(_c(bb), f32), ptr(_c(wreg), f32), ptr(_c(breg), f32), float(aw), B, K, N, D, 0, ptr(out), ptr(m3), ptr(mb), ptr(t), stream_ptr())
        ctx.save_for_backward(W3, Wb, wreg, m3, mb, t, gptr)
        ctx.dims, ctx.aw, ctx.atoms = (B, K, N, D), float(aw), h3.shape[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        W3, Wb, wreg, m3, mb, t, gptr = ctx.saved_tensors
        B, K, N, D = ctx.dims
        dev = dout.device
        dh3, dxc, dY = (torch.empty(s, dtype=f32, device=dev) for s in ((ctx.atoms, D), (B * K, D), (B, N, D)))
        dW3, dWb = torch.empty(D, D, dtype=f32, device=dev), torch.empty(D, D, dtype=f32, device=dev)
        db3, dbb = torch.empty(D, dtype=f32, device=dev), torch.empty(D, dtype=f32, device=dev)
        dwreg, dbreg = torch.empty(1, D, dtype=f32, device=dev), torch.empty(1, dtype=f32, device=dev)
        call("conan_stage2_head_sums_bwd", ptr(_c(dout)), ptr(_c(W3)), ptr(_c(Wb)), ptr(_c(wreg)), ptr(m3), ptr(mb), ptr(t), ptr(gptr), ctx.aw, B, K, N, D, 0,
             ptr(dh3), ptr(dxc), ptr(dY), ptr(dW3), ptr(db3), ptr(dWb), ptr(dbb), ptr(dwreg), ptr(dbreg), stream_ptr())
        return dY, dh3, None, dxc, dW3, db3, dWb, dbb, dwreg, dbreg, None, None


def stage2_head_sums(Y: Tensor, h3: Tensor, graph_ptr: Tensor, xc: Tensor, lin3d, linbary, linreg, agg_weight: float, K: int) -> Tensor:
    """stage2_head(segment_sum(h3, graph_ptr, G), xc, fgw_readout(Y, K, 0), ...) with both sums inside the head's launches: Y [B,N,D] the solver's
    barycenter features, h3 [atoms,D] per atom, xc [B*K,D] -> [B,1].  Callers check stage2_head_sums_supported."""
    return _Stage2HeadSumsFn.apply(Y, h3, graph_ptr, xc, lin3d.weight, lin3d.bias, linbary.weight, linbary.bias, linreg.weight, linreg.bias, agg_weight, K)


def stage2_head_sums_supported(D: int, K: int, readout_mode: int) -> bool:
    return bool(lib().conan_stage2_head_sums_supported(int(D), int(K), int(readout_mode)))


class _UnaryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, op):
        x = _c(x)
        y = torch.empty_like(x)
        call("conan_unary_fwd", ptr(x, f32), x.numel(), op, ptr(y), stream_ptr())
        ctx.op = op
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        call("conan_unary_bwd", ptr(y), ptr(_c(dy)), y.numel(), ctx.op, ptr(dx), stream_ptr())
        return dx, None


def relu(x: Tensor) -> Tensor:
    return _UnaryFn.apply(x, 0)


def sigmoid(x: Tensor) -> Tensor:
    return _UnaryFn.apply(x, 1)


def shifted_softplus(x: Tensor) -> Tensor:
    return _UnaryFn.apply(x, 2)


class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, weight, padding_idx):
        z, weight = _c(z), _c(weight)
        out = torch.empty(z.shape[0], weight.shape[1], dtype=f32, device=weight.device)
        call("conan_embedding_fwd", ptr(z, i64), ptr(weight, f32), z.shape[0], weight.shape[1], weight.shape[0], ptr(out), stream_ptr())
        ctx.save_for_backward(z, weight)
        ctx.shape, ctx.padding_idx = weight.shape, padding_idx
        return out

    @staticmethod
    def backward(ctx, dout):
        z, weight = ctx.saved_tensors
        rows, H = ctx.shape
        if rows <= 128 and wgrad.claim((weight.data_ptr(),), (H, rows), flush_if_pending=False):
            # inside a deferred backward pass (FlatGradients.backward): dW = onehot(z)^T dout is one more job of the batched node-level weight-gradient
            # launch (≈ 16 us at cfg2 for the one-hot build and its share of the batch, against 34 us for the two kernels of conan_embedding_bwd)
            dout = _c(dout)
            onehot = torch.empty(z.shape[0], rows, dtype=f32, device=dout.device)
            call("conan_onehot_rows", ptr(z), z.shape[0], rows, -1 if ctx.padding_idx is None else ctx.padding_idx, ptr(onehot), stream_ptr())
            dw, _ = wgrad.plain(onehot, dout, z.shape[0], H, rows, None, weight, False)
            return None, dw, None
        dw = torch.empty(ctx.shape, dtype=f32, device=dout.device)
        ws = torch.empty(int(lib().conan_embedding_bwd_ws(z.shape[0], ctx.shape[1], ctx.shape[0])), dtype=f32, device=dout.device)
        call("conan_embedding_bwd", ptr(z), ptr(_c(dout)), z.shape[0], ctx.shape[1], ctx.shape[0],
             -1 if ctx.padding_idx is None else ctx.padding_idx, ptr(dw), ptr(ws), stream_ptr())
        return None, dw, None


def embedding(z: Tensor, weight: Tensor, padding_idx: Optional[int] = 0) -> Tensor:
    return _EmbeddingFn.apply(z, weight, padding_idx)


# ------------------------------------------------------------------------------------------------ continuous filter pieces
def rbf_expand(graph: RadiusGraph, offset: Tensor, coeff: float) -> Tensor:
    """GaussianSmearing of every edge distance -> [max_edges, Gs] (rows >= E untouched).  No gradient (pos is an input)."""
    Gs = offset.shape[0]
    out = torch.empty(graph.max_edges, Gs, dtype=f32, device=offset.device)
    call("conan_rbf_fwd", ptr(graph.dist), ptr(graph.num_edges_dev), graph.max_edges, ptr(_c(offset), f32), Gs, float(coeff),
         ptr(out), stream_ptr())
    return out


class _CutoffScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w_raw, graph):
        out = torch.empty_like(w_raw)
        call("conan_cutoff_scale", ptr(graph.dist), ptr(graph.num_edges_dev), graph.max_edges, w_raw.shape[1], graph.cutoff,
             ptr(_c(w_raw)), ptr(out), stream_ptr())
        ctx.graph = graph
        return out

    @staticmethod
    def backward(ctx, dout):
        g = ctx.graph
        dout = _c(dout)
        din = torch.empty_like(dout)
        call("conan_cutoff_scale", ptr(g.dist), ptr(g.num_edges_dev), g.max_edges, dout.shape[1], g.cutoff, ptr(dout), ptr(din),
             stream_ptr())
        return din, None


def cutoff_scale(w_raw: Tensor, graph: RadiusGraph) -> Tensor:
    return _CutoffScaleFn.apply(w_raw, graph)


FUSED_FILTER_BACKWARD = True      # tools / tests switch the round-3 pair of kernels back on to compare (never read from the environment)


class _FilterFn(torch.autograd.Function):
    """Fused filter generator (conan_filter_fwd).  Its output must be consumed by `cfconv(..., pre_cutoff_grad=True)`:
    the incoming gradient g is then w.r.t. the un-scaled filter.  Backward: dw2 = g^T h1 (conan_linear_wgrad), then ONE pass
    (conan_filter_bwd) for gpre = (g w2) * ssp'(h1) and dw1 = gpre^T rbf, with gpre kept in registers and rbf regenerated."""

    @staticmethod
    def forward(ctx, graph, offset, coeff, w1, b1, w2, b2, use_pairs):
        F, Gs = w1.shape
        dev = w1.device
        need_grad = any(ctx.needs_input_grad[3:7])
        dist, cnt = (graph.pairs().pair_dist, graph.num_pairs_dev) if use_pairs else (graph.dist, graph.num_edges_dev)
        W = torch.empty(graph.max_edges, F, dtype=f32, device=dev)
        h1 = torch.empty(graph.max_edges, F, dtype=f32, device=dev) if need_grad else None
        call("conan_filter_fwd", ptr(dist), ptr(cnt), graph.max_edges, ptr(_c(offset), f32), Gs, float(coeff),
             graph.cutoff, F, ptr(_c(w1), f32), ptr(_c(b1), f32), ptr(_c(w2), f32), ptr(_c(b2), f32), ptr(W), ptr(h1), stream_ptr())
        ctx.graph, ctx.coeff, ctx.rows = graph, float(coeff), (dist, cnt)
        ctx.save_for_backward(offset, w1, w2, h1)
        return W

    @staticmethod
    def backward(ctx, dW):
        offset, w1, w2, h1 = ctx.saved_tensors
        g_ = ctx.graph
        dist, md = ctx.rows                          # per-edge or per-pair distances and their device-side count
        F, Gs = w1.shape
        ME = g_.max_edges
        dev = dW.device
        g = _c(dW)                                   # already multiplied by C(d): cfconv(..., pre_cutoff_grad=True)
        gmax = _take_gmax(dW, g) if F == 128 else None      # max |g|, when the producer tracked it and nothing touched g since: the two kernels below run on fp16 planes
        if gmax is not None and FUSED_FILTER_BACKWARD and lib().conan_filter_bwd2_supported(Gs, F):      # both layers' gradients in one pass over g and h1
            (dw1, db1), (dw2, db2) = wgrad.filter_bwd2(g, h1, dist, _c(offset), ctx.coeff, w1, _c(w2), ME, md, gmax)
            return None, None, None, dw1, db1, dw2, db2, None
        dw2, db2 = wgrad.plain(g, h1, ME, F, F, md, w2, True, gmax=gmax)
        if lib().conan_filter_bwd_supported(Gs, F):              # (g @ w2) * ssp'(h1) and its contraction with rbf(dist) in one pass
            dw1, db1 = wgrad.filter_bwd(g, h1, dist, _c(offset), ctx.coeff, w1, _c(w2), ME, md, gmax=gmax)
        else:
            dh1 = torch.empty_like(g)
            call("conan_linear_fwd", ptr(g), ptr(_c(w2)), None, ptr(h1), ME, F, F, 1, 2, ptr(md), ptr(dh1), stream_ptr())   # (g @ w2) * ssp'(h1)
            dw1, db1 = wgrad.plain(dh1, None, ME, Gs, F, md, w1, True, rbf=(dist, _c(offset), ctx.coeff))      # rbf(dist) regenerated inside the GEMM
        return None, None, None, dw1, db1, dw2, db2, None


def filter_fused_supported(num_gaussians: int, num_filters: int) -> bool:
    return bool(lib().conan_filter_fused_supported(int(num_gaussians), int(num_filters)))


def filter_generate(graph: "RadiusGraph", offset: Tensor, coeff: float, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
                    use_pairs: bool = True) -> Tensor:
    """Filter rows mlp(rbf(d)) * C(d) -> [max_edges, F].  use_pairs=True: ONE row per undirected pair (d_ij = d_ji), to be
    consumed by `cfconv(..., pre_cutoff_grad=True, use_pairs=True)`; False: one row per directed edge."""
    return _FilterFn.apply(graph, offset, coeff, w1, b1, w2, b2, use_pairs)


def filter_cfconv_supported(num_gaussians: int, num_filters: int) -> bool:
    return bool(lib().conan_filter_cfconv_fwd_supported(int(num_gaussians), int(num_filters)))


def filter_cfconv(x: Tensor, graph: "RadiusGraph", offset: Tensor, coeff: float, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
    """CFConv's edge half in ONE launch, forward only (conan_filter_cfconv_fwd): out[i] = sum_{j in N(i)} x[j] * (mlp(rbf(d_ij)) * C(d_ij)) with the
    filter rows generated per directed edge and consumed on the spot — no [E, F] tensor exists.  Inference only: raises when a gradient is
    required (the training step's backward reads the filter tensor that `filter_generate` + `cfconv` save)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, w1, b1, w2, b2)):
        raise RuntimeError("filter_cfconv is forward-only: use filter_generate + cfconv when gradients are needed")
    x = _c(x)
    out = torch.empty_like(x)
    call("conan_filter_cfconv_fwd", ptr(x, f32), ptr(graph.dist), ptr(graph.col), ptr(graph.tgt), ptr(graph.num_edges_dev), graph.max_edges,
         ptr(_c(offset), f32), offset.shape[0], float(coeff), graph.cutoff, w1.shape[0], ptr(_c(w1), f32), ptr(_c(b1), f32), ptr(_c(w2), f32),
         ptr(_c(b2), f32), graph.num_atoms, ptr(out), stream_ptr())
    return out


FUSED_CFCONV_BACKWARD = True      # dx and the pair gradient in one launch (conan_cfconv_bwd_xw_pairs); tools / tests switch it off to compare


class _CFConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, graph, pre_cutoff_grad=False, use_pairs=False):
        x, W = _c(x), _c(W)
        out = torch.empty_like(x)
        pid = graph.pairs().pid if use_pairs else None
        F = x.shape[1]
        # max |dW| of the pair gradient (F = 128): one device float per CFConv, raised with atomicMax by the backward kernel that writes the pair
        # gradient.  Something has to clear it before every backward pass without a fill launch of its own: the fused backward (dx + pair gradient in
        # one launch) has no kernel in front of it, so this forward launch does (zero_slot) — fresh on every forward / backward pair, captured or not.
        ctx.gmax = None
        if use_pairs and F == 128 and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and FUSED_CFCONV_BACKWARD and pre_cutoff_grad:
            ctx.gmax = torch.empty(1, dtype=f32, device=x.device)
        call("conan_cfconv_fwd", ptr(x, f32), ptr(W, f32), ptr(graph.rowptr), ptr(graph.col), ptr(pid), graph.num_atoms, F,
             ptr(out), ptr(ctx.gmax), stream_ptr())
        ctx.graph, ctx.pre, ctx.pairs = graph, pre_cutoff_grad, use_pairs
        ctx.save_for_backward(x, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, W = ctx.saved_tensors
        g = ctx.graph
        dout = _c(dout)
        dx = dW = None
        F = x.shape[1]
        if ctx.gmax is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            # dx and the pair gradient from ONE walk of the by-source CSR (the expression and the bits of conan_cfconv_bwd_w_pairs)
            t_rowptr, t_eid = g.transpose()
            dx = torch.empty_like(x)
            dW = torch.empty_like(W)
            # The forward launch cleared this word ONCE: a second backward through the same forward (retain_graph) must not raise a maximum on top
            # of the first pass's — a much smaller second gradient would be put on the fp16 planes with the first one's power of two.  The word is
            # consumed here; a re-entry takes the pair of kernels below, whose dx kernel clears a slot of its own (same bits, one launch more).
            gmax, ctx.gmax = ctx.gmax, None
            call("conan_cfconv_bwd_xw_pairs", ptr(W), ptr(x), ptr(dout), ptr(t_rowptr), ptr(t_eid), ptr(g.tgt), ptr(g.pid), ptr(g.pair_e0), ptr(g.pair_e1),
                 ptr(g.pair_dist), float(g.cutoff), g.num_atoms, F, ptr(dx), ptr(dW), ptr(gmax), stream_ptr())
            _tag_gmax(dW, gmax)
            return dx, dW, None, None, None
        # max |dW| of the pair gradient (F = 128): one device float per CFConv backward, raised by conan_cfconv_bwd_w_pairs with atomicMax.  It is
        # cleared by the dx kernel that runs right before it on this stream (zero_slot) — fresh on every backward pass, no fill launch, and
        # nothing lives on the graph object (round 4 kept a zeroed pool there: stale once a graph object outlived one backward).
        want_gmax = ctx.needs_input_grad[1] and ctx.pairs and F == 128
        gmax = torch.empty(1, dtype=f32, device=x.device) if want_gmax else None
        if ctx.needs_input_grad[0]:
            t_rowptr, t_eid = g.transpose()
            dx = torch.empty_like(x)
            call("conan_cfconv_bwd_x", ptr(W), ptr(dout), ptr(t_rowptr), ptr(t_eid), ptr(g.tgt), ptr(g.pid) if ctx.pairs else None,
                 g.num_atoms, F, ptr(dx), ptr(gmax), stream_ptr())
        elif gmax is not None:
            gmax.zero_()
        if ctx.needs_input_grad[1]:
            dW = torch.empty_like(W)
            if ctx.pairs:
                if not ctx.pre:
                    raise RuntimeError("use_pairs requires pre_cutoff_grad=True (the pair gradient includes the cosine cutoff)")
                call("conan_cfconv_bwd_w_pairs", ptr(x), ptr(dout), ptr(g.num_pairs_dev), g.max_edges, ptr(g.pair_e0), ptr(g.pair_e1), ptr(g.col),
                     ptr(g.tgt), F, ptr(g.pair_dist), float(g.cutoff), ptr(dW), ptr(gmax), stream_ptr())
                if gmax is not None:
                    _tag_gmax(dW, gmax)
            else:
                call("conan_cfconv_bwd_w", ptr(x), ptr(dout), ptr(g.num_edges_dev), g.max_edges, ptr(g.col), ptr(g.tgt), F,
                     ptr(g.dist) if ctx.pre else None, float(g.cutoff or 0.0), ptr(dW), stream_ptr())
        return dx, dW, None, None, None


def cfconv(x: Tensor, W: Tensor, graph: RadiusGraph, pre_cutoff_grad: bool = False, use_pairs: bool = False) -> Tensor:
    """out[i] = sum_{j in N(i)} x[j] * W[(j->i)]   (CFConv.propagate).
    pre_cutoff_grad=True: the gradient returned for W is already multiplied by the cosine cutoff C(d_e), i.e. it is the
    gradient w.r.t. the un-scaled filter (used with `filter_generate`, whose backward then skips its own scaling pass)."""
    return _CFConvFn.apply(x, W, graph, pre_cutoff_grad, use_pairs)


class _SegmentSumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph_ptr, num_graphs):
        x = _c(x)
        out = torch.empty(num_graphs, x.shape[1], dtype=f32, device=x.device)
        call("conan_segment_sum_fwd", ptr(x, f32), ptr(graph_ptr, i32), num_graphs, x.shape[1], ptr(out), stream_ptr())
        ctx.save_for_backward(graph_ptr)
        ctx.shape, ctx.G = x.shape, num_graphs
        return out

    @staticmethod
    def backward(ctx, dout):
        (gp,) = ctx.saved_tensors
        dx = torch.empty(ctx.shape, dtype=f32, device=dout.device)
        call("conan_segment_sum_bwd", ptr(_c(dout)), ptr(gp), ctx.G, ctx.shape[1], ptr(dx), stream_ptr())
        return dx, None, None


def segment_sum(x: Tensor, graph_ptr: Tensor, num_graphs: int) -> Tensor:
    """Sum readout per conformer graph (SumAggregation)."""
    return _SegmentSumFn.apply(x, graph_ptr, num_graphs)


# ------------------------------------------------------------------------------------------------ FGW barycenter
class _DensifyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, graph, N, shift, a, b, adjacency=True):
        feat = _c(feat)
        G, d = graph.num_graphs, feat.shape[1]
        dev = feat.device
        Ys = torch.empty(G, N, d, dtype=f32, device=dev)
        # adjacency=False: features only — the solver reads the structure from the graph's ragged lists (fgw_barycenter_batched(adjacency=graph))
        Cs = torch.empty(G, N, N, dtype=f32, device=dev) if adjacency else torch.empty(0, dtype=f32, device=dev)
        minmax = torch.empty(G, 2, dtype=f32, device=dev)
        call("conan_fgw_densify", ptr(feat, f32), ptr(graph.graph_ptr), ptr(graph.rowptr), ptr(graph.col), G, N, d, shift, a, b,
             ptr(Ys), ptr(Cs) if adjacency else None, ptr(minmax), stream_ptr())
        ctx.save_for_backward(feat, minmax)
        ctx.graph, ctx.args = graph, (N, shift, a, b)
        ctx.mark_non_differentiable(Cs)
        ctx.set_materialize_grads(False)          # no [G,N,N] zero tensor for the adjacency's "gradient" (a 5 us fill per step)
        return Ys, Cs

    @staticmethod
    def backward(ctx, dYs, _dCs):
        if dYs is None:
            return None, None, None, None, None, None, None
        feat, minmax = ctx.saved_tensors
        N, shift, a, b = ctx.args
        g = ctx.graph
        dfeat = torch.empty_like(feat)
        call("conan_fgw_densify_bwd", ptr(feat), ptr(_c(dYs)), ptr(g.graph_ptr), ptr(minmax), g.num_graphs, N, feat.shape[1],
             shift, a, b, ptr(dfeat), stream_ptr())
        return dfeat, None, None, None, None, None, None


def fgw_densify(feat: Tensor, graph: RadiusGraph, max_nodes: int, shift: float, a: float = 0.1, b: float = 2.0, adjacency: bool = True):
    """to_dense_batch + shift + normalize_tensor per conformer slab, and to_dense_adj (schnet_no_sum.py:242-252).  adjacency=False: the [G,N,N]
    adjacency tensors are not built (the second result is empty) — pass the graph itself to `fgw_barycenter_batched(adjacency=graph)`."""
    return _DensifyFn.apply(feat, graph, max_nodes, float(shift), float(a), float(b), bool(adjacency))


PROD_FGW = dict(alpha=0.1, epsilon=0.1, max_iter=5, tol=1e-2, inner_tol=1e-4, num_iter_max=5, stop_thr=1e-2,
                fixed_structure=False, fixed_features=False, warmstart=True)       # schnet_no_sum.py:281-306


FGW_SOLVERS = {"PGD": 0, "PPA": 1, "BAPG": 2}               # the `solver` codes of the FGW entry points (bregman.py:8-67)
_LOSS_CODE = {"square_loss": 0, "kl_loss": 1}               # conan_fgw_params.loss_fun


def _symmetric_code(symmetric) -> int:
    """The `symmetric` code of the FGW entry points: True -> 1, False -> 0, None -> -1 (decided per coupling solve)."""
    if symmetric is True:
        return 1
    if symmetric is False:
        return 0
    if symmetric is None:
        return -1
    raise ValueError(f"symmetric must be True, False or None, not {symmetric!r}")


def _fgw_params(alpha, epsilon, max_iter, tol, inner_tol, num_iter_max, stop_thr, fixed_structure, fixed_features, warmstart, loss_fun,
                cs_small_int=False) -> FgwParams:
    return FgwParams(float(alpha), float(epsilon), int(max_iter), float(tol), float(inner_tol), int(num_iter_max), float(stop_thr),
                     int(bool(fixed_structure)), int(bool(fixed_features)), int(bool(warmstart)), _LOSS_CODE[loss_fun], int(bool(cs_small_int)))


def _barycenter_save(ctx, Ys, Cs, p, lambdas, Y, C, T, loss_code, fs, ff) -> bool:
    """What a barycenter forward (inputs Ys, Cs, ps, p, lambdas, init_C, init_Y, params, in this order) keeps for _barycenter_backward, shared
    by _FgwBarycenterFn and _FgwMixupBarycenterFn -> whether C is differentiable.
    Gradients beyond Ys (conan_fgw_barycenter_bwd_full): the last update steps are differentiable in Cs, p, lambdas (and init_C / init_Y under
    fixed_structure / fixed_features), as in the reference.  Every model asks for Ys only: that path saves and launches exactly what it
    always did, and C stays non-differentiable."""
    need = ctx.needs_input_grad
    want = dict(Ys=need[0] and not ff, Cs=need[1] and Cs is not None and not fs, p=need[3] and p is not None,
                lam=need[4] and lambdas is not None, init_C=need[5] and fs, init_Y=need[6] and ff)
    ctx.full = any(want[k] for k in ("Cs", "p", "lam", "init_C", "init_Y")) or (need[0] and ff)
    c_diff = want["init_C"] if fs else (want["Cs"] or want["p"] or want["lam"])
    if not ctx.full:
        ctx.save_for_backward(T, p, lambdas)
    else:
        kl = loss_code == 1
        ctx.want, ctx.flags = want, (loss_code, int(fs), int(ff))
        keep_Ys = want["lam"] and not ff
        keep_Cs = (want["Cs"] or want["lam"]) and not fs
        keep_Y = want["p"] and not ff
        keep_C = not fs and (want["p"] or (kl and (want["Cs"] or want["lam"])))
        ctx.save_for_backward(T, p, lambdas, Ys if keep_Ys else None, Cs if keep_Cs else None, Y if keep_Y else None,
                              C if keep_C else None)
    return c_diff


def _barycenter_backward(ctx, dY, dC):
    """The gradients of the last update steps at the saved couplings (ctx as _barycenter_save left it) for the eight forward inputs."""
    if not ctx.full:
        if dY is None:
            return (None,) * 8
        T, p, lambdas = ctx.saved_tensors
        B, K, N, d = ctx.dims
        dYs = torch.empty(B, K, N, d, dtype=f32, device=dY.device)
        call("conan_fgw_barycenter_bwd", ptr(T), ptr(_c(dY)), ptr(p), ptr(lambdas), B, K, N, d, ptr(dYs), stream_ptr())
        return dYs, None, None, None, None, None, None, None
    if dY is None and dC is None:
        return (None,) * 8
    T, p, lambdas, Ys, Cs, Y, C = ctx.saved_tensors
    B, K, N, d = ctx.dims
    w = ctx.want
    loss, fs, ff = ctx.flags
    dev = T.device
    new = lambda want, *shape: torch.empty(*shape, dtype=f32, device=dev) if want else None
    dYs, dCs = new(w["Ys"], B, K, N, d), new(w["Cs"], B, K, N, N)
    dp = torch.empty_like(p) if w["p"] else None
    dlam = torch.empty_like(lambdas) if w["lam"] else None
    dinit_C, dinit_Y = new(w["init_C"], B, N, N), new(w["init_Y"], B, N, d)
    ws = torch.empty(int(lib().conan_fgw_barycenter_bwd_full_workspace_bytes(B, K, N, d)), dtype=torch.uint8, device=dev)
    opt = lambda t: ptr(_c(t)) if t is not None else None
    call("conan_fgw_barycenter_bwd_full", ptr(T), ptr(Ys), ptr(Cs), ptr(Y), ptr(C), opt(dY), opt(dC), ptr(p), ptr(lambdas), B, K, N, d,
         loss, fs, ff, ptr(dYs), ptr(dCs), ptr(dp), ptr(dlam), ptr(dinit_C), ptr(dinit_Y), ptr(ws), stream_ptr())
    return dYs, dCs, None, dp, dlam, dinit_C, dinit_Y, None


class _FgwBarycenterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Ys, Cs, ps, p, lambdas, init_C, init_Y, params):
        adj = params.get("adjacency")             # a RadiusGraph: the input graphs' structure straight from its ragged lists, Cs unused
        Ys = _c(Ys)
        Cs = _c(Cs) if adj is None else None
        B, K, N, d = Ys.shape
        if adj is not None and adj.num_graphs != B * K:
            raise RuntimeError(f"adjacency graph holds {adj.num_graphs} conformer graphs, Ys holds {B} x {K}")
        dev = Ys.device
        prm = _fgw_params(params["alpha"], params["epsilon"], params["max_iter"], params["tol"], params["inner_tol"], params["num_iter_max"],
                          params["stop_thr"], params["fixed_structure"], params["fixed_features"], params["warmstart"],
                          params.get("loss_fun", "square_loss"), params.get("cs_small_int", False))
        Y = torch.empty(B, N, d, dtype=f32, device=dev)
        C = torch.empty(B, N, N, dtype=f32, device=dev)
        T = torch.empty(B, K, N, N, dtype=f32, device=dev)
        T_iter = torch.empty(prm.max_iter, B, K, N, N, dtype=f32, device=dev) if params.get("keep_iterates") else None
        info = torch.empty(B, 4, dtype=i32, device=dev)
        errs = torch.empty(B, 2, prm.max_iter, dtype=f32, device=dev)
        solver = FGW_SOLVERS[params.get("solver", "PGD")]
        symmetric = _symmetric_code(params.get("symmetric", True))
        ws_bytes = lib().conan_fgw_workspace_bytes(B, K, N, d, int(adj is not None), solver, symmetric)
        ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
        common = (ptr(ps), ptr(p), ptr(lambdas), ptr(init_C), ptr(init_Y), B, K, N, d, ctypes.byref(prm), solver, symmetric,
                  ptr(Y), ptr(C), ptr(T), ptr(T_iter), ptr(info), ptr(errs), ptr(ws), stream_ptr())
        if adj is None:
            call("conan_fgw_barycenter_fwd", ptr(Ys, f32), ptr(Cs, f32), *common)
        else:       # a RadiusGraph: its four lists in place of Cs
            call("conan_fgw_barycenter_fwd_ragged", ptr(Ys, f32), ptr(adj.graph_ptr, i32), ptr(adj.rowptr, i32), ptr(adj.col, i32), ptr(adj.tgt, i32),
                 *common)
        ctx.dims = (B, K, N, d)
        ctx.set_materialize_grads(False)          # C, T, info, errs carry no gradient: without this autograd fills four zero tensors per backward
        c_diff = _barycenter_save(ctx, Ys, Cs, p, lambdas, Y, C, T, prm.loss_fun, bool(params["fixed_structure"]), bool(params["fixed_features"]))
        nd = (T, info, errs) if c_diff else (C, T, info, errs)
        if T_iter is None:
            ctx.mark_non_differentiable(*nd)
            return Y, C, T, info, errs
        ctx.mark_non_differentiable(*nd, T_iter)
        return Y, C, T, info, errs, T_iter

    @staticmethod
    def backward(ctx, dY, dC=None, *_):
        return _barycenter_backward(ctx, dY, dC)


def fgw_barycenter_batched(Ys: Tensor, Cs: Tensor, ps: Optional[Tensor] = None, p: Optional[Tensor] = None,
                           lambdas: Optional[Tensor] = None, init_C: Optional[Tensor] = None, init_Y: Optional[Tensor] = None,
                           **params):
    """B independent FGW barycenters.  Ys [B,K,N,d], Cs [B,K,N,N] -> Y [B,N,d], C [B,N,N], T [B,K,N,N], info [B,4], errs [B,2,max_iter]
    (+ T_iter [max_iter,B,K,N,N] with keep_iterates=True: the couplings after every outer iteration, barycenter.py:196).
    Gradients flow through the last update steps with the final couplings held constant, like the reference (barycenter.py:120): Y to Ys,
    p and lambdas (to init_Y instead of Ys under fixed_features); C to Cs, p and lambdas (to init_C under fixed_structure).  ps gets none.
    With only Ys requiring grad (every model) C is non-differentiable and the backward is conan_fgw_barycenter_bwd alone.
    `adjacency=graph` (a RadiusGraph with B * K conformer graphs, Cs=None): the input structures are to_dense_adj of those graphs, read by the
    coupling kernels from the ragged neighbour lists — no [B,K,N,N] tensor exists (what the models do).
    `solver` = "PGD" (default: the models' solver), "PPA" or "BAPG" — the reference's three coupling solvers (bregman.py:8-67); info[:, 3] bit 2
    is raised for a molecule whose BAPG / PPA iterate had a zero row or column sum (the reference's NaN case).
    `symmetric` = True (default: the models' solve), False (directed graphs / asymmetric structure matrices: the cost of bregman.py:98-128
    averages the problem and its transpose) or None (decided per coupling solve by torch.allclose(C, C^T, atol=1e-10) on the barycenter
    structure and the input graph, as the reference's every fgw() call does); False / None run the general kernels for every solver."""
    if params.get("solver", "PGD") not in FGW_SOLVERS:
        raise ValueError("Unknown solver '%s'. Pick one in ['PGD', 'PPA', 'BAPG']." % params["solver"])
    _symmetric_code(params.get("symmetric", True))
    prm = dict(PROD_FGW)
    prm.update(params)
    opt = lambda t: _c(t) if t is not None else None
    return _FgwBarycenterFn.apply(Ys, Cs, opt(ps), opt(p), opt(lambdas), opt(init_C), opt(init_Y), prm)


def _pair_params(alpha, epsilon, max_iter, tol, num_iter_max, stop_thr, loss_fun, solver, symmetric):
    if solver not in FGW_SOLVERS:
        raise ValueError("Unknown solver '%s'. Pick one in ['PGD', 'PPA', 'BAPG']." % solver)
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    # conan_fgw_pair_fwd reads alpha, epsilon, max_iter, tol, num_iter_max, stop_thr and loss_fun; the other fields are ignored
    prm = _fgw_params(alpha, epsilon, max_iter, tol, tol, num_iter_max, stop_thr, True, True, False, loss_fun)
    return prm, FGW_SOLVERS[solver], _symmetric_code(None if symmetric is None else bool(symmetric))


def _pair_tensor(t, name, *shape, keep_graph=False):
    if not t.is_cuda:
        raise NotImplementedError(f"the pairwise FGW solve runs on the GPU only: {name} is a CPU tensor")
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must have shape {list(shape)}, not {list(t.shape)}")
    return _c((t if keep_graph else t.detach()).to(f32))


def _pair_prepare(M, C1, C2, p, q, G0, keep_graph=False, keep_start_graph=False):
    """The checked, contiguous fp32 operands of conan_fgw_pair_fwd, n1 != n2 embedded in N = max(n1, n2) with massless nodes -> (M, C1, C2, p, q, G0,
    (B, N, n1, n2)).  keep_graph: the inputs are not detached, so that torch differentiates the conversion and the embedding (G0 only with
    keep_start_graph: the unrolled gradient reaches the start)."""
    if M.dim() != 3:
        raise ValueError(f"M must be [B,n1,n2], not {list(M.shape)}")
    B, n1, n2 = M.shape
    kg = dict(keep_graph=keep_graph)
    M, C1, C2 = _pair_tensor(M, "M", B, n1, n2, **kg), _pair_tensor(C1, "C1", B, n1, n1, **kg), _pair_tensor(C2, "C2", B, n2, n2, **kg)
    p = None if p is None else _pair_tensor(p, "p", B, n1, **kg)
    q = None if q is None else _pair_tensor(q, "q", B, n2, **kg)
    G0 = None if G0 is None else _pair_tensor(G0, "G0", B, n1, n2, keep_graph=keep_start_graph)
    dev, N = M.device, max(n1, n2)
    if n1 != n2:
        def pad(t, *shape):
            out = torch.zeros(B, *shape, dtype=f32, device=dev)
            out[(slice(None),) + tuple(slice(0, k) for k in t.shape[1:])] = t
            return out
        p = pad(torch.full((B, n1), 1.0 / n1, dtype=f32, device=dev) if p is None else p, N)
        q = pad(torch.full((B, n2), 1.0 / n2, dtype=f32, device=dev) if q is None else q, N)
        M, C1, C2 = pad(M, N, N), pad(C1, N, N), pad(C2, N, N)
        G0 = None if G0 is None else pad(G0, N, N)
    return M, C1, C2, p, q, G0, (B, N, n1, n2)


def _pair_fwd(M, C1, C2, p, q, G0, B, N, prm, solver_code, sym_code, with_dist):
    """conan_fgw_pair_fwd on prepared operands -> T [B,N,N], fgw_dist [B] or None, info, errs."""
    dev = M.device
    T = torch.empty(B, N, N, dtype=f32, device=dev)
    dist = torch.empty(B, dtype=f32, device=dev) if with_dist else None
    info = torch.empty(B, 4, dtype=i32, device=dev)
    errs = torch.empty(B, (prm.max_iter + 9) // 10, dtype=f32, device=dev)
    ws = torch.empty(int(lib().conan_fgw_pair_workspace_bytes(B, N, solver_code, sym_code)), dtype=torch.uint8, device=dev)
    call("conan_fgw_pair_fwd", ptr(M, f32), ptr(C1, f32), ptr(C2, f32), ptr(p), ptr(q), ptr(G0), B, N, ctypes.byref(prm), solver_code, sym_code,
         ptr(T), ptr(dist), ptr(info), ptr(errs), ptr(ws), stream_ptr())
    return T, dist, info, errs


def fgw_pair_batched(M: Tensor, C1: Tensor, C2: Tensor, p: Optional[Tensor] = None, q: Optional[Tensor] = None, G0: Optional[Tensor] = None, *,
                     alpha: float = 0.5, epsilon: float = 0.1, max_iter: int = 100, tol: float = 1e-5, num_iter_max: int = 100,
                     stop_thr: float = 1e-5, loss_fun: str = "square_loss", solver: str = "PGD", symmetric=None, with_dist: bool = True):
    """B independent entropic FGW coupling solves, the reference's fgw(M, C1, C2, p, q, ...) (bregman.py:8-279), in one launch of the pair form of
    the general coupling kernels (one workgroup per pair).  M [B,n1,n2] (any cost matrix, used as given), C1 [B,n1,n1], C2 [B,n2,n2], p [B,n1] /
    q [B,n2] or None (uniform), G0 [B,n1,n2] or None (outer(p, q)) -> T [B,n1,n2], fgw_dist [B] (None with with_dist=False), info [B,4] int32 =
    {PGD / PPA / BAPG iterations, Sinkhorn iterations, flags (bit 2: a node with mass had a zero row / column sum), symmetric decision taken},
    errs [B, ceil(max_iter / 10)] = ||T - Tprev|| at every 10th iteration (NaN where not executed).
    max_iter / tol are the solve's own; num_iter_max / stop_thr the Sinkhorn keywords numItermax / stopThr; solver "PGD", "PPA" or "BAPG";
    symmetric True, False or None (decided per pair by torch.allclose(C, C^T, atol=1e-10) on C1 and C2, inside the kernel).  n1 != n2 is solved
    embedded in a square problem of max(n1, n2) nodes whose extra nodes carry no mass (zero rows / columns of M, C1, C2, zero weights): the
    leading block is the reference's rectangular problem.  Non-contiguous inputs are copied.  The outputs carry no gradient: fgw_pair_distance is
    the same solve with a differentiable fgw_dist (the gradient at the returned plan)."""
    prm, solver_code, sym_code = _pair_params(alpha, epsilon, max_iter, tol, num_iter_max, stop_thr, loss_fun, solver, symmetric)
    M, C1, C2, p, q, G0, (B, N, n1, n2) = _pair_prepare(M, C1, C2, p, q, G0)
    T, dist, info, errs = _pair_fwd(M, C1, C2, p, q, G0, B, N, prm, solver_code, sym_code, with_dist)
    return (T if n1 == n2 else T[:, :n1, :n2]), dist, info, errs


def _pair_list_stack(Ms, C1s, C2s, ps, qs, G0s, keep_graph=False, keep_start_graph=False):
    """The ragged pairs of fgw_pair_list embedded in the common Np = max over all n1_b, n2_b -> (M, C1, C2, p, q, G0, sizes)."""
    B = len(Ms)
    if B == 0 or len(C1s) != B or len(C2s) != B:
        raise ValueError("Ms, C1s and C2s must be non-empty lists of the same length")
    for t in list(Ms) + list(C1s) + list(C2s):
        if not t.is_cuda:
            raise NotImplementedError("the pairwise FGW solve runs on the GPU only: got a CPU tensor")
    dev = Ms[0].device
    sizes = [tuple(int(k) for k in m.shape) for m in Ms]
    Np = max(max(s) for s in sizes)

    def stack(ts, cols, default=None, keep=keep_graph):
        out = torch.zeros(B, *([Np] * cols), dtype=f32, device=dev)
        for b in range(B):
            t = ts[b] if ts is not None and ts[b] is not None else default(b)
            out[(b,) + tuple(slice(0, k) for k in t.shape)] = (t if keep else t.detach()).to(f32)
        return out

    G0 = None
    if G0s is not None and any(g is not None for g in G0s):
        if any(g is None for g in G0s):
            raise ValueError("G0s must hold a start plan for every pair or for none")
        G0 = stack(G0s, 2, keep=keep_start_graph)
    return (stack(Ms, 2), stack(C1s, 2), stack(C2s, 2), stack(ps, 1, lambda b: torch.full((sizes[b][0],), 1.0 / sizes[b][0], device=dev)),
            stack(qs, 1, lambda b: torch.full((sizes[b][1],), 1.0 / sizes[b][1], device=dev)), G0, sizes)


def fgw_pair_list(Ms, C1s, C2s, ps=None, qs=None, G0s=None, **params):
    """fgw_pair_batched for pairs of different sizes: Ms[b] [n1_b,n2_b], C1s[b], C2s[b], ps[b] / qs[b] / G0s[b] (the lists, or single entries,
    may be None).  Every pair is embedded in the common Np = max over all n1_b, n2_b with massless nodes and the batch is ONE launch.
    Returns ([T_b [n1_b,n2_b]], fgw_dist [B], info [B,4], errs).  No gradient: fgw_pair_distance_list is the differentiable form."""
    M, C1, C2, p, q, G0, sizes = _pair_list_stack(Ms, C1s, C2s, ps, qs, G0s)
    T, dist, info, errs = fgw_pair_batched(M, C1, C2, p, q, G0, **params)
    return [T[b, :n1, :n2] for b, (n1, n2) in enumerate(sizes)], dist, info, errs


def _mixup_tensor(t, name, *shape, keep_graph=False):
    if not t.is_cuda:
        raise NotImplementedError(f"the FGWMixup solve runs on the GPU only: {name} is a CPU tensor")
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must have shape {list(shape)}, not {list(t.shape)}")
    return _c((t if keep_graph else t.detach()).to(f32))


def _mixup_step(rho, epoch, eps):
    rho, epoch, eps = float(rho), int(epoch), float(eps)
    if not (rho > 0 and math.isfinite(rho)):
        raise ValueError(f"rho must be positive and finite, not {rho}")
    if epoch <= 0:
        raise ValueError(f"epoch must be positive, not {epoch}")
    return rho, epoch, eps


def _acc_prepare(M, A, Bm, a, b, X0, n1, n2, keep_graph=False, keep_start_graph=False):
    """The checked, contiguous fp32 operands of conan_fgw_acc_pair_fwd, N1 != N2 and own sizes embedded in N = max(N1, N2) with massless nodes
    -> (M, A, Bm, a, b, X0, (B, N, N1, N2)).  keep_graph: the inputs are not detached, so that torch differentiates the conversion and the
    embedding (X0 only with keep_start_graph: the unrolled gradient reaches the start, the fixed-plan one does not)."""
    if M.dim() != 3:
        raise ValueError(f"M must be [B,N1,N2], not {list(M.shape)}")
    B, N1, N2 = M.shape
    kg = dict(keep_graph=keep_graph)
    M, A, Bm = _mixup_tensor(M, "M", B, N1, N2, **kg), _mixup_tensor(A, "A", B, N1, N1, **kg), _mixup_tensor(Bm, "Bm", B, N2, N2, **kg)
    a = None if a is None else _mixup_tensor(a, "a", B, N1, **kg)
    b = None if b is None else _mixup_tensor(b, "b", B, N2, **kg)
    X0 = None if X0 is None else _mixup_tensor(X0, "X0", B, N1, N2, keep_graph=keep_start_graph)
    dev, N = M.device, max(N1, N2)
    if N1 != N2 or n1 is not None or n2 is not None:
        def own(n, Nc):
            n = torch.full((B,), Nc, device=dev) if n is None else torch.as_tensor(n, device=dev).reshape(B)
            return (torch.arange(N, device=dev)[None, :] < n[:, None]).to(f32), n.to(f32)

        def pad(t, *shape):
            out = torch.zeros(B, *shape, dtype=f32, device=dev)
            out[(slice(None),) + tuple(slice(0, k) for k in t.shape[1:])] = t
            return out
        (m1, c1), (m2, c2) = own(n1, N1), own(n2, N2)
        a = m1 / c1[:, None] if a is None else pad(a, N) * m1
        b = m2 / c2[:, None] if b is None else pad(b, N) * m2
        M, A, Bm = pad(M, N, N), pad(A, N, N), pad(Bm, N, N)
        X0 = None if X0 is None else pad(X0, N, N)
    return M, A, Bm, a, b, X0, (B, N, N1, N2)


def _acc_fwd(M, A, Bm, a, b, X0, B, N, alpha, rho, epoch, eps):
    """conan_fgw_acc_pair_fwd on prepared operands -> X [B,N,N], objs, info."""
    dev = M.device
    X = torch.empty(B, N, N, dtype=f32, device=dev)
    objs = torch.empty(B, (epoch + 9) // 10, dtype=f32, device=dev)
    info = torch.empty(B, 4, dtype=i32, device=dev)
    ws = torch.empty(int(lib().conan_fgw_acc_pair_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)
    call("conan_fgw_acc_pair_fwd", ptr(M, f32), ptr(A, f32), ptr(Bm, f32), ptr(a), ptr(b), ptr(X0), B, N, float(alpha), rho, epoch, eps,
         ptr(X), ptr(objs), ptr(info), ptr(ws), stream_ptr())
    return X, objs, info


def fgw_acc_pair_batched(M: Tensor, A: Tensor, Bm: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, X0: Optional[Tensor] = None, *,
                         alpha: float, rho: float, epoch: int = 200, eps: float = 1e-5, n1: Optional[Tensor] = None, n2: Optional[Tensor] = None):
    """B independent FGWMixup coupling solves, the reference's fused_ACC_torch(M, A, B, a, b, X, alpha, epoch, eps, rho) (barycenter.py:228-256:
    accelerated mirror descent, not the Bregman solve of fgw_pair_batched(solver="BAPG")), in one launch, one workgroup per pair.
    M [B,N1,N2], A [B,N1,N1], Bm [B,N2,N2] (untransposed in the gradient, as the reference has it), a [B,N1] / b [B,N2] or None (uniform), X0
    [B,N1,N2] the start or None (a b^T) -> X [B,N1,N2], objs [B, ceil(epoch / 10)] (the objective of every check that ran, the stopping one
    included; NaN elsewhere), info [B,4] int32 = {epochs run, checks stored = the reference's len(obj_list), flags, 0}; flags bit 2: a row or
    column with mass had a zero or non-finite sum (the reference's NaN, computed here too).
    n1 [B] / n2 [B] int (optional): the pairs' own sizes inside the [N1,N2] container (uniform weights are then uniform over the own nodes).
    N1 != N2 and own sizes are solved embedded in a square problem of max(N1, N2) nodes whose extra nodes carry no mass: their entries stay
    exactly zero (no 1e-10 is added there), so the leading block is the reference's rectangular solve.  One consequence: a weight the caller
    sets to ZERO means "absent", where the reference lifts such entries by 1e-10 per epoch.  fp32 in and out, fp64 inside.  No gradient:
    fgw_acc_pair_distance is the same solve with the differentiable FGWMixup distance of the returned plan.  fgw_acc_pair_unrolled is the same
    solve with the reference's gradient through the unrolled epochs on the plan and the distance."""
    rho, epoch, eps = _mixup_step(rho, epoch, eps)
    M, A, Bm, a, b, X0, (B, N, N1, N2) = _acc_prepare(M, A, Bm, a, b, X0, n1, n2)
    X, objs, info = _acc_fwd(M, A, Bm, a, b, X0, B, N, alpha, rho, epoch, eps)
    return (X if N1 == N2 else X[:, :N1, :N2]), objs, info


def _mixup_barycenter_fwd(Ys, Cs, ps, p, lambdas, init_C, init_Y, prm, rho, epoch, eps, keep_iterates):
    """conan_fgw_mixup_barycenter_fwd on prepared operands -> Y, C, T, info, errs, T_iter (or None)."""
    B, K, N, d = Ys.shape
    dev = Ys.device
    Y = torch.empty(B, N, d, dtype=f32, device=dev)
    C = torch.empty(B, N, N, dtype=f32, device=dev)
    T = torch.empty(B, K, N, N, dtype=f32, device=dev)
    T_iter = torch.empty(prm.max_iter, B, K, N, N, dtype=f32, device=dev) if keep_iterates else None
    info = torch.empty(B, 4, dtype=i32, device=dev)
    errs = torch.empty(B, 2, prm.max_iter, dtype=f32, device=dev)
    ws = torch.empty(int(lib().conan_fgw_mixup_workspace_bytes(B, K, N, d)), dtype=torch.uint8, device=dev)
    call("conan_fgw_mixup_barycenter_fwd", ptr(Ys, f32), ptr(Cs, f32), ptr(ps), ptr(p), ptr(lambdas), ptr(init_C), ptr(init_Y), B, K, N, d,
         ctypes.byref(prm), rho, epoch, eps, ptr(Y), ptr(C), ptr(T), ptr(T_iter), ptr(info), ptr(errs), ptr(ws), stream_ptr())
    return Y, C, T, info, errs, T_iter


class _FgwMixupBarycenterFn(torch.autograd.Function):
    """fgw_mixup_barycenter_batched with gradients: forward is conan_fgw_mixup_barycenter_fwd on the prepared fp32 operands, backward that of
    _FgwBarycenterFn (the FGWMixup barycenter ends with the same three update steps: _barycenter_save / _barycenter_backward), at the couplings of
    the last outer iteration, held constant.  params = (conan_fgw_params, rho, epoch, eps, keep_iterates)."""
    @staticmethod
    def forward(ctx, Ys, Cs, ps, p, lambdas, init_C, init_Y, params):
        prm, rho, epoch, eps, keep_iterates = params
        Y, C, T, info, errs, T_iter = _mixup_barycenter_fwd(Ys, Cs, ps, p, lambdas, init_C, init_Y, prm, rho, epoch, eps, keep_iterates)
        ctx.dims = tuple(Ys.shape)
        ctx.set_materialize_grads(False)
        c_diff = _barycenter_save(ctx, Ys, Cs, p, lambdas, Y, C, T, prm.loss_fun, bool(prm.fixed_structure), bool(prm.fixed_features))
        nd = (T, info, errs) if c_diff else (C, T, info, errs)
        if T_iter is None:
            ctx.mark_non_differentiable(*nd)
            return Y, C, T, info, errs
        ctx.mark_non_differentiable(*nd, T_iter)
        return Y, C, T, info, errs, T_iter

    @staticmethod
    def backward(ctx, dY, dC=None, *_):
        return _barycenter_backward(ctx, dY, dC)


def fgw_mixup_barycenter_batched(Ys: Tensor, Cs: Tensor, ps: Optional[Tensor] = None, p: Optional[Tensor] = None, lambdas: Optional[Tensor] = None,
                                 init_C: Optional[Tensor] = None, init_Y: Optional[Tensor] = None, *, alpha: float = 0.5, rho: float = 1.0,
                                 max_iter: int = 100, tol: float = 1e-9, epoch: int = 100, eps: float = 1e-5, fixed_structure: bool = False,
                                 fixed_features: bool = False, loss_fun: str = "square_loss", keep_iterates: bool = False):
    """B independent FGWMixup barycenters, the reference's fgw_barycenters_BAPG (barycenter.py:259-390): the outer loop of fgw_barycenter_batched
    (same updates, error norms and stop rule) around the coupling solve of fgw_acc_pair_batched, run for every input graph in every outer
    iteration from p ps[s]^T with `epoch` epochs at most and `eps` (the reference: 100 and 1e-5) and the caller's rho.
    Ys [B,K,N,d], Cs [B,K,N,N] (may be directed), ps [B,K,N] / p [B,N] or None (uniform), lambdas [K] or None, init_C [B,N,N] or None
    (Cs[:,0]), init_Y [B,N,d] or None (zeros) -> Y [B,N,d], C [B,N,N], T [B,K,N,N], info [B,4] int32 = {outer iterations, epochs summed over
    couplings and iterations, 0, flags}, errs [B,2,max_iter] (+ T_iter [max_iter,B,K,N,N] with keep_iterates=True).  Flags bit 2: a row or
    column with mass had a zero or non-finite sum (the molecule's outputs are then NaN, as the reference's).  Zero entries of p / ps are
    nodes without mass (the embedding of other sizes); see fgw_acc_pair_batched.
    Gradients flow through the last update steps with the couplings T of the last outer iteration held constant, the convention of
    fgw_barycenter_batched (and the same backward kernels): Y to Ys, p and lambdas (to init_Y instead of Ys under fixed_features); C to Cs, p
    and lambdas (to init_C under fixed_structure; with init_C=None there, C is Cs[:, 0] and gets none).  ps, T, info, errs and T_iter get none;
    no double backward.  This is NOT the reference's gradient, which back-propagates through all `epoch` epochs of every coupling solve; a finite
    difference of this function moves the plan, so it does not check this gradient.  With only Ys requiring grad C is non-differentiable and
    the backward is conan_fgw_barycenter_bwd alone.  A molecule whose flags have bit 2 (NaN outputs) gives NaN gradients for its own inputs
    and, through the sum over molecules, for lambdas; they are not masked.  With no input requiring grad, or under torch.no_grad(), nothing
    is saved and the call is the forward launch alone.  fgw_mixup_barycenter_unrolled is the same solve with the reference's gradient through
    every epoch of every coupling solve."""
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    rho, epoch, eps = _mixup_step(rho, epoch, eps)
    if Ys.dim() != 4:
        raise ValueError(f"Ys must be [B,K,N,d], not {list(Ys.shape)}")
    B, K, N, d = Ys.shape
    kg = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (Ys, Cs, p, lambdas, init_C, init_Y))
    opt = lambda t, name, *shape: None if t is None else _mixup_tensor(t, name, *shape, keep_graph=kg)
    Ys, Cs = opt(Ys, "Ys", B, K, N, d), opt(Cs, "Cs", B, K, N, N)
    ps = None if ps is None else _mixup_tensor(ps, "ps", B, K, N)
    p, lambdas = opt(p, "p", B, N), opt(lambdas, "lambdas", K)
    init_C, init_Y = opt(init_C, "init_C", B, N, N), opt(init_Y, "init_Y", B, N, d)
    if fixed_features and init_Y is None:
        raise ValueError("If Y is fixed it must be initialized")
    prm = _fgw_params(alpha, 0.0, max_iter, tol, 0.0, 1, 0.0, fixed_structure, fixed_features, False, loss_fun)
    if kg:
        return _FgwMixupBarycenterFn.apply(Ys, Cs, ps, p, lambdas, init_C, init_Y, (prm, rho, epoch, eps, bool(keep_iterates)))
    res = _mixup_barycenter_fwd(Ys, Cs, ps, p, lambdas, init_C, init_Y, prm, rho, epoch, eps, keep_iterates)
    return res[:5] if res[5] is None else res


# ------------------------------------------------------------------- the reference's gradient through the unrolled barycenter (fgw_mixup_grad.hip)
class _FgwMixupUnrolledFn(torch.autograd.Function):
    """fgw_mixup_barycenter_batched's solve (conan_fgw_mixup_barycenter_fwd_record: the same launches plus device-to-device copies of the fp64
    state) with conan_fgw_mixup_barycenter_bwd as its backward: the gradient through every epoch of every coupling solve of every outer iteration,
    as the reference's autograd delivers it, from the cotangents of Y and C to Ys, Cs, ps, p, lambdas, init_C and init_Y.  Kept from the forward:
    the inputs, info and the state record.  params = (conan_fgw_params, rho, epoch, eps, keep_iterates).  No double backward, no host
    synchronisation."""
    @staticmethod
    def forward(ctx, Ys, Cs, ps, p, lambdas, init_C, init_Y, params):
        prm, rho, epoch, eps, keep_iterates = params
        B, K, N, d = Ys.shape
        dev = Ys.device
        Y = torch.empty(B, N, d, dtype=f32, device=dev)
        C = torch.empty(B, N, N, dtype=f32, device=dev)
        T = torch.empty(B, K, N, N, dtype=f32, device=dev)
        T_iter = torch.empty(prm.max_iter, B, K, N, N, dtype=f32, device=dev) if keep_iterates else None
        info = torch.empty(B, 4, dtype=i32, device=dev)
        errs = torch.empty(B, 2, prm.max_iter, dtype=f32, device=dev)
        record = torch.empty((prm.max_iter + 1) * B * (N * N + N * d), dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib().conan_fgw_mixup_workspace_bytes(B, K, N, d)), dtype=torch.uint8, device=dev)
        call("conan_fgw_mixup_barycenter_fwd_record", ptr(Ys, f32), ptr(Cs, f32), ptr(ps), ptr(p), ptr(lambdas), ptr(init_C), ptr(init_Y), B, K, N, d,
             ctypes.byref(prm), rho, epoch, eps, ptr(Y), ptr(C), ptr(T), ptr(T_iter), ptr(info), ptr(errs), ptr(record), ptr(ws), stream_ptr())
        ctx.save_for_backward(Ys, Cs, ps, p, lambdas, init_Y, info, record)
        ctx.dims, ctx.params, ctx.has_init_C = (B, K, N, d), (prm, rho, epoch, eps), init_C is not None
        ctx.set_materialize_grads(False)
        nd = (T, info, errs) if T_iter is None else (T, info, errs, T_iter)
        ctx.mark_non_differentiable(*nd)
        return (Y, C) + nd

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dY, dC=None, *_):
        if dY is None and dC is None:
            return (None,) * 8
        Ys, Cs, ps, p, lambdas, init_Y, info, record = ctx.saved_tensors
        B, K, N, d = ctx.dims
        prm, rho, epoch, eps = ctx.params
        need = ctx.needs_input_grad
        dev = Ys.device
        dY = None if dY is None else _c(dY.to(f32))
        dC = None if dC is None else _c(dC.to(f32))
        new = lambda want, *shape: torch.empty(*shape, dtype=f32, device=dev) if want else None
        start_in_Cs = not ctx.has_init_C                  # the start is Cs[:, 0]: its gradient goes there
        dYs = new(need[0], B, K, N, d)
        dCs = new(need[1], B, K, N, N)
        dps = new(need[2] and ps is not None, B, K, N)
        dp = new(need[3] and p is not None, B, N)
        dlam = new(need[4] and lambdas is not None, K)
        dinit_C = new(need[5] if ctx.has_init_C else need[1], B, N, N)
        dinit_Y = new(need[6] and init_Y is not None, B, N, d)
        nbytes = int(lib().conan_fgw_mixup_barycenter_bwd_workspace_bytes(B, K, N, d, epoch))
        if nbytes == 0:
            raise NotImplementedError(f"the unrolled FGWMixup barycenter gradient does not support N = {N}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        call("conan_fgw_mixup_barycenter_bwd", ptr(Ys, f32), ptr(Cs, f32), ptr(ps), ptr(p), ptr(lambdas), ptr(init_Y), B, K, N, d, ctypes.byref(prm),
             rho, epoch, eps, ptr(info), ptr(record), ptr(dY), ptr(dC), ptr(dYs), ptr(dCs), ptr(dps), ptr(dp), ptr(dlam), ptr(dinit_C), ptr(dinit_Y),
             None, None, ptr(ws), stream_ptr())
        if start_in_Cs and dCs is not None:
            dCs[:, 0] += dinit_C
            dinit_C = None
        return dYs, dCs, dps, dp, dlam, dinit_C, dinit_Y, None


def fgw_mixup_barycenter_unrolled(Ys: Tensor, Cs: Tensor, ps: Optional[Tensor] = None, p: Optional[Tensor] = None, lambdas: Optional[Tensor] = None,
                                  init_C: Optional[Tensor] = None, init_Y: Optional[Tensor] = None, *, alpha: float = 0.5, rho: float = 1.0,
                                  max_iter: int = 100, tol: float = 1e-9, epoch: int = 100, eps: float = 1e-5, fixed_structure: bool = False,
                                  fixed_features: bool = False, loss_fun: str = "square_loss", keep_iterates: bool = False):
    """fgw_mixup_barycenter_batched's solve (same arguments, defaults, checks and return tuple; Y, C, T, info, errs and T_iter bit-identical)
    whose Y and C carry the gradient that torch autograd forms through the reference's fgw_barycenters_BAPG (barycenter.py:259-390: its
    coupling solves run with autograd on): through the update steps, the feature costs and every epoch of every coupling solve of every outer
    iteration — the total derivative, not the one at couplings held constant that fgw_mixup_barycenter_batched delivers.  Gradients reach Ys,
    Cs, ps, p, lambdas, init_C and init_Y.  With init_C=None the start is Cs[:, 0] and its gradient goes there; with init_Y=None the start is
    a constant zero.  T, info, errs and T_iter are not differentiable (a deviation: the reference's log["T"] has a graph), and the stop
    decisions carry no gradient.  A weight that is exactly zero marks an absent node: it gets exactly 0 in all its entries.  A molecule whose
    info flags have bit 2 gets NaN in its own gradients and, through the sum over molecules, in dlambdas.
    The forward adds device-to-device copies of the barycenter's fp64 state after init and after every update to the batched op's launches:
    (max_iter + 1) * B * (N^2 + N d) * 8 bytes, kept for the backward with the inputs and info.  The backward (conan_fgw_mixup_barycenter_bwd)
    is 2 max_iter + 1 launches: per outer iteration, descending, one workgroup per coupling that replays the solve (with the forward's
    objective checks, so it stops where the forward did), forms the update steps' partials, walks the half-steps in reverse and differentiates
    the feature cost, then one workgroup per molecule that sums the couplings' shares; one last launch rounds to fp32.  A molecule that ran
    fewer outer iterations (info[:, 0], read on the device) leaves the earlier launches at once.  Its workspace holds the record of one
    solve's half-steps per coupling, reused by every outer iteration: B * K * 2 epoch * N^2 * 8 bytes (2.2 GB at B K = 1280, N = 33, epoch
    100), plus B K (4 N^2 + 2 N d) * 8 bytes of accumulators and five N x N fp64 matrices per coupling above N = 61.  When no input requires
    grad, or under torch.no_grad(), nothing beyond the batched op's forward runs and nothing is saved.  No double backward, no host
    synchronisation in either direction."""
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    rho, epoch, eps = _mixup_step(rho, epoch, eps)
    if Ys.dim() != 4:
        raise ValueError(f"Ys must be [B,K,N,d], not {list(Ys.shape)}")
    B, K, N, d = Ys.shape
    kg = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (Ys, Cs, ps, p, lambdas, init_C, init_Y))
    opt = lambda t, name, *shape: None if t is None else _mixup_tensor(t, name, *shape, keep_graph=kg)
    Ys, Cs = opt(Ys, "Ys", B, K, N, d), opt(Cs, "Cs", B, K, N, N)
    ps, p, lambdas = opt(ps, "ps", B, K, N), opt(p, "p", B, N), opt(lambdas, "lambdas", K)
    init_C, init_Y = opt(init_C, "init_C", B, N, N), opt(init_Y, "init_Y", B, N, d)
    if fixed_features and init_Y is None:
        raise ValueError("If Y is fixed it must be initialized")
    prm = _fgw_params(alpha, 0.0, max_iter, tol, 0.0, 1, 0.0, fixed_structure, fixed_features, False, loss_fun)
    if kg:
        return _FgwMixupUnrolledFn.apply(Ys, Cs, ps, p, lambdas, init_C, init_Y, (prm, rho, epoch, eps, bool(keep_iterates)))
    res = _mixup_barycenter_fwd(Ys, Cs, ps, p, lambdas, init_C, init_Y, prm, rho, epoch, eps, keep_iterates)
    return res[:5] if res[5] is None else res


class _FgwPairDistFn(torch.autograd.Function):
    """fgw_dist of B square pairs as a differentiable value: forward runs `run()` -> (dist [B], T [B,N,N], info, errs) (the solve with its own
    distance kernel, or conan_fgw_pair_dist of a given plan: the distance is never formed twice), backward is conan_fgw_pair_dist_bwd at that
    plan, which is a constant (the reference solves the barycenter's couplings under torch.no_grad() too, barycenter.py:120).  M, C1, C2 [B,N,N]
    and p, q [B,N] or None are the prepared fp32 operands; only the gradients that are needed are computed.  No double backward."""
    @staticmethod
    def forward(ctx, M, C1, C2, p, q, run, alpha, loss_code):
        dist, T, info, errs = run()
        ctx.save_for_backward(C1, C2, p, q, T)
        ctx.alpha, ctx.loss_code = float(alpha), int(loss_code)
        ctx.mark_non_differentiable(*(t for t in (T, info, errs) if t is not None))
        return dist, T, info, errs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        C1, C2, p, q, T = ctx.saved_tensors
        B, N, _n = T.shape
        want = ctx.needs_input_grad[:5]
        out = [torch.empty(B, *([N] * k), dtype=f32, device=T.device) if w else None for w, k in zip(want, (2, 2, 2, 1, 1))]
        call("conan_fgw_pair_dist_bwd", ptr(C1, f32), ptr(C2, f32), ptr(p), ptr(q), ptr(T, f32), ptr(_c(g.to(f32)), f32), B, N, ctx.alpha, ctx.loss_code,
             *(ptr(t) for t in out), stream_ptr())
        return (*out, None, None, None)


def fgw_pair_distance(M: Tensor, C1: Tensor, C2: Tensor, p: Optional[Tensor] = None, q: Optional[Tensor] = None, G0: Optional[Tensor] = None, *,
                      alpha: float = 0.5, epsilon: float = 0.1, max_iter: int = 100, tol: float = 1e-5, num_iter_max: int = 100,
                      stop_thr: float = 1e-5, loss_fun: str = "square_loss", solver: str = "PGD", symmetric=None, return_plan: bool = False):
    """The FGW distances of B pairs as a loss: fgw_pair_batched's solve (same arguments, same launch, same bits of fgw_dist) -> dist [B], which
    carries gradients to M, C1, C2, p and q — those of (1 - alpha) sum(M * T) + alpha gwloss(init_matrix(C1, C2, p, q), T) at the RETURNED plan T,
    held constant (conan_fgw_pair_dist_bwd).  This is not the reference's log["fgw_dist"].backward(), which unrolls every Sinkhorn sweep.  T and G0
    get no gradient; no double backward.  Rectangular pairs are embedded as in fgw_pair_batched and the gradients come back in the caller's
    shapes; only the gradients of inputs that require grad are computed.  return_plan: (dist, T [B,n1,n2], info, errs), the last three without
    gradient."""
    prm, solver_code, sym_code = _pair_params(alpha, epsilon, max_iter, tol, num_iter_max, stop_thr, loss_fun, solver, symmetric)
    M, C1, C2, p, q, G0, (B, N, n1, n2) = _pair_prepare(M, C1, C2, p, q, G0, keep_graph=True)

    def run():
        T, dist, info, errs = _pair_fwd(M, C1, C2, p, q, G0, B, N, prm, solver_code, sym_code, True)
        return dist, T, info, errs

    dist, T, info, errs = _FgwPairDistFn.apply(M, C1, C2, p, q, run, alpha, prm.loss_fun)
    return (dist, (T if n1 == n2 else T[:, :n1, :n2]), info, errs) if return_plan else dist


def fgw_pair_distance_list(Ms, C1s, C2s, ps=None, qs=None, G0s=None, *, return_plan: bool = False, **params):
    """fgw_pair_distance for pairs of different sizes (the lists of fgw_pair_list, one launch) -> dist [B]; with return_plan
    (dist, [T_b [n1_b,n2_b]], info, errs)."""
    M, C1, C2, p, q, G0, sizes = _pair_list_stack(Ms, C1s, C2s, ps, qs, G0s, keep_graph=True)
    dist, T, info, errs = fgw_pair_distance(M, C1, C2, p, q, G0, return_plan=True, **params)
    return (dist, [T[b, :n1, :n2] for b, (n1, n2) in enumerate(sizes)], info, errs) if return_plan else dist


def fgw_pair_dist(M: Tensor, C1: Tensor, C2: Tensor, T: Tensor, p: Optional[Tensor] = None, q: Optional[Tensor] = None, *, alpha: float = 0.5,
                  loss_fun: str = "square_loss") -> Tensor:
    """The reference's log["fgw_dist"] of the plans T [B,N,N] (conan_fgw_pair_dist; square problems: embed rectangular ones as fgw_pair_batched
    does): (1 - alpha) sum(M * T) + alpha * gwloss(init_matrix(C1, C2, p, q, loss_fun), T), bregman.py:163-164 -> [B].  When one of M, C1, C2, p, q
    requires grad the result carries the gradient at the given plan to them (conan_fgw_pair_dist_bwd; T gets none); the value is the same."""
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    B, N, _ = M.shape
    kg = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (M, C1, C2, p, q))
    M, C1, C2 = (_pair_tensor(t, n, B, N, N, keep_graph=kg) for t, n in ((M, "M"), (C1, "C1"), (C2, "C2")))
    T = _pair_tensor(T, "T", B, N, N)
    p = None if p is None else _pair_tensor(p, "p", B, N, keep_graph=kg)
    q = None if q is None else _pair_tensor(q, "q", B, N, keep_graph=kg)

    def run():
        out = torch.empty(B, dtype=f32, device=M.device)
        call("conan_fgw_pair_dist", ptr(M, f32), ptr(C1, f32), ptr(C2, f32), ptr(p), ptr(q), ptr(T, f32), B, N, float(alpha),
             _LOSS_CODE[loss_fun], ptr(out), stream_ptr())
        return out, T, None, None

    return _FgwPairDistFn.apply(M, C1, C2, p, q, run, alpha, _LOSS_CODE[loss_fun])[0] if kg else run()[0]


def fgw_acc_pair_distance(M: Tensor, A: Tensor, Bm: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, X0: Optional[Tensor] = None, *,
                          alpha: float, rho: float, epoch: int = 200, eps: float = 1e-5, n1: Optional[Tensor] = None, n2: Optional[Tensor] = None,
                          return_plan: bool = False):
    """The FGWMixup distances of B pairs as a loss: fgw_acc_pair_batched's solve (same arguments, same launch, same bits of X) -> dist [B],
    the distance the reference's commented lines describe (barycenter.py:348-350) at the returned plan X:
        (1 - alpha) <M, X> + alpha (<c1, X> - 2 <A X Bm, X>),   c1 = (A o A) a 1^T + 1 b^T (Bm o Bm),
    that is the solve's final objective plus alpha <c1, X>.  It is formed once, by conan_fgw_pair_dist on the solved plan with C2 = Bm^T (the
    kernel's C1 X C2^T is then FGWMixup's untransposed A X Bm on directed graphs), and carries gradients to M, A, Bm, a and b — those of the
    formula at the RETURNED plan, held constant (conan_fgw_pair_dist_bwd).  This is not what back-propagating through the reference's epochs gives;
    X and X0 get no gradient; no double backward; a finite difference of this function moves the plan, so it does not check this gradient.
    Rectangular and own-size pairs are embedded as in fgw_acc_pair_batched and the gradients come back in the caller's shapes.
    return_plan: (dist, X [B,N1,N2], objs, info), the last three as fgw_acc_pair_batched returns them, without gradient.
    fgw_acc_pair_unrolled delivers the gradient through the unrolled epochs instead."""
    rho, epoch, eps = _mixup_step(rho, epoch, eps)
    M, A, Bm, a, b, X0, (B, N, N1, N2) = _acc_prepare(M, A, Bm, a, b, X0, n1, n2, keep_graph=True)
    Bt = _c(Bm.transpose(1, 2))

    def run():
        X, objs, info = _acc_fwd(M, A, Bm, a, b, X0, B, N, alpha, rho, epoch, eps)
        dist = torch.empty(B, dtype=f32, device=M.device)
        call("conan_fgw_pair_dist", ptr(M, f32), ptr(A, f32), ptr(Bt, f32), ptr(a), ptr(b), ptr(X, f32), B, N, float(alpha), _LOSS_CODE["square_loss"],
             ptr(dist), stream_ptr())
        return dist, X, info, objs

    dist, X, info, objs = _FgwPairDistFn.apply(M, A, Bt, a, b, run, alpha, _LOSS_CODE["square_loss"])
    return (dist, (X if N1 == N2 else X[:, :N1, :N2]), objs, info) if return_plan else dist


# ------------------------------------------------------------------- the reference's gradient through the unrolled epochs (fgw_acc_grad.hip)
def _acc_dist(M, A, Bm, a, b, X, B, N, alpha):
    """fgw_acc_pair_distance's value at the plan X: conan_fgw_pair_dist with C2 = Bm^T -> dist [B]."""
    dist = torch.empty(B, dtype=f32, device=M.device)
    call("conan_fgw_pair_dist", ptr(M, f32), ptr(A, f32), ptr(_c(Bm.transpose(1, 2)), f32), ptr(a), ptr(b), ptr(X, f32), B, N, float(alpha),
         _LOSS_CODE["square_loss"], ptr(dist), stream_ptr())
    return dist


def _pair_unrolled_backward(ctx, saved, gX, gdist, entry, ws_query, ws_args, scalars, what, n_chk):
    """The backward of the three pair-form unrolled ops: `entry`(M, A, Bm, a, b, X0, B, N, *scalars, info, gX, gdist, dM, dA, dBm, da, db, dX0,
    n_chk null check outputs, workspace, stream) -> the gradients of M, A, Bm, a, b, X0 (None where not needed).  `ws_query`(B, N, *ws_args) = 0
    says that N is not supported: NotImplementedError naming `what`."""
    M, A, Bm, a, b, X0, info = saved
    B, N = ctx.dims
    dev = M.device
    gX = None if gX is None else _c(gX.to(f32))
    gdist = None if gdist is None else _c(gdist.to(f32))
    need = ctx.needs_input_grad
    dM, dA, dBm = (torch.empty(B, N, N, dtype=f32, device=dev) for _ in range(3))
    da = torch.empty(B, N, dtype=f32, device=dev) if a is not None and need[3] else None
    db = torch.empty(B, N, dtype=f32, device=dev) if b is not None and need[4] else None
    dX0 = torch.empty(B, N, N, dtype=f32, device=dev) if X0 is not None and need[5] else None
    nbytes = int(getattr(lib(), ws_query)(B, N, *ws_args))
    if nbytes == 0:
        raise NotImplementedError(f"the unrolled {what} gradient does not support N = {N}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call(entry, ptr(M, f32), ptr(A, f32), ptr(Bm, f32), ptr(a), ptr(b), ptr(X0), B, N, *scalars, ptr(info), ptr(gX), ptr(gdist), ptr(dM), ptr(dA),
         ptr(dBm), ptr(da), ptr(db), ptr(dX0), *(None,) * n_chk, ptr(ws), stream_ptr())
    return dM if need[0] else None, dA if need[1] else None, dBm if need[2] else None, da, db, dX0


class _FgwAccUnrolledFn(torch.autograd.Function):
    """fgw_acc_pair_batched's launch and fgw_acc_pair_distance's distance with conan_fgw_acc_pair_bwd as their backward: the gradient through the
    executed epochs, as the reference's autograd delivers it, from the cotangents of X and dist to M, A, Bm, a, b and X0.  The backward is ONE
    launch that replays the epochs from the saved inputs (nothing but the inputs and info is kept from the forward).  No double backward, no
    host synchronisation."""
    @staticmethod
    def forward(ctx, M, A, Bm, a, b, X0, dims, alpha, rho, epoch, eps):
        B, N = dims
        X, objs, info = _acc_fwd(M, A, Bm, a, b, X0, B, N, alpha, rho, epoch, eps)
        dist = _acc_dist(M, A, Bm, a, b, X, B, N, alpha)
        ctx.save_for_backward(M, A, Bm, a, b, X0, info)
        ctx.dims, ctx.alpha, ctx.rho, ctx.epoch = dims, float(alpha), float(rho), int(epoch)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(objs, info)
        return X, dist, objs, info

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gX, gdist, *_):
        if gX is None and gdist is None:
            return (None,) * 11
        return _pair_unrolled_backward(ctx, ctx.saved_tensors, gX, gdist, "conan_fgw_acc_pair_bwd", "conan_fgw_acc_pair_bwd_workspace_bytes", (ctx.epoch,),
                                       (ctx.alpha, ctx.rho, ctx.epoch), "FGWMixup", 1) + (None,) * 5


def fgw_acc_pair_unrolled(M: Tensor, A: Tensor, Bm: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, X0: Optional[Tensor] = None, *,
                          alpha: float, rho: float, epoch: int = 200, eps: float = 1e-5, n1: Optional[Tensor] = None, n2: Optional[Tensor] = None):
    """fgw_acc_pair_batched's solve and fgw_acc_pair_distance's distance (same arguments, same launches, same bits) -> (X, dist, objs, info),
    where X and dist carry the reference's gradient through the unrolled epochs (its fused_ACC_torch is differentiable torch code,
    barycenter.py:228-256) to M, A, Bm, a, b, and to X0 when one is given: the total derivative, not the one at a plan held constant that
    fgw_acc_pair_distance delivers.  One backward launch per backward call (conan_fgw_acc_pair_bwd) serves both cotangents: it replays the epochs
    the forward ran (info[:, 0], read on the device), recording the fp64 input of every half-step, and walks them in reverse.  a / b given as
    None (uniform) get none; info and objs are not differentiable (the reference's obj_list is: a deviation), and the stop decision carries no
    gradient.  A node without mass (a_i = 0, b_j = 0, the padding of rectangular and own-size pairs) gets exactly 0 in its rows / columns of
    every gradient and in da_i / db_j, where the reference — which lifts such entries by 1e-10 — gives a finite da_i; a pair with info flags
    bit 2 (a zero or non-finite line sum) gets NaN gradients, as the reference's autograd gives.  Rectangular and own-size pairs are embedded as in
    fgw_acc_pair_batched and the gradients come back in the caller's shapes.  The backward's workspace is B * (2 epoch + 3) * N^2 * 8 bytes, N =
    max(N1, N2): the record of the half-steps alone is B * 2 epoch * N^2 * 8 bytes (3.5 MB per 33 x 33 pair at the default epoch = 200), plus
    five N x N fp64 matrices per pair above N = 61; the caller chooses the cap.  When no input requires grad nothing is saved and nothing
    beyond the two forward launches runs.  No double backward, no host synchronisation in either direction."""
    rho, epoch, eps = _mixup_step(rho, epoch, eps)
    kg = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (M, A, Bm, a, b, X0))
    M, A, Bm, a, b, X0, (B, N, N1, N2) = _acc_prepare(M, A, Bm, a, b, X0, n1, n2, keep_graph=kg, keep_start_graph=kg)
    if kg:
        X, dist, objs, info = _FgwAccUnrolledFn.apply(M, A, Bm, a, b, X0, (B, N), alpha, rho, epoch, eps)
    else:
        X, objs, info = _acc_fwd(M, A, Bm, a, b, X0, B, N, alpha, rho, epoch, eps)
        dist = _acc_dist(M, A, Bm, a, b, X, B, N, alpha)
    return (X if N1 == N2 else X[:, :N1, :N2]), dist, objs, info


# ------------------------------------------------------------------- the reference's gradient through the unrolled pair solve (fgw_pair_grad.hip)
class _FgwPairUnrolledFn(torch.autograd.Function):
    """fgw_pair_batched's launch with conan_fgw_pair_bwd as its backward: the gradient through the executed PGD / PPA iterations and their
    Sinkhorn sweeps, as the reference's autograd delivers it, from the cotangents of T and fgw_dist to M, C1, C2, p, q and G0.  The backward
    is ONE launch that replays the iterations from the saved inputs (nothing but the inputs and info is kept from the forward).  No double
    backward, no host synchronisation."""
    @staticmethod
    def forward(ctx, M, C1, C2, p, q, G0, dims, prm, solver_code, sym_code, exact):
        B, N = dims
        T, dist, info, errs = _pair_fwd(M, C1, C2, p, q, G0, B, N, prm, solver_code, sym_code, True)
        ctx.save_for_backward(M, C1, C2, p, q, G0, info)
        # exact: the caller's alpha, epsilon, stop_thr as Python floats (the forward's parameter block holds their fp32 roundings; the replay runs in
        # fp64 on what the reference's fp64 run is given)
        ctx.dims, ctx.cfg = dims, (*exact[:2], int(prm.max_iter), int(prm.num_iter_max), exact[2], solver_code, sym_code)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(info, errs)
        return T, dist, info, errs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gT, gdist, *_):
        if gT is None and gdist is None:
            return (None,) * 11
        max_iter, num_iter_max = ctx.cfg[2:4]
        return _pair_unrolled_backward(ctx, ctx.saved_tensors, gT, gdist, "conan_fgw_pair_bwd", "conan_fgw_pair_bwd_workspace_bytes", (max_iter, num_iter_max),
                                       ctx.cfg, "pairwise FGW", 2) + (None,) * 5


def _pair_unrolled_params(alpha, epsilon, max_iter, tol, num_iter_max, stop_thr, loss_fun, solver, symmetric):
    prm, solver_code, sym_code = _pair_params(alpha, epsilon, max_iter, tol, num_iter_max, stop_thr, loss_fun, solver, symmetric)
    if solver == "BAPG":
        raise NotImplementedError("the unrolled pairwise FGW gradient covers solver 'PGD' and 'PPA': 'BAPG' is not implemented")
    if loss_fun != "square_loss":
        raise NotImplementedError("the unrolled pairwise FGW gradient covers loss_fun 'square_loss': 'kl_loss' is not implemented")
    return prm, solver_code, sym_code


def fgw_pair_unrolled(M: Tensor, C1: Tensor, C2: Tensor, p: Optional[Tensor] = None, q: Optional[Tensor] = None, G0: Optional[Tensor] = None, *,
                      alpha: float = 0.5, epsilon: float = 0.1, max_iter: int = 100, tol: float = 1e-5, num_iter_max: int = 100,
                      stop_thr: float = 1e-5, loss_fun: str = "square_loss", solver: str = "PGD", symmetric=None):
    """fgw_pair_batched's solve (same arguments, same launch, same bits) -> (T, fgw_dist, info, errs), where T and fgw_dist carry the reference's
    gradient through the unrolled solve — what torch autograd forms through its fgw (bregman.py:70-167: every executed PGD / PPA iteration and
    every Sinkhorn sweep inside it) — to M, C1, C2, p, q, and to G0 when one is given: the total derivative, not the one at a plan held
    constant that fgw_pair_distance delivers.  One backward launch per backward call (conan_fgw_pair_bwd) serves both cotangents: it replays in
    fp64 the iterations the forward ran (info[:, 0], read on the device), recording every iteration's input plan and deciding its Sinkhorn sweep
    count by the reference's rule, and walks them in reverse.  Solver "PGD" or "PPA", the square loss, symmetric True / False / None; "BAPG" and
    "kl_loss" raise NotImplementedError.  p / q given as None (uniform) get none; info and errs are not differentiable (the reference's
    log["err"] is: a deviation), and the stop decisions carry no gradient.  A node without mass (p_i = 0, q_j = 0, the padding of rectangular
    and own-size pairs) gets exactly 0 in its rows / columns of every gradient and in dp_i / dq_j, where the reference's log(0) gives NaN; a
    pair with info flags bit 2, or whose replay meets a non-finite plan or, under PPA, the logarithm of an exact zero of a plan, gets NaN
    gradients, as the reference's autograd gives, beside healthy pairs that keep theirs.  Rectangular pairs are embedded as in fgw_pair_batched
    and the gradients come back in the caller's shapes; a leaf shared by the batch (an expanded M) gets the sum.  The backward's workspace is
    B * ((max_iter + 3) N^2 + (4 num_iter_max + 2) N) * 8 bytes, N = max(n1, n2) (1.0 MB per 33 x 33 pair at the defaults; 76 KB at the models'
    max_iter = 5, num_iter_max = 5), plus five N x N fp64 matrices per pair above N = 61; the caller chooses the caps.  When no input requires grad
    nothing is saved and nothing beyond the forward runs.  No double backward, no host synchronisation in either direction."""
    prm, solver_code, sym_code = _pair_unrolled_params(alpha, epsilon, max_iter, tol, num_iter_max, stop_thr, loss_fun, solver, symmetric)
    kg = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (M, C1, C2, p, q, G0))
    M, C1, C2, p, q, G0, (B, N, n1, n2) = _pair_prepare(M, C1, C2, p, q, G0, keep_graph=kg, keep_start_graph=kg)
    if kg:
        T, dist, info, errs = _FgwPairUnrolledFn.apply(M, C1, C2, p, q, G0, (B, N), prm, solver_code, sym_code, (float(alpha), float(epsilon), float(stop_thr)))
    else:
        T, dist, info, errs = _pair_fwd(M, C1, C2, p, q, G0, B, N, prm, solver_code, sym_code, True)
    return (T if n1 == n2 else T[:, :n1, :n2]), dist, info, errs


def fgw_pair_unrolled_list(Ms, C1s, C2s, ps=None, qs=None, G0s=None, **params):
    """fgw_pair_unrolled for pairs of different sizes (the lists of fgw_pair_list, one forward and one backward launch) ->
    ([T_b [n1_b,n2_b]], fgw_dist [B], info, errs); the gradients reach the list entries in their own shapes, and a pair's bits do not depend on
    the batch it is part of."""
    _pair_unrolled_params(0.5, 0.1, 1, 1e-5, 1, 1e-5, params.get("loss_fun", "square_loss"), params.get("solver", "PGD"), None)      # the refusals first
    kg = torch.is_grad_enabled() and any(t is not None and t.requires_grad for ts in (Ms, C1s, C2s, ps, qs, G0s) if ts is not None for t in ts)
    M, C1, C2, p, q, G0, sizes = _pair_list_stack(Ms, C1s, C2s, ps, qs, G0s, keep_graph=kg, keep_start_graph=kg)
    T, dist, info, errs = fgw_pair_unrolled(M, C1, C2, p, q, G0, **params)
    return [T[b, :n1, :n2] for b, (n1, n2) in enumerate(sizes)], dist, info, errs


# ------------------------------------------------------------- the reference's gradient through the unrolled BAPG pair solve (fgw_bregman_grad.hip)
class _FgwBregmanUnrolledFn(torch.autograd.Function):
    """fgw_pair_batched(solver="BAPG")'s launch with conan_fgw_bregman_bwd as its backward: the gradient through the executed Bregman half-steps,
    as the reference's autograd delivers it through fgw_bregman, from the cotangents of T and fgw_dist to M, C1, C2, p, q and G0.  The backward
    is ONE launch that replays the iterations from the saved inputs (nothing but the inputs and info is kept from the forward).  No double
    backward, no host synchronisation."""
    @staticmethod
    def forward(ctx, M, C1, C2, p, q, G0, dims, prm, sym_code, exact):
        B, N = dims
        T, dist, info, errs = _pair_fwd(M, C1, C2, p, q, G0, B, N, prm, FGW_SOLVERS["BAPG"], sym_code, True)
        ctx.save_for_backward(M, C1, C2, p, q, G0, info)
        # exact: the caller's alpha, epsilon as Python floats (the forward's parameter block holds their fp32 roundings; the replay runs in fp64 on
        # what the reference's fp64 run is given)
        ctx.dims, ctx.cfg = dims, (*exact, int(prm.max_iter), int(prm.loss_fun), sym_code)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(info, errs)
        return T, dist, info, errs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gT, gdist, *_):
        if gT is None and gdist is None:
            return (None,) * 10
        return _pair_unrolled_backward(ctx, ctx.saved_tensors, gT, gdist, "conan_fgw_bregman_bwd", "conan_fgw_bregman_bwd_workspace_bytes", (ctx.cfg[2],),
                                       ctx.cfg, "BAPG FGW", 2) + (None,) * 4


def fgw_bregman_unrolled(M: Tensor, C1: Tensor, C2: Tensor, p: Optional[Tensor] = None, q: Optional[Tensor] = None, G0: Optional[Tensor] = None, *,
                         alpha: float = 0.5, epsilon: float = 0.1, max_iter: int = 1000, tol: float = 1e-9, loss_fun: str = "square_loss",
                         symmetric=None):
    """fgw_pair_batched(solver="BAPG")'s solve (same launch, same bits) -> (T, fgw_dist, info, errs), where T and fgw_dist carry the reference's
    gradient through the unrolled solve — what torch autograd forms through its fgw_bregman (bregman.py:170-279: every executed Bregman
    half-step) — to M, C1, C2, p, q, and to G0 when one is given: the total derivative, not the one at a plan held constant that
    fgw_pair_distance delivers.  One backward launch per backward call (conan_fgw_bregman_bwd) serves both cotangents: it replays in fp64 the
    iterations the forward ran (info[:, 0], read on the device, never re-decided), recording every half-step's input plan, and walks the
    half-steps in reverse.  loss_fun "square_loss" or "kl_loss", symmetric True / False / None.  p / q given as None (uniform) get none; info
    and errs are not differentiable (the reference's log["err"] is: a deviation), and the stop decisions carry no gradient.  A node without mass
    (p_i = 0, q_j = 0, the padding of rectangular and own-size pairs) gets exactly 0 in its rows / columns of every gradient and in dp_i / dq_j,
    where the reference's 0 / 0 gives NaN; a pair with info flags bit 2, or whose replay meets a zero sum or a non-finite plan, gets NaN
    gradients, as the reference's autograd gives, beside healthy pairs that keep theirs.  Rectangular pairs are embedded as in fgw_pair_batched
    and the gradients come back in the caller's shapes; a leaf shared by the batch (an expanded M) gets the sum.  The backward's workspace is
    B * (2 max_iter + 4) N^2 * 8 bytes, N = max(n1, n2) (1.8 MB per 33 x 33 pair at max_iter = 100, 17.5 MB at the default 1000), plus five
    N x N fp64 matrices per pair above N = 61; the cap is the caller's choice.  When no input requires grad nothing is saved and nothing beyond
    the forward runs.  No double backward, no host synchronisation in either direction."""
    prm, _, sym_code = _pair_params(alpha, epsilon, max_iter, tol, 1, 1e-9, loss_fun, "BAPG", symmetric)
    kg = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (M, C1, C2, p, q, G0))
    M, C1, C2, p, q, G0, (B, N, n1, n2) = _pair_prepare(M, C1, C2, p, q, G0, keep_graph=kg, keep_start_graph=kg)
    if kg:
        T, dist, info, errs = _FgwBregmanUnrolledFn.apply(M, C1, C2, p, q, G0, (B, N), prm, sym_code, (float(alpha), float(epsilon)))
    else:
        T, dist, info, errs = _pair_fwd(M, C1, C2, p, q, G0, B, N, prm, FGW_SOLVERS["BAPG"], sym_code, True)
    return (T if n1 == n2 else T[:, :n1, :n2]), dist, info, errs


def fgw_bregman_unrolled_list(Ms, C1s, C2s, ps=None, qs=None, G0s=None, **params):
    """fgw_bregman_unrolled for pairs of different sizes (the lists of fgw_pair_list, one forward and one backward launch) ->
    ([T_b [n1_b,n2_b]], fgw_dist [B], info, errs); the gradients reach the list entries in their own shapes, and a pair's bits do not depend on
    the batch it is part of."""
    kg = torch.is_grad_enabled() and any(t is not None and t.requires_grad for ts in (Ms, C1s, C2s, ps, qs, G0s) if ts is not None for t in ts)
    M, C1, C2, p, q, G0, sizes = _pair_list_stack(Ms, C1s, C2s, ps, qs, G0s, keep_graph=kg, keep_start_graph=kg)
    T, dist, info, errs = fgw_bregman_unrolled(M, C1, C2, p, q, G0, **params)
    return [T[b, :n1, :n2] for b, (n1, n2) in enumerate(sizes)], dist, info, errs


# ------------------------------------------------------------------------------------------------ entropic OT on its own (sinkhorn.hip)
SINKHORN_METHODS = {"sinkhorn_log": 0, "sinkhorn": 1}


def _sinkhorn_tensor(t, name, shapes, dtype=f32, keep_graph=False):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise NotImplementedError(f"the Sinkhorn solve runs on the GPU only: {name} is a CPU tensor")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"{name} must have shape {' or '.join(str(list(sh)) for sh in shapes)}, not {list(t.shape)}")
    return _c((t if keep_graph else t.detach()).to(dtype))


def _sinkhorn_prepare(M, a, b, warmstart, n1, n2, method, keep_graph=False, keep_vec_graph=False):
    """The checked, contiguous operands of conan_sinkhorn_fwd -> (M, a, b, wu, wv, n1, n2, (B, N1, N2, method code)).  M [B,N1,N2], or [N1,N2]
    shared by the B problems of a / b / n1 / n2 (m_batch_stride = 0).  keep_graph: M stays attached to autograd; keep_vec_graph: a, b and
    warmstart[0] too (the unrolled gradient)."""
    if method not in SINKHORN_METHODS:
        raise ValueError("Unknown method '%s'." % method)
    if not torch.is_tensor(M) or not M.is_cuda:
        raise NotImplementedError("the Sinkhorn solve runs on the GPU only: M is a CPU tensor")
    if M.dim() not in (2, 3):
        raise ValueError(f"M must be [B,N1,N2] or [N1,N2], not {list(M.shape)}")
    N1, N2 = int(M.shape[-2]), int(M.shape[-1])
    if M.dim() == 3:
        B = int(M.shape[0])
    else:
        B = next((int(t.shape[0]) for t in (b, a, n1, n2) if t is not None and t.dim() == (1 if t is n1 or t is n2 else 2)), 1)
    M = _sinkhorn_tensor(M, "M", [(B, N1, N2), (N1, N2)], keep_graph=keep_graph)
    vec = lambda t, name, n, keep=False: None if t is None else _sinkhorn_tensor(t, name, [(B, n)] + ([(n,)] if B == 1 else []), keep_graph=keep)
    a, b = vec(a, "a", N1, keep_vec_graph), vec(b, "b", N2, keep_vec_graph)
    wu, wv = (None, None) if warmstart is None else (vec(warmstart[0], "warmstart[0]", N1, keep_vec_graph), vec(warmstart[1], "warmstart[1]", N2))
    n1 = None if n1 is None else _sinkhorn_tensor(n1, "n1", [(B,)], i32)
    n2 = None if n2 is None else _sinkhorn_tensor(n2, "n2", [(B,)], i32)
    return M, a, b, wu, wv, n1, n2, (B, N1, N2, SINKHORN_METHODS[method])


def _sinkhorn_fwd(M, a, b, wu, wv, n1, n2, B, N1, N2, code, reg, num_iter_max, stop_thr):
    """conan_sinkhorn_fwd on prepared operands -> T [B,N1,N2], loss [B], log_u [B,N1], log_v [B,N2], info [B,4], errs.  No host synchronisation."""
    dev = M.device
    T = torch.empty(B, N1, N2, dtype=f32, device=dev)
    loss = torch.empty(B, dtype=f32, device=dev)
    log_u, log_v = torch.empty(B, N1, dtype=f32, device=dev), torch.empty(B, N2, dtype=f32, device=dev)
    info = torch.empty(B, 4, dtype=i32, device=dev)
    errs = torch.empty(B, (int(num_iter_max) + 9) // 10, dtype=f32, device=dev)
    ws = torch.empty(max(int(lib().conan_sinkhorn_workspace_bytes(B, N1, N2)), 1), dtype=torch.uint8, device=dev)
    call("conan_sinkhorn_fwd", ptr(M, f32), ptr(a), ptr(b), ptr(wu), ptr(wv), ptr(n1), ptr(n2), B, N1, N2, N1 * N2 if M.dim() == 3 else 0,
         float(reg), code, int(num_iter_max), float(stop_thr), ptr(T), ptr(loss), ptr(log_u), ptr(log_v), ptr(info), ptr(errs), ptr(ws), stream_ptr())
    return T, loss, log_u, log_v, info, errs


def sinkhorn_batched(M: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, *, reg: float, method: str = "sinkhorn_log",
                     num_iter_max: int = 1000, stop_thr: float = 1e-9, warmstart=None, n1: Optional[Tensor] = None, n2: Optional[Tensor] = None):
    """B independent entropic OT problems in one launch (one workgroup per problem): the reference's sinkhorn_log (method "sinkhorn_log",
    sinkhorn.py:318-450) or sinkhorn_knopp ("sinkhorn", :207-315).  M [B,N1,N2] costs, or [N1,N2] shared by the whole batch; a [B,N1] / b [B,N2]
    marginals or None (uniform over the problem's own size); warmstart (log_u [B,N1], log_v [B,N2]) or None; n1 / n2 [B] int32 device tensors: the
    problems' own sizes inside the container, or None.  Rectangular problems are solved as they are.
    -> T [B,N1,N2], loss [B] = sum(M * T), log_u [B,N1], log_v [B,N2] (for "sinkhorn" the logs of its u, v), info [B,4] int32 = {niter (the
    reference's log["niter"]), flags (bit 0: stopped on err < stop_thr, bit 1: Knopp's numerical-errors exit, bit 2: the exact log-domain path was
    taken), checks executed, 0}, errs [B, ceil(num_iter_max / 10)] (log["err"]; NaN where not executed).  Outside a problem's own block every
    output is zero.  A problem's bits do not depend on the batch, its position or the container.  The Knopp exit is decided on fp64 values, so it
    follows the reference's fp64 run (fp32 exp underflows earlier).  No gradient (sinkhorn_loss is the differentiable form) and no host
    synchronisation."""
    M, a, b, wu, wv, n1, n2, (B, N1, N2, code) = _sinkhorn_prepare(M, a, b, warmstart, n1, n2, method)
    return _sinkhorn_fwd(M, a, b, wu, wv, n1, n2, B, N1, N2, code, reg, num_iter_max, stop_thr)


def _sinkhorn_list_stack(Ms, as_, bs, warmstarts, container, keep_graph=False, keep_vec_graph=False):
    """Ragged problems in one container [B,N1,N2] (default: the largest n1 and n2) with their sizes on the device.  keep_graph / keep_vec_graph
    as _sinkhorn_prepare."""
    B = len(Ms)
    if B == 0:
        raise ValueError("Ms must be a non-empty list")
    for t in Ms:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise NotImplementedError("the Sinkhorn solve runs on the GPU only: got a CPU tensor")
    dev = Ms[0].device
    sizes = [tuple(int(k) for k in m.shape) for m in Ms]
    N1, N2 = container if container is not None else (max(s[0] for s in sizes), max(s[1] for s in sizes))
    if any(s[0] > N1 or s[1] > N2 for s in sizes):
        raise ValueError("container is smaller than a problem")

    def stack(ts, shape, axis, keep=False):
        if ts is None or all(t is None for t in ts):
            return None
        out = torch.zeros(B, *shape, dtype=f32, device=dev)
        for k in range(B):
            t = ts[k]
            if t is None or t.numel() == 0:       # uniform over the problem's own size
                out[k, :sizes[k][axis]] = 1.0 / sizes[k][axis]
            else:
                out[(k,) + tuple(slice(0, n) for n in t.shape)] = (t if keep else t.detach()).to(f32)
        return out

    M = stack(Ms, (N1, N2), 0, keep=keep_graph)
    warm = None
    if warmstarts is not None and any(w is not None for w in warmstarts):
        if any(w is None for w in warmstarts):
            raise ValueError("warmstarts must hold a warm start for every problem or for none")
        warm = (stack([w[0] for w in warmstarts], (N1,), 0, keep=keep_vec_graph), stack([w[1] for w in warmstarts], (N2,), 1))
    n1 = torch.tensor([s[0] for s in sizes], dtype=i32, device=dev)
    n2 = torch.tensor([s[1] for s in sizes], dtype=i32, device=dev)
    return M, stack(as_, (N1,), 0, keep=keep_vec_graph), stack(bs, (N2,), 1, keep=keep_vec_graph), warm, n1, n2, sizes


def sinkhorn_list(Ms, as_=None, bs=None, *, warmstarts=None, container=None, **params):
    """sinkhorn_batched for problems of different sizes: Ms[k] [n1_k,n2_k], as_[k] / bs[k] / warmstarts[k] (the lists, or single entries of
    as_ / bs, may be None: uniform).  ONE launch through the per-problem sizes: no problem is embedded in a larger one, each runs over its own
    rows and columns inside the container (N1, N2) (default: the largest sizes).
    -> ([T_k [n1_k,n2_k]], loss [B], [log_u_k], [log_v_k], info [B,4], errs)."""
    M, a, b, warm, n1, n2, sizes = _sinkhorn_list_stack(Ms, as_, bs, warmstarts, container)
    T, loss, lu, lv, info, errs = sinkhorn_batched(M, a, b, warmstart=warm, n1=n1, n2=n2, **params)
    return ([T[k, :s[0], :s[1]] for k, s in enumerate(sizes)], loss, [lu[k, :s[0]] for k, s in enumerate(sizes)],
            [lv[k, :s[1]] for k, s in enumerate(sizes)], info, errs)


class _SinkhornLossFn(torch.autograd.Function):
    """loss[B] = sum(M * T) of the solved plans as a differentiable value under the project's fixed-plan convention (fgw_pair_distance's): the
    plan is a constant of the backward, dM = gout * T (a torch multiply on the saved plan), nothing flows to a, b or the warm start.  No double
    backward."""
    @staticmethod
    def forward(ctx, M, run):
        T, loss, log_u, log_v, info, errs = run()
        ctx.save_for_backward(T)
        ctx.shared = M.dim() == 2
        ctx.mark_non_differentiable(T, log_u, log_v, info, errs)
        return loss, T, log_u, log_v, info, errs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        (T,) = ctx.saved_tensors
        dM = g.to(f32)[:, None, None] * T
        return (dM.sum(0) if ctx.shared else dM), None


def sinkhorn_loss(M: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, *, reg: float, method: str = "sinkhorn_log",
                  num_iter_max: int = 1000, stop_thr: float = 1e-9, warmstart=None, n1: Optional[Tensor] = None, n2: Optional[Tensor] = None,
                  return_plan: bool = False, grad: str = "plan"):
    """The entropic OT costs sum(M * T) of B problems as a loss: sinkhorn_batched's solve (same arguments, same launch, same bits) -> loss [B].
    grad="plan" (default): it carries the gradient at the RETURNED plan, held constant, to M: dM = gout * T; a, b and the warm start get none.
    grad="unrolled": the reference's gradient through every Sinkhorn sweep to M, a, b and warmstart[0] (sinkhorn_unrolled; with return_plan the
    plan carries it too).  No double backward; no host synchronisation.  return_plan: (loss, T, log_u, log_v, info, errs)."""
    if grad == "unrolled":
        T, loss, log_u, log_v, info, errs = sinkhorn_unrolled(M, a, b, reg=reg, method=method, num_iter_max=num_iter_max, stop_thr=stop_thr,
                                                              warmstart=warmstart, n1=n1, n2=n2)
        return (loss, T, log_u, log_v, info, errs) if return_plan else loss
    if grad != "plan":
        raise ValueError("grad must be 'plan' or 'unrolled', not %r" % (grad,))
    Mp, a, b, wu, wv, n1, n2, (B, N1, N2, code) = _sinkhorn_prepare(M, a, b, warmstart, n1, n2, method, keep_graph=True)
    out = _SinkhornLossFn.apply(Mp, lambda: _sinkhorn_fwd(Mp.detach(), a, b, wu, wv, n1, n2, B, N1, N2, code, reg, num_iter_max, stop_thr))
    return out if return_plan else out[0]


# --------------------------------------------------------------------------- the reference's unrolled gradient (sinkhorn_grad.hip)
class _SinkhornUnrolledFn(torch.autograd.Function):
    """sinkhorn_batched's launch with conan_sinkhorn_bwd as its backward: the gradient through the S executed sweeps, as the reference's autograd
    delivers it, from the cotangents of T and loss to M, a, b and warmstart[0].  The backward is ONE launch that recomputes the sweeps from the
    saved inputs (nothing but the inputs and info is kept from the forward).  No double backward, no host synchronisation."""
    @staticmethod
    def forward(ctx, M, a, b, wu, wv, n1, n2, dims, reg, num_iter_max, stop_thr):
        B, N1, N2, code = dims
        T, loss, log_u, log_v, info, errs = _sinkhorn_fwd(M, a, b, wu, wv, n1, n2, B, N1, N2, code, reg, num_iter_max, stop_thr)
        ctx.save_for_backward(M, a, b, wu, wv, n1, n2, info)
        ctx.dims, ctx.reg, ctx.num_iter_max = dims, float(reg), int(num_iter_max)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(log_u, log_v, info, errs)
        return T, loss, log_u, log_v, info, errs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gT, gloss, *_):
        M, a, b, wu, wv, n1, n2, info = ctx.saved_tensors
        B, N1, N2, code = ctx.dims
        if gT is None and gloss is None:
            return (None,) * 11
        dev = M.device
        gT = None if gT is None else _c(gT.to(f32))
        gloss = None if gloss is None else _c(gloss.to(f32))
        need = ctx.needs_input_grad
        dM = torch.empty(B, N1, N2, dtype=f32, device=dev)
        da = torch.empty(B, N1, dtype=f32, device=dev) if a is not None and need[1] else None
        db = torch.empty(B, N2, dtype=f32, device=dev) if b is not None and need[2] else None
        dwu = torch.empty(B, N1, dtype=f32, device=dev) if wu is not None and need[3] else None
        nbytes = int(lib().conan_sinkhorn_bwd_workspace_bytes(B, N1, N2, ctx.num_iter_max))
        if nbytes == 0:
            raise NotImplementedError(f"the unrolled Sinkhorn gradient does not support the container {N1} x {N2}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        call("conan_sinkhorn_bwd", ptr(M, f32), ptr(a), ptr(b), ptr(wu), ptr(wv), ptr(n1), ptr(n2), B, N1, N2, N1 * N2 if M.dim() == 3 else 0,
             ctx.reg, code, ctx.num_iter_max, ptr(info), ptr(gloss), ptr(gT), ptr(dM), ptr(da), ptr(db), ptr(dwu), ptr(ws), stream_ptr())
        like = lambda g, t: None if g is None else g.reshape(t.shape)
        return ((dM.sum(0) if M.dim() == 2 else dM) if need[0] else None, like(da, a), like(db, b), like(dwu, wu)) + (None,) * 7


def sinkhorn_unrolled(M: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, *, reg: float, method: str = "sinkhorn_log",
                      num_iter_max: int = 1000, stop_thr: float = 1e-9, warmstart=None, n1: Optional[Tensor] = None, n2: Optional[Tensor] = None):
    """sinkhorn_batched (same arguments, same ONE launch, same bits) -> (T, loss, log_u, log_v, info, errs), where T and loss carry the
    reference's gradient through the unrolled Sinkhorn sweeps (its sinkhorn / sinkhorn2 are differentiable torch code) to M, a, b and
    warmstart[0]: one backward launch (conan_sinkhorn_bwd) that recomputes the executed sweeps, runs them in reverse and forms dM from the
    stored vector histories.  A 2-D shared M gets the sum over the batch; a / b given as None (uniform) get none; warmstart[1] gets none (the
    first column pass overwrites v; the reference's .grad is None there too); log_u, log_v, info, errs are not differentiable; the stop decision
    carries no gradient.  An entry a_i = 0 (b_j = 0) gets gradient 0 and contributes nothing (the reference: NaN at that entry for
    sinkhorn_log, NaN everywhere for Knopp).  The backward's workspace is (2 num_iter_max + 1) (N1 + N2) * 8 bytes per problem (1 MB per
    33 x 33 problem at num_iter_max = 1000): the caller chooses the cap.  No double backward, no host synchronisation in either direction."""
    M, a, b, wu, wv, n1, n2, dims = _sinkhorn_prepare(M, a, b, warmstart, n1, n2, method, keep_graph=True, keep_vec_graph=True)
    return _SinkhornUnrolledFn.apply(M, a, b, wu, wv, n1, n2, dims, reg, num_iter_max, stop_thr)


def sinkhorn_unrolled_list(Ms, as_=None, bs=None, *, warmstarts=None, container=None, **params):
    """sinkhorn_unrolled for problems of different sizes in ONE launch each way (arguments and result as sinkhorn_list): the plans and loss
    carry the unrolled gradient to the entries of Ms, as_, bs and to warmstarts[k][0]."""
    M, a, b, warm, n1, n2, sizes = _sinkhorn_list_stack(Ms, as_, bs, warmstarts, container, keep_graph=True, keep_vec_graph=True)
    T, loss, lu, lv, info, errs = sinkhorn_unrolled(M, a, b, warmstart=warm, n1=n1, n2=n2, **params)
    return ([T[k, :s[0], :s[1]] for k, s in enumerate(sizes)], loss, [lu[k, :s[0]] for k, s in enumerate(sizes)],
            [lv[k, :s[1]] for k, s in enumerate(sizes)], info, errs)


# ------------------------------------------------------------------------- the reference's other three Sinkhorn solvers (sinkhorn_ext.hip)
SINKHORN_EXT_METHODS = {"greenkhorn": 2, "sinkhorn_stabilized": 3, "sinkhorn_epsilon_scaling": 4}
_SINKHORN_EXT_ITERS = {"greenkhorn": 10000, "sinkhorn_stabilized": 1000, "sinkhorn_epsilon_scaling": 100}      # the reference's numItermax defaults


def _sinkhorn_ext_prepare(M, a, b, warmstart, n1, n2, method, keep_graph=False):
    if method not in SINKHORN_EXT_METHODS:
        raise ValueError("Unknown method '%s'." % method)
    M, a, b, _wu, _wv, n1, n2, (B, N1, N2, _) = _sinkhorn_prepare(M, a, b, None, n1, n2, "sinkhorn", keep_graph=keep_graph)
    f64 = torch.float64                                                   # the potentials travel as fp64 (see conan_sinkhorn_ext_fwd)
    vec = lambda t, name, n: _sinkhorn_tensor(t, name, [(B, n)] + ([(n,)] if B == 1 else []), f64)
    wu, wv = (None, None) if warmstart is None else (vec(warmstart[0], "warmstart[0]", N1), vec(warmstart[1], "warmstart[1]", N2))
    return M, a, b, wu, wv, n1, n2, (B, N1, N2, SINKHORN_EXT_METHODS[method])


def _sinkhorn_ext_fwd(M, a, b, wu, wv, n1, n2, B, N1, N2, code, reg, num_iter_max, stop_thr, tau, print_period, epsilon0, num_inner_iter_max):
    """conan_sinkhorn_ext_fwd on prepared operands.  No host synchronisation."""
    dev = M.device
    nerr = int(lib().conan_sinkhorn_ext_nerr(code, int(num_iter_max), int(print_period)))
    if nerr < 0:
        raise ValueError("num_iter_max and print_period must be positive")
    T = torch.empty(B, N1, N2, dtype=f32, device=dev)
    loss = torch.empty(B, dtype=f32, device=dev)
    log_u, log_v = torch.empty(B, N1, dtype=f32, device=dev), torch.empty(B, N2, dtype=f32, device=dev)
    alpha, beta = torch.empty(B, N1, dtype=torch.float64, device=dev), torch.empty(B, N2, dtype=torch.float64, device=dev)
    info, extra = torch.empty(B, 4, dtype=i32, device=dev), torch.empty(B, 4, dtype=i32, device=dev)
    errs = torch.empty(B, nerr, dtype=f32, device=dev)
    ws = torch.empty(max(int(lib().conan_sinkhorn_ext_workspace_bytes(B, N1, N2)), 1), dtype=torch.uint8, device=dev)
    call("conan_sinkhorn_ext_fwd", ptr(M, f32), ptr(a), ptr(b), ptr(wu), ptr(wv), ptr(n1), ptr(n2), B, N1, N2, N1 * N2 if M.dim() == 3 else 0,
         float(reg), code, int(num_iter_max), float(stop_thr), float(tau), int(print_period), float(epsilon0), int(num_inner_iter_max),
         ptr(T), ptr(loss), ptr(log_u), ptr(log_v), ptr(alpha), ptr(beta), ptr(info), ptr(errs) if nerr else None, ptr(extra), ptr(ws), stream_ptr())
    return T, loss, log_u, log_v, alpha, beta, info, errs, extra


def _sinkhorn_ext_params(method, num_iter_max, print_period):
    if method not in SINKHORN_EXT_METHODS:
        raise ValueError("Unknown method '%s'." % method)
    it = _SINKHORN_EXT_ITERS[method] if num_iter_max is None else num_iter_max
    pp = (10 if method == "sinkhorn_epsilon_scaling" else 20) if print_period is None else print_period
    return it, pp


def sinkhorn_ext_batched(M: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, *, reg: float, method: str,
                         num_iter_max: Optional[int] = None, stop_thr: float = 1e-9, tau: float = 1e3, print_period: Optional[int] = None,
                         epsilon0: float = 1e4, num_inner_iter_max: int = 100, warmstart=None, n1: Optional[Tensor] = None,
                         n2: Optional[Tensor] = None):
    """B independent entropic OT problems in one launch by the reference's "greenkhorn" (sinkhorn.py:453-532), "sinkhorn_stabilized" (:535-685)
    or "sinkhorn_epsilon_scaling" (:688-786), with its defaults (num_iter_max 10000 / 1000 / 100, print_period 20 / 10).  M, a, b, n1, n2 as
    sinkhorn_batched; warmstart: (log u, log v) for greenkhorn, (alpha, beta) in cost units for the other two.
    -> T [B,N1,N2], loss [B] = sum(M * T), log_u [B,N1], log_v [B,N2] (greenkhorn: log u, log v; else the reference's logu, logv),
    alpha [B,N1], beta [B,N2] (fp64: the reference's log["alpha"], log["beta"]; zeros for greenkhorn; a warm start is read as fp64 too, since the
    potentials of epsilon scaling carry an offset of ~epsilon0 log n that fp32 resolves to 2e-3 only), info [B,4] int32 = {the reference's iteration
    index at exit, flags (bit 0: stopped on the threshold, bit 1: the NaN exit), checks executed, absorptions (epsilon scaling: inner solves that
    ran to their cap)}, errs [B,nerr] (the error list, NaN where not executed; greenkhorn: nerr = 0), extra [B,4] int32 = {sweeps / steps
    executed (epsilon scaling: over all inner solves), absorptions, inner NaN exits, inner iteration of the last one}.
    The control flow follows the reference's fp64 run.  No gradient and no host synchronisation."""
    it, pp = _sinkhorn_ext_params(method, num_iter_max, print_period)
    M, a, b, wu, wv, n1, n2, (B, N1, N2, code) = _sinkhorn_ext_prepare(M, a, b, warmstart, n1, n2, method)
    return _sinkhorn_ext_fwd(M, a, b, wu, wv, n1, n2, B, N1, N2, code, reg, it, stop_thr, tau, pp, epsilon0, num_inner_iter_max)


def sinkhorn_ext_list(Ms, as_=None, bs=None, *, warmstarts=None, container=None, **params):
    """sinkhorn_ext_batched for problems of different sizes in ONE launch (as sinkhorn_list; warm starts are stacked as fp32 here)
    -> ([T_k], loss [B], [log_u_k], [log_v_k], [alpha_k], [beta_k], info [B,4], errs, extra [B,4])."""
    M, a, b, warm, n1, n2, sizes = _sinkhorn_list_stack(Ms, as_, bs, warmstarts, container)
    T, loss, lu, lv, al, be, info, errs, extra = sinkhorn_ext_batched(M, a, b, warmstart=warm, n1=n1, n2=n2, **params)
    rows = lambda t: [t[k, :s[0]] for k, s in enumerate(sizes)]
    cols = lambda t: [t[k, :s[1]] for k, s in enumerate(sizes)]
    return [T[k, :s[0], :s[1]] for k, s in enumerate(sizes)], loss, rows(lu), cols(lv), rows(al), cols(be), info, errs, extra


class _SinkhornExtLossFn(torch.autograd.Function):
    """_SinkhornLossFn for the nine outputs of the ext solve: dM = gout * T at the returned plan, held constant."""
    @staticmethod
    def forward(ctx, M, run):
        T, loss, *rest = run()
        ctx.save_for_backward(T)
        ctx.shared = M.dim() == 2
        ctx.mark_non_differentiable(T, *rest)
        return (loss, T, *rest)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        (T,) = ctx.saved_tensors
        dM = g.to(f32)[:, None, None] * T
        return (dM.sum(0) if ctx.shared else dM), None


def sinkhorn_ext_loss(M: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, *, reg: float, method: str,
                      num_iter_max: Optional[int] = None, stop_thr: float = 1e-9, tau: float = 1e3, print_period: Optional[int] = None,
                      epsilon0: float = 1e4, num_inner_iter_max: int = 100, warmstart=None, n1: Optional[Tensor] = None,
                      n2: Optional[Tensor] = None, return_plan: bool = False):
    """The costs sum(M * T) of sinkhorn_ext_batched's solve (same arguments, same launch, same bits) as a loss [B] with the project's fixed-plan
    gradient dM = gout * T; a, b and the warm start get none; no double backward; no host synchronisation.  return_plan: (loss, T, log_u,
    log_v, alpha, beta, info, errs, extra), all but the first without gradient."""
    it, pp = _sinkhorn_ext_params(method, num_iter_max, print_period)
    Mp, a, b, wu, wv, n1, n2, (B, N1, N2, code) = _sinkhorn_ext_prepare(M, a, b, warmstart, n1, n2, method, keep_graph=True)
    out = _SinkhornExtLossFn.apply(Mp, lambda: _sinkhorn_ext_fwd(Mp.detach(), a, b, wu, wv, n1, n2, B, N1, N2, code, reg, it, stop_thr, tau, pp,
                                                                 epsilon0, num_inner_iter_max))
    return out if return_plan else out[0]


class _MseLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        pred, target = _c(pred), _c(target)
        if pred.shape != target.shape:
            raise RuntimeError(f"mse_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} must have the same shape")
        loss = torch.empty((), dtype=f32, device=pred.device)
        dpred = torch.empty_like(pred)
        call("conan_mse_loss_fwd", ptr(pred, f32), ptr(target, f32), pred.numel(), ptr(loss), ptr(dpred), stream_ptr())
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        if g.is_cuda and g.dtype == f32 and g.numel() == 1:        # the seed of loss.backward() (1, or 1 / world_size): one HIP launch, no aten kernel in the step
            out = torch.empty_like(dpred)
            call("conan_scale_scalar", ptr(dpred), ptr(_c(g)), dpred.numel(), ptr(out), stream_ptr())
            return out, None
        return dpred * g, None


def mse_loss(pred: Tensor, target: Tensor) -> Tensor:
    """mean((pred - target)^2) with its gradient formed in the same launch (the reference's nn.MSELoss criterion, common.py)."""
    return _MseLossFn.apply(pred, target)


class _BceLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight):
        pred, target = _c(pred), _c(target)
        if pred.shape != target.shape:
            raise RuntimeError(f"bce_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} must have the same shape")
        loss = torch.empty((), dtype=f32, device=pred.device)
        dpred = torch.empty_like(pred)
        call("conan_bce_loss_fwd", ptr(pred, f32), ptr(target, f32), ptr(weight, f32), 0 if weight is None else weight.numel(), pred.numel(),
             ptr(loss), ptr(dpred), stream_ptr())
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        if g.is_cuda and g.dtype == f32 and g.numel() == 1:        # the seed of loss.backward(): one HIP launch, as in _MseLossFn
            out = torch.empty_like(dpred)
            call("conan_scale_scalar", ptr(dpred), ptr(_c(g)), dpred.numel(), ptr(out), stream_ptr())
            return out, None, None
        return dpred * g, None, None


def bce_loss(pred: Tensor, target: Tensor, weight: Optional[Tensor] = None) -> Tensor:
    """torch.nn.functional.binary_cross_entropy(pred, target, weight) (mean reduction) with its gradient formed in the same launch: the criterion
    of the reference's classification models (`classification_loss`, common.py:210-217).  Same terms as torch's kernel and its backward: both
    logarithms clamped at -100, the gradient's denominator at 1e-12.  `weight`: None, one element (the reference's class weight,
    train_val.py:62) or one per prediction; it is moved to pred's device and dtype without a host synchronisation.  The gradient goes to `pred`
    only.  A prediction outside [0, 1] gives NaN where torch raises a device-side assert (which aborts the process).  No host synchronisation."""
    if weight is not None:
        if not isinstance(weight, Tensor) or weight.numel() not in (1, pred.numel()):
            raise ValueError(f"bce_loss: weight must be a tensor of 1 or {pred.numel()} elements"
                             + (f", got {weight.numel()}" if isinstance(weight, Tensor) else f", got {type(weight).__name__}"))
        weight = _c(weight.detach().to(device=pred.device, dtype=pred.dtype, non_blocking=True).reshape(-1))
    return _BceLossFn.apply(pred, target, weight)


class _ReadoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Y, K, mode):
        Y = _c(Y)
        B, N, d = Y.shape
        out = torch.empty(B * K, d, dtype=f32, device=Y.device)
        call("conan_fgw_readout_fwd", ptr(Y, f32), B, K, N, d, mode, ptr(out), stream_ptr())
        ctx.save_for_backward(Y)
        ctx.K, ctx.mode = K, mode
        return out

    @staticmethod
    def backward(ctx, dout):
        (Y,) = ctx.saved_tensors
        B, N, d = Y.shape
        dY = torch.empty_like(Y)
        call("conan_fgw_readout_bwd", ptr(Y), ptr(_c(dout)), B, ctx.K, N, d, ctx.mode, ptr(dY), stream_ptr())
        return dY, None, None


def fgw_readout(Y: Tensor, num_conformers: int, mode: int = 0) -> Tensor:
    """[B,N,d] -> [B*K,d]: sum over barycenter nodes, repeated K times (schnet_no_sum.py:308-312); mode 1 = ViSNet variant."""
    return _ReadoutFn.apply(Y, num_conformers, mode)
