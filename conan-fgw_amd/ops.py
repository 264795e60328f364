"""Operators of the ConAN hot path on MI355X: thin torch.autograd wrappers over the C-ABI (include/conan_fgw_hip.h).

torch is used for device memory, streams and autograd bookkeeping only; every computation below is a HIP kernel of
libconan_fgw_hip.so.  All ops require CUDA(ROCm) tensors and raise otherwise.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import wgrad
from ._lib import _c, call, f32, i32, i64, lib, ptr, stream_ptr


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


# ------------------------------------------------------------------------------------------------ optimal transport (ot_ops.py)
# The FGW, FGWMixup and Sinkhorn solvers' host layer lives in ot_ops.py.  Its public names, and the private ones that tests, tools and the golden
# generators reach, stay reachable here: `ops.<name>` is `ot_ops.<name>`.
from .ot_ops import *                                                                                        # noqa: E402,F401,F403
from .ot_ops import (_LOSS_CODE, _acc_fwd, _acc_prepare, _pair_fwd, _pair_list_stack, _pair_params, _pair_prepare,      # noqa: E402,F401
                     _pair_unrolled_params, _sinkhorn_list_stack)
