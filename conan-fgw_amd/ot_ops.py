"""Host layer of the optimal-transport library: the FGW barycenter, the pairwise FGW and FGWMixup solves, their fixed-plan and unrolled
gradients, and the Sinkhorn family, as thin torch.autograd wrappers over the C-ABI (include/conan_fgw_hip*.h).

torch is used for device memory, streams, autograd bookkeeping and the embedding of ragged problems only; every solve and gradient is a HIP
kernel of libconan_fgw_hip.so.  Imports nothing from ops.py, which re-exports this module's names (`ops.fgw_pair_batched` is
`ot_ops.fgw_pair_batched`).  The plumbing every solver family shares is defined once, right below.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
from torch import Tensor

from ._lib import FgwParams, _c, call, f32, i32, lib, ptr, stream_ptr

__all__ = ["PROD_FGW", "FGW_SOLVERS", "SINKHORN_METHODS", "SINKHORN_EXT_METHODS",
           "fgw_barycenter_batched", "fgw_pair_batched", "fgw_pair_list", "fgw_acc_pair_batched", "fgw_mixup_barycenter_batched",
           "fgw_mixup_barycenter_unrolled", "fgw_pair_distance", "fgw_pair_distance_list", "fgw_pair_dist", "fgw_acc_pair_distance",
           "fgw_acc_pair_unrolled", "fgw_pair_unrolled", "fgw_pair_unrolled_list", "fgw_bregman_unrolled", "fgw_bregman_unrolled_list",
           "sinkhorn_batched", "sinkhorn_list", "sinkhorn_loss", "sinkhorn_hists_batched", "sinkhorn_hists_loss", "sinkhorn_unrolled", "sinkhorn_unrolled_list", "sinkhorn_ext_batched",
           "sinkhorn_ext_list", "sinkhorn_ext_loss"]


# ------------------------------------------------------------------------------------------------ plumbing shared by every solver family
def _operand(t, family, name, shapes, dtype=f32, keep_graph=False):
    """One operand of the `family` solve ("pairwise FGW", "FGWMixup", "Sinkhorn"), checked (on the GPU, one of `shapes`) -> contiguous `dtype`;
    detached unless keep_graph, which lets torch differentiate the conversion.  The only place that looks at the device."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise NotImplementedError(f"the {family} solve runs on the GPU only: {name} is a CPU tensor")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"{name} must have shape {' or '.join(str(list(sh)) for sh in shapes)}, not {list(t.shape)}")
    return _c((t if keep_graph else t.detach()).to(dtype))


def _pair_operands(family, names, dims, tensors, keep_graph, keep_start_graph):
    """The checked fp32 operands of a pair-form solve (cost, the two structures, the two weight vectors or None, a start plan or None; `names`
    and `dims` are the family's words for them in its messages) -> the six.  The start keeps its graph only with keep_start_graph."""
    M = tensors[0]
    if M.dim() != 3:
        raise ValueError(f"M must be [B,{dims}], not {list(M.shape)}")
    B, n1, n2 = M.shape
    shapes = ((B, n1, n2), (B, n1, n1), (B, n2, n2), (B, n1), (B, n2), (B, n1, n2))
    keep = (keep_graph,) * 5 + (keep_start_graph,)
    optional = (False,) * 3 + (True,) * 3           # the weights and the start may be None; the cost and the structures may not
    return [None if t is None and opt else _operand(t, family, name, [shape], keep_graph=kg)
            for t, name, shape, kg, opt in zip(tensors, names, shapes, keep, optional)]


def _embed(t, *shape):
    """t [B, ...] as the leading block of zeros [B, *shape] (None stays None): the massless nodes of an embedded problem."""
    if t is None:
        return None
    out = torch.zeros(t.shape[0], *shape, dtype=f32, device=t.device)
    out[(slice(None),) + tuple(slice(0, k) for k in t.shape[1:])] = t
    return out


def _crop(T, n1, n2):
    """The caller's [B,n1,n2] block of an embedded plan (the plan itself when it was not embedded)."""
    return T if n1 == n2 else T[:, :n1, :n2]


def _unstack(t, sizes, axes=(0, 1)):
    """The ragged problems' own blocks of a stacked result, as views: t[b, :sizes[b][ax] for ax in axes] (plans: both axes; rows: (0,); columns:
    (1,))."""
    return [t[(b,) + tuple(slice(0, s[ax]) for ax in axes)] for b, s in enumerate(sizes)]


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _check_loss_fun(loss_fun):
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")


# ------------------------------------------------------------------------------------------------ FGW barycenter
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


def _barycenter_outputs(B, K, N, d, max_iter, keep_iterates, dev):
    """The outputs of a barycenter forward -> Y [B,N,d], C [B,N,N], T [B,K,N,N], T_iter [max_iter,B,K,N,N] or None, info [B,4], errs [B,2,max_iter]."""
    new = lambda *shape, dtype=f32: torch.empty(*shape, dtype=dtype, device=dev)
    return (new(B, N, d), new(B, N, N), new(B, K, N, N), new(max_iter, B, K, N, N) if keep_iterates else None, new(B, 4, dtype=i32),
            new(B, 2, max_iter))


def _barycenter_return(ctx, Y, C, T, info, errs, T_iter, c_diff):
    """The return tail of a barycenter forward: only Y (and C with c_diff) is differentiable; T_iter is returned when there is one."""
    rest = (T, info, errs) if T_iter is None else (T, info, errs, T_iter)
    ctx.mark_non_differentiable(*(rest if c_diff else (C,) + rest))
    return (Y, C) + rest


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
        Y, C, T, T_iter, info, errs = _barycenter_outputs(B, K, N, d, prm.max_iter, params.get("keep_iterates"), dev)
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
        return _barycenter_return(ctx, Y, C, T, info, errs, T_iter, c_diff)

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
    _check_loss_fun(loss_fun)
    # conan_fgw_pair_fwd reads alpha, epsilon, max_iter, tol, num_iter_max, stop_thr and loss_fun; the other fields are ignored
    prm = _fgw_params(alpha, epsilon, max_iter, tol, tol, num_iter_max, stop_thr, True, True, False, loss_fun)
    return prm, FGW_SOLVERS[solver], _symmetric_code(None if symmetric is None else bool(symmetric))


def _pair_embed(M, C1, C2, p, q, G0):
    """Checked operands with n1 != n2 embedded in N = max(n1, n2): zero rows / columns, uniform weights formed over the own nodes first."""
    B, n1, n2 = M.shape
    dev, N = M.device, max(n1, n2)
    if n1 != n2:
        p = _embed(torch.full((B, n1), 1.0 / n1, dtype=f32, device=dev) if p is None else p, N)
        q = _embed(torch.full((B, n2), 1.0 / n2, dtype=f32, device=dev) if q is None else q, N)
        M, C1, C2, G0 = (_embed(t, N, N) for t in (M, C1, C2, G0))
    return M, C1, C2, p, q, G0, (B, N, n1, n2)


def _pair_prepare(M, C1, C2, p, q, G0, keep_graph=False, keep_start_graph=False):
    """The checked, contiguous fp32 operands of conan_fgw_pair_fwd, n1 != n2 embedded in N = max(n1, n2) with massless nodes -> (M, C1, C2, p, q, G0,
    (B, N, n1, n2)).  keep_graph: the inputs are not detached, so that torch differentiates the conversion and the embedding (G0 only with
    keep_start_graph: the unrolled gradient reaches the start)."""
    return _pair_embed(*_pair_operands("pairwise FGW", ("M", "C1", "C2", "p", "q", "G0"), "n1,n2", (M, C1, C2, p, q, G0), keep_graph,
                                       keep_start_graph))


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
    return _crop(T, n1, n2), dist, info, errs


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
    return _unstack(T, sizes), dist, info, errs


def _mixup_step(rho, epoch, eps):
    rho, epoch, eps = float(rho), int(epoch), float(eps)
    if not (rho > 0 and math.isfinite(rho)):
        raise ValueError(f"rho must be positive and finite, not {rho}")
    if epoch <= 0:
        raise ValueError(f"epoch must be positive, not {epoch}")
    return rho, epoch, eps


def _acc_embed(M, A, Bm, a, b, X0, n1, n2):
    """Checked operands with N1 != N2 and own sizes embedded in N = max(N1, N2): zero rows / columns, weights masked to the own nodes (uniform
    ones formed as mask / count)."""
    B, N1, N2 = M.shape
    dev, N = M.device, max(N1, N2)
    if N1 != N2 or n1 is not None or n2 is not None:
        def own(n, Nc):
            n = torch.full((B,), Nc, device=dev) if n is None else torch.as_tensor(n, device=dev).reshape(B)
            return (torch.arange(N, device=dev)[None, :] < n[:, None]).to(f32), n.to(f32)
        (m1, c1), (m2, c2) = own(n1, N1), own(n2, N2)
        a = m1 / c1[:, None] if a is None else _embed(a, N) * m1
        b = m2 / c2[:, None] if b is None else _embed(b, N) * m2
        M, A, Bm, X0 = (_embed(t, N, N) for t in (M, A, Bm, X0))
    return M, A, Bm, a, b, X0, (B, N, N1, N2)


def _acc_prepare(M, A, Bm, a, b, X0, n1, n2, keep_graph=False, keep_start_graph=False):
    """The checked, contiguous fp32 operands of conan_fgw_acc_pair_fwd, N1 != N2 and own sizes embedded in N = max(N1, N2) with massless nodes
    -> (M, A, Bm, a, b, X0, (B, N, N1, N2)).  keep_graph: the inputs are not detached, so that torch differentiates the conversion and the
    embedding (X0 only with keep_start_graph: the unrolled gradient reaches the start, the fixed-plan one does not)."""
    return _acc_embed(*_pair_operands("FGWMixup", ("M", "A", "Bm", "a", "b", "X0"), "N1,N2", (M, A, Bm, a, b, X0), keep_graph, keep_start_graph),
                      n1, n2)


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
    return _crop(X, N1, N2), objs, info


def _mixup_barycenter_fwd(Ys, Cs, ps, p, lambdas, init_C, init_Y, prm, rho, epoch, eps, keep_iterates):
    """conan_fgw_mixup_barycenter_fwd on prepared operands -> Y, C, T, info, errs, T_iter (or None)."""
    B, K, N, d = Ys.shape
    dev = Ys.device
    Y, C, T, T_iter, info, errs = _barycenter_outputs(B, K, N, d, prm.max_iter, keep_iterates, dev)
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
        return _barycenter_return(ctx, Y, C, T, info, errs, T_iter, c_diff)

    @staticmethod
    def backward(ctx, dY, dC=None, *_):
        return _barycenter_backward(ctx, dY, dC)


def _mixup_barycenter(fn, ps_grad, Ys, Cs, ps, p, lambdas, init_C, init_Y, alpha, rho, max_iter, tol, epoch, eps, fixed_structure, fixed_features,
                      loss_fun, keep_iterates):
    """The body of fgw_mixup_barycenter_batched and fgw_mixup_barycenter_unrolled: refusals, checked operands, then the Function `fn` when an
    input requires grad (ps counts, and keeps its graph, only with ps_grad) and the plain forward launch otherwise."""
    _check_loss_fun(loss_fun)
    rho, epoch, eps = _mixup_step(rho, epoch, eps)
    if Ys.dim() != 4:
        raise ValueError(f"Ys must be [B,K,N,d], not {list(Ys.shape)}")
    B, K, N, d = Ys.shape
    kg = _wants_grad(Ys, Cs, ps if ps_grad else None, p, lambdas, init_C, init_Y)
    opt = lambda t, name, *shape, keep=kg: None if t is None else _operand(t, "FGWMixup", name, [shape], keep_graph=keep)
    Ys, Cs = opt(Ys, "Ys", B, K, N, d), opt(Cs, "Cs", B, K, N, N)
    ps, p, lambdas = opt(ps, "ps", B, K, N, keep=kg and ps_grad), opt(p, "p", B, N), opt(lambdas, "lambdas", K)
    init_C, init_Y = opt(init_C, "init_C", B, N, N), opt(init_Y, "init_Y", B, N, d)
    if fixed_features and init_Y is None:
        raise ValueError("If Y is fixed it must be initialized")
    prm = _fgw_params(alpha, 0.0, max_iter, tol, 0.0, 1, 0.0, fixed_structure, fixed_features, False, loss_fun)
    if kg:
        return fn.apply(Ys, Cs, ps, p, lambdas, init_C, init_Y, (prm, rho, epoch, eps, bool(keep_iterates)))
    res = _mixup_barycenter_fwd(Ys, Cs, ps, p, lambdas, init_C, init_Y, prm, rho, epoch, eps, keep_iterates)
    return res[:5] if res[5] is None else res


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
    return _mixup_barycenter(_FgwMixupBarycenterFn, False, Ys, Cs, ps, p, lambdas, init_C, init_Y, alpha, rho, max_iter, tol, epoch, eps,
                             fixed_structure, fixed_features, loss_fun, keep_iterates)


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
        Y, C, T, T_iter, info, errs = _barycenter_outputs(B, K, N, d, prm.max_iter, keep_iterates, dev)
        record = torch.empty((prm.max_iter + 1) * B * (N * N + N * d), dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib().conan_fgw_mixup_workspace_bytes(B, K, N, d)), dtype=torch.uint8, device=dev)
        call("conan_fgw_mixup_barycenter_fwd_record", ptr(Ys, f32), ptr(Cs, f32), ptr(ps), ptr(p), ptr(lambdas), ptr(init_C), ptr(init_Y), B, K, N, d,
             ctypes.byref(prm), rho, epoch, eps, ptr(Y), ptr(C), ptr(T), ptr(T_iter), ptr(info), ptr(errs), ptr(record), ptr(ws), stream_ptr())
        ctx.save_for_backward(Ys, Cs, ps, p, lambdas, init_Y, info, record)
        ctx.dims, ctx.params, ctx.has_init_C = (B, K, N, d), (prm, rho, epoch, eps), init_C is not None
        ctx.set_materialize_grads(False)
        return _barycenter_return(ctx, Y, C, T, info, errs, T_iter, True)

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
    return _mixup_barycenter(_FgwMixupUnrolledFn, True, Ys, Cs, ps, p, lambdas, init_C, init_Y, alpha, rho, max_iter, tol, epoch, eps,
                             fixed_structure, fixed_features, loss_fun, keep_iterates)


def _pair_dist(M, C1, C2, p, q, T, B, N, alpha, loss_code):
    """conan_fgw_pair_dist on prepared operands: the FGW distance of the plans T -> dist [B].  With C2 = Bm^T and the square loss it is the
    FGWMixup distance (fgw_acc_pair_distance)."""
    dist = torch.empty(B, dtype=f32, device=M.device)
    call("conan_fgw_pair_dist", ptr(M, f32), ptr(C1, f32), ptr(C2, f32), ptr(p), ptr(q), ptr(T, f32), B, N, float(alpha), loss_code, ptr(dist),
         stream_ptr())
    return dist


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
    return (dist, _crop(T, n1, n2), info, errs) if return_plan else dist


def fgw_pair_distance_list(Ms, C1s, C2s, ps=None, qs=None, G0s=None, *, return_plan: bool = False, **params):
    """fgw_pair_distance for pairs of different sizes (the lists of fgw_pair_list, one launch) -> dist [B]; with return_plan
    (dist, [T_b [n1_b,n2_b]], info, errs)."""
    M, C1, C2, p, q, G0, sizes = _pair_list_stack(Ms, C1s, C2s, ps, qs, G0s, keep_graph=True)
    dist, T, info, errs = fgw_pair_distance(M, C1, C2, p, q, G0, return_plan=True, **params)
    return (dist, _unstack(T, sizes), info, errs) if return_plan else dist


def fgw_pair_dist(M: Tensor, C1: Tensor, C2: Tensor, T: Tensor, p: Optional[Tensor] = None, q: Optional[Tensor] = None, *, alpha: float = 0.5,
                  loss_fun: str = "square_loss") -> Tensor:
    """The reference's log["fgw_dist"] of the plans T [B,N,N] (conan_fgw_pair_dist; square problems: embed rectangular ones as fgw_pair_batched
    does): (1 - alpha) sum(M * T) + alpha * gwloss(init_matrix(C1, C2, p, q, loss_fun), T), bregman.py:163-164 -> [B].  When one of M, C1, C2, p, q
    requires grad the result carries the gradient at the given plan to them (conan_fgw_pair_dist_bwd; T gets none); the value is the same."""
    _check_loss_fun(loss_fun)
    B, N, _ = M.shape
    kg = _wants_grad(M, C1, C2, p, q)
    M, C1, C2 = (_operand(t, "pairwise FGW", n, [(B, N, N)], keep_graph=kg) for t, n in ((M, "M"), (C1, "C1"), (C2, "C2")))
    T = _operand(T, "pairwise FGW", "T", [(B, N, N)])
    p, q = (None if t is None else _operand(t, "pairwise FGW", n, [(B, N)], keep_graph=kg) for t, n in ((p, "p"), (q, "q")))
    run = lambda: (_pair_dist(M, C1, C2, p, q, T, B, N, alpha, _LOSS_CODE[loss_fun]), T, None, None)
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
        return _pair_dist(M, A, Bt, a, b, X, B, N, alpha, _LOSS_CODE["square_loss"]), X, info, objs

    dist, X, info, objs = _FgwPairDistFn.apply(M, A, Bt, a, b, run, alpha, _LOSS_CODE["square_loss"])
    return (dist, _crop(X, N1, N2), objs, info) if return_plan else dist


# ------------------------------------------------------------------- the reference's gradient through the unrolled epochs (fgw_acc_grad.hip)
def _acc_fwd_dist(M, A, Bm, a, b, X0, B, N, alpha, rho, epoch, eps):
    """fgw_acc_pair_batched's launch, then fgw_acc_pair_distance's value at its plan (conan_fgw_pair_dist with C2 = Bm^T) -> X, dist, objs, info."""
    X, objs, info = _acc_fwd(M, A, Bm, a, b, X0, B, N, alpha, rho, epoch, eps)
    return X, _pair_dist(M, A, _c(Bm.transpose(1, 2)), a, b, X, B, N, alpha, _LOSS_CODE["square_loss"]), objs, info


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


def _pair_unrolled(prepare, operands, fn, fn_args, forward):
    """The three pair-form unrolled entry points: `prepare` the six operands (attached to autograd when one requires grad), then `fn`.apply(six,
    (B, N), *fn_args) or, with nothing to differentiate, the plain `forward`(six, B, N); the plan is cropped to the caller's shape."""
    kg = _wants_grad(*operands)
    *six, (B, N, n1, n2) = prepare(*operands, keep_graph=kg, keep_start_graph=kg)
    T, dist, r2, r3 = fn.apply(*six, (B, N), *fn_args) if kg else forward(*six, B, N)
    return _crop(T, n1, n2), dist, r2, r3


def _pair_unrolled_list(solve, lists, params):
    """The list forms of fgw_pair_unrolled and fgw_bregman_unrolled: the ragged pairs stacked (attached to autograd when an entry requires
    grad), ONE `solve`, the plans unstacked."""
    kg = _wants_grad(*(t for ts in lists if ts is not None for t in ts))
    *six, sizes = _pair_list_stack(*lists, keep_graph=kg, keep_start_graph=kg)
    T, dist, info, errs = solve(*six, **params)
    return _unstack(T, sizes), dist, info, errs


class _FgwAccUnrolledFn(torch.autograd.Function):
    """fgw_acc_pair_batched's launch and fgw_acc_pair_distance's distance with conan_fgw_acc_pair_bwd as their backward: the gradient through the
    executed epochs, as the reference's autograd delivers it, from the cotangents of X and dist to M, A, Bm, a, b and X0.  The backward is ONE
    launch that replays the epochs from the saved inputs (nothing but the inputs and info is kept from the forward).  No double backward, no
    host synchronisation."""
    @staticmethod
    def forward(ctx, M, A, Bm, a, b, X0, dims, alpha, rho, epoch, eps):
        B, N = dims
        X, dist, objs, info = _acc_fwd_dist(M, A, Bm, a, b, X0, B, N, alpha, rho, epoch, eps)
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
    return _pair_unrolled(lambda *ts, **keep: _acc_prepare(*ts, n1, n2, **keep), (M, A, Bm, a, b, X0), _FgwAccUnrolledFn, (alpha, rho, epoch, eps),
                          lambda *ts: _acc_fwd_dist(*ts, alpha, rho, epoch, eps))


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
    return _pair_unrolled(_pair_prepare, (M, C1, C2, p, q, G0), _FgwPairUnrolledFn,
                          (prm, solver_code, sym_code, (float(alpha), float(epsilon), float(stop_thr))),
                          lambda *ts: _pair_fwd(*ts, prm, solver_code, sym_code, True))


def fgw_pair_unrolled_list(Ms, C1s, C2s, ps=None, qs=None, G0s=None, **params):
    """fgw_pair_unrolled for pairs of different sizes (the lists of fgw_pair_list, one forward and one backward launch) ->
    ([T_b [n1_b,n2_b]], fgw_dist [B], info, errs); the gradients reach the list entries in their own shapes, and a pair's bits do not depend on
    the batch it is part of."""
    _pair_unrolled_params(0.5, 0.1, 1, 1e-5, 1, 1e-5, params.get("loss_fun", "square_loss"), params.get("solver", "PGD"), None)      # the refusals first
    return _pair_unrolled_list(fgw_pair_unrolled, (Ms, C1s, C2s, ps, qs, G0s), params)


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
    return _pair_unrolled(_pair_prepare, (M, C1, C2, p, q, G0), _FgwBregmanUnrolledFn, (prm, sym_code, (float(alpha), float(epsilon))),
                          lambda *ts: _pair_fwd(*ts, prm, FGW_SOLVERS["BAPG"], sym_code, True))


def fgw_bregman_unrolled_list(Ms, C1s, C2s, ps=None, qs=None, G0s=None, **params):
    """fgw_bregman_unrolled for pairs of different sizes (the lists of fgw_pair_list, one forward and one backward launch) ->
    ([T_b [n1_b,n2_b]], fgw_dist [B], info, errs); the gradients reach the list entries in their own shapes, and a pair's bits do not depend on
    the batch it is part of."""
    return _pair_unrolled_list(fgw_bregman_unrolled, (Ms, C1s, C2s, ps, qs, G0s), params)


# ------------------------------------------------------------------------------------------------ entropic OT on its own (sinkhorn.hip)
SINKHORN_METHODS = {"sinkhorn_log": 0, "sinkhorn": 1}


def _sinkhorn_vec(t, name, B, n, dtype=f32, keep_graph=False):
    """A per-problem vector of the Sinkhorn solve: [B,n] or, for B = 1, [n]."""
    return _operand(t, "Sinkhorn", name, [(B, n)] + ([(n,)] if B == 1 else []), dtype, keep_graph)


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
    M = _operand(M, "Sinkhorn", "M", [(B, N1, N2), (N1, N2)], keep_graph=keep_graph)
    vec = lambda t, name, n, keep=False: None if t is None else _sinkhorn_vec(t, name, B, n, keep_graph=keep)
    a, b = vec(a, "a", N1, keep_vec_graph), vec(b, "b", N2, keep_vec_graph)
    wu, wv = (None, None) if warmstart is None else (vec(warmstart[0], "warmstart[0]", N1, keep_vec_graph), vec(warmstart[1], "warmstart[1]", N2))
    n1 = None if n1 is None else _operand(n1, "Sinkhorn", "n1", [(B,)], i32)
    n2 = None if n2 is None else _operand(n2, "Sinkhorn", "n2", [(B,)], i32)
    return M, a, b, wu, wv, n1, n2, (B, N1, N2, SINKHORN_METHODS[method])


def _sinkhorn_outputs(B, N1, N2, dev):
    """The outputs both Sinkhorn forwards share -> T [B,N1,N2], loss [B], log_u [B,N1], log_v [B,N2], info [B,4]."""
    new = lambda *shape, dtype=f32: torch.empty(*shape, dtype=dtype, device=dev)
    return new(B, N1, N2), new(B), new(B, N1), new(B, N2), new(B, 4, dtype=i32)


def _sinkhorn_fwd(M, a, b, wu, wv, n1, n2, B, N1, N2, code, reg, num_iter_max, stop_thr):
    """conan_sinkhorn_fwd on prepared operands -> T [B,N1,N2], loss [B], log_u [B,N1], log_v [B,N2], info [B,4], errs.  No host synchronisation."""
    dev = M.device
    T, loss, log_u, log_v, info = _sinkhorn_outputs(B, N1, N2, dev)
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
    return _unstack(T, sizes), loss, _unstack(lu, sizes, (0,)), _unstack(lv, sizes, (1,)), info, errs


class _SinkhornLossFn(torch.autograd.Function):
    """loss[B] = sum(M * T) of the solved plans as a differentiable value under the project's fixed-plan convention (fgw_pair_distance's): the
    plan is a constant of the backward, dM = gout * T (a torch multiply on the saved plan), nothing flows to a, b or the warm start.  `run()`
    is sinkhorn_batched's forward (six outputs) or sinkhorn_ext_batched's (nine): (T, loss, *rest) -> (loss, T, *rest).  No double backward."""
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


# --------------------------------------------------------------------------- several histograms at once: a 2-D b (sinkhorn_hists.hip)
def _sinkhorn_hists_prepare(M, a, b, warmstart, n1, n2, nh, keep_graph=False):
    """The checked, contiguous operands of conan_sinkhorn_hists_fwd -> (M, a, b, wu, wv, n1, n2, nh, (B, N1, N2, H)).  M [B,N1,N2], or [N1,N2]
    shared by the B problems of b (m_batch_stride = 0); b [B,N2,H]."""
    if not torch.is_tensor(M) or not M.is_cuda:
        raise NotImplementedError("the Sinkhorn solve runs on the GPU only: M is a CPU tensor")
    if M.dim() not in (2, 3):
        raise ValueError(f"M must be [B,N1,N2] or [N1,N2], not {list(M.shape)}")
    if not torch.is_tensor(b) or b.dim() != 3:
        raise ValueError("b must be [B,N2,H]" + (f", not {list(b.shape)}" if torch.is_tensor(b) else ""))
    N1, N2 = int(M.shape[-2]), int(M.shape[-1])
    B, H = int(b.shape[0]), int(b.shape[2])
    M = _operand(M, "Sinkhorn", "M", [(B, N1, N2), (N1, N2)], keep_graph=keep_graph)
    b = _operand(b, "Sinkhorn", "b", [(B, N2, H)])
    a = None if a is None else _sinkhorn_vec(a, "a", B, N1)
    wu, wv = (None, None) if warmstart is None else (_operand(warmstart[0], "Sinkhorn", "warmstart[0]", [(B, N1, H)]),
                                                     _operand(warmstart[1], "Sinkhorn", "warmstart[1]", [(B, N2, H)]))
    size = lambda t, name: None if t is None else _operand(t, "Sinkhorn", name, [(B,)], i32)
    return M, a, b, wu, wv, size(n1, "n1"), size(n2, "n2"), size(nh, "nh"), (B, N1, N2, H)


def _sinkhorn_hists_fwd(M, a, b, wu, wv, n1, n2, nh, B, N1, N2, H, reg, num_iter_max, stop_thr):
    """conan_sinkhorn_hists_fwd on prepared operands -> loss [B,H], log_u [B,N1,H], log_v [B,N2,H], info [B,4], errs.  No host synchronisation."""
    dev = M.device
    new = lambda *shape, dtype=f32: torch.empty(*shape, dtype=dtype, device=dev)
    loss, log_u, log_v, info = new(B, H), new(B, N1, H), new(B, N2, H), new(B, 4, dtype=i32)
    errs = new(B, (int(num_iter_max) + 9) // 10)
    ws = torch.empty(max(int(lib().conan_sinkhorn_hists_workspace_bytes(B, N1, N2, H)), 1), dtype=torch.uint8, device=dev)
    call("conan_sinkhorn_hists_fwd", ptr(M, f32), ptr(a), ptr(b), ptr(wu), ptr(wv), ptr(n1), ptr(n2), ptr(nh), B, N1, N2, H,
         N1 * N2 if M.dim() == 3 else 0, float(reg), int(num_iter_max), float(stop_thr), ptr(loss), ptr(log_u), ptr(log_v), ptr(info), ptr(errs),
         ptr(ws), stream_ptr())
    return loss, log_u, log_v, info, errs


def sinkhorn_hists_batched(M: Tensor, a: Optional[Tensor], b: Tensor, *, reg: float, num_iter_max: int = 1000, stop_thr: float = 1e-9,
                           warmstart=None, n1: Optional[Tensor] = None, n2: Optional[Tensor] = None, nh: Optional[Tensor] = None):
    """B one-to-many entropic OT problems in one launch (one workgroup per problem): the reference's sinkhorn_knopp with a 2-D b
    (sinkhorn.py:207-315): per problem one cost matrix, one source histogram and H target histograms, solved JOINTLY: one Frobenius error over
    all H columns decides the stop, and a numerical error in any column restores the previous u, v of all.  M [B,N1,N2] costs, or [N1,N2] shared
    by the whole batch; a [B,N1] or None (uniform over the problem's own rows); b [B,N2,H]; warmstart (log_u [B,N1,H], log_v [B,N2,H]) or None;
    n1 / n2 / nh [B] int32 device tensors: the problems' own sizes inside the containers, or None.
    -> loss [B,H] (the H transport costs; no plan is formed), log_u [B,N1,H], log_v [B,N2,H], info [B,4] int32 = {niter, flags (bit 0: stopped on
    err < stop_thr, bit 1: the numerical-errors exit), checks executed, 0}, errs [B, ceil(num_iter_max / 10)] (NaN where not executed).  Outside a
    problem's own block every output is zero; a problem's bits do not depend on the batch, its position or the container.  (N1, N2, H) whose
    scaling matrices do not fit the LDS (H > conan_sinkhorn_hists_max_hists(N1, N2)) is refused.  No gradient (sinkhorn_hists_loss is the
    differentiable form) and no host synchronisation."""
    M, a, b, wu, wv, n1, n2, nh, (B, N1, N2, H) = _sinkhorn_hists_prepare(M, a, b, warmstart, n1, n2, nh)
    return _sinkhorn_hists_fwd(M, a, b, wu, wv, n1, n2, nh, B, N1, N2, H, reg, num_iter_max, stop_thr)


class _SinkhornHistsLossFn(torch.autograd.Function):
    """loss [B,H] of sinkhorn_hists_batched as a differentiable value under the fixed-plan convention: u, v are constants of the backward,
    dM = K o sum_k g_k u_k v_k^T from conan_sinkhorn_hists_loss_bwd (K recomputed, no [H,N1,N2] tensor); an M shared by the batch gets the sum
    over the problems.  `run()` is _sinkhorn_hists_fwd.  No double backward."""
    @staticmethod
    def forward(ctx, M, run, sizes, reg):
        loss, log_u, log_v, info, errs = run()
        ctx.save_for_backward(M, log_u, log_v, *(t for t in sizes if t is not None))
        ctx.have, ctx.reg = [t is not None for t in sizes], reg
        ctx.mark_non_differentiable(log_u, log_v, info, errs)
        return loss, log_u, log_v, info, errs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        M, log_u, log_v, *rest = ctx.saved_tensors
        rest = iter(rest)
        n1, n2, nh = (next(rest) if h else None for h in ctx.have)
        B, N1, H = log_u.shape
        N2 = log_v.shape[1]
        dM = torch.empty(B, N1, N2, dtype=f32, device=M.device)
        call("conan_sinkhorn_hists_loss_bwd", ptr(M, f32), ptr(log_u), ptr(log_v), ptr(_c(g.to(f32))), ptr(n1), ptr(n2), ptr(nh), B, N1, N2, H,
             N1 * N2 if M.dim() == 3 else 0, ctx.reg, ptr(dM), stream_ptr())
        return (dM.sum(0) if M.dim() == 2 else dM), None, None, None


def sinkhorn_hists_loss(M: Tensor, a: Optional[Tensor], b: Tensor, *, reg: float, num_iter_max: int = 1000, stop_thr: float = 1e-9,
                        warmstart=None, n1: Optional[Tensor] = None, n2: Optional[Tensor] = None, nh: Optional[Tensor] = None,
                        return_log: bool = False):
    """The costs of sinkhorn_hists_batched as a loss: the same arguments, the same launch, the same bits -> loss [B,H], which carries the gradient
    at the RETURNED u, v, held constant, to M: dM = K o sum_k g_k u_k v_k^T (one backward launch; an M shared by the batch gets the sum over the
    problems); a, b and the warm start get none.  No double backward; no host synchronisation.  return_log: (loss, log_u, log_v, info, errs)."""
    Mp, a, b, wu, wv, n1, n2, nh, (B, N1, N2, H) = _sinkhorn_hists_prepare(M, a, b, warmstart, n1, n2, nh, keep_graph=True)
    out = _SinkhornHistsLossFn.apply(Mp, lambda: _sinkhorn_hists_fwd(Mp.detach(), a, b, wu, wv, n1, n2, nh, B, N1, N2, H, reg, num_iter_max, stop_thr),
                                     (n1, n2, nh), float(reg))
    return out if return_log else out[0]


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
    return _unstack(T, sizes), loss, _unstack(lu, sizes, (0,)), _unstack(lv, sizes, (1,)), info, errs


# ------------------------------------------------------------------------- the reference's other three Sinkhorn solvers (sinkhorn_ext.hip)
SINKHORN_EXT_METHODS = {"greenkhorn": 2, "sinkhorn_stabilized": 3, "sinkhorn_epsilon_scaling": 4}
_SINKHORN_EXT_ITERS = {"greenkhorn": 10000, "sinkhorn_stabilized": 1000, "sinkhorn_epsilon_scaling": 100}      # the reference's numItermax defaults


def _sinkhorn_ext_prepare(M, a, b, warmstart, n1, n2, method, keep_graph=False):
    """_sinkhorn_prepare for a method _sinkhorn_ext_params has accepted; the potentials of the warm start travel as fp64 (see conan_sinkhorn_ext_fwd)."""
    M, a, b, _wu, _wv, n1, n2, (B, N1, N2, _) = _sinkhorn_prepare(M, a, b, None, n1, n2, "sinkhorn", keep_graph=keep_graph)
    wu, wv = (None, None) if warmstart is None else (_sinkhorn_vec(warmstart[0], "warmstart[0]", B, N1, torch.float64),
                                                     _sinkhorn_vec(warmstart[1], "warmstart[1]", B, N2, torch.float64))
    return M, a, b, wu, wv, n1, n2, (B, N1, N2, SINKHORN_EXT_METHODS[method])


def _sinkhorn_ext_fwd(M, a, b, wu, wv, n1, n2, B, N1, N2, code, reg, num_iter_max, stop_thr, tau, print_period, epsilon0, num_inner_iter_max):
    """conan_sinkhorn_ext_fwd on prepared operands.  No host synchronisation."""
    dev = M.device
    nerr = int(lib().conan_sinkhorn_ext_nerr(code, int(num_iter_max), int(print_period)))
    if nerr < 0:
        raise ValueError("num_iter_max and print_period must be positive")
    T, loss, log_u, log_v, info = _sinkhorn_outputs(B, N1, N2, dev)
    alpha, beta = torch.empty(B, N1, dtype=torch.float64, device=dev), torch.empty(B, N2, dtype=torch.float64, device=dev)
    extra, errs = torch.empty(B, 4, dtype=i32, device=dev), torch.empty(B, nerr, dtype=f32, device=dev)
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
    rows, cols = (lambda t: _unstack(t, sizes, (0,))), (lambda t: _unstack(t, sizes, (1,)))
    return _unstack(T, sizes), loss, rows(lu), cols(lv), rows(al), cols(be), info, errs, extra


def sinkhorn_ext_loss(M: Tensor, a: Optional[Tensor] = None, b: Optional[Tensor] = None, *, reg: float, method: str,
                      num_iter_max: Optional[int] = None, stop_thr: float = 1e-9, tau: float = 1e3, print_period: Optional[int] = None,
                      epsilon0: float = 1e4, num_inner_iter_max: int = 100, warmstart=None, n1: Optional[Tensor] = None,
                      n2: Optional[Tensor] = None, return_plan: bool = False):
    """The costs sum(M * T) of sinkhorn_ext_batched's solve (same arguments, same launch, same bits) as a loss [B] with the project's fixed-plan
    gradient dM = gout * T; a, b and the warm start get none; no double backward; no host synchronisation.  return_plan: (loss, T, log_u,
    log_v, alpha, beta, info, errs, extra), all but the first without gradient."""
    it, pp = _sinkhorn_ext_params(method, num_iter_max, print_period)
    Mp, a, b, wu, wv, n1, n2, (B, N1, N2, code) = _sinkhorn_ext_prepare(M, a, b, warmstart, n1, n2, method, keep_graph=True)
    out = _SinkhornLossFn.apply(Mp, lambda: _sinkhorn_ext_fwd(Mp.detach(), a, b, wu, wv, n1, n2, B, N1, N2, code, reg, it, stop_thr, tau, pp,
                                                              epsilon0, num_inner_iter_max))
    return out if return_plan else out[0]
