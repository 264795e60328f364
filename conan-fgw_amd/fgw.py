"""Functional boundary of the FGW solver, mirroring the reference's signature
(conan_fgw/src/model/fgw/barycenter.py:7-31 `fgw_barycenters`, :393-399 `normalize_tensor`; bregman.py:8-279 `fgw`, `fgw_projected`,
`fgw_bregman` — the coupling solve between two attributed graphs on its own, with `fgw_distance`, its differentiable distance, and
`fgw_pairwise_distances` over an ensemble on top; barycenter.py:228-390 `fused_ACC_torch`, `fgw_barycenters_BAPG` — FGWMixup's accelerated
mirror descent and the barycenter around it, with `fgw_mixup_distance`, the differentiable distance of that solve; the barycenter and the
distance carry gradients at the solved couplings, held constant: see their docstrings for this and the other deviations;
`fused_ACC_unrolled` and `fgw_mixup_distance_unrolled` are the pair solve and its distance with the reference's own gradient, the one torch
autograd forms through every epoch of fused_ACC_torch; `fgw_unrolled`, `fgw_distance_unrolled` and `fgw_pairwise_distances_unrolled` are
`fgw`, `fgw_distance` and `fgw_pairwise_distances` with the reference's own gradient too, the one torch autograd forms through every PGD / PPA
iteration and Sinkhorn sweep of its fgw; `fgw_bregman_unrolled` and `fgw_bregman_distance_unrolled` are `fgw_bregman` and its distance with
the gradient torch autograd forms through every Bregman half-step of the reference's fgw_bregman, for both losses; `fgw_barycenters_BAPG_unrolled` is `fgw_barycenters_BAPG` with the gradient torch autograd forms
through the reference's, i.e. through every epoch of every coupling solve of every outer iteration).

Same argument names, defaults and error behaviour (`ValueError` for unknown `loss_fun` / `stop_criterion` / `solver`,
barycenter.py:33-44).  `loss_fun` = "square_loss" (every model) or "kl_loss" (utils.py:20-32,76-87).  All three coupling solvers of the
reference (bregman.py:8-67): `solver="PGD"` (every model), `"PPA"` (PGD with the proximal term -epsilon log(T), bregman.py:127-128) and
`"BAPG"` (Bregman projections, fgw_bregman, bregman.py:170-279; the Sinkhorn keywords numItermax / stopThr / method are ignored, as in the
reference).  BAPG's multiplicative iteration underflows where the reference's does (small epsilon, wide features): a zero row or column sum
of an iterate gives NaN outputs, as the reference's, and the reference's warning.  `symmetric` as in the reference (bregman.py:98-128,
:199-222), for all three solvers and both losses: True (every model), False (directed graphs, asymmetric structure or cost matrices: the
gradient averages the problem and its transpose) or None (decided in every coupling solve by torch.allclose(C, C^T, atol=1e-10) on the
current barycenter structure and the input graph).  `stop_criterion="loss"` exists in the reference but is broken there and
raises `NotImplementedError`.  Input graphs of any size (n_s != N, ragged lists) are solved by embedding them in a square problem with
massless nodes (below).  Differentiable like the reference, whose couplings are solved under torch.no_grad() (barycenter.py:120): Y and
C carry gradients to Ys, Cs, p and lambdas (to init_Y / init_C instead under fixed_features / fixed_structure); ps gets none.  Runs on
the GPU only (PPA / BAPG, or symmetric other than True, with CPU tensors: `NotImplementedError`).
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Sequence, Union

import torch
from torch import Tensor

from . import ops, ot_ops


def _embed_graphs(N, Ys_l, Cs_l, ps, p, sizes, d, dev):
    """The massless embedding of fgw_barycenters and fgw_barycenters_BAPG (see the comment in fgw_barycenters) -> (embedded, Np, Ys_l, Cs_l, ps,
    p_embedded): with input graphs of other sizes everything is padded to Np = max(N, max n_s) nodes and the weights, given or uniform, carry
    zeros for the extra nodes; otherwise the arguments come back as they are (p_embedded None)."""
    Np = max([N] + sizes)
    embedded = Np != N or any(n != N for n in sizes)
    if not embedded:
        return False, Np, Ys_l, Cs_l, ps, None

    def pad(t, *shape):
        out = torch.zeros(*shape, dtype=torch.float32, device=dev)
        out[tuple(slice(0, k) for k in t.shape)] = t
        return out
    ps_l = [torch.ones(n, device=dev) / n for n in sizes] if ps is None else [q.to(torch.float32).to(dev) for q in (ps.unbind(0) if torch.is_tensor(ps) else ps)]
    p_full = (torch.ones(N, device=dev) / N) if p is None else p.to(torch.float32).to(dev)
    return True, Np, [pad(y, Np, d) for y in Ys_l], [pad(c, Np, Np) for c in Cs_l], [pad(q, Np) for q in ps_l], pad(p_full, Np)


def _seeded_init_C(N, seed, device):
    """barycenter.py:61-65 / :303-306: torch.manual_seed(seed); xalea = torch.randn(N, 2); C = dist(xalea, xalea) — a host-side random
    squared-distance matrix (utils.py:154-171 with X is Y: clamped at 0, zero diagonal).  Reproduced draw for draw, including the
    reference's re-seeding of the global generator; N x 2 numbers of initialisation, not the solver."""
    torch.manual_seed(seed)
    xalea = torch.randn(N, 2)
    a2 = torch.einsum("ij,ij->i", xalea, xalea)
    c0 = -2 * (xalea @ xalea.T)
    c0 += a2[:, None]
    c0 += a2[None, :]
    return (torch.clamp(c0, min=0) * (1 - torch.eye(N))).to(device)


def _embed_init(init_C, init_Y, N, Np, d, dev):
    """init_C [N,N] / init_Y [N,d] (or None) inside the embedded problem's Np nodes: the extra rows and columns are zero."""
    ic = torch.zeros(Np, Np, dtype=torch.float32, device=dev); ic[:N, :N] = init_C.to(torch.float32)
    if init_Y is not None:
        iy = torch.zeros(Np, d, dtype=torch.float32, device=dev); iy[:N] = init_Y.to(torch.float32)
        init_Y = iy
    return ic, init_Y


def fgw_barycenters(N, Ys: Sequence[Tensor], Cs: Sequence[Tensor], ps=None, p=None, lambdas=None, loss_fun="square_loss",
                    epsilon=0.1, symmetric=True, alpha=0.5, max_iter=100, tol=1e-9, solver="PGD", stop_criterion="barycenter",
                    warmstartT=False, verbose=False, log=False, init_C=None, init_Y=None, fixed_structure=False,
                    fixed_features=False, seed=0, **kwargs):
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    if stop_criterion not in ["barycenter", "loss"]:
        raise ValueError(f"Unknown `stop_criterion='{stop_criterion}'`. Use one of: {'barycenter', 'loss'}.")
    if solver not in ["PGD", "PPA", "BAPG"]:
        raise ValueError("Unknown solver '%s'. Pick one in ['PGD', 'PPA', 'BAPG']." % solver)
    if stop_criterion != "barycenter":
        raise NotImplementedError("only stop_criterion='barycenter' (the path every ConAN model takes, schnet_no_sum.py:281-306) is "
                                  "implemented on this backend")
    symmetric = None if symmetric is None else bool(symmetric)           # (bregman.py:103-106: None is decided per call, else truthiness)
    method = kwargs.pop("method", "sinkhorn_log")
    if solver != "BAPG" and str(method).lower() != "sinkhorn_log":      # (fgw_bregman takes no Sinkhorn keywords, bregman.py:52-67)
        raise NotImplementedError("only method='sinkhorn_log' is implemented")
    num_iter_max = int(kwargs.pop("numItermax", 100))          # sinkhorn.py:12
    stop_thr = float(kwargs.pop("stopThr", 1e-5))              # sinkhorn.py:13
    if fixed_structure and init_C is None:
        raise ValueError("If C is fixed it must be initialized")
    if fixed_features and init_Y is None:
        raise ValueError("If Y is fixed it must be initialized")

    N = int(N)
    if (solver != "PGD" or symmetric is not True) and not all(torch.is_tensor(y) and y.is_cuda for y in (Ys.unbind(0) if torch.is_tensor(Ys) else Ys)):
        what = f"solver='{solver}'" if symmetric is True else f"symmetric={symmetric}"
        raise NotImplementedError(f"{what} runs on the GPU only: pass CUDA (ROCm) tensors")
    Ys_l = [y.to(torch.float32) for y in (Ys.unbind(0) if torch.is_tensor(Ys) else Ys)]
    Cs_l = [c.to(torch.float32) for c in (Cs.unbind(0) if torch.is_tensor(Cs) else Cs)]
    K, d = len(Ys_l), Ys_l[0].shape[1]
    sizes = [int(y.shape[0]) for y in Ys_l]
    if len(Cs_l) != K or any(tuple(c.shape) != (n, n) for c, n in zip(Cs_l, sizes)):
        raise ValueError("Cs[s] must be a square matrix over the nodes of Ys[s]")
    # Input graphs whose node counts differ from N or from each other (barycenter.py:50-67 takes any; no ConAN model does this: the glue pads
    # every conformer to N, schnet_no_sum.py:242-252).  The kernels solve square problems, so the call is embedded in one of size
    # Np = max(N, max n_s): the extra nodes carry NO mass (p_i = 0 / ps[s]_j = 0), zero features and no edges.  A massless node's row / column of
    # every coupling is exactly zero in the Sinkhorn scaling (u_i = p_i / (K v)_i), it adds nothing to any product, and the barycenter update
    # keeps its row of Y and its row / column of C at zero (fgw_small.hip: the divisions by p are guarded) — the leading N x N / N x n_s blocks
    # are the reference's rectangular problem, term for term.
    dev = Ys_l[0].device
    embedded, Np, Ys_l, Cs_l, ps, p_embedded = _embed_graphs(N, Ys_l, Cs_l, ps, p, sizes, d, dev)
    Ys_t, Cs_t = torch.stack(Ys_l), torch.stack(Cs_l)
    if init_C is None:
        init_C = _seeded_init_C(N, seed, Ys_t.device)
    N_user = N
    if embedded:
        init_C, init_Y = _embed_init(init_C, init_Y, N, Np, d, dev)
        N = Np
    ps_t = None
    if ps is not None:
        ps_t = (torch.stack(list(ps)) if not torch.is_tensor(ps) else ps).to(torch.float32).view(1, K, N)
    p_t = p_embedded.view(1, N) if embedded else (p.to(torch.float32).view(1, N) if p is not None else None)
    lam = None
    if lambdas is not None:
        if not torch.is_tensor(lambdas) and any(torch.is_tensor(l) for l in lambdas):
            # a list of (0-d) tensors: stacked, so that a lambda that requires grad keeps its graph (torch.as_tensor would drop it)
            lam = torch.stack([torch.as_tensor(l, dtype=torch.float32, device=Ys_t.device).reshape(()) for l in lambdas])
        else:
            lam = torch.as_tensor(lambdas, dtype=torch.float32, device=Ys_t.device)
    # adjacency-like inputs (integers in [0, 255]: what to_dense_adj produces) take the byte-wide LDS layout of the N <= 64 kernel
    small_int = bool(((Cs_t == Cs_t.round()) & (Cs_t >= 0) & (Cs_t <= 255)).all())
    res = ot_ops.fgw_barycenter_batched(
        Ys_t.view(1, K, N, d), Cs_t.view(1, K, N, N), ps=ps_t, p=p_t, lambdas=lam,
        init_C=init_C.to(torch.float32).view(1, N, N), init_Y=None if init_Y is None else init_Y.to(torch.float32).view(1, N, d),
        alpha=alpha, epsilon=epsilon, max_iter=max_iter, tol=tol, inner_tol=1e-4, num_iter_max=num_iter_max, stop_thr=stop_thr,
        fixed_structure=fixed_structure, fixed_features=fixed_features, warmstart=warmstartT, loss_fun=loss_fun, keep_iterates=bool(log),
        cs_small_int=small_int, solver=solver, symmetric=symmetric)
    Y, C, T, info, errs = res[:5]
    if solver != "PGD" and int(info[0, 3].item()) & 4:
        # an iterate with a zero row / column sum: the reference's NaN case, where it only warns (bregman.py:159-162, :270-273)
        warnings.warn("Solver failed to produce a transport plan. You might want to increase the regularization parameter `epsilon`.")
    if embedded:
        Y, C = Y[:, :N_user], C[:, :N_user, :N_user]
    if not log:
        return Y[0], C[0]
    outer = int(info[0, 0].item())
    T_iter = res[5]
    # log["Ms"] (barycenter.py:82,177,220): the feature costs dist(Y, Ys[s]) of the returned barycenter — clamped squared
    # euclidean distances (utils.py:154-171); a by-product for the caller's inspection, formed here from the outputs
    Yd = Y[0]
    y2 = (Yd * Yd).sum(1)
    Yin = [Ys_t[s, :sizes[s]] for s in range(K)]              # (an embedded call: the caller's own nodes)
    Ms = [torch.clamp(y2[:, None] + (Yin[s] * Yin[s]).sum(1)[None, :] - 2.0 * (Yd @ Yin[s].T), min=0) for s in range(K)]
    log_ = {"err_feature": [errs[0, 0, i] for i in range(outer)], "err_structure": [errs[0, 1, i] for i in range(outer)],
            "Ts_iter": [[T_iter[i, 0, s, :N_user, :sizes[s]] for s in range(K)] for i in range(outer)],           # barycenter.py:196
            "T": [T[0, s, :N_user, :sizes[s]] for s in range(K)],
            "p": p if p is not None else torch.ones(N_user, device=Y.device) / N_user,
            "Ms": Ms,
            "n_outer": outer, "n_pgd": int(info[0, 1].item()), "n_sinkhorn": int(info[0, 2].item())}
    return Y[0], C[0], log_


def fused_ACC_torch(M, A, B, a=None, b=None, X=None, alpha=0, epoch=200, eps=1e-5, rho=1e-1):
    """FGWMixup's coupling solve between two attributed graphs, the reference's fused_ACC_torch (barycenter.py:228-256): accelerated mirror
    descent on X from a b^T (or the given X), at most `epoch` epochs, stopped when the objective's relative change between two checks (every
    10th epoch) falls below eps -> (X, obj_list).  M [n1,n2], A [n1,n1], B [n2,n2] (any sizes: n1 != n2 is embedded with massless nodes).
    Deviations from the reference: a / b given as None mean uniform weights (the reference forms a dot product there); the plan carries no
    gradient (the reference's would unroll every epoch; to train through the solve use fgw_mixup_distance, the gradient of the distance at the
    returned plan); the run is an fp64 iteration on the fp32 inputs, so counts and values follow the reference's fp64 run; a weight that is exactly
    ZERO marks an absent node whose entries stay zero (the reference lifts them by 1e-10 every epoch).  A NaN result (exp under- / overflow at
    small rho) is the reference's NaN.  Runs on the GPU only.  fused_ACC_unrolled is this solve with the reference's differentiable plan."""
    for name, t in (("M", M), ("A", A), ("B", B), ("a", a), ("b", b), ("X", X)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"fused_ACC_torch runs on the GPU only: pass CUDA (ROCm) tensors ({name} is not one)")
    one = lambda t: None if t is None else t.unsqueeze(0)
    Xo, objs, info = ot_ops.fgw_acc_pair_batched(one(M), one(A), one(B), one(a), one(b), one(X), alpha=alpha, rho=rho, epoch=epoch, eps=eps)
    stored = int(info[0, 1].item())
    return Xo[0], [objs[0, k] for k in range(stored)]


def fgw_mixup_distance(M, A, B, a=None, b=None, X=None, alpha=0, epoch=200, eps=1e-5, rho=1e-1, log=False):
    """The FGWMixup distance of two attributed graphs as a differentiable value: fused_ACC_torch's arguments, defaults and solve, and the
    distance the reference's commented lines describe (barycenter.py:348-350) at the plan X that solve returns,
        (1 - alpha) <M, X> + alpha (<c1, X> - 2 <A X B, X>),   c1 = (A o A) a 1^T + 1 b^T (B o B)
    (the solve's final objective plus alpha <c1, X>), as a 0-d tensor that carries gradients to M, A, B, a and b.  The gradient is that of this
    formula at the solve's plan X, held constant — the treatment the barycenter gives its couplings (barycenter.py:120) — and NOT what
    back-propagating through the reference's fused_ACC_torch gives, which unrolls every epoch into the graph.  X (the start) and the plan get no
    gradient; there is no double backward.  A finite difference of this function moves the plan, so it does not check this gradient.
    log=True: (dist, {"T": the plan (no gradient, fused_ACC_torch's bits), "obj_list": fused_ACC_torch's list}).  Runs on the GPU only.
    fgw_mixup_distance_unrolled is this distance with the gradient through the unrolled epochs."""
    for name, t in (("M", M), ("A", A), ("B", B), ("a", a), ("b", b), ("X", X)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"fgw_mixup_distance runs on the GPU only: pass CUDA (ROCm) tensors ({name} is not one)")
    one = lambda t: None if t is None else t.unsqueeze(0)
    dist, Xo, objs, info = ot_ops.fgw_acc_pair_distance(one(M), one(A), one(B), one(a), one(b), one(X), alpha=alpha, rho=rho, epoch=epoch, eps=eps,
                                                     return_plan=True)
    if not log:
        return dist[0]
    stored = int(info[0, 1].item())
    return dist[0], {"T": Xo[0], "obj_list": [objs[0, k] for k in range(stored)]}


def _unrolled_pair(fn, M, A, B, a, b, X, alpha, epoch, eps, rho):
    for name, t in (("M", M), ("A", A), ("B", B), ("a", a), ("b", b), ("X", X)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"{fn} runs on the GPU only: pass CUDA (ROCm) tensors ({name} is not one)")
    one = lambda t: None if t is None else t.unsqueeze(0)
    Xo, dist, objs, info = ot_ops.fgw_acc_pair_unrolled(one(M), one(A), one(B), one(a), one(b), one(X), alpha=alpha, rho=rho, epoch=epoch, eps=eps)
    stored = int(info[0, 1].item())
    return Xo[0], dist[0], [objs[0, k] for k in range(stored)]


def fused_ACC_unrolled(M, A, B, a=None, b=None, X=None, alpha=0, epoch=200, eps=1e-5, rho=1e-1):
    """fused_ACC_torch (same arguments, defaults, solve and bits) -> (X, obj_list) with a DIFFERENTIABLE plan: X carries the gradient the
    reference's fused_ACC_torch delivers under torch autograd, back through every executed epoch, to M, A, B, a, b and to the start X when one
    is given (ops.fgw_acc_pair_unrolled: one backward launch that replays the epochs and walks them in reverse).  Deviations from the
    reference beyond fused_ACC_torch's: obj_list carries no gradient; a node whose weight is exactly ZERO gets gradient 0 (the reference: a
    finite value from the entries it lifts by 1e-10); no double backward.  A NaN solve gives NaN gradients.  Runs on the GPU only."""
    Xo, _dist, objs = _unrolled_pair("fused_ACC_unrolled", M, A, B, a, b, X, alpha, epoch, eps, rho)
    return Xo, objs


def fgw_mixup_distance_unrolled(M, A, B, a=None, b=None, X=None, alpha=0, epoch=200, eps=1e-5, rho=1e-1, log=False):
    """fgw_mixup_distance (same arguments, defaults, solve, value and bits) with the TOTAL derivative: the 0-d distance carries the gradient of
        (1 - alpha) <M, X> + alpha (<c1, X> - 2 <A X B, X>),   c1 = (A o A) a 1^T + 1 b^T (B o B)
    to M, A, B, a, b and the start X with the plan X moving with them — what back-propagating this formula through the reference's
    fused_ACC_torch gives — where fgw_mixup_distance holds the plan fixed.  A central difference of this function (at a fixed epoch count)
    does check this gradient.  log=True: (dist, {"T": the plan, which carries the unrolled gradient too, "obj_list": fused_ACC_torch's list,
    without gradient}).  No double backward.  Runs on the GPU only."""
    Xo, dist, objs = _unrolled_pair("fgw_mixup_distance_unrolled", M, A, B, a, b, X, alpha, epoch, eps, rho)
    return (dist, {"T": Xo, "obj_list": objs}) if log else dist


def _barycenters_BAPG(name, solve, N, Ys, Cs, ps, p, lambdas, loss_fun, alpha, max_iter, tol, rho, log, init_C, init_Y, fixed_structure,
                      fixed_features, seed):
    """fgw_barycenters_BAPG and fgw_barycenters_BAPG_unrolled around their op `solve` (ops.fgw_mixup_barycenter_batched / _unrolled): the
    reference's checks, the embedding of other sizes, the seeded start and the log."""
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    if fixed_structure and init_C is None:
        raise ValueError("If C is fixed it must be initialized")
    if fixed_features and init_Y is None:
        raise ValueError("If Y is fixed it must be initialized")
    N = int(N)
    Ys_in = Ys.unbind(0) if torch.is_tensor(Ys) else Ys
    if not all(torch.is_tensor(y) and y.is_cuda for y in Ys_in):
        raise NotImplementedError(f"{name} runs on the GPU only: pass CUDA (ROCm) tensors")
    Ys_l = [y.to(torch.float32) for y in Ys_in]
    Cs_l = [c.to(torch.float32) for c in (Cs.unbind(0) if torch.is_tensor(Cs) else Cs)]
    K, d = len(Ys_l), Ys_l[0].shape[1]
    sizes = [int(y.shape[0]) for y in Ys_l]
    if len(Cs_l) != K or any(tuple(c.shape) != (n, n) for c, n in zip(Cs_l, sizes)):
        raise ValueError("Cs[s] must be a square matrix over the nodes of Ys[s]")
    dev = Ys_l[0].device
    embedded, Np, Ys_l, Cs_l, ps_e, p_embedded = _embed_graphs(N, Ys_l, Cs_l, ps, p, sizes, d, dev)
    if init_C is None:
        init_C = _seeded_init_C(N, seed, dev)
    N_user = N
    if embedded:
        init_C, init_Y = _embed_init(init_C, init_Y, N, Np, d, dev)
        N = Np
    ps_t = None if ps_e is None else (torch.stack(list(ps_e)) if not torch.is_tensor(ps_e) else ps_e).to(torch.float32).to(dev).view(1, K, N)
    p_t = p_embedded.view(1, N) if embedded else (None if p is None else p.to(torch.float32).to(dev).view(1, N))
    lam = None
    if lambdas is not None:
        if torch.is_tensor(lambdas):
            lam = lambdas.to(torch.float32).to(dev)
        elif any(torch.is_tensor(l) for l in lambdas):
            # a list of (0-d) tensors: stacked, so that a lambda that requires grad keeps its graph (as fgw_barycenters does)
            lam = torch.stack([torch.as_tensor(l, dtype=torch.float32, device=dev).reshape(()) for l in lambdas])
        else:
            lam = torch.as_tensor([float(l) for l in lambdas], dtype=torch.float32, device=dev)
    res = solve(
        torch.stack(Ys_l).view(1, K, N, d), torch.stack(Cs_l).view(1, K, N, N), ps=ps_t, p=p_t, lambdas=lam,
        init_C=init_C.to(torch.float32).to(dev).view(1, N, N), init_Y=None if init_Y is None else init_Y.to(torch.float32).to(dev).view(1, N, d),
        alpha=alpha, rho=rho, max_iter=max_iter, tol=tol, epoch=100, eps=1e-5, fixed_structure=fixed_structure, fixed_features=fixed_features,
        loss_fun=loss_fun, keep_iterates=bool(log))
    Y, C, T, info, errs = res[:5]
    Y, C = Y[0, :N_user], C[0, :N_user, :N_user]
    if not log:
        return Y, C
    outer = int(info[0, 0].item())
    T_iter = res[5]
    # log["Ms"] (barycenter.py:355,386): dist(Y, Ys[s]) of the returned barycenter; a by-product for inspection, without gradient
    Ms = [feature_cost(Y.detach(), Ys_l[s][:sizes[s]].detach()) for s in range(K)]
    log_ = {"err_feature": [errs[0, 0, i] for i in range(outer)], "err_structure": [errs[0, 1, i] for i in range(outer)],
            "Ts_iter": [[T_iter[i, 0, s, :N_user, :sizes[s]] for s in range(K)] for i in range(outer)],
            "T": [T[0, s, :N_user, :sizes[s]] for s in range(K)],
            "p": p if p is not None else torch.ones(N_user, device=dev) / N_user,
            "Ms": Ms, "n_outer": outer, "n_inner": int(info[0, 1].item())}
    return Y, C, log_


def fgw_barycenters_BAPG(N, Ys: Sequence[Tensor], Cs: Sequence[Tensor], ps=None, p=None, lambdas=None, loss_fun="square_loss", alpha=0.5,
                         max_iter=100, tol=1e-9, rho=1.0, verbose=False, log=False, init_C=None, init_Y=None, fixed_structure=False,
                         fixed_features=False, seed=0, **kwargs):
    """The FGWMixup barycenter, the reference's fgw_barycenters_BAPG (barycenter.py:259-390): the outer loop of fgw_barycenters around
    fused_ACC_torch (100 epochs at most, eps = 1e-5, the caller's rho, always from p ps[s]^T).  This is not fgw_barycenters(solver="BAPG"),
    which runs the Bregman projections of fgw_bregman.  Same argument names, defaults, ValueErrors, return values and log keys as the
    reference (the log also carries n_outer and n_inner, the outer iterations and the epochs summed over all coupling solves).  Cs may be
    directed.  Input graphs of other sizes are embedded with massless nodes, as in fgw_barycenters.
    Differentiable in the project's fixed-plan convention, the one fgw_barycenters uses: Y and C carry gradients to Ys, Cs, p and lambdas (to
    init_Y / init_C instead of Ys / Cs under fixed_features / fixed_structure); ps gets none, nor do log["T"], log["Ts_iter"] and log["Ms"].  The
    gradient is that of the last update steps (update_feature_matrix, update_square_loss / update_kl_loss) at the couplings T[s] of the last outer
    iteration, held constant — the treatment fgw_barycenters gives its couplings (barycenter.py:120) — and NOT what the reference's
    fgw_barycenters_BAPG gives under autograd, which back-propagates through all 100 epochs of every fused_ACC_torch call.  There is no double
    backward.  A finite difference of this function moves the plan, so it does not check this gradient.  Gradients of embedded inputs arrive in
    the caller's own shapes, and a node without mass receives exactly zero.  A run that ends in NaN (below) gives NaN gradients.
    Other deviations: ps=None means uniform weights (the reference raises a TypeError); the run is an fp64 iteration on the fp32 inputs, so
    iteration counts follow the reference's fp64 run; a weight that is exactly ZERO marks an absent node (the reference lifts its entries by
    1e-10 every epoch); a NaN result (exp under- / overflow at small rho) is the reference's NaN.  Runs on the GPU only.
    fgw_barycenters_BAPG_unrolled is the same solve with the reference's gradient through every epoch of every coupling solve."""
    return _barycenters_BAPG("fgw_barycenters_BAPG", ot_ops.fgw_mixup_barycenter_batched, N, Ys, Cs, ps, p, lambdas, loss_fun, alpha, max_iter, tol, rho,
                             log, init_C, init_Y, fixed_structure, fixed_features, seed)


def fgw_barycenters_BAPG_unrolled(N, Ys: Sequence[Tensor], Cs: Sequence[Tensor], ps=None, p=None, lambdas=None, loss_fun="square_loss", alpha=0.5,
                                  max_iter=100, tol=1e-9, rho=1.0, verbose=False, log=False, init_C=None, init_Y=None, fixed_structure=False,
                                  fixed_features=False, seed=0, **kwargs):
    """fgw_barycenters_BAPG (same arguments, ValueErrors, embedding of other sizes, return values and log keys, the same solve bit for bit)
    whose Y and C carry the gradient that torch autograd forms through the reference's fgw_barycenters_BAPG (barycenter.py:259-390, whose
    coupling solves run with autograd on): through the update steps, the feature costs and every epoch of every fused_ACC_torch call of every
    outer iteration, not at couplings held constant.  Gradients reach Ys, Cs, ps, p, lambdas, init_C and init_Y; those of embedded (other-size)
    inputs arrive in the caller's shapes, and a node without mass receives exactly zero.  ps=None and p=None mean uniform weights and get no
    gradient; the seeded random init_C (when none is given) is a constant; lambdas given as a list of 0-d tensors keeps its graph.
    Deviations: log["T"], log["Ts_iter"] and log["Ms"] carry no gradient (the reference's have a graph); the stop decisions carry none; a
    weight that is exactly zero marks an absent node; a run that ends in NaN gives NaN gradients.  No double backward.  The backward replays
    every coupling solve (ops.fgw_mixup_barycenter_unrolled states its launches and workspace).  Runs on the GPU only."""
    return _barycenters_BAPG("fgw_barycenters_BAPG_unrolled", ot_ops.fgw_mixup_barycenter_unrolled, N, Ys, Cs, ps, p, lambdas, loss_fun, alpha, max_iter,
                             tol, rho, log, init_C, init_Y, fixed_structure, fixed_features, seed)


_FAILED = "Solver failed to produce a transport plan. You might want to increase the regularization parameter `epsilon`."


def _pair_solve(M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, solver, log, num_iter_max=100, stop_thr=1e-5, distance=False):
    """One pair through ops.fgw_pair_batched (B = 1); the reference's return value.  distance: through ops.fgw_pair_distance, fgw_distance's."""
    for name, t in (("M", M), ("C1", C1), ("C2", C2), ("p", p), ("q", q), ("G0", G0)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"fgw runs on the GPU only: pass CUDA (ROCm) tensors ({name} is not one)")
    one = lambda t: None if t is None else t.unsqueeze(0)
    kw = dict(alpha=alpha, epsilon=epsilon, max_iter=max_iter, tol=tol, num_iter_max=num_iter_max, stop_thr=stop_thr, loss_fun=loss_fun, solver=solver,
              symmetric=symmetric)
    if distance:
        dist, T, info, errs = ot_ops.fgw_pair_distance(one(M), one(C1), one(C2), one(p), one(q), one(G0), return_plan=True, **kw)
    else:
        T, dist, info, errs = ot_ops.fgw_pair_batched(one(M), one(C1), one(C2), one(p), one(q), one(G0), with_dist=bool(log), **kw)
    T = T[0]
    # bregman.py:159-162 (PGD / PPA: the plan's total mass) and :267-270 (BAPG: a NaN), one host synchronisation as in the reference
    failed = bool(torch.isnan(T).any()) if solver == "BAPG" else bool(abs(T.sum() - 1) > 1e-5)
    if failed:
        warnings.warn(_FAILED)
    if not log:
        return dist[0] if distance else T
    n_iter, n_sk = int(info[0, 0].item()), int(info[0, 1].item())
    log_ = {"err": [errs[0, i] for i in range((n_iter + 9) // 10)], "fgw_dist": dist[0].detach() if distance else dist[0], "n_iter": n_iter, "n_sinkhorn": n_sk}
    if distance:
        log_["T"] = T
        return dist[0], log_
    return T, log_


def _check_projected(loss_fun, solver, method, warmstart, kwargs):
    """fgw_projected's refusals, in its order -> the Sinkhorn keywords (numItermax, stopThr)."""
    if solver not in ["PGD", "PPA"]:
        raise ValueError("Unknown solver '%s'. Pick one in ['PGD', 'PPA']." % solver)
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    if warmstart:
        raise NotImplementedError("warmstart=True is broken in the reference (torch.log of a Python int, bregman.py:113) and not implemented here")
    if str(method).lower() != "sinkhorn_log":
        raise NotImplementedError("only method='sinkhorn_log' is implemented")
    return int(kwargs.pop("numItermax", 100)), float(kwargs.pop("stopThr", 1e-5))          # sinkhorn.py:12-13


def fgw_projected(M, C1, C2, p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=100, tol=1e-5,
                  solver="PGD", method="sinkhorn_log", warmstart=False, verbose=False, log=False, **kwargs):
    """The reference's fgw_projected (bregman.py:70-167): the entropic FGW coupling between two attributed graphs by projected gradient
    ("PGD") or proximal point ("PPA") iterations with a log-domain Sinkhorn inside, on the GPU.  M [n1,n2] feature cost, C1 [n1,n1], C2 [n2,n2]
    structures, p / q marginals, G0 start plan; keywords numItermax (100) / stopThr (1e-5) go to the Sinkhorn.  Returns T [n1,n2]; with log=True
    (T, {"err": [||T - Tprev|| at every 10th iteration], "fgw_dist": 0-d tensor, "n_iter": int, "n_sinkhorn": int}).  Same ValueErrors and the
    same "Solver failed" warning (|sum(T) - 1| > 1e-5) as the reference.  Deviations: p=None / q=None mean uniform marginals (the reference's own
    default crashes in torch.outer(None, None)); warmstart=True raises NotImplementedError (the reference's branch calls torch.log on a Python
    int and raises TypeError); a method other than "sinkhorn_log", CPU tensors ("GPU only") and verbose printing are not implemented
    (NotImplementedError for the first two, verbose is ignored); the outputs carry NO gradient (the reference would back-propagate through the
    unrolled iterations; not built here).  To train through the distance use fgw_distance (one pair) or fgw_pairwise_distances (an ensemble):
    the gradient of fgw_dist at the returned plan."""
    num_iter_max, stop_thr = _check_projected(loss_fun, solver, method, warmstart, kwargs)
    return _pair_solve(M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, solver, log, num_iter_max, stop_thr)


def fgw_bregman(M, C1, C2, p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=1000, tol=1e-9,
                marginal_loss=False, verbose=False, log=False):
    """The reference's fgw_bregman (bregman.py:170-279): the same coupling by alternating Bregman projections (BAPG), on the GPU.  Arguments and
    return value as fgw_projected (n_sinkhorn is 0; the reference's log["loss"] is not formed); the warning is the reference's, for a NaN plan.
    Deviations: as fgw_projected, and marginal_loss=True raises NotImplementedError (no caller of the reference sets it)."""
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    if marginal_loss:
        raise NotImplementedError("marginal_loss=True is not implemented")
    return _pair_solve(M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, "BAPG", log)


def fgw(M, C1, C2, p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=100, tol=1e-5, solver="PGD",
        method="sinkhorn_log", warmstart=False, verbose=False, log=False, **kwargs):
    """The reference's fgw (bregman.py:8-67): fgw_projected for solver "PGD" / "PPA", fgw_bregman for "BAPG" (which, as in the reference, takes
    no Sinkhorn keywords, no method and no warmstart).  See fgw_projected for the return value and the deviations."""
    if solver in ["PGD", "PPA"]:
        return fgw_projected(M, C1, C2, p=p, q=q, loss_fun=loss_fun, epsilon=epsilon, symmetric=symmetric, alpha=alpha, G0=G0, max_iter=max_iter,
                             tol=tol, solver=solver, method=method, warmstart=warmstart, verbose=verbose, log=log, **kwargs)
    elif solver == "BAPG":
        return fgw_bregman(M, C1, C2, p=p, q=q, loss_fun=loss_fun, epsilon=epsilon, symmetric=symmetric, alpha=alpha, G0=G0, max_iter=max_iter,
                           tol=tol, verbose=verbose, log=log)
    raise ValueError("Unknown solver '%s'. Pick one in ['PGD', 'PPA', 'BAPG']." % solver)


def fgw_distance(M, C1, C2, p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=100, tol=1e-5,
                 solver="PGD", method="sinkhorn_log", warmstart=False, verbose=False, log=False, **kwargs):
    """The FGW distance of two attributed graphs as a differentiable value: fgw's arguments, defaults, errors and warning, and the value of its
    log["fgw_dist"] bit for bit, as a 0-d tensor that carries gradients to M, C1, C2, p and q.  The gradient is that of
    (1 - alpha) sum(M * T) + alpha gwloss(init_matrix(C1, C2, p, q, loss_fun), T) at the solve's plan T, held constant — the treatment the
    barycenter gives its couplings (barycenter.py:120) — and NOT what the reference's log["fgw_dist"].backward() gives, which unrolls every Sinkhorn
    sweep into the graph.  T and G0 get no gradient; there is no double backward.  A finite difference of this function moves the plan, so it does
    not check this gradient.  log=True: (dist, {"T": the plan (no gradient), "err", "fgw_dist", "n_iter", "n_sinkhorn"})."""
    if solver in ["PGD", "PPA"]:
        num_iter_max, stop_thr = _check_projected(loss_fun, solver, method, warmstart, kwargs)
    elif solver == "BAPG":
        if loss_fun not in ("square_loss", "kl_loss"):
            raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
        num_iter_max, stop_thr = 100, 1e-5
    else:
        raise ValueError("Unknown solver '%s'. Pick one in ['PGD', 'PPA', 'BAPG']." % solver)
    return _pair_solve(M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, solver, log, num_iter_max, stop_thr, distance=True)


def _pair_solve_unrolled(fn, M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, solver, method, warmstart, kwargs):
    """The refusals of the unrolled names, then one pair through ops.fgw_pair_unrolled (B = 1) -> (T, dist, log without "fgw_dist" / "T")."""
    if solver not in ("PGD", "PPA", "BAPG"):
        raise ValueError("Unknown solver '%s'. Pick one in ['PGD', 'PPA', 'BAPG']." % solver)
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    if solver == "BAPG":
        raise NotImplementedError(f"{fn} covers solver 'PGD' and 'PPA': 'BAPG' is not implemented")
    if loss_fun == "kl_loss":
        raise NotImplementedError(f"{fn} covers loss_fun 'square_loss': 'kl_loss' is not implemented")
    if kwargs.pop("marginal_loss", False):
        raise NotImplementedError("marginal_loss=True is not implemented")
    num_iter_max, stop_thr = _check_projected(loss_fun, solver, method, warmstart, kwargs)
    for name, t in (("M", M), ("C1", C1), ("C2", C2), ("p", p), ("q", q), ("G0", G0)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"{fn} runs on the GPU only: pass CUDA (ROCm) tensors ({name} is not one)")
    one = lambda t: None if t is None else t.unsqueeze(0)
    T, dist, info, errs = ot_ops.fgw_pair_unrolled(one(M), one(C1), one(C2), one(p), one(q), one(G0), alpha=alpha, epsilon=epsilon, max_iter=max_iter, tol=tol,
                                                num_iter_max=num_iter_max, stop_thr=stop_thr, loss_fun=loss_fun, solver=solver, symmetric=symmetric)
    T = T[0]
    if bool(abs(T.detach().sum() - 1) > 1e-5):                              # bregman.py:159-162, one host synchronisation as in the reference
        warnings.warn(_FAILED)
    n_iter, n_sk = int(info[0, 0].item()), int(info[0, 1].item())
    return T, dist[0], {"err": [errs[0, i] for i in range((n_iter + 9) // 10)], "n_iter": n_iter, "n_sinkhorn": n_sk}


def fgw_unrolled(M, C1, C2, p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=100, tol=1e-5, solver="PGD",
                 method="sinkhorn_log", warmstart=False, verbose=False, log=False, **kwargs):
    """fgw (same arguments, defaults, solve, warning and bits) with DIFFERENTIABLE outputs, as the reference's call delivers them: T, and with
    log=True log["fgw_dist"], carry the gradient torch autograd forms through the reference's fgw — back through every executed PGD / PPA
    iteration and every Sinkhorn sweep — to M, C1, C2, p, q and to G0 when one is given (ops.fgw_pair_unrolled: one backward launch that replays
    the iterations and walks them in reverse).  solver "PGD" or "PPA" and the square loss; "BAPG", "kl_loss", warmstart=True, another method and
    marginal_loss raise NotImplementedError.  Deviations from the reference beyond fgw's: log["err"] carries no gradient; a node whose weight is
    exactly ZERO gets gradient 0 (the reference: NaN from log(0)); no double backward.  A solve the reference's autograd answers with NaN (PPA
    after entries of the plan have underflowed to zero) gives NaN gradients.  Runs on the GPU only."""
    T, dist, log_ = _pair_solve_unrolled("fgw_unrolled", M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, solver, method, warmstart, kwargs)
    if not log:
        return T
    log_["fgw_dist"] = dist
    return T, log_


def fgw_distance_unrolled(M, C1, C2, p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=100, tol=1e-5,
                          solver="PGD", method="sinkhorn_log", warmstart=False, verbose=False, log=False, **kwargs):
    """fgw_distance (same arguments, defaults, solve, value and bits) with the TOTAL derivative: the 0-d distance carries the gradient of
    log["fgw_dist"] with the plan moving with the inputs — the reference's log["fgw_dist"].backward() — to M, C1, C2, p, q and the start G0, where
    fgw_distance holds the plan fixed.  A central difference of this function (at fixed iteration and sweep counts) does check this gradient.
    log=True: (dist, {"T": the plan, which carries the unrolled gradient too, "err", "fgw_dist" (detached), "n_iter", "n_sinkhorn"}).  Refusals
    and deviations as fgw_unrolled.  Runs on the GPU only."""
    T, dist, log_ = _pair_solve_unrolled("fgw_distance_unrolled", M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, solver, method, warmstart,
                                         kwargs)
    if not log:
        return dist
    log_["fgw_dist"], log_["T"] = dist.detach(), T
    return dist, log_


def _bregman_solve_unrolled(fn, M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, marginal_loss):
    """The refusals of the unrolled BAPG names, then one pair through ops.fgw_bregman_unrolled (B = 1) -> (T, dist, log without "fgw_dist" / "T")."""
    if loss_fun not in ("square_loss", "kl_loss"):
        raise ValueError(f"Unknown `loss_fun='{loss_fun}'`. Use one of: {'square_loss', 'kl_loss'}.")
    if marginal_loss:
        raise NotImplementedError("marginal_loss=True is not implemented")
    for name, t in (("M", M), ("C1", C1), ("C2", C2), ("p", p), ("q", q), ("G0", G0)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"{fn} runs on the GPU only: pass CUDA (ROCm) tensors ({name} is not one)")
    one = lambda t: None if t is None else t.unsqueeze(0)
    T, dist, info, errs = ot_ops.fgw_bregman_unrolled(one(M), one(C1), one(C2), one(p), one(q), one(G0), alpha=alpha, epsilon=epsilon, max_iter=max_iter,
                                                   tol=tol, loss_fun=loss_fun, symmetric=symmetric)
    T, dist = T[0], dist[0]
    if bool(torch.isnan(T.detach()).any()):                                 # bregman.py:267-270, one host synchronisation as in the reference
        warnings.warn(_FAILED)
    # bregman.py:274-275: fgw_dist - alpha sum(constC o T), constC = f1(C1) p 1^T + 1 (f2(C2) q)^T of init_matrix (utils.py:20-64), in torch
    n1, n2 = M.shape
    pw = torch.full((n1,), 1.0 / n1, dtype=T.dtype, device=T.device) if p is None else p.to(T.dtype)
    qw = torch.full((n2,), 1.0 / n2, dtype=T.dtype, device=T.device) if q is None else q.to(T.dtype)
    a, b = C1.to(T.dtype), C2.to(T.dtype)
    f1, f2 = (a * a, b * b) if loss_fun == "square_loss" else (a * torch.log(a + 1e-15) - a, b)
    constC = (f1 @ pw)[:, None] + (f2 @ qw)[None, :]
    n_iter = int(info[0, 0].item())
    return T, dist, {"err": [errs[0, i] for i in range((n_iter + 9) // 10)], "loss": dist - alpha * torch.sum(constC * T), "n_iter": n_iter, "n_sinkhorn": 0}


def fgw_bregman_unrolled(M, C1, C2, p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=1000, tol=1e-9,
                         marginal_loss=False, verbose=False, log=False):
    """fgw_bregman (same arguments, defaults, solve, warning and bits) with DIFFERENTIABLE outputs, as the reference's call delivers them: T, and
    with log=True log["fgw_dist"] and log["loss"], carry the gradient torch autograd forms through the reference's fgw_bregman — back through
    every executed Bregman half-step — to M, C1, C2, p, q and to G0 when one is given (ops.fgw_bregman_unrolled: one backward launch that
    replays the iterations and walks the half-steps in reverse).  Both losses, symmetric True / False / None.  log=True: (T, {"err", "fgw_dist",
    "loss", "n_iter", "n_sinkhorn": 0}); log["loss"] is the reference's fgw_dist - alpha sum(constC * T) (bregman.py:274-275), formed in torch
    from T, fgw_dist and the constC torch computes from C1, C2, p, q, so its gradient is the reference's by composition.  marginal_loss=True
    raises NotImplementedError.  Deviations from the reference beyond fgw_bregman's: log["err"] carries no gradient; a node whose weight is
    exactly ZERO gets gradient 0 (the reference: NaN from 0 / 0); no double backward.  A solve the reference answers with a NaN plan gives NaN
    gradients and the reference's warning.  The backward's workspace is (2 max_iter + 4) N^2 * 8 bytes, N = max(n1, n2): 1.8 MB at N = 33 for
    max_iter = 100, 17.5 MB for the default 1000 (whatever the iterations run: the count stays on the device); the cap is the caller's choice.
    Runs on the GPU only."""
    T, dist, log_ = _bregman_solve_unrolled("fgw_bregman_unrolled", M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol, marginal_loss)
    if not log:
        return T
    log_["fgw_dist"] = dist
    return T, log_


def fgw_bregman_distance_unrolled(M, C1, C2, p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=1000,
                                  tol=1e-9, marginal_loss=False, verbose=False, log=False):
    """fgw_distance(solver="BAPG")'s value and bits with the TOTAL derivative, under fgw_bregman's signature: the 0-d distance carries the gradient
    of the reference's log["fgw_dist"].backward() through fgw_bregman — the plan moving with the inputs — to M, C1, C2, p, q and the start G0,
    where fgw_distance holds the plan fixed.  A central difference of this function (at a fixed iteration count) does check this gradient.
    log=True: (dist, {"T": the plan, which carries the unrolled gradient too, "err", "fgw_dist" (detached), "loss", "n_iter", "n_sinkhorn": 0}).
    Refusals, deviations and workspace ((2 max_iter + 4) N^2 * 8 bytes: 1.8 MB at N = 33 for max_iter = 100, 17.5 MB for 1000) as
    fgw_bregman_unrolled.  Runs on the GPU only."""
    T, dist, log_ = _bregman_solve_unrolled("fgw_bregman_distance_unrolled", M, C1, C2, p, q, G0, loss_fun, epsilon, symmetric, alpha, max_iter, tol,
                                            marginal_loss)
    if not log:
        return dist
    log_["fgw_dist"], log_["T"] = dist.detach(), T
    return dist, log_


def feature_cost(Y: Tensor, Z: Tensor) -> Tensor:
    """dist(Y, Z) of the reference (utils.py:154-171): the squared Euclidean distances of the feature rows, clamped at 0 -> [n1,n2]."""
    return torch.clamp((Y * Y).sum(1)[:, None] + (Z * Z).sum(1)[None, :] - 2.0 * (Y @ Z.T), min=0)


def _pairwise(name, Ys, Cs, ps, kw, with_grad, without_grad):
    """The all-pairs matrix of fgw_pairwise_distances: with_grad / without_grad = (batched, list) forms that return the distances [npairs]."""
    G = len(Ys)
    if len(Cs) != G or (ps is not None and len(ps) != G):
        raise ValueError("Ys, Cs (and ps) must have one entry per graph")
    if not all(torch.is_tensor(t) and t.is_cuda for t in list(Ys) + list(Cs)):
        raise NotImplementedError(f"{name} runs on the GPU only: pass CUDA (ROCm) tensors")
    grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in list(Ys) + list(Cs) + list(ps or []))
    keep = (lambda t: t) if grad else (lambda t: t.detach())
    Ys = [keep(y).to(torch.float32) for y in Ys]
    out = torch.zeros(G, G, dtype=torch.float32, device=Ys[0].device)
    ia, ib = torch.triu_indices(G, G, 1).tolist() if G > 1 else ([], [])
    if not ia:
        return out
    Ms = [feature_cost(Ys[a], Ys[b]) for a, b in zip(ia, ib)]
    pick = lambda ts, idx: None if ts is None else [ts[i] for i in idx]
    batched, lst = with_grad if grad else without_grad
    if len({int(y.shape[0]) for y in Ys}) == 1:
        st = lambda ts: None if ts is None else torch.stack([keep(t).to(torch.float32) for t in ts])
        dist = batched(torch.stack(Ms), st(pick(Cs, ia)), st(pick(Cs, ib)), st(pick(ps, ia)), st(pick(ps, ib)), **kw)
    else:
        dist = lst(Ms, pick(Cs, ia), pick(Cs, ib), pick(ps, ia), pick(ps, ib), **kw)
    out[ia, ib] = dist
    out[ib, ia] = dist
    return out


_PLAIN_PAIRS = (lambda *a, **k: ot_ops.fgw_pair_batched(*a, **k)[1], lambda *a, **k: ot_ops.fgw_pair_list(*a, **k)[1])


def fgw_pairwise_distances(Ys: Sequence[Tensor], Cs: Sequence[Tensor], ps=None, alpha=0.5, epsilon=0.1, loss_fun="square_loss", symmetric=None,
                           max_iter=100, tol=1e-5, solver="PGD", numItermax=100, stopThr=1e-5) -> Tensor:
    """The FGW distance matrix of G attributed graphs (the conformers of an ensemble): Ys[g] [n_g,d] features, Cs[g] [n_g,n_g] structures, ps[g]
    node weights or None (uniform) -> [G,G], symmetric with a zero diagonal.  The G (G - 1) / 2 pairs a < b are solved in ONE
    ops.fgw_pair_batched call (the list form when the sizes differ) with M = feature_cost(Ys[a], Ys[b]), formed by torch per pair ahead of
    the call; entry (a, b) is fgw(M, Cs[a], Cs[b], ps[a], ps[b], ..., log=True)'s log["fgw_dist"], bit for bit.
    When any of Ys, Cs, ps requires grad the result carries gradients to them (earlier versions silently returned none): every entry is
    fgw_distance's value with its gradient at the solved plan (ops.fgw_pair_distance); feature_cost, the stacking of the pairs and the scatter into
    the matrix stay in torch and are differentiated by torch.  The values are the same bits either way; with no input requiring grad the calls issued
    are the same as before."""
    kw = dict(alpha=alpha, epsilon=epsilon, max_iter=max_iter, tol=tol, num_iter_max=numItermax, stop_thr=stopThr, loss_fun=loss_fun, solver=solver,
              symmetric=symmetric)
    return _pairwise("fgw_pairwise_distances", Ys, Cs, ps, kw, (ot_ops.fgw_pair_distance, ot_ops.fgw_pair_distance_list), _PLAIN_PAIRS)


def fgw_pairwise_distances_unrolled(Ys: Sequence[Tensor], Cs: Sequence[Tensor], ps=None, alpha=0.5, epsilon=0.1, loss_fun="square_loss", symmetric=None,
                                    max_iter=100, tol=1e-5, solver="PGD", numItermax=100, stopThr=1e-5) -> Tensor:
    """fgw_pairwise_distances (same arguments, defaults, calls and bits of the matrix) with the TOTAL derivative: when any of Ys, Cs, ps requires
    grad every entry carries the gradient of fgw_distance_unrolled — through every iteration of its pair's solve (ops.fgw_pair_unrolled: one
    forward and one backward launch for all pairs) — and reaches Ys through feature_cost, Cs and ps.  solver "PGD" or "PPA", the square loss."""
    kw = dict(alpha=alpha, epsilon=epsilon, max_iter=max_iter, tol=tol, num_iter_max=numItermax, stop_thr=stopThr, loss_fun=loss_fun, solver=solver,
              symmetric=symmetric)
    if solver == "BAPG" or (solver in ("PGD", "PPA") and loss_fun == "kl_loss"):
        ot_ops._pair_unrolled_params(**kw)                                     # (raises: NotImplementedError under the new names)
    return _pairwise("fgw_pairwise_distances_unrolled", Ys, Cs, ps, kw,
                     (lambda *a, **k: ot_ops.fgw_pair_unrolled(*a, **k)[1], lambda *a, **k: ot_ops.fgw_pair_unrolled_list(*a, **k)[1]), _PLAIN_PAIRS)


def normalize_tensor(tensor: Tensor, a: float, b: float) -> Tensor:
    """a + (t - min) * (b - a) / (max - min) over the whole tensor (barycenter.py:393-399), on the densify kernel."""
    flat = tensor.reshape(1, -1).to(torch.float32).contiguous()
    n = flat.shape[1]
    dev = flat.device
    g = object.__new__(ops.RadiusGraph)
    g.num_graphs, g.num_atoms = 1, 1
    g.graph_ptr = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    g.rowptr = torch.zeros(2, dtype=torch.int32, device=dev)
    g.col = torch.zeros(1, dtype=torch.int32, device=dev)
    Ys, _ = ops.fgw_densify(flat.view(1, n), g, 1, 0.0, a, b)
    return Ys.view(tensor.shape)
