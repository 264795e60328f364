"""Entropic optimal transport, mirroring the reference's conan_fgw/src/model/fgw/sinkhorn.py: `sinkhorn` with all five of its methods, `sinkhorn_log`,
`sinkhorn_knopp`, `greenkhorn`, `sinkhorn_stabilized`, `sinkhorn_epsilon_scaling` and `sinkhorn2`, with its signatures and defaults, on the batched
HIP kernels of csrc/sinkhorn.hip and csrc/sinkhorn_ext.hip (one workgroup per problem, rectangular problems solved as they are), plus
`wasserstein_pairwise_distances`, the alpha = 0 sibling of `fgw.fgw_pairwise_distances`.

Same return values (`log=True`: the reference's dict with the reference's keys), the same warnings with the reference's texts, the same
`ValueError` for an unknown method, the same warm starts: (log u, log v) for "sinkhorn_log", "sinkhorn" and "greenkhorn", (alpha, beta) in cost
units for "sinkhorn_stabilized" and "sinkhorn_epsilon_scaling".

Several histograms at once: b [n2,H] (the reference's one-to-many form: one M, one a, H target histograms) returns the H transport costs [H],
no plan, from `sinkhorn`, `sinkhorn2`, `sinkhorn_knopp` and `sinkhorn_log`.  Method "sinkhorn" solves the columns JOINTLY as the reference
does (csrc/sinkhorn_hists.hip through ops.sinkhorn_hists_loss: one Frobenius error over all n2 H entries decides the stop, a numerical error
in any column restores the previous u, v of all; log: {"err", "niter", "u" [n1,H], "v" [n2,H]}; warmstart = (log u [n1,H], log v [n2,H])).
Method "sinkhorn_log" solves each column on its own, as the reference's loop does: H problems of ONE ops.sinkhorn_loss launch with M shared;
log: {"log_u", "log_v", "u", "v"} as [n,H]; warmstart = a list of H pairs; "did not converge" is given once if any column ran out, whatever
`warn` says (the reference does not hand `warn` to its inner calls); H = 1 without a warm start is solved, where the reference crashes.
grad="plan": the costs carry the fixed-plan gradient to M (Knopp: dM = K o sum_k g_k u_k v_k^T from one backward launch, no [H,n1,n2]
tensor); grad="unrolled" with a 2-D b raises NotImplementedError.

Deviations, each a `NotImplementedError`: a 2-D `b` with "greenkhorn", "sinkhorn_stabilized" or "sinkhorn_epsilon_scaling" (the reference has
no such form: its stabilized solver raises TypeError there); CPU tensors (the solve runs on the GPU only).  `verbose` is ignored.  Epsilon scaling warns ONCE when any of its inner solves ran to
`numInnerItermax` (the reference warns once per such solve, always from the same line, which Python's default filter shows once as well), and
once, with the last one's iteration, when inner solves left on numerical errors.  Outputs are fp32 (`alpha`, `beta` of the last two methods:
fp64, since epsilon scaling's potentials carry an offset of ~epsilon0 log n that fp32 resolves to 2e-3 only); the iteration runs in fp64, so iteration
counts, error lists, absorptions and the numerical-errors exits follow the reference's fp64 run, not its fp32 run (fp32 exp underflows earlier,
and an fp32 run cannot reach stopThr = 1e-9).

Gradients.  `sinkhorn`, `sinkhorn_log`, `sinkhorn_knopp`, `sinkhorn2` and `wasserstein_pairwise_distances` take grad="plan" (default) or
grad="unrolled".  "plan": the plan carries no gradient; `sinkhorn2`'s value carries the gradient to M at the returned plan, held constant (the
project's fixed-plan convention, fgw.fgw_distance's); a, b and the warm start get none.  "unrolled": the reference's gradient, autograd through
every executed Sinkhorn sweep, from one backward launch (csrc/sinkhorn_grad.hip): the returned plan requires grad, `sinkhorn2`'s value carries
the full gradient, and M, a, b and warmstart[0] receive it (warmstart[1] gets none, as in the reference: the first column pass overwrites v).
Deviation: an entry a_i = 0 (b_j = 0) gets gradient 0 and contributes nothing, where the reference's sinkhorn_log gives NaN at that entry and
its Knopp NaN everywhere.  The backward keeps (2 numItermax + 1) (n1 + n2) fp64 values per problem (1 MB for 33 x 33 at numItermax = 1000).
grad="unrolled" with "greenkhorn", "sinkhorn_stabilized" or "sinkhorn_epsilon_scaling" raises NotImplementedError; any other value of grad
raises ValueError.  No double backward.
"""
from __future__ import annotations

import warnings
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import ot_ops
from .fgw import feature_cost

_NOT_CONVERGED = ("Sinkhorn did not converge. You might want to increase the number of iterations `numItermax` or the regularization "
                  "parameter `reg`.")


def _check_grad(grad, ext_method=None):
    if grad not in ("plan", "unrolled"):
        raise ValueError("grad must be 'plan' or 'unrolled', not %r" % (grad,))
    if grad == "unrolled" and ext_method is not None:
        raise NotImplementedError(f"grad='unrolled' is not implemented for method='{ext_method}': only 'sinkhorn_log' and 'sinkhorn' have the "
                                  "unrolled gradient")


def _solve(a, b, M, reg, method, numItermax, stopThr, log, warn, warmstart, cost=False, grad="plan"):
    """One problem through ops (B = 1) with the reference's return value and warnings (one host synchronisation, as fgw._pair_solve)."""
    _check_grad(grad)
    if b is not None and torch.is_tensor(b) and b.dim() > 1:
        return _solve_hists(a, b, M, reg, method, numItermax, stopThr, log, warn, warmstart, grad)
    tensors = [("M", M), ("a", a), ("b", b)] + ([] if warmstart is None else [("warmstart[0]", warmstart[0]), ("warmstart[1]", warmstart[1])])
    for name, t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"sinkhorn runs on the GPU only: pass CUDA (ROCm) tensors ({name} is not one)")
    a = None if a is None or len(a) == 0 else a.unsqueeze(0)                # sinkhorn.py:221-224: an empty histogram means uniform
    b = None if b is None or len(b) == 0 else b.unsqueeze(0)
    warm = None if warmstart is None else (warmstart[0].unsqueeze(0), warmstart[1].unsqueeze(0))
    kw = dict(reg=reg, method=method, num_iter_max=numItermax, stop_thr=stopThr, warmstart=warm)
    if grad == "unrolled":
        T, loss, log_u, log_v, info, errs = ot_ops.sinkhorn_unrolled(M.unsqueeze(0), a, b, **kw)
    elif cost:
        loss, T, log_u, log_v, info, errs = ot_ops.sinkhorn_loss(M.unsqueeze(0), a, b, return_plan=True, **kw)
    else:
        T, loss, log_u, log_v, info, errs = ot_ops.sinkhorn_batched(M.unsqueeze(0), a, b, **kw)
    res = loss[0] if cost else T[0]
    if not (log or warn or method == "sinkhorn"):
        return res
    niter, flags, nchk, _ = info[0].tolist()
    if flags & 2:
        warnings.warn("Warning: numerical errors at iteration %d" % niter)
    elif not flags & 1 and warn:
        warnings.warn(_NOT_CONVERGED)
    if not log:
        return res
    log_ = {"err": [errs[0, i] for i in range(nchk)], "niter": niter}
    if method == "sinkhorn_log":
        log_["log_u"], log_["log_v"] = log_u[0], log_v[0]
    log_["u"], log_["v"] = torch.exp(log_u[0]), torch.exp(log_v[0])
    return res, log_


def _solve_hists(a, b, M, reg, method, numItermax, stopThr, log, warn, warmstart, grad):
    """The reference's one-to-many form, b [n2,H]: the H transport costs of one M and one a against the H columns of b, with the reference's
    return value and warnings (one host synchronisation).  "sinkhorn": the joint Knopp solve of ops.sinkhorn_hists_loss (B = 1).
    "sinkhorn_log": the H columns as H problems of ONE ops.sinkhorn_loss launch with M shared, each with its own stop, as the reference's loop."""
    if b.dim() != 2:
        raise ValueError(f"b must be [n2] or [n2,H], not {list(b.shape)}")
    H = int(b.shape[1])
    per_column = method == "sinkhorn_log"
    if warmstart is None:
        warms = []
    elif per_column:
        if len(warmstart) != H or any(w is None for w in warmstart):
            raise ValueError("warmstart must be a list of one (log u, log v) pair per column of b, or None")
        warms = [t for w in warmstart for t in w]
    else:
        warms = list(warmstart)
    tensors = [("M", M), ("a", a), ("b", b)] + [("warmstart", t) for t in warms]
    for name, t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"several histograms at once (a 2-D b) run on the GPU only: pass CUDA (ROCm) tensors ({name} is not one)")
    if grad == "unrolled":
        raise NotImplementedError("grad='unrolled' is not implemented for several histograms at once (a 2-D b): the costs carry the fixed-plan "
                                  "gradient (grad='plan') only")
    a = None if a is None or len(a) == 0 else a
    kw = dict(reg=reg, num_iter_max=numItermax, stop_thr=stopThr)
    if per_column:
        warm = None if warmstart is None else (torch.stack([w[0] for w in warmstart]), torch.stack([w[1] for w in warmstart]))
        cost, _T, log_u, log_v, info, _errs = ot_ops.sinkhorn_loss(M, None if a is None else a.unsqueeze(0).expand(H, -1), b.t(), method=method,
                                                                   warmstart=warm, return_plan=True, **kw)
        if not bool((info[:, 1] & 1).all()):                               # (the reference's inner calls are not handed `warn`: they warn by default)
            warnings.warn(_NOT_CONVERGED)
        if not log:
            return cost
        log_u, log_v = log_u.t(), log_v.t()
        return cost, {"log_u": log_u, "log_v": log_v, "u": torch.exp(log_u), "v": torch.exp(log_v)}
    warm = None if warmstart is None else (warmstart[0].unsqueeze(0), warmstart[1].unsqueeze(0))
    loss, log_u, log_v, info, errs = ot_ops.sinkhorn_hists_loss(M.unsqueeze(0), None if a is None else a.unsqueeze(0), b.unsqueeze(0), warmstart=warm,
                                                                return_log=True, **kw)
    niter, flags, nchk, _ = info[0].tolist()
    if flags & 2:
        warnings.warn("Warning: numerical errors at iteration %d" % niter)
    elif not flags & 1 and warn:
        warnings.warn(_NOT_CONVERGED)
    if not log:
        return loss[0]
    return loss[0], {"err": [errs[0, i] for i in range(nchk)], "niter": niter, "u": torch.exp(log_u[0]), "v": torch.exp(log_v[0])}


def sinkhorn_knopp(a, b, M, reg, numItermax=1000, stopThr=1e-9, verbose=False, log=False, warn=True, warmstart=None, grad="plan", **kwargs):
    """The reference's sinkhorn_knopp (sinkhorn.py:207-315): T [n1,n2]; log=True: (T, {"err", "niter", "u", "v"}).  The numerical-errors exit
    (a zero K^T u, a NaN or Inf in u or v: the previous u, v are returned, with the reference's warning) is decided on fp64 values.
    b [n2,H]: the H costs [H] instead of a plan, solved jointly (one error over all columns, one exit); u, v of the log are [n1,H], [n2,H]."""
    return _solve(a, b, M, reg, "sinkhorn", numItermax, stopThr, log, warn, warmstart, grad=grad)


def sinkhorn_log(a, b, M, reg, numItermax=1000, stopThr=1e-9, verbose=False, log=False, warn=True, warmstart=None, grad="plan", **kwargs):
    """The reference's sinkhorn_log (sinkhorn.py:318-450): T [n1,n2]; log=True: (T, {"err", "niter", "log_u", "log_v", "u", "v"}).
    b [n2,H]: the H costs [H], every column solved on its own in one launch; log=True: (costs, {"log_u", "log_v", "u", "v"}) as [n,H]."""
    return _solve(a, b, M, reg, "sinkhorn_log", numItermax, stopThr, log, warn, warmstart, grad=grad)


def _solve_ext(a, b, M, reg, method, numItermax, stopThr, log, warn, warmstart, cost=False, **params):
    """One problem through ops.sinkhorn_ext_* (B = 1) with the reference's return value, log dict and warnings (one host synchronisation)."""
    if b is not None and torch.is_tensor(b) and b.dim() > 1:
        raise NotImplementedError("several histograms at once (a 2-D b) are not implemented: solve them one by one, or as a batch with a shared M "
                                  "through ops.sinkhorn_ext_batched")
    tensors = [("M", M), ("a", a), ("b", b)] + ([] if warmstart is None else [("warmstart[0]", warmstart[0]), ("warmstart[1]", warmstart[1])])
    for name, t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise NotImplementedError(f"method='{method}' is not implemented for CPU tensors: {method} runs on the GPU only ({name} is not a CUDA "
                                      "(ROCm) tensor)")
    a = None if a is None or len(a) == 0 else a.unsqueeze(0)
    b = None if b is None or len(b) == 0 else b.unsqueeze(0)
    warm = None if warmstart is None else (warmstart[0].unsqueeze(0), warmstart[1].unsqueeze(0))
    kw = dict(reg=reg, method=method, num_iter_max=numItermax, stop_thr=stopThr, warmstart=warm, **params)
    if cost:
        loss, T, log_u, log_v, alpha, beta, info, errs, extra = ot_ops.sinkhorn_ext_loss(M.unsqueeze(0), a, b, return_plan=True, **kw)
    else:
        T, loss, log_u, log_v, alpha, beta, info, errs, extra = ot_ops.sinkhorn_ext_batched(M.unsqueeze(0), a, b, **kw)
    res = loss[0] if cost else T[0]
    niter, flags, nchk, last = info[0].tolist()
    if method == "sinkhorn_epsilon_scaling":
        _sweeps, _nabs, nan_exits, nan_iter = extra[0].tolist()
        if nan_exits:
            warnings.warn("Numerical errors at iteration %d" % nan_iter)
        if last:                                                           # inner solves that ran to numInnerItermax (the reference calls them with warn=True)
            warnings.warn(_NOT_CONVERGED)
        if not flags & 1 and warn:
            warnings.warn(_NOT_CONVERGED)
    elif flags & 2:
        warnings.warn("Numerical errors at iteration %d" % niter)
    elif not flags & 1 and warn:
        warnings.warn(_NOT_CONVERGED)
    if not log:
        return res
    if method == "greenkhorn":
        return res, {"n_iter": niter, "u": torch.exp(log_u[0]), "v": torch.exp(log_v[0])}
    al, be = alpha[0], beta[0]
    log_ = {"err": [errs[0, i] for i in range(nchk)], "alpha": al, "beta": be, "warmstart": (al, be)}
    if method == "sinkhorn_stabilized":
        log_.update(n_iter=niter, logu=log_u[0], logv=log_v[0])
    else:
        log_["niter"] = niter
    return res, log_


def greenkhorn(a, b, M, reg, numItermax=10000, stopThr=1e-9, verbose=False, log=False, warn=True, warmstart=None):
    """The reference's greenkhorn (sinkhorn.py:453-532; Altschuler et al. 2017): T [n1,n2]; log=True: (T, {"n_iter", "u", "v"}).
    warmstart = (log u, log v)."""
    return _solve_ext(a, b, M, reg, "greenkhorn", numItermax, stopThr, log, warn, warmstart)


def sinkhorn_stabilized(a, b, M, reg, numItermax=1000, tau=1e3, stopThr=1e-9, warmstart=None, verbose=False, print_period=20, log=False, warn=True,
                        **kwargs):
    """The reference's sinkhorn_stabilized (sinkhorn.py:535-685; Schmitzer 2016) for a 1-D b: T [n1,n2]; log=True: (T, {"err", "n_iter", "logu",
    "logv", "alpha", "beta", "warmstart"}).  warmstart = (alpha, beta) in cost units.  The NaN exit (previous u, v returned, "Numerical errors at
    iteration %d") is decided on fp64 values."""
    _check_grad(kwargs.get("grad", "plan"), "sinkhorn_stabilized")        # (the signature stays the reference's: grad arrives in **kwargs)
    return _solve_ext(a, b, M, reg, "sinkhorn_stabilized", numItermax, stopThr, log, warn, warmstart, tau=tau, print_period=print_period)


def sinkhorn_epsilon_scaling(a, b, M, reg, numItermax=100, epsilon0=1e4, numInnerItermax=100, tau=1e3, stopThr=1e-9, warmstart=None, verbose=False,
                             print_period=10, log=False, warn=True, **kwargs):
    """The reference's sinkhorn_epsilon_scaling (sinkhorn.py:688-786): T [n1,n2]; log=True: (T, {"err", "alpha", "beta", "warmstart", "niter"}).
    The whole outer loop runs inside one launch.  warmstart = (alpha, beta) in cost units; numItermax is raised to 35 as in the reference."""
    _check_grad(kwargs.get("grad", "plan"), "sinkhorn_epsilon_scaling")
    return _solve_ext(a, b, M, reg, "sinkhorn_epsilon_scaling", numItermax, stopThr, log, warn, warmstart, tau=tau, print_period=print_period,
                      epsilon0=epsilon0, num_inner_iter_max=numInnerItermax)


def sinkhorn(a, b, M, reg, method="sinkhorn_log", numItermax=100, stopThr=1e-5, verbose=False, log=False, warn=True, warmstart=None, grad="plan",
             **kwargs):
    """The reference's sinkhorn (sinkhorn.py:6-91): the entropic OT plan between the histograms a [n1] and b [n2] (empty: uniform) for the cost
    M [n1,n2], by method "sinkhorn_log", "sinkhorn" (Knopp), "greenkhorn", "sinkhorn_stabilized" or "sinkhorn_epsilon_scaling" (the last two take
    tau, print_period, and epsilon0, numInnerItermax, through **kwargs).  warmstart and grad ("plan" / "unrolled"): see the module docstring,
    also for the deviations."""
    m = str(method).lower()
    _check_grad(grad, m if m in ot_ops.SINKHORN_EXT_METHODS else None)
    if m == "greenkhorn":                                                  # (the reference hands greenkhorn no **kwargs)
        return greenkhorn(a, b, M, reg, numItermax=numItermax, stopThr=stopThr, log=log, warn=warn, warmstart=warmstart)
    if m == "sinkhorn_stabilized":
        return sinkhorn_stabilized(a, b, M, reg, numItermax=numItermax, stopThr=stopThr, warmstart=warmstart, log=log, warn=warn, **kwargs)
    if m == "sinkhorn_epsilon_scaling":
        return sinkhorn_epsilon_scaling(a, b, M, reg, numItermax=numItermax, stopThr=stopThr, warmstart=warmstart, log=log, warn=warn, **kwargs)
    if m not in ot_ops.SINKHORN_METHODS:
        raise ValueError("Unknown method '%s'." % method)
    return _solve(a, b, M, reg, m, numItermax, stopThr, log, warn, warmstart, grad=grad)


def sinkhorn2(a, b, M, reg, method="sinkhorn", numItermax=1000, stopThr=1e-9, verbose=False, log=False, warn=False, warmstart=None, grad="plan",
              **kwargs):
    """The reference's sinkhorn2 (sinkhorn.py:94-204): the transport cost sum(M * T) of the entropic plan as a 0-d tensor (log=True: with the
    solver's log).  grad="plan": it carries the gradient dM = T at the returned plan, held constant; a and b get none.  grad="unrolled": the
    reference's gradient through the sweeps to M, a, b and warmstart[0].  b [n2,H]: the H costs [H] (module docstring), grad="plan" only."""
    m = str(method).lower()
    _check_grad(grad, m if m == "sinkhorn_stabilized" else None)
    if m == "sinkhorn_stabilized":
        return _solve_ext(a, b, M, reg, m, numItermax, stopThr, log, warn, warmstart, cost=True, tau=kwargs.get("tau", 1e3),
                          print_period=kwargs.get("print_period", 20))
    if m not in ot_ops.SINKHORN_METHODS:                                      # (the reference's sinkhorn2 knows neither greenkhorn nor epsilon scaling)
        raise ValueError("Unknown method '%s'." % method)
    return _solve(a, b, M, reg, m, numItermax, stopThr, log, warn, warmstart, cost=True, grad=grad)


def wasserstein_pairwise_distances(Ys: Sequence[Tensor], ps=None, reg=0.1, method="sinkhorn_log", numItermax=100, stopThr=1e-5,
                                   grad="plan") -> Tensor:
    """The entropic Wasserstein cost matrix of G feature clouds (the conformers of an ensemble), the structure-free (alpha = 0) sibling of
    fgw.fgw_pairwise_distances: Ys[g] [n_g,d], ps[g] weights or None (uniform) -> [G,G], symmetric with a zero diagonal.  The G (G - 1) / 2 pairs
    a < b are solved in ONE launch (per-problem sizes when the clouds differ in size) with M = fgw.feature_cost(Ys[a], Ys[b]); entry (a, b) is
    sinkhorn2(ps[a], ps[b], M, reg, method=method, numItermax=numItermax, stopThr=stopThr), bit for bit.  When any of Ys requires grad the result
    carries gradients to them: sinkhorn2's fixed-plan gradient to every M, and torch's through feature_cost; ps get none.  grad="unrolled":
    sinkhorn2's unrolled gradient instead, to every M and to ps."""
    _check_grad(grad)
    G = len(Ys)
    if ps is not None and len(ps) != G:
        raise ValueError("Ys and ps must have one entry per cloud")
    m = str(method).lower()
    if m not in ot_ops.SINKHORN_METHODS:
        raise ValueError("Unknown method '%s'." % method)
    if not all(torch.is_tensor(t) and t.is_cuda for t in Ys):
        raise NotImplementedError("wasserstein_pairwise_distances runs on the GPU only: pass CUDA (ROCm) tensors")
    Ys = [y.to(torch.float32) for y in Ys]
    out = torch.zeros(G, G, dtype=torch.float32, device=Ys[0].device)
    ia, ib = torch.triu_indices(G, G, 1).tolist() if G > 1 else ([], [])
    if not ia:
        return out
    Ms = [feature_cost(Ys[i], Ys[j]) for i, j in zip(ia, ib)]
    pick = lambda idx: None if ps is None else [ps[i] for i in idx]
    kw = dict(reg=reg, method=m, num_iter_max=numItermax, stop_thr=stopThr, grad=grad)
    unrolled = grad == "unrolled"
    if len({int(y.shape[0]) for y in Ys}) == 1:
        st = lambda ts: None if ts is None else torch.stack([(t if unrolled else t.detach()).to(torch.float32) for t in ts])
        cost = ot_ops.sinkhorn_loss(torch.stack(Ms), st(pick(ia)), st(pick(ib)), **kw)
    else:
        M, a, b, _w, n1, n2, _sizes = ot_ops._sinkhorn_list_stack(Ms, pick(ia), pick(ib), None, None, keep_graph=True, keep_vec_graph=unrolled)
        cost = ot_ops.sinkhorn_loss(M, a, b, n1=n1, n2=n2, **kw)
    out[ia, ib] = cost
    out[ib, ia] = cost
    return out
