"""fp64 restatement, in plain torch on the CPU, of what conan_fgw_bregman_bwd computes (csrc/fgw_bregman_grad.hip): the Bregman half-steps of the
reference's fgw_bregman (bregman.py:170-279) run again with every half-step's input plan recorded, then the reverse walk written out by hand,
no autograd.  tests/test_fgw_bregman_unrolled_cpu.py holds it to torch autograd through the reference's own fgw_bregman
(tests/golden/fgw_bregman_unrollgrad_*.npz) at 1e-9; the GPU tests use it where no fixture exists (residency, ragged batches).

The project's conventions, massless rule included: an entry whose row or column has no mass (p_i = 0 or q_j = 0) is exactly zero in every plan,
its scaling factor is 0, the cotangent is held at zero there, and dp_i / dq_j of such a node is 0.  The distance is the reference's
log["fgw_dist"], always from the untransposed init_matrix (bregman.py:272)."""
import numpy as np
import torch

from fgw_acc_grad_ref import F64, grad_error  # noqa: F401  (grad_error: the project's yardstick, re-exported)
from fgw_pair_unrolled_ref import is_symmetric  # noqa: F401

ZERO = torch.zeros((), dtype=F64)
TINY = 1e-15


def _t(x):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(F64)


def _loss(C1, C2, kl):
    """f1(C1), f1'(C1), f2(C2), f2'(C2), h(C2), h'(C2) of init_matrix."""
    if kl:
        return C1 * torch.log(C1 + TINY) - C1, torch.log(C1 + TINY) + C1 / (C1 + TINY) - 1, C2, torch.ones_like(C2), torch.log(C2 + TINY), 1 / (C2 + TINY)
    return C1 * C1, 2 * C1, C2 * C2, 2 * C2, 2 * C2, torch.full_like(C2, 2.0)


def _half(M, C1, h, T, m, col, alpha, eps, sym, live):
    """One half-step with input plan T -> X, E, s, scaling, T'."""
    if sym:
        df = -2 * alpha * (C1 @ T @ h.T) + (1 - alpha) * M
    else:
        df = -alpha * (C1 @ T @ h.T + C1.T @ T @ h) + (1 - alpha) * M
    X = torch.where(live, torch.exp(-df / eps), ZERO)
    E = T * X
    s = E.sum(0 if col else 1)
    sc = torch.where(m > 0, m / s, ZERO)
    return X, E, s, sc, (E * sc[None, :] if col else sc[:, None] * E)


def distance(M, C1, C2, p, q, T, alpha, kl):
    f1, _, f2, _, h, _ = _loss(C1, C2, kl)
    constC = (f1 @ p)[:, None] + (f2 @ q)[None, :]
    return (1 - alpha) * (M * T).sum() + alpha * ((constC - C1 @ T @ h.T) * T).sum()


def unrolled(M, C1, C2, p, q, G0=None, *, alpha, epsilon, iters, loss_fun="square_loss", symmetric=True, dT=None, ddist=None):
    """The replay of `iters` iterations and the reverse walk -> dict(T, dist, dM, dC1, dC2, dp, dq, dG0 (None without a start), flagged).
    symmetric None: the reference's allclose decision."""
    M, C1, C2, p, q, G0, dT = (_t(x) for x in (M, C1, C2, p, q, G0, dT))
    kl = loss_fun == "kl_loss"
    sym = is_symmetric(C1, C2) if symmetric is None else bool(symmetric)
    f1, f1d, f2, f2d, h, hd = _loss(C1, C2, kl)
    live = (p[:, None] > 0) & (q[None, :] > 0)
    T = torch.where(live, G0 if G0 is not None else p[:, None] * q[None, :], ZERO)
    rec, flagged = [], False
    for k in range(2 * iters):
        col = bool(k & 1)
        m = q if col else p
        rec.append(T)
        _, _, s, _, T = _half(M, C1, h, T, m, col, alpha, epsilon, sym, live)
        if bool(((m > 0) & ~(s > 0)).any()) or not bool(torch.isfinite(T).all()):
            flagged = True
    out = dict(T=T.numpy(), flagged=flagged)
    if flagged:
        return out
    out["dist"] = float(distance(M, C1, C2, p, q, T, alpha, kl))
    dd = 0.0 if ddist is None else float(ddist)
    r, c = T.sum(1), T.sum(0)
    constC = (f1 @ p)[:, None] + (f2 @ q)[None, :]
    Gb = (ZERO.expand_as(T) if dT is None else dT) + dd * ((1 - alpha) * M + alpha * (constC - C1 @ T @ h.T - C1.T @ T @ h))
    Gb = torch.where(live, Gb, ZERO)
    dM = dd * (1 - alpha) * T
    dC1 = dd * alpha * (f1d * r[:, None] * p[None, :] - T @ h @ T.T)
    dC2 = dd * alpha * (f2d * c[:, None] * q[None, :] - hd * (T.T @ C1 @ T))
    dp, dq = dd * alpha * (f1.T @ r), dd * alpha * (f2.T @ c)
    for k in range(2 * iters - 1, -1, -1):
        col = bool(k & 1)
        m, Tk = (q if col else p), rec[k]
        X, E, s, sc, Tn = _half(M, C1, h, Tk, m, col, alpha, epsilon, sym, live)
        g = (Gb * Tn).sum(0 if col else 1)
        dm = torch.where(m > 0, g / torch.where(m > 0, m, ZERO + 1), ZERO)
        gs = torch.where(m > 0, g / torch.where(m > 0, s, ZERO + 1), ZERO)
        if col:
            dq = dq + dm
            dE = Gb * sc[None, :] - gs[None, :]
        else:
            dp = dp + dm
            dE = Gb * sc[:, None] - gs[:, None]
        dE = torch.where(live, dE, ZERO)
        D = -dE * E / epsilon
        dM = dM + (1 - alpha) * D
        if sym:
            dC1 = dC1 - 2 * alpha * (D @ h @ Tk.T)
            dh = -2 * alpha * (D.T @ C1 @ Tk)
            Gb = dE * X - 2 * alpha * (C1.T @ D @ h)
        else:
            dC1 = dC1 - alpha * (D @ h @ Tk.T + Tk @ h @ D.T)
            dh = -alpha * (D.T @ C1 @ Tk + Tk.T @ C1 @ D)
            Gb = dE * X - alpha * (C1.T @ D @ h + C1 @ D @ h.T)
        Gb = torch.where(live, Gb, ZERO)
        dC2 = dC2 + hd * dh
    if G0 is None:
        dp, dq = dp + Gb @ q, dq + Gb.T @ p
    pp, qq = (p[:, None] > 0) & (p[None, :] > 0), (q[:, None] > 0) & (q[None, :] > 0)
    out.update(dM=torch.where(live, dM, ZERO).numpy(), dC1=torch.where(pp, dC1, ZERO).numpy(), dC2=torch.where(qq, dC2, ZERO).numpy(),
               dp=torch.where(p > 0, dp, ZERO).numpy(), dq=torch.where(q > 0, dq, ZERO).numpy(),
               dG0=None if G0 is None else torch.where(live, Gb, ZERO).numpy())
    return out


def fixed_plan(M, C1, C2, p, q, T, *, alpha, loss_fun="square_loss"):
    """The gradient of fgw_dist at the plan T HELD CONSTANT (fgw_distance's convention) -> dict(dM, dC1, dC2, dp, dq)."""
    M, C1, C2, p, q, T = (_t(x) for x in (M, C1, C2, p, q, T))
    f1, f1d, f2, f2d, h, hd = _loss(C1, C2, loss_fun == "kl_loss")
    r, c = T.sum(1), T.sum(0)
    return dict(dM=((1 - alpha) * T).numpy(), dC1=(alpha * (f1d * r[:, None] * p[None, :] - T @ h @ T.T)).numpy(),
                dC2=(alpha * (f2d * c[:, None] * q[None, :] - hd * (T.T @ C1 @ T))).numpy(), dp=(alpha * (f1.T @ r)).numpy(), dq=(alpha * (f2.T @ c)).numpy())
