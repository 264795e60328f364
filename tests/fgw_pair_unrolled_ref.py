"""fp64 restatement, in plain torch on the CPU, of what conan_fgw_pair_bwd computes (csrc/fgw_pair_grad.hip): the PGD / PPA outer iterations of
the reference's fgw_projected (bregman.py:70-167) around sinkhorn_log (sinkhorn.py:388-450) run again with every iteration's input plan and
sweep count recorded, then the reverse walk written out by hand, no autograd.  tests/test_fgw_pair_unrolled_cpu.py holds it to torch autograd
through the reference's own fgw (tests/golden/fgw_unrollgrad_*.npz) at 1e-9 and to a central finite difference; the GPU tests use it where no
fixture exists (residency, ragged batches).

Sinkhorn runs in its scaling form (u = exp f, v = exp g, K = exp(Mr - column maximum)): every term of the walk is u_i K_ij v_j, which does
not depend on the gauge.  The project's conventions, massless rule included: an entry whose row or column has no mass (p_i = 0 or q_j = 0) is
exactly zero in every plan, never enters a sum and is a constant of the solve: the cotangent is held at zero there, and dp_i / dq_j of such a
node is 0.  The distance is the reference's log["fgw_dist"], always from the untransposed init_matrix (bregman.py:164)."""
import numpy as np
import torch

from fgw_acc_grad_ref import F64, grad_error  # noqa: F401  (grad_error: the project's yardstick, re-exported)

ZERO = torch.zeros((), dtype=F64)


def _t(x):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(F64)


def is_symmetric(C1, C2):
    """symmetric=None: the reference's torch.allclose(C, C.T, atol=1e-10) on both structures."""
    return bool(torch.allclose(C1, C1.T, atol=1e-10) and torch.allclose(C2, C2.T, atol=1e-10))


def _consts(C1, C2, p, q, alpha, sym):
    """The T-independent part of tens without (1 - alpha) M: 2 alpha (c 1^T + 1 r^T), or alpha ((c + c') 1^T + 1 (r + r')^T)."""
    c, r = (C1 * C1) @ p, (C2 * C2) @ q
    if sym:
        return 2 * alpha * (c[:, None] + r[None, :])
    ct, rt = (C1 * C1).T @ p, (C2 * C2).T @ q
    return alpha * ((c + ct)[:, None] + (r + rt)[None, :])


def _tens(M, C1, C2, T, const, alpha, eps, sym, ppa, live):
    if sym:
        tens = const - 4 * alpha * (C1 @ T @ C2.T) + (1 - alpha) * M
    else:
        tens = const - 2 * alpha * (C1 @ T @ C2.T + C1.T @ T @ C2) + (1 - alpha) * M
    if ppa:
        tens = tens - eps * torch.log(torch.where(live, T, torch.ones((), dtype=F64)))
    return tens


def _kernel(tens, eps, live):
    Mr = torch.where(live, -tens / eps, torch.full((), -np.inf, dtype=F64))
    ref = Mr.max(0).values
    ref = torch.where(torch.isfinite(ref), ref, ZERO)
    return torch.where(live, torch.exp(Mr - ref[None, :]), ZERO)


def sinkhorn_sweeps(K, p, q, num_iter_max, stop_thr, fixed=None):
    """sinkhorn_log's loop from zero potentials (sinkhorn.py:413-433) -> (us, vs): u^0 .. u^S, v^0 .. v^S (v^0 is never read).  The error is
    evaluated where ii % 10 == 0 and the loop leaves below stop_thr; fixed: a sweep count that replaces the decision."""
    u = torch.where(p > 0, torch.ones((), dtype=F64), ZERO)
    v = torch.zeros_like(q)
    us, vs = [u], [v]
    for ii in range(num_iter_max if fixed is None else fixed):
        s = K.T @ u
        v = torch.where(q > 0, q / torch.where(q > 0, s, torch.ones((), dtype=F64)), ZERO)
        s = K @ v
        u = torch.where(p > 0, p / torch.where(p > 0, s, torch.ones((), dtype=F64)), ZERO)
        us.append(u); vs.append(v)
        if fixed is None and ii % 10 == 0:
            if float(torch.linalg.norm(v * (K.T @ u) - q)) < stop_thr:
                break
    return us, vs


def pair_forward(M, C1, C2, p, q, G0, *, alpha, epsilon, solver, sym, iters, num_iter_max, stop_thr, sweeps=None, record=None):
    """`iters` outer iterations, no outer stop test -> the final plan (fp64 tensors in, tensor out).  sweeps: per-iteration sweep counts held
    fixed (else decided by sinkhorn_log's rule); record: a list that receives (T_k, S_k) of every iteration."""
    live = (p[:, None] > 0) & (q[None, :] > 0)
    T = torch.where(live, p[:, None] * q[None, :] if G0 is None else G0, ZERO)
    const = _consts(C1, C2, p, q, alpha, sym)
    for k in range(iters):
        K = _kernel(_tens(M, C1, C2, T, const, alpha, epsilon, sym, solver == "PPA", live), epsilon, live)
        us, vs = sinkhorn_sweeps(K, p, q, num_iter_max, stop_thr, None if sweeps is None else int(sweeps[k]))
        if record is not None:
            record.append((T, len(us) - 1))
        T = us[-1][:, None] * K * vs[-1][None, :]
    return T


def pair_distance(M, C1, C2, p, q, T, alpha):
    const = ((C1 * C1) @ p)[:, None] + ((C2 * C2) @ q)[None, :]
    return (1 - alpha) * (M * T).sum() + alpha * ((const - 2 * (C1 @ T @ C2.T)) * T).sum()


def pair_grad_ref(M, C1, C2, p=None, q=None, G0=None, *, alpha, epsilon, solver="PGD", symmetric=True, iters, num_iter_max, stop_thr, sweeps=None,
                  dT=None, ddist=None):
    """The gradients of sum(dT o T) + ddist * fgw_dist(T) for one pair after `iters` executed outer iterations, as fp64 numpy arrays: T, dist,
    sweeps (the S_k), dM, dC1, dC2, dp, dq, dG0 (None without G0).  p / q None: uniform (their gradients are still returned)."""
    M, C1, C2, G0, dT = _t(M), _t(C1), _t(C2), _t(G0), _t(dT)
    n1, n2 = M.shape
    p = torch.full((n1,), 1.0 / n1, dtype=F64) if p is None else _t(p)
    q = torch.full((n2,), 1.0 / n2, dtype=F64) if q is None else _t(q)
    alpha, eps, om = float(alpha), float(epsilon), 1.0 - float(alpha)
    sym = is_symmetric(C1, C2) if symmetric is None else bool(symmetric)
    ppa = solver == "PPA"
    live = (p[:, None] > 0) & (q[None, :] > 0)
    one = torch.ones((), dtype=F64)
    rec = []
    T = pair_forward(M, C1, C2, p, q, G0, alpha=alpha, epsilon=eps, solver=solver, sym=sym, iters=iters, num_iter_max=num_iter_max,
                     stop_thr=stop_thr, sweeps=sweeps, record=rec)
    dist = pair_distance(M, C1, C2, p, q, T, alpha)
    const = _consts(C1, C2, p, q, alpha, sym)

    Gb = torch.zeros_like(M) if dT is None else dT.clone()
    dM, dC1, dC2, dp, dq = torch.zeros_like(M), torch.zeros_like(C1), torch.zeros_like(C2), torch.zeros_like(p), torch.zeros_like(q)
    if ddist is not None:                                                 # the seed and the direct partials of fgw_dist at the final plan
        dd = float(ddist)
        r, c = T.sum(1), T.sum(0)
        cc = ((C1 * C1) @ p)[:, None] + ((C2 * C2) @ q)[None, :]
        Gb = Gb + dd * (om * M + alpha * cc - 2 * alpha * (C1 @ T @ C2.T + C1.T @ T @ C2))
        dM = dd * om * T
        dC1 = dd * alpha * 2 * (C1 * (r[:, None] * p[None, :]) - T @ C2 @ T.T)
        dC2 = dd * alpha * 2 * (C2 * (c[:, None] * q[None, :]) - T.T @ C1 @ T)
        dp = dd * alpha * ((C1 * C1).T @ r)
        dq = dd * alpha * ((C2 * C2).T @ c)
    Gb = torch.where(live, Gb, ZERO)

    for T_k, S in reversed(rec):
        K = _kernel(_tens(M, C1, C2, T_k, const, alpha, eps, sym, ppa, live), eps, live)
        us, vs = sinkhorn_sweeps(K, p, q, num_iter_max, stop_thr, S)
        # the Sinkhorn reverse walk (csrc/sinkhorn_grad.hip) with plan cotangent Gb and loss cotangent 0
        Tn = us[S][:, None] * K * vs[S][None, :]
        fb, gb = (Gb * Tn).sum(1), (Gb * Tn).sum(0)
        la, lb, acc = torch.zeros_like(p), torch.zeros_like(q), torch.zeros_like(M)
        for t in range(S, 0, -1):
            z = torch.where(p > 0, fb * us[t] / torch.where(p > 0, p, one), ZERO)
            la = la + fb
            gb = gb - vs[t] * (K.T @ z)
            w = torch.where(q > 0, gb * vs[t] / torch.where(q > 0, q, one), ZERO)
            lb = lb + gb
            fb = -us[t - 1] * (K @ w)
            gb = torch.zeros_like(gb)
            acc = acc + z[:, None] * vs[t][None, :] + us[t - 1][:, None] * w[None, :]
        D = -(Gb * Tn - K * acc) / eps                                    # d tens
        dp = dp + torch.where(p > 0, la / torch.where(p > 0, p, one), ZERO)
        dq = dq + torch.where(q > 0, lb / torch.where(q > 0, q, one), ZERO)
        rho, kap = D.sum(1), D.sum(0)
        dM = dM + om * D
        if sym:
            dC1 = dC1 + 4 * alpha * (C1 * (rho[:, None] * p[None, :])) - 4 * alpha * D @ C2 @ T_k.T
            dC2 = dC2 + 4 * alpha * (C2 * (kap[:, None] * q[None, :])) - 4 * alpha * D.T @ C1 @ T_k
            dp = dp + 2 * alpha * ((C1 * C1).T @ rho)
            dq = dq + 2 * alpha * ((C2 * C2).T @ kap)
            Gn = -4 * alpha * C1.T @ D @ C2
        else:
            dC1 = dC1 + 2 * alpha * C1 * (rho[:, None] * p[None, :] + p[:, None] * rho[None, :]) - 2 * alpha * (D @ C2 @ T_k.T + T_k @ C2 @ D.T)
            dC2 = dC2 + 2 * alpha * C2 * (kap[:, None] * q[None, :] + q[:, None] * kap[None, :]) - 2 * alpha * (D.T @ C1 @ T_k + T_k.T @ C1 @ D)
            dp = dp + alpha * ((C1 * C1).T @ rho + (C1 * C1) @ rho)
            dq = dq + alpha * ((C2 * C2).T @ kap + (C2 * C2) @ kap)
            Gn = -2 * alpha * (C1.T @ D @ C2 + C1 @ D @ C2.T)
        if ppa:
            Gn = Gn - eps * D / torch.where(live, T_k, one)
        Gb = torch.where(live, Gn, ZERO)

    dG0 = None
    if G0 is None:
        dp, dq = dp + Gb @ q, dq + Gb.T @ p
    else:
        dG0 = Gb
    dp, dq = torch.where(p > 0, dp, ZERO), torch.where(q > 0, dq, ZERO)
    pp, qq = (p[:, None] > 0) & (p[None, :] > 0), (q[:, None] > 0) & (q[None, :] > 0)
    out = dict(T=T, dist=dist, dM=torch.where(live, dM, ZERO), dC1=torch.where(pp, dC1, ZERO), dC2=torch.where(qq, dC2, ZERO), dp=dp, dq=dq, dG0=dG0)
    out = {k: (None if v is None else v.numpy()) for k, v in out.items()}
    # PPA takes the logarithm of every input plan: an exact zero at an entry with mass is the reference's NaN in every gradient (flags bit 2)
    out["nan"] = bool(ppa and any(bool(((T_k == 0) & live).any()) for T_k, _ in rec)) or not all(np.isfinite(v).all() for v in out.values() if v is not None)
    if out["nan"]:
        for k in ("dM", "dC1", "dC2", "dp", "dq", "dG0"):
            if out[k] is not None:
                out[k] = np.full_like(out[k], np.nan)
    out["sweeps"] = np.array([s for _, s in rec], dtype=np.int32)
    return out
