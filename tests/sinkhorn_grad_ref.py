"""fp64 numpy restatement of the gradient through the unrolled Sinkhorn sweeps (csrc/sinkhorn_grad.hip, ops.sinkhorn_unrolled), in log-domain
form, written from the chain rule of the iteration

    g^t = log b - LSE_i(Mr + f^(t-1)),   f^t = log a - LSE_j(Mr + g^t),   t = 1..S,   Mr = -M / reg,   T = exp(Mr + f^S + g^S)

which both "sinkhorn_log" and "sinkhorn" (Knopp, f = log u, g = log v) are.  Test infrastructure: tests/test_sinkhorn_grad_cpu.py holds it to
the stored autograd runs of the reference (tests/golden/grad_sinkhorn_*.npz); the GPU tests use it where no fixture exists.

    sinkhorn_grad_ref(a, b, M, reg, S, method, warmstart=None, gl=1.0, dT=None) -> dict(T, dM, da, db, dwu)

the gradients of  gl * sum(M * T) + sum(dT * T)  after S sweeps.  A zero weight a_i (b_j) is skipped: it contributes nothing and its own
gradient is 0 (the reference gives NaN there).  sweeps_of(niter, numerr) is the number of sweeps behind a reference run's log["niter"]."""
import numpy as np


def sweeps_of(niter, numerr=False):
    """The loop index at exit is niter: a break at a check or the end of the loop has executed niter + 1 sweeps; Knopp's numerical-errors exit
    restores the previous u, v: niter sweeps."""
    return int(niter) + (0 if numerr else 1)


def _lse(x, axis):
    mx = np.max(x, axis=axis, keepdims=True)
    mx = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide="ignore"):
        return np.log(np.sum(np.exp(x - mx), axis=axis)) + np.squeeze(mx, axis=axis)


def sinkhorn_grad_ref(a, b, M, reg, S, method="sinkhorn_log", warmstart=None, gl=1.0, dT=None):
    M = np.asarray(M, dtype=np.float64)
    n1, n2 = M.shape
    a = np.full(n1, 1.0 / n1) if a is None else np.asarray(a, dtype=np.float64)
    b = np.full(n2, 1.0 / n2) if b is None else np.asarray(b, dtype=np.float64)
    dT = np.zeros_like(M) if dT is None else np.asarray(dT, dtype=np.float64)
    reg = float(reg)
    Mr = -M / reg
    with np.errstate(divide="ignore"):
        la, lb = np.log(a), np.log(b)
    if warmstart is not None:
        f0, g0 = (np.asarray(w, dtype=np.float64) for w in warmstart)
    elif method == "sinkhorn":
        f0, g0 = np.full(n1, -np.log(n1)), np.full(n2, -np.log(n2))
    else:
        f0, g0 = np.zeros(n1), np.zeros(n2)
    F, G = [f0], [g0]
    for _ in range(S):
        g = lb - _lse(Mr + F[-1][:, None], 0)
        F.append(la - _lse(Mr + g[None, :], 1))
        G.append(g)
    T = np.exp(Mr + F[S][:, None] + G[S][None, :])
    Tb = gl * M + dT
    fb, gb = (Tb * T).sum(1), (Tb * T).sum(0)
    lab, lbb, acc = np.zeros(n1), np.zeros(n2), np.zeros_like(M)
    ok_a, ok_b = a > 0, b > 0
    for t in range(S, 0, -1):
        E = np.exp(Mr + F[t][:, None] + G[t][None, :])                    # row pass t: softmax_j of row i is E_ij / a_i
        z = np.where(ok_a, fb / np.where(ok_a, a, 1.0), 0.0)
        lab += fb
        gb = gb - E.T @ z
        acc += z[:, None] * E
        fb = np.zeros(n1)
        E = np.exp(Mr + F[t - 1][:, None] + G[t][None, :])                # column pass t: softmax_i of column j is E_ij / b_j
        w = np.where(ok_b, gb / np.where(ok_b, b, 1.0), 0.0)
        lbb += gb
        fb = fb - E @ w
        acc += E * w[None, :]
        gb = np.zeros(n2)
    dMr = -acc + Tb * T
    return dict(T=T, dM=gl * T - dMr / reg, da=np.where(ok_a, lab / np.where(ok_a, a, 1.0), 0.0),
                db=np.where(ok_b, lbb / np.where(ok_b, b, 1.0), 0.0), dwu=fb)
