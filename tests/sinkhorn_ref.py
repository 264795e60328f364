"""fp64 restatement on the CPU of the two Sinkhorn iterations that conan_fgw_amd.sinkhorn runs on the GPU, written from the algorithm (Cuturi 2013;
the log-domain form of Peyre & Cuturi, Computational Optimal Transport, 4.4) with the stopping rule of the reference's fgw/sinkhorn.py.  It is the
yardstick of the GPU tests where no stored fixture exists; tests/test_sinkhorn_cpu.py holds it to every fixture's fp64 run.

    sinkhorn_ref(a, b, M, reg, method, numItermax, stopThr, warmstart=None) -> (T, log)

log = {"err": [floats], "niter": int, "log_u", "log_v", "u", "v", "warn": "" | "noconv" | "numerr", "loss": float}."""
import torch

f64 = torch.float64


def sinkhorn_ref(a, b, M, reg, method="sinkhorn_log", numItermax=1000, stopThr=1e-9, warmstart=None):
    M = torch.as_tensor(M).to(f64)
    n1, n2 = M.shape
    a = torch.full((n1,), 1.0 / n1, dtype=f64) if a is None or len(a) == 0 else torch.as_tensor(a).to(f64)
    b = torch.full((n2,), 1.0 / n2, dtype=f64) if b is None or len(b) == 0 else torch.as_tensor(b).to(f64)
    warm = None if warmstart is None else tuple(torch.as_tensor(w).to(f64) for w in warmstart)
    errs, warn, ii = [], "", 0
    if method == "sinkhorn_log":
        Mr = -M / reg
        f, g = (torch.zeros(n1, dtype=f64), torch.zeros(n2, dtype=f64)) if warm is None else warm
        la, lb = torch.log(a), torch.log(b)
        plan = lambda: torch.exp(Mr + f[:, None] + g[None, :])
        stopped = False
        for ii in range(numItermax):
            g = lb - torch.logsumexp(Mr + f[:, None], dim=0)
            f = la - torch.logsumexp(Mr + g[None, :], dim=1)
            if ii % 10 == 0:
                err = float(torch.linalg.vector_norm(plan().sum(0) - b))
                errs.append(err)
                if err < stopThr:
                    stopped = True
                    break
        if not stopped:
            warn = "noconv"
        T = plan()
        log_u, log_v = f, g
    elif method == "sinkhorn":
        K = torch.exp(M / (-reg))
        u, v = (torch.full((n1,), 1.0 / n1, dtype=f64), torch.full((n2,), 1.0 / n2, dtype=f64)) if warm is None else (torch.exp(warm[0]), torch.exp(warm[1]))
        Ka = (1.0 / a)[:, None] * K          # (a zero weight: an infinite row, u_i = 0)
        left = False
        for ii in range(numItermax):
            pu, pv = u, v
            ktu = K.T @ u
            v = b / ktu
            u = 1.0 / (Ka @ v)
            if bool((ktu == 0).any()) or not bool(torch.isfinite(u).all()) or not bool(torch.isfinite(v).all()):
                u, v, warn, left = pu, pv, "numerr", True
                break
            if ii % 10 == 0:
                err = float(torch.linalg.vector_norm(torch.einsum("i,ij,j->j", u, K, v) - b))      # the column marginal of diag(u) K diag(v)
                errs.append(err)
                if err < stopThr:
                    left = True
                    break
        if not left:
            warn = "noconv"
        T = u[:, None] * K * v[None, :]
        log_u, log_v = torch.log(u), torch.log(v)
    else:
        raise ValueError("Unknown method '%s'." % method)
    return T, {"err": errs, "niter": ii, "log_u": log_u, "log_v": log_v, "u": torch.exp(log_u), "v": torch.exp(log_v), "warn": warn,
               "loss": float((M * T).sum())}


def fair(errs, niter, numItermax, stopThr, warn=""):
    """The condition under which an iteration count can be compared between two implementations: no check sits near the threshold."""
    if warn == "numerr":
        return True
    if not errs:
        return False
    if errs[-1] < stopThr:
        return errs[-1] <= 0.6 * stopThr and all(e >= 1.5 * stopThr for e in errs[:-1])
    return errs[-1] >= 1.5 * stopThr
