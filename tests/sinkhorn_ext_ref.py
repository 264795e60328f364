"""fp64 restatement on the CPU of the three solvers that csrc/sinkhorn_ext.hip runs on the GPU, written from the algorithms: Greenkhorn (Altschuler,
Weed & Rigollet 2017: greedy coordinate updates of the scalings on the row or column whose marginal is violated most) and the stabilized scaling
iteration with absorption of large scalings into the dual potentials, alone and under epsilon scaling (Schmitzer 2016), each with the stopping
rules of the reference's fgw/sinkhorn.py.  It is the yardstick of the GPU tests where no stored fixture exists; tests/test_sinkhorn_ext_cpu.py
holds it to every fixture's fp64 run.  Besides the results it reports what decides whether counts can be compared between two implementations:
absorption counts, Greenkhorn's stopping value at every step and the relative gap of every arg-max it took.

    greenkhorn_ref(a, b, M, reg, numItermax, stopThr, warmstart)                       -> (T, log)
    stabilized_ref(a, b, M, reg, numItermax, tau, stopThr, warmstart, print_period)    -> (T, log)
    epsilon_scaling_ref(a, b, M, reg, numItermax, epsilon0, numInnerItermax, tau, stopThr, warmstart, print_period) -> (T, log)

Every log has "warn" ("" / "noconv" / "numerr") and "loss"; numpy arrays in, numpy arrays out."""
import numpy as np


def _uniform(n):
    """The reference builds its uniform vectors (default marginals, initial and reset scalings) in fp32, whatever the precision of the run."""
    return np.full(n, np.float64(np.float32(1.0 / n)))


def _inputs(a, b, M, warmstart):
    M = np.asarray(M, dtype=np.float64)
    n1, n2 = M.shape
    a = _uniform(n1) if a is None or len(a) == 0 else np.asarray(a, dtype=np.float64)
    b = _uniform(n2) if b is None or len(b) == 0 else np.asarray(b, dtype=np.float64)
    warm = None if warmstart is None else tuple(np.asarray(w, dtype=np.float64) for w in warmstart)
    return a, b, M, n1, n2, warm


def _top_gap(x):
    """Relative gap between the largest and the second largest entry (inf for a single entry)."""
    if len(x) < 2:
        return np.inf
    top = np.partition(x, -2)[-2:]
    return float((top[1] - top[0]) / top[1]) if top[1] > 0 else 0.0


def greenkhorn_ref(a, b, M, reg, numItermax=10000, stopThr=1e-9, warmstart=None):
    """log: n_iter, u, v, stop_vals (the stopping value of every executed step), gaps (per step: the smallest relative gap that decided it: the
    chosen maximum against the runner-up of its own vector, and the row maximum against the column maximum)."""
    a, b, M, n1, n2, warm = _inputs(a, b, M, warmstart)
    with np.errstate(all="ignore"):
        K = np.exp(-M / reg)
        u, v = (_uniform(n1), _uniform(n2)) if warm is None else (np.exp(warm[0]), np.exp(warm[1]))
        P = u[:, None] * K * v[None, :]
        r, c = P.sum(1) - a, P.sum(0) - b                                 # violations of the two marginals, kept up to date incrementally
        stop_vals, gaps, ii, warn = [], [], 0, "noconv"
        for ii in range(numItermax):
            ar, ac = np.abs(r), np.abs(c)
            i, j = int(np.argmax(ar)), int(np.argmax(ac))
            big = max(ar[i], ac[j])
            stop_vals.append(float(big))
            between = abs(ar[i] - ac[j]) / big if big > 0 else 0.0
            if ar[i] > ac[j]:                                             # rescale row i to its marginal
                gaps.append(min(between, _top_gap(ar)))
                new = a[i] / (K[i] @ v)
                r[i] = (new * K[i]) @ v - a[i]
                c += K[i] * (new - u[i]) * v
                u[i] = new
            else:                                                         # rescale column j
                gaps.append(min(between, _top_gap(ac)))
                new = b[j] / (K[:, j] @ u)
                r += (new - v[j]) * K[:, j] * u
                c[j] = new * (K[:, j] @ u) - b[j]
                v[j] = new
            if big <= stopThr:
                warn = ""
                break
        T = u[:, None] * K * v[None, :]
    return T, {"n_iter": ii, "u": u, "v": v, "stop_vals": stop_vals, "gaps": gaps, "warn": warn, "loss": float((M * T).sum())}


def stabilized_ref(a, b, M, reg, numItermax=1000, tau=1e3, stopThr=1e-9, warmstart=None, print_period=20):
    """log: err, n_iter, logu, logv, alpha, beta, absorptions, sweeps."""
    a, b, M, n1, n2, warm = _inputs(a, b, M, warmstart)
    f, g = (np.zeros(n1), np.zeros(n2)) if warm is None else (warm[0].copy(), warm[1].copy())
    with np.errstate(all="ignore"):
        kernel = lambda: np.exp(-(M - f[:, None] - g[None, :]) / reg)
        plan = lambda: np.exp(-(M - f[:, None] - g[None, :]) / reg + np.log(u)[:, None] + np.log(v)[None, :])
        u, v = _uniform(n1), _uniform(n2)
        K, errs, absorptions, warn, err, ii = kernel(), [], 0, "noconv", 1.0, 0
        for ii in range(numItermax):
            pu, pv = u, v
            v = b / (K.T @ u)
            u = a / (K @ v)
            if np.max(np.abs(u)) > tau or np.max(np.abs(v)) > tau:        # absorb the scalings into the potentials (a NaN maximum compares false)
                f, g = f + reg * np.log(u), g + reg * np.log(v)
                u, v = _uniform(n1), _uniform(n2)
                K = kernel()
                absorptions += 1
            if ii % print_period == 0:
                err = float(np.linalg.norm(plan().sum(0) - b))
                errs.append(err)
            if err <= stopThr:
                warn = ""
                break
            if np.isnan(u).any() or np.isnan(v).any():
                u, v, warn = pu, pv, "numerr"
                break
        T = plan()
        lu, lv = np.log(u), np.log(v)
    return T, {"err": errs, "n_iter": ii, "logu": f / reg + lu, "logv": g / reg + lv, "alpha": f + reg * lu, "beta": g + reg * lv,
               "absorptions": absorptions, "sweeps": ii + 1, "warn": warn, "loss": float(np.nansum(M * T))}


def epsilon_scaling_ref(a, b, M, reg, numItermax=100, epsilon0=1e4, numInnerItermax=100, tau=1e3, stopThr=1e-9, warmstart=None, print_period=10):
    """log: err, niter, alpha, beta, inner (one dict per inner solve: n_iter, err, warn, absorptions), ncap (inner solves that ran to their cap),
    sweeps (over all inner solves)."""
    a, b, M, n1, n2, warm = _inputs(a, b, M, warmstart)
    f, g = (np.zeros(n1), np.zeros(n2)) if warm is None else warm
    numItermax = max(35, numItermax)
    errs, inner, err, warn, ii, T = [], [], 1.0, "noconv", 0, None
    for ii in range(numItermax):
        regi = (epsilon0 - reg) * np.exp(-ii) + reg
        T, li = stabilized_ref(a, b, M, regi, numInnerItermax, tau, stopThr, (f, g), 20)
        f, g = li["alpha"], li["beta"]
        inner.append({k: li[k] for k in ("n_iter", "err", "warn", "absorptions")})
        if ii % print_period == 0:
            err = float(np.linalg.norm(T.sum(0) - b) ** 2 + np.linalg.norm(T.sum(1) - a) ** 2)
            errs.append(err)
        if err <= stopThr and ii > 35:
            warn = ""
            break
    return T, {"err": errs, "niter": ii, "alpha": f, "beta": g, "inner": inner, "ncap": sum(1 for x in inner if x["warn"] == "noconv"),
               "sweeps": sum(x["n_iter"] + 1 for x in inner), "warn": warn, "loss": float(np.nansum(M * T))}


def greenkhorn_fair(stop_vals, gaps, n_iter, numItermax, stopThr, converged):
    """Conditions (b) and (c) of tests/test_sinkhorn_ext_cpu.py: every arg-max decided by a relative gap of at least 1e-9, and, for a converged
    run, the exit step's stopping value <= stopThr / 1.001 with every earlier one >= 1.001 stopThr."""
    if not gaps or min(gaps) < 1e-9:
        return False
    if not converged:
        return n_iter == numItermax - 1 and min(stop_vals) >= 1.001 * stopThr
    return stop_vals[-1] <= stopThr / 1.001 and all(s >= 1.001 * stopThr for s in stop_vals[:-1])
