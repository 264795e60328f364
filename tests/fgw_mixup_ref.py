"""fp64 restatement on the CPU of what conan_fgw_amd runs on the GPU for FGWMixup: the accelerated mirror descent between two attributed graphs
(fgw.fused_ACC_torch) and the barycenter around it (fgw.fgw_barycenters_BAPG), written from the algorithm (Ma et al., "Fused Gromov-Wasserstein
Graph Mixup for Graph-level Classifications", 2023, Alg. 2 with the stopping rule of the reference's fgw/barycenter.py).  It is the yardstick of the
GPU tests where no stored fixture exists; tests/test_fgw_mixup_cpu.py holds it to every fixture's fp64 run.

    acc_ref(M, A, B, a, b, X0, alpha, rho, epoch, eps) -> X, log          log = {"objs": stored objectives, "checks": every objective formed,
                                                                                 "rel": the relative changes compared with eps, "epochs": int}
    mixup_ref(N, Ys, Cs, ps, p, lambdas, ...) -> Y, C, log                log = {"T", "err_feature", "err_structure", "epochs": [outer][s], "rel"}

One epoch, ii = 0 .. epoch - 1, from X = a b^T:
    X += 1e-10;  X *= exp((4 alpha A X B - (1 - alpha) M) / rho), rows scaled to a;  the same again, columns scaled to b;
    ii > 0 and ii % 10 == 0: obj = sum(((1 - alpha) M - 2 alpha A X B) * X); stop if |obj - last| / |last| < eps, else store obj.
The embedding rule of the GPU kernels is part of it: an entry whose row or column carries no mass stays exactly zero (no 1e-10, scaling factor 0),
so a rectangular problem may be passed embedded in a square one with massless nodes and gives the same numbers in its leading block."""
import numpy as np


def acc_ref(M, A, B, a=None, b=None, X0=None, *, alpha, rho, epoch=200, eps=1e-5):
    M, A, B = (np.asarray(t, np.float64) for t in (M, A, B))
    n1, n2 = M.shape
    a = np.full(n1, 1.0 / n1) if a is None else np.asarray(a, np.float64)
    b = np.full(n2, 1.0 / n2) if b is None else np.asarray(b, np.float64)
    mass = (a > 0)[:, None] & (b > 0)[None, :]
    X = np.where(mass, np.outer(a, b) if X0 is None else np.asarray(X0, np.float64), 0.0)
    objs, checks, rel, ran = [], [], [], epoch
    with np.errstate(all="ignore"):
        for ii in range(epoch):
            X = np.where(mass, X + 1e-10, 0.0)
            X = np.where(mass, np.exp((4 * alpha * (A @ X @ B) - (1 - alpha) * M) / rho) * X, 0.0)
            X = X * np.where(a > 0, a / X.sum(1), 0.0)[:, None]
            X = np.where(mass, np.exp((4 * alpha * (A @ X @ B) - (1 - alpha) * M) / rho) * X, 0.0)
            X = X * np.where(b > 0, b / X.sum(0), 0.0)[None, :]
            if ii > 0 and ii % 10 == 0:
                obj = float((((1 - alpha) * M - 2 * alpha * (A @ X @ B)) * X).sum())
                checks.append(obj)
                if objs:
                    rel.append(abs((obj - objs[-1]) / objs[-1]))
                    if rel[-1] < eps:
                        ran = ii + 1
                        break
                objs.append(obj)
    return X, {"objs": objs, "checks": checks, "rel": rel, "epochs": ran}


def sqdist(X, Y):
    c = -2.0 * (X @ Y.T)
    c += (X * X).sum(1)[:, None]
    c += (Y * Y).sum(1)[None, :]
    return np.maximum(c, 0.0)


def mixup_ref(N, Ys, Cs, ps=None, p=None, lambdas=None, *, init_C, init_Y=None, alpha=0.5, rho=1.0, max_iter=100, tol=1e-9, epoch=100, eps=1e-5,
              fixed_structure=False, fixed_features=False, loss_fun="square_loss"):
    """Ys[s] [n_s,d], Cs[s] [n_s,n_s] of any sizes; init_C [N,N] is required (the seeded random start is the caller's)."""
    Ys = [np.asarray(y, np.float64) for y in Ys]
    Cs = [np.asarray(c, np.float64) for c in Cs]
    S, d = len(Ys), Ys[0].shape[1]
    ps = [np.full(len(y), 1.0 / len(y)) for y in Ys] if ps is None else [np.asarray(q, np.float64) for q in ps]
    p = np.full(N, 1.0 / N) if p is None else np.asarray(p, np.float64)
    lambdas = [1.0 / S] * S if lambdas is None else [float(l) for l in lambdas]
    C = np.asarray(init_C, np.float64)
    Y = np.zeros((N, d)) if init_Y is None else np.asarray(init_Y, np.float64)
    err_f = err_s = 1e15
    log = {"err_feature": [], "err_structure": [], "epochs": [], "rel": [], "Ts_iter": []}
    cpt = 0
    T = []
    with np.errstate(all="ignore"):
        while (err_f > tol or err_s > tol) and cpt < max_iter:
            Cprev, Yprev = C, Y
            T, ep = [], []
            for s in range(S):
                X, lg = acc_ref(sqdist(Y, Ys[s]), C, Cs[s], p, ps[s], alpha=alpha, rho=rho, epoch=epoch, eps=eps)
                T.append(X); ep.append(lg["epochs"]); log["rel"] += lg["rel"]
            log["epochs"].append(ep)
            if not fixed_features:
                Y = sum(lambdas[s] * (T[s] @ Ys[s]) for s in range(S)) / p[:, None]
            if not fixed_structure:
                h = (lambda c: c) if loss_fun == "square_loss" else (lambda c: np.log(np.maximum(c, 1e-15)))
                tmp = sum(lambdas[s] * (T[s] @ h(Cs[s]) @ T[s].T) for s in range(S)) / np.outer(p, p)
                C = tmp if loss_fun == "square_loss" else np.exp(tmp)
            err_f = 0.0 if fixed_features else float(np.linalg.norm(Y - Yprev))
            err_s = 0.0 if fixed_structure else float(np.linalg.norm(C - Cprev))
            log["err_feature"].append(err_f); log["err_structure"].append(err_s); log["Ts_iter"].append(T)
            cpt += 1
    log["T"] = T
    return Y, C, log


def fair(values, thr):
    """No value that is compared with a threshold sits near it (the factors of tests/sinkhorn_ref.py::fair): counts can then be compared
    between two implementations."""
    return all(v <= 0.6 * thr or v >= 1.5 * thr for v in values)
