"""Plain numpy fp64 restatement of Sinkhorn-Knopp for several histograms at once (the reference's sinkhorn_knopp with b [n2,H],
sinkhorn.py:207-315): the joint iteration with its one stop and its one numerical-errors exit, the H costs, and the fixed-plan gradient of the
costs to M, dM = K o sum_k g_k u_k v_k^T.  Independent of torch and of the library; tests/test_sinkhorn_hists_cpu.py pins it to the stored
runs of the reference."""
import numpy as np


def knopp_hists(M, a, b, reg, num_iter_max, stop_thr, warm=None):
    """-> dict(loss [H], u [n1,H], v [n2,H], err (the evaluated checks), niter, warn: "" / "noconv" / "numerr")."""
    M, b = np.asarray(M, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n1, n2 = M.shape
    H = b.shape[1]
    a = np.full(n1, 1.0 / n1) if a is None or len(a) == 0 else np.asarray(a, dtype=np.float64)
    if warm is None:
        u, v = np.full((n1, H), 1.0 / n1), np.full((n2, H), 1.0 / n2)
    else:
        u, v = np.exp(np.asarray(warm[0], dtype=np.float64)), np.exp(np.asarray(warm[1], dtype=np.float64))
    err, warn, ii = [], "noconv", 0
    with np.errstate(all="ignore"):
        K = np.exp(M / -float(reg))
        Kp = (1.0 / a)[:, None] * K
        for ii in range(int(num_iter_max)):
            uprev, vprev = u, v
            KtU = K.T @ u
            v = b / KtU
            u = 1.0 / (Kp @ v)
            if (KtU == 0).any() or not np.isfinite(u).all() or not np.isfinite(v).all():
                u, v, warn = uprev, vprev, "numerr"
                break
            if ii % 10 == 0:
                e = float(np.sqrt(((v * (K.T @ u) - b) ** 2).sum()))
                err.append(e)
                if e < stop_thr:
                    warn = ""
                    break
        loss = np.einsum("ik,ij,jk,ij->k", u, K, v, M)
    return dict(loss=loss, u=u, v=v, err=np.array(err, dtype=np.float64), niter=ii, warn=warn)


def loss_grad_M(M, u, v, g, reg):
    """dM [n1,n2] of sum_k g_k loss_k at constant u, v: K o (u diag(g) v^T)."""
    M = np.asarray(M, dtype=np.float64)
    return np.exp(M / -float(reg)) * ((np.asarray(u, dtype=np.float64) * np.asarray(g, dtype=np.float64)[None, :]) @ np.asarray(v, dtype=np.float64).T)
