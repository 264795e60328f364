"""fp64 restatement, in plain torch on the CPU, of what conan_fgw_acc_pair_bwd computes (csrc/fgw_acc_grad.hip): the epochs of FGWMixup's coupling
solve run `epochs` times from a b^T (or X0) with the input of every half-step recorded, then the reverse walk written out by hand, no autograd.
tests/test_fgw_acc_grad_cpu.py holds it to torch autograd through the reference's own fused_ACC_torch (tests/golden/grad_acc_*.npz) at 1e-9 and
to a central finite difference; the GPU tests use it where no fixture exists (batches, own sizes).

The project's conventions, massless rule included: an entry whose row or column has no mass (a_i = 0 or b_j = 0) is never lifted by 1e-10, its
scaling factor is 0, it stays exactly zero and is a constant of the solve: the cotangent is held at zero there, and da_i / db_j of such a node is 0
(the reference divides by the weight).  The distance is ops.fgw_acc_pair_distance's,
    (1 - alpha) <M, X> + alpha (<c1, X> - 2 <A X Bm, X>),   c1 = (A o A) a 1^T + 1 b^T (Bm o Bm)."""
import numpy as np
import torch

F64 = torch.float64


def grad_error(got, want, cotangent=1.0):
    """The error of a gradient against its yardstick: the Frobenius norm of the difference over that of the yardstick.  Where the yardstick is
    zero up to its own fp64 rounding — its norm is below 1e-12 of the cotangent's, e.g. n1 = 1, where the plan is b whatever M, A, B and a
    are — that ratio measures noise against noise; the difference is then taken relative to the cotangent (W for sum(W * X), 1 for the
    distance), which is the size of the terms the zero is a sum of."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.linalg.norm(np.asarray(cotangent, dtype=np.float64)))
    n = float(np.linalg.norm(want))
    return float(np.linalg.norm(got - want)) / (n if n > 1e-12 * scale else scale)


def _t(x):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(F64)


def acc_forward(M, A, Bm, a, b, X0, alpha, rho, epochs, record=None):
    """`epochs` epochs, no objective checks -> X (fp64 tensors in, tensor out); record: a list that receives every half-step's input."""
    live = (a[:, None] > 0) & (b[None, :] > 0)
    X = torch.where(live, a[:, None] * b[None, :] if X0 is None else X0, torch.zeros((), dtype=F64))
    for _ in range(epochs):
        X = X + 1e-10 * live
        for w, dim in ((a, 1), (b, 0)):
            if record is not None:
                record.append(X)
            Z = torch.where(live, torch.exp((4 * alpha * (A @ X) @ Bm - (1 - alpha) * M) / rho), torch.zeros((), dtype=F64)) * X
            r = Z.sum(dim)
            f = torch.where(w > 0, w / r, torch.zeros((), dtype=F64))
            X = Z * (f[:, None] if dim == 1 else f[None, :])
    return X


def acc_distance(M, A, Bm, a, b, X, alpha):
    c1 = ((A * A) @ a)[:, None] + (b @ (Bm * Bm))[None, :]
    return (1 - alpha) * (M * X).sum() + alpha * ((c1 * X).sum() - 2 * (((A @ X) @ Bm) * X).sum())


def acc_grad_ref(M, A, Bm, a=None, b=None, X0=None, *, alpha, rho, epochs, dX=None, ddist=None):
    """The gradients of sum(dX o X) + ddist * distance(X) for one pair, as fp64 numpy arrays: X, dist, dM, dA, dBm, da, db, dX0 (None without X0).
    a / b None: uniform (their gradients are still returned)."""
    M, A, Bm, X0, dX = _t(M), _t(A), _t(Bm), _t(X0), _t(dX)
    n1, n2 = M.shape
    a = torch.full((n1,), 1.0 / n1, dtype=F64) if a is None else _t(a)
    b = torch.full((n2,), 1.0 / n2, dtype=F64) if b is None else _t(b)
    alpha, rho, om = float(alpha), float(rho), 1.0 - float(alpha)
    zero = torch.zeros((), dtype=F64)
    live = (a[:, None] > 0) & (b[None, :] > 0)
    rec = []
    X = acc_forward(M, A, Bm, a, b, X0, alpha, rho, epochs, rec)
    dist = acc_distance(M, A, Bm, a, b, X, alpha)

    Gb = torch.zeros_like(M) if dX is None else dX.clone()
    dM, dA, dB, da, db = torch.zeros_like(M), torch.zeros_like(A), torch.zeros_like(Bm), torch.zeros_like(a), torch.zeros_like(b)
    if ddist is not None:
        dd = float(ddist)
        r, c = X.sum(1), X.sum(0)
        c1 = ((A * A) @ a)[:, None] + (b @ (Bm * Bm))[None, :]
        AX, Y = A @ X, X @ Bm.T
        Gb = Gb + dd * (om * M + alpha * c1 - 2 * alpha * (AX @ Bm + A.T @ Y))
        dM = dd * om * X
        dA = dd * alpha * (2 * A * (r[:, None] * a[None, :]) - 2 * Y @ X.T)
        dB = dd * alpha * (2 * Bm * (b[:, None] * c[None, :]) - 2 * AX.T @ X)
        da = dd * alpha * ((A * A).T @ r)
        db = dd * alpha * ((Bm * Bm) @ c)
    Gb = torch.where(live, Gb, zero)

    for h in range(len(rec) - 1, -1, -1):
        X_h, col = rec[h], h % 2 == 1
        w = b if col else a
        line = (lambda v: v[None, :]) if col else (lambda v: v[:, None])
        AX = A @ X_h
        E = torch.where(live, torch.exp((4 * alpha * AX @ Bm - om * M) / rho), zero)
        Z = E * X_h
        r = Z.sum(0 if col else 1)
        f = torch.where(w > 0, w / r, zero)
        s = f * (Gb * Z).sum(0 if col else 1)
        q = torch.where(w > 0, s / torch.where(w > 0, w, torch.ones((), dtype=F64)), zero)
        if col:
            db = db + q
        else:
            da = da + q
        dZ = line(f) * (Gb - line(q))
        dG = dZ * Z / rho
        dM = dM - om * dG
        H = dG @ Bm.T
        Gb = dZ * E + torch.where(live, 4 * alpha * A.T @ H, zero)
        dA = dA + 4 * alpha * H @ X_h.T
        dB = dB + 4 * alpha * AX.T @ dG
    dX0 = None
    if X0 is None:
        da, db = da + Gb @ b, db + Gb.T @ a
    else:
        dX0 = Gb
    da, db = torch.where(a > 0, da, zero), torch.where(b > 0, db, zero)
    out = dict(X=X, dist=dist, dM=dM, dA=dA, dBm=dB, da=da, db=db, dX0=dX0)
    return {k: (None if v is None else v.numpy()) for k, v in out.items()}
