"""fp64 yardsticks of the differentiable FGWMixup pair (fgw.fgw_barycenters_BAPG, fgw.fgw_mixup_distance), as plain torch formulas that autograd
differentiates at a GIVEN coupling: the project's fixed-plan convention.  Written from the update rules (Peyre, Cuturi, Solomon 2016, eq. 14 / 15
with the order corrected; Vayer et al. 2019 for the features) and from the FGWMixup objective (Ma et al. 2023); tests/test_fgw_mixup_grad_cpu.py
holds them to every mixup_grad_* fixture's fp64 run.

    update_steps(T, Ys, Cs, p, lam, init_C, init_Y, kl, fs, ff) -> Y [B,N,d], C [B,N,N]       the three update steps on T [B,K,N,N]
    mixup_distance(M, A, Bm, a, b, X, alpha) -> [B]                                            the FGWMixup distance at the plan X [B,n1,n2]
"""
import numpy as np
import torch


def fixture_problem(g):
    """A mixup_grad_* fixture as the square fp64 problem the kernels solve: everything embedded in Np = max(N, max n_s) nodes, the extra nodes
    without mass -> dict of B = 1 tensors (Ys, Cs, p, lam, init_C, init_Y or None, T = the fixture's r64 couplings) and kl, fs, ff, N, Np, sizes."""
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    K, n_max, d = g["Ys"].shape
    Np = max(N, n_max)

    def pad(a, *shape):
        out = np.zeros(shape, np.float64)
        out[tuple(slice(0, k) for k in a.shape)] = a
        return torch.from_numpy(out)[None]
    prob = dict(Ys=pad(g["Ys"], K, Np, d), Cs=pad(g["Cs"], K, Np, Np), T=pad(g["r64_T"], K, Np, Np), init_C=pad(g["init_C"], Np, Np),
                init_Y=pad(g["init_Y"], Np, d) if "init_Y" in g.files else None,
                p=pad(g["p"] if "p" in g.files else np.full(N, 1.0 / N), Np),
                lam=torch.from_numpy(g["lambdas"].astype(np.float64)) if "lambdas" in g.files else torch.full((K,), 1.0 / K, dtype=torch.float64))
    prob.update(kl=str(g["loss_fun"]) == "kl_loss", fs=bool(g["fixed_structure"]), ff=bool(g["fixed_features"]), N=N, Np=Np, sizes=sizes)
    return prob


def update_steps(T, Ys, Cs, p, lam, init_C, init_Y, kl, fs, ff):
    """Y = diag(1/p) sum_s lam_s T_s Ys_s;  C = (sum_s lam_s T_s h(Cs_s) T_s^T) / (p p^T) with h = identity (square loss) or
    C = exp(the same with h = log max(., 1e-15)) (KL);  Y = init_Y / C = init_C under fixed_features / fixed_structure.
    T [B,K,N,N], Ys [B,K,N,d], Cs [B,K,N,N], p [B,N], lam [K].  A node without mass (p_i = 0) keeps a zero row of Y and a zero row and column
    of C, and gets no gradient (the guard of the kernels)."""
    mass = p > 0
    pinv = torch.where(mass, 1.0 / torch.where(mass, p, torch.ones_like(p)), torch.zeros_like(p))
    if ff:
        Y = init_Y
    else:
        Y = pinv[:, :, None] * torch.einsum("k,bkij,bkjc->bic", lam, T, Ys)
    if fs:
        C = init_C
    else:
        X = torch.log(torch.clamp(Cs, min=1e-15)) if kl else Cs
        S = torch.einsum("k,bkij,bkjl,bkml->bim", lam, T, X, T) * pinv[:, :, None] * pinv[:, None, :]
        C = torch.exp(S) * (mass[:, :, None] & mass[:, None, :]) if kl else S
    return Y, C


def mixup_distance(M, A, Bm, a, b, X, alpha):
    """(1 - alpha) <M, X> + alpha (<c1, X> - 2 <A X Bm, X>),  c1 = (A o A) a 1^T + 1 b^T (Bm o Bm): the solve's final objective
    sum(((1 - alpha) M - 2 alpha A X Bm) * X) plus alpha <c1, X>.  Bm enters untransposed.  M [B,n1,n2], A [B,n1,n1], Bm [B,n2,n2], a [B,n1],
    b [B,n2], X [B,n1,n2] -> [B]."""
    c1 = ((A * A) @ a[:, :, None]) + (b[:, None, :] @ (Bm * Bm))
    return (1 - alpha) * (M * X).sum((1, 2)) + alpha * ((c1 * X).sum((1, 2)) - 2 * ((A @ X @ Bm) * X).sum((1, 2)))
