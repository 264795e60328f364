"""fp64 restatement, on the CPU, of what conan_fgw_mixup_barycenter_bwd computes (csrc/fgw_mixup_grad.hip): the gradient of the FGWMixup
barycenter (fgw.fgw_barycenters_BAPG_unrolled) through every epoch of every coupling solve of every outer iteration, written as a hand reverse
pass — the chain below composed with fgw_acc_grad_ref.acc_grad_ref, no autograd.  tests/test_fgw_mixup_unrolled_cpu.py holds it to torch autograd
through the reference's own fgw_barycenters_BAPG (tests/golden/grad_mixup_unrolled_*.npz) at 1e-9 and to a central finite difference of
fgw_mixup_ref.mixup_ref; the GPU tests use it where no fixture exists.

One square problem of N nodes (other sizes embedded with massless nodes: embed()).  Forward, t = 0 .. n - 1 from (C_0, Y_0) = (init_C, init_Y or 0):
    M_s = clamp(|y_i|^2 + |z_j|^2 - 2 y_i.z_j, 0);  X_s = ACC(M_s, C_t, Cs_s, p, ps_s), counts[t][s] epochs from p ps_s^T
    Y_t+1 = diag(1/p) sum_s lam_s X_s Ys_s;  C_t+1 = sum_s lam_s X_s h(Cs_s) X_s^T / (p p^T)   (kl: exp of it, h = log max(., 1e-15))
Backward from (Yb, Cb) = the cotangents, t = n - 1 .. 0:
    (a) U = Yb / p, V = Cb / (p p^T) (kl: Cb o C_t+1 / (p p^T));  Xb_s = lam_s (U Ys_s^T + V X_s h(Cs_s)^T + V^T X_s h(Cs_s)) and the direct
        partials: dYs_s += lam_s X_s^T U, dCs_s += lam_s (X_s^T V X_s) o h', dlam_s += <U, X_s Ys_s> + <X_s^T V X_s, h(Cs_s)>,
        dp_i -= (Yb_i . Y_t+1,i + sum_j (W_ij + W_ji)) / p_i, W = Cb o C_t+1 (kl: o log C_t+1)
    (b) acc_grad_ref(dX = Xb_s) -> dM_s, dA_s (summed into Cb_t), dB_s (into dCs_s), da (into dp), db (into dps_s)
    (c) through the clamp (mask: unclamped >= 0): Yb_t += 2 (diag(rowsum dM) Y_t - dM Ys_s), dYs_s += 2 (diag(colsum dM) Ys_s - dM^T Y_t)
Under fixed_features / fixed_structure the state stays at init_Y / init_C, the update's cotangent passes through unchanged and collects the
(c) / (b) terms of every iteration.  A node without mass gets exactly zero everywhere."""
import numpy as np

from fgw_acc_grad_ref import acc_grad_ref, grad_error  # noqa: F401  (grad_error: re-exported for the tests)


def embed(N, Ys, Cs, ps=None, p=None, init_C=None, init_Y=None):
    """Lists of own-size graphs -> the square problem of Np = max(N, max n_s) nodes: dict(Ys [K,Np,d], Cs [K,Np,Np], ps [K,Np], p [Np],
    init_C [Np,Np], init_Y [Np,d] or None, Np, sizes).  Absent weights are uniform over the own nodes."""
    K, d = len(Ys), np.asarray(Ys[0]).shape[1]
    sizes = [len(y) for y in Ys]
    Np = max([N] + sizes)
    out = dict(Ys=np.zeros((K, Np, d)), Cs=np.zeros((K, Np, Np)), ps=np.zeros((K, Np)), p=np.zeros(Np), init_C=np.zeros((Np, Np)), init_Y=None,
               Np=Np, sizes=sizes)
    for s, n in enumerate(sizes):
        out["Ys"][s, :n] = Ys[s]
        out["Cs"][s, :n, :n] = Cs[s]
        out["ps"][s, :n] = 1.0 / n if ps is None else ps[s]
    out["p"][:N] = 1.0 / N if p is None else p
    out["init_C"][:N, :N] = init_C
    if init_Y is not None:
        out["init_Y"] = np.zeros((Np, d))
        out["init_Y"][:N] = init_Y
    return out


def _sq(Y, Z):
    return -2.0 * (Y @ Z.T) + (Y * Y).sum(1)[:, None] + (Z * Z).sum(1)[None, :]


def mixup_unrolled_ref(Ys, Cs, ps, p, lam, init_C, init_Y=None, *, alpha, rho, counts, gY=None, gC=None, kl=False, fs=False, ff=False):
    """counts[t][s]: the epochs of coupling s in outer iteration t (len(counts) outer iterations).  -> dict of fp64 arrays: Y, C, T [K,N,N] (the
    last plans), dYs, dCs, dps, dp, dlam, dinit_C, dinit_Y (None without init_Y)."""
    Ys, Cs, ps, p, lam, C = (np.asarray(v, np.float64) for v in (Ys, Cs, ps, p, lam, init_C))
    K, N, d = Ys.shape
    Y = np.zeros((N, d)) if init_Y is None else np.asarray(init_Y, np.float64)
    mass = p > 0
    pinv = np.where(mass, 1.0 / np.where(mass, p, 1.0), 0.0)
    pp = pinv[:, None] * pinv[None, :]
    with np.errstate(divide="ignore"):
        h = np.log(np.maximum(Cs, 1e-15)) if kl else Cs
        hp = np.where(Cs >= 1e-15, 1.0 / np.where(Cs >= 1e-15, Cs, 1.0), 0.0) if kl else np.ones_like(Cs)
    states, T = [(C, Y)], None
    for ep in counts:
        T = np.stack([acc_grad_ref(np.maximum(_sq(Y, Ys[s]), 0.0), C, Cs[s], p, ps[s], alpha=alpha, rho=rho, epochs=int(ep[s]),
                                   dX=np.zeros((N, N)))["X"] for s in range(K)])
        if not ff:
            Y = pinv[:, None] * sum(lam[s] * (T[s] @ Ys[s]) for s in range(K))
        if not fs:
            S = sum(lam[s] * (T[s] @ h[s] @ T[s].T) for s in range(K)) * pp
            C = np.exp(S) * (mass[:, None] & mass[None, :]) if kl else S
        states.append((C, Y))

    Yb = np.zeros((N, d)) if gY is None else np.asarray(gY, np.float64).copy()
    Cb = np.zeros((N, N)) if gC is None else np.asarray(gC, np.float64).copy()
    dYs, dCs, dps, dp, dlam = np.zeros_like(Ys), np.zeros_like(Cs), np.zeros_like(ps), np.zeros_like(p), np.zeros_like(lam)
    for t in range(len(counts) - 1, -1, -1):
        (C0, Y0), (C1, Y1) = states[t], states[t + 1]
        U = np.zeros((N, d)) if ff else Yb * pinv[:, None]
        V = np.zeros((N, N)) if fs else (Cb * C1 if kl else Cb) * pp
        if not ff:
            dp -= (Yb * Y1).sum(1) * pinv
        if not fs:
            with np.errstate(divide="ignore", invalid="ignore"):
                W = Cb * C1
                W = np.where(W != 0.0, W * np.log(C1), 0.0) if kl else W
            dp -= (W.sum(1) + W.sum(0)) * pinv
        Yn = Yb.copy() if ff else np.zeros((N, d))
        Cn = Cb.copy() if fs else np.zeros((N, N))
        for s in range(K):
            raw = _sq(Y0, Ys[s])
            M = np.maximum(raw, 0.0)
            fwd = acc_grad_ref(M, C0, Cs[s], p, ps[s], alpha=alpha, rho=rho, epochs=int(counts[t][s]), dX=np.zeros((N, N)))
            X = fwd["X"]
            G = X.T @ V @ X
            Xb = lam[s] * (U @ Ys[s].T + V @ X @ h[s].T + V.T @ X @ h[s])
            dYs[s] += lam[s] * (X.T @ U)
            dCs[s] += lam[s] * G * hp[s]
            dlam[s] += (U * (X @ Ys[s])).sum() + (G * h[s]).sum()
            g = acc_grad_ref(M, C0, Cs[s], p, ps[s], alpha=alpha, rho=rho, epochs=int(counts[t][s]), dX=Xb)
            Cn += g["dA"]
            dCs[s] += g["dBm"]
            dp += g["da"]
            dps[s] += g["db"]
            dM = np.where(raw >= 0.0, g["dM"], 0.0)
            Yn += 2.0 * (dM.sum(1)[:, None] * Y0 - dM @ Ys[s])
            dYs[s] += 2.0 * (dM.sum(0)[:, None] * Ys[s] - dM.T @ Y0)
        Yb, Cb = Yn, Cn
    live = mass[:, None] & mass[None, :]
    dp = np.where(mass, dp, 0.0)
    return dict(Y=states[-1][1], C=states[-1][0], T=T, dYs=dYs, dCs=dCs, dps=dps, dp=dp, dlam=dlam, dinit_C=np.where(live, Cb, 0.0),
                dinit_Y=None if init_Y is None else np.where(mass[:, None], Yb, 0.0))


GRADS = ("dYs", "dCs", "dps", "dp", "dlambdas", "dinit_C", "dinit_Y")
TAGS = {"gY": (True, False), "gC": (False, True), "gB": (True, True)}          # which of the cotangents gw (of Y), gc (of C) a tag's loss uses


def fixture_problem(g):
    """A grad_mixup_unrolled_* fixture as the arguments of mixup_unrolled_ref (the square embedded problem) -> (args, kwargs, N, sizes).
    gY / gC are left to the caller (embed_cotangents)."""
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    K = len(sizes)
    Ys = [g["Ys"][s, :sizes[s]].astype(np.float64) for s in range(K)]
    Cs = [g["Cs"][s, :sizes[s], :sizes[s]].astype(np.float64) for s in range(K)]
    ps = [g["ps"][s, :sizes[s]].astype(np.float64) for s in range(K)]
    p = g["p"] if "p" in g.files else np.full(N, 1.0 / N, np.float32)          # (the fixtures pass uniform weights as fp32 values)
    e = embed(N, Ys, Cs, ps, p.astype(np.float64), g["init_C"].astype(np.float64),
              g["init_Y"].astype(np.float64) if "init_Y" in g.files else None)
    lam = (g["lambdas"] if "lambdas" in g.files else np.full(K, 1.0 / K, np.float32)).astype(np.float64)
    kw = dict(alpha=float(g["alpha"]), rho=float(g["rho"]), counts=g["epochs"].tolist(), kl=str(g["loss_fun"]) == "kl_loss",
              fs=bool(g["fixed_structure"]), ff=bool(g["fixed_features"]))
    return (e["Ys"], e["Cs"], e["ps"], e["p"], lam, e["init_C"], e["init_Y"]), kw, N, sizes


def embed_cotangents(g, tag, Np):
    """gw [N,d], gc [N,N] of the fixture, zero-padded to Np nodes; None where the tag's loss does not use one."""
    N, d = g["gw"].shape
    use_y, use_c = TAGS[tag]
    gY, gC = np.zeros((Np, d)), np.zeros((Np, Np))
    gY[:N], gC[:N, :N] = g["gw"], g["gc"]
    return (gY if use_y else None), (gC if use_c else None)


def cut(r, N, sizes, n_max):
    """mixup_unrolled_ref's gradients in the fixture's shapes (Ys [K,n_max,d], p [N], ...)."""
    out = dict(dYs=r["dYs"][:, :n_max], dCs=r["dCs"][:, :n_max, :n_max], dps=r["dps"][:, :n_max], dp=r["dp"][:N], dlambdas=r["dlam"],
               dinit_C=r["dinit_C"][:N, :N])
    if r["dinit_Y"] is not None:
        out["dinit_Y"] = r["dinit_Y"][:N]
    return out


def cotangent_norm(g, tag):
    use_y, use_c = TAGS[tag]
    return float(np.sqrt((np.linalg.norm(g["gw"]) ** 2 if use_y else 0.0) + (np.linalg.norm(g["gc"]) ** 2 if use_c else 0.0)))
