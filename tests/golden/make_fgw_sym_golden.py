"""Generates tests/golden/fgw_sym_*.npz: the reference's fgw_barycenters with symmetric=False / None (barycenter.py:7-225 -> bregman.py:98-128
for PGD / PPA, :199-222 for BAPG) on directed graphs and asymmetric float matrices.

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).  Like make_fgw_solver_golden.py it imports the reference's own FGW solver (through
make_fgw_golden's helpers) and records inputs plus the reference's outputs in fp32 ("r32") and fp64 ("r64"), with the fp64 run's iteration
counts (its Counter: one fgw() call per coupling solve, Sinkhorn calls and iterations for PGD / PPA, pairs of torch.exp calls for BAPG).  No
reference source is copied.  The notebook call (notebooks/fgw.ipynb on cfm_log, kl_loss, epsilon 0.05) is recorded truncated to 3 outer
iterations: past that the reference's own fp64 runs of the same problem drift apart.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_sym_golden.py [name ...]
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

from make_fgw_golden import ref_bary  # noqa: E402  (imports the reference)
from make_fgw_solver_golden import PROD, Counter  # noqa: E402

SYM_CODE = {True: 1, False: 0, None: -1}


def run_ref(Ys, Cs, sizes, N, dtype, solver, ps=None, p=None, lambdas=None, init_C="first", **over):
    """Ys [K,n_max,d] / Cs [K,n_max,n_max] zero-padded, sizes[s] = rows of graph s the reference sees."""
    K = len(sizes)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    args = dict(PROD); args.update(over)
    Ysl = [t(Ys[s, :sizes[s]]).requires_grad_(True) for s in range(K)]
    Csl = [t(Cs[s, :sizes[s], :sizes[s]]) for s in range(K)]
    psl = [torch.ones(n, dtype=dtype) / n for n in sizes] if ps is None else [t(ps[s, :sizes[s]]) for s in range(K)]
    lam = torch.ones(K, dtype=dtype) / K if lambdas is None else t(lambdas)
    ic = (Csl[0] if sizes[0] == N else None) if isinstance(init_C, str) else init_C
    with Counter() as cnt:
        Y, C, log = ref_bary.fgw_barycenters(N=N, Ys=Ysl, Cs=Csl, ps=psl, p=None if p is None else t(p), lambdas=lam, init_C=ic,
                                             solver=solver, **args)
    outer = len(log["err_feature"])
    inner = sum(c[2] // 2 if solver == "BAPG" else c[0] for c in cnt.calls)
    sk = 0 if solver == "BAPG" else sum(c[1] for c in cnt.calls)
    assert len(cnt.calls) == outer * K
    gw = torch.from_numpy(np.random.RandomState(7).normal(size=tuple(Y.shape))).to(dtype)
    (Y * gw).sum().backward()
    n_max = Ys.shape[1]
    T = np.zeros((K, N, n_max))
    dYs = np.zeros(Ys.shape)
    for s in range(K):
        T[s, :, :sizes[s]] = log["T"][s].detach().numpy()
        dYs[s, :sizes[s]] = Ysl[s].grad.numpy()
    return dict(Y=Y.detach().numpy(), C=C.detach().numpy(), T=T, err_feature=np.array([float(e) for e in log["err_feature"]]),
                err_structure=np.array([float(e) for e in log["err_structure"]]), inner=np.int64(inner), sinkhorn=np.int64(sk), dYs=dYs,
                grad_w=gw.numpy())


def directed(seed, K, n, d, dens=0.3):
    """Directed random 0/1 graphs (no self loops, no symmetrisation) with positive features."""
    rng = np.random.RandomState(seed)
    Ys = rng.uniform(0.1, 2.0, size=(K, n, d)).astype(np.float32)
    Cs = ((rng.random_sample((K, n, n)) < dens) & ~np.eye(n, dtype=bool)).astype(np.float32)
    return Ys, Cs


def asym_float(seed, K, n, d):
    """Asymmetric float structure matrices (a cost / similarity that is not a distance), entries in (0.05, 1)."""
    rng = np.random.RandomState(seed)
    Ys = rng.uniform(0.1, 2.0, size=(K, n, d)).astype(np.float32)
    Cs = rng.uniform(0.05, 1.0, size=(K, n, n)).astype(np.float32)
    return Ys, Cs


def ragged_directed(seed, sizes, d):
    rng = np.random.RandomState(seed)
    n_max = max(sizes)
    Ys = np.zeros((len(sizes), n_max, d), np.float32)
    Cs = np.zeros((len(sizes), n_max, n_max), np.float32)
    for s, n in enumerate(sizes):
        Ys[s, :n] = rng.uniform(0.1, 2.0, size=(n, d))
        Cs[s, :n, :n] = (rng.random_sample((n, n)) < 0.35) & ~np.eye(n, dtype=bool)
    return Ys, Cs


CASES = [
    # name, solver, inputs, sizes (None: all N), N, overrides
    ("pgd_k4_n12_d8_dir", "PGD", lambda: directed(41, 4, 12, 8), None, 12, dict(symmetric=False)),
    ("ppa_k4_n12_d8_dir", "PPA", lambda: directed(41, 4, 12, 8), None, 12, dict(symmetric=False)),
    ("bapg_k4_n12_d8_dir", "BAPG", lambda: directed(41, 4, 12, 8), None, 12, dict(symmetric=False, epsilon=1.0)),
    ("pgd_kl_k3_n10_d8_float", "PGD", lambda: asym_float(42, 3, 10, 8), None, 10, dict(symmetric=False, loss_fun="kl_loss")),
    ("ppa_kl_k3_n10_d8_float", "PPA", lambda: asym_float(42, 3, 10, 8), None, 10, dict(symmetric=False, loss_fun="kl_loss")),
    ("bapg_kl_k3_n10_d8_float", "BAPG", lambda: asym_float(42, 3, 10, 8), None, 10, dict(symmetric=False, loss_fun="kl_loss", epsilon=1.0)),
    ("pgd_k5_n33_d16_float", "PGD", lambda: asym_float(43, 5, 33, 16), None, 33, dict(symmetric=False, epsilon=0.5)),
    ("pgd_k2_n80_d8_dir", "PGD", lambda: directed(44, 2, 80, 8, 0.1), None, 80, dict(symmetric=False, epsilon=1.0)),
    ("ppa_kl_k2_n72_d8_float", "PPA", lambda: asym_float(45, 2, 72, 8), None, 72, dict(symmetric=False, loss_fun="kl_loss", epsilon=1.0)),
    ("bapg_k2_n70_d8_dir", "BAPG", lambda: directed(46, 2, 70, 8, 0.1), None, 70, dict(symmetric=False, epsilon=2.0)),
    ("none_ppa_k4_n12_d8_dir", "PPA", lambda: directed(41, 4, 12, 8), None, 12, dict(symmetric=None)),
    ("none_bapg_k4_n12_d8_dir", "BAPG", lambda: directed(41, 4, 12, 8), None, 12, dict(symmetric=None, epsilon=1.0)),
    ("pgd_ragged_N7", "PGD", lambda: ragged_directed(47, [9, 6, 8], 3), [9, 6, 8], 7, dict(symmetric=False)),
]


def save(name, solver, Ys, Cs, sizes, N, over, extra_in=None, ref_kw=None):
    ref_kw = ref_kw or {}
    r64 = run_ref(Ys, Cs, sizes, N, torch.float64, solver, **ref_kw, **over)
    for k in ("Y", "C", "T", "dYs"):
        assert np.isfinite(r64[k]).all(), (name, k, "the fp64 reference is not finite: not a fixture")
    r32 = run_ref(Ys, Cs, sizes, N, torch.float32, solver, **ref_kw, **over)
    prm = dict(PROD); prm.update(over)
    small_int = bool(np.all((Cs == np.round(Cs)) & (Cs >= 0) & (Cs <= 255)))
    rec = dict(Ys=Ys, Cs=Cs.astype(np.uint8) if small_int else Cs.astype(np.float32), sizes=np.array(sizes, np.int32), N=np.int32(N),
               solver=np.array(solver), symmetric=np.int32(SYM_CODE[prm["symmetric"]]),
               alpha=np.float64(prm["alpha"]), epsilon=np.float64(prm["epsilon"]), max_iter=np.int32(prm["max_iter"]), tol=np.float64(prm["tol"]),
               num_iter_max=np.int32(prm["numItermax"]), stop_thr=np.float64(prm["stopThr"]), warmstart=np.int32(prm["warmstartT"]),
               fixed_structure=np.int32(prm["fixed_structure"]), loss_fun=np.array(prm["loss_fun"]))
    rec.update(extra_in or {})
    for tag, rr in (("r32", r32), ("r64", r64)):
        for k, v in rr.items():
            if tag == "r64" and k == "grad_w":
                continue
            rec[f"{tag}_{k}"] = v.astype(np.float32) if (tag == "r32" and v.dtype.kind == "f") else v
    path = os.path.join(HERE, f"fgw_sym_{name}.npz")
    np.savez_compressed(path, **rec)
    rel = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    print(f"{name}: {os.path.getsize(path) // 1024} KB outer64={len(r64['err_feature'])} outer32={len(r32['err_feature'])} "
          f"inner64={int(r64['inner'])} inner32={int(r32['inner'])} sk64={int(r64['sinkhorn'])} relY={rel(r32['Y'], r64['Y']):.2e} "
          f"relC={rel(r32['C'], r64['C']):.2e} relT={rel(r32['T'], r64['T']):.2e}")


def notebook(max_iter=3):
    """notebooks/fgw.ipynb's call on cfm_log (symmetric=False, kl_loss, epsilon 0.05, alpha 0.5, random init_C of seed 0), truncated."""
    g = np.load(os.path.join(HERE, "cfm_log.npz"))
    N = int(g["N"])
    Ys, Cs, ps, lam = g["Ys"].astype(np.float32), g["Cs"].astype(np.float32), g["ps"].astype(np.float32), g["lambdas"].astype(np.float32)
    over = dict(symmetric=False, loss_fun="kl_loss", warmstartT=True, epsilon=0.05, alpha=0.5, max_iter=max_iter, tol=1e-5, numItermax=50,
                stopThr=5e-2)
    p = np.ones(N, np.float32) / N
    save(f"notebook_cfm_it{max_iter}", "PGD", Ys, Cs, [N] * len(Ys), N, over,
         extra_in=dict(ps=ps, lambdas=lam), ref_kw=dict(ps=ps, p=p, lambdas=lam, init_C=None))


def main():
    only = sys.argv[1:]
    for name, solver, make, sizes, N, over in CASES:
        if only and name not in only:
            continue
        Ys, Cs = make()
        save(name, solver, Ys, Cs, sizes or [N] * len(Ys), N, over)
    if not only or "notebook" in only:
        notebook(3)


if __name__ == "__main__":
    main()
