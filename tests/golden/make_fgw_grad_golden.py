"""Generates tests/golden/fgw_grad_*.npz: gradients of the reference's fgw_barycenters (barycenter.py:7-225) with respect to every input,
for the loss  sum(Y * gw) + sum(C * gc)  (gw, gc: normal draws of the recorded seeds).  The reference solves the couplings under
torch.no_grad() (barycenter.py:120), so autograd differentiates its last update steps (utils.py:67-95) and, under fixed_features /
fixed_structure, init_Y / init_C.  Every input is a leaf that requires grad; the names of the inputs whose .grad the reference fills are
recorded in `grads`, the others stay None.

RUNS ONLY IN THE BUILD CONTAINER (needs the reference).  Like make_fgw_sym_golden.py it imports the reference's own FGW solver (through
make_fgw_golden's helpers) and records inputs plus the reference's outputs (Y, C, T) and gradients in fp32 ("r32") and fp64 ("r64").  No
reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_grad_golden.py [name ...]
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
from make_fgw_solver_golden import PROD  # noqa: E402

SYM_CODE = {True: 1, False: 0, None: -1}
GW_SEED, GC_SEED = 7, 8


def run_ref(inp, N, dtype, solver, over):
    Ys, Cs, sizes = inp["Ys"], inp["Cs"], [int(n) for n in inp["sizes"]]
    K = len(sizes)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True)
    args = dict(PROD); args.update(over)
    Ysl = [t(Ys[s, :sizes[s]]) for s in range(K)]
    Csl = [t(Cs[s, :sizes[s], :sizes[s]]) for s in range(K)]
    psl = [t(np.ones(n) / n) for n in sizes]
    p = t(inp["p"]) if "p" in inp else None
    lam = t(inp["lambdas"]) if "lambdas" in inp else None
    ic = t(inp["init_C"])
    iy = t(inp["init_Y"]) if "init_Y" in inp else None
    Y, C, log = ref_bary.fgw_barycenters(N=N, Ys=Ysl, Cs=Csl, ps=psl, p=p, lambdas=lam, init_C=ic, init_Y=iy, solver=solver, **args)
    gw = torch.from_numpy(np.random.RandomState(GW_SEED).normal(size=tuple(Y.shape))).to(dtype)
    gc = torch.from_numpy(np.random.RandomState(GC_SEED).normal(size=tuple(C.shape))).to(dtype)
    ((Y * gw).sum() + (C * gc).sum()).backward()
    n_max = Ys.shape[1]
    T = np.zeros((K, N, n_max))
    for s in range(K):
        T[s, :, :sizes[s]] = log["T"][s].detach().numpy()
    out = dict(Y=Y.detach().numpy(), C=C.detach().numpy(), T=T)
    grads = []
    if Ysl[0].grad is not None:
        dYs = np.zeros(Ys.shape)
        for s in range(K):
            dYs[s, :sizes[s]] = Ysl[s].grad.numpy()
        out["dYs"] = dYs; grads.append("Ys")
    if Csl[0].grad is not None:
        dCs = np.zeros(Cs.shape)
        for s in range(K):
            dCs[s, :sizes[s], :sizes[s]] = Csl[s].grad.numpy()
        out["dCs"] = dCs; grads.append("Cs")
    for name, leaf in (("p", p), ("lambdas", lam), ("init_C", ic), ("init_Y", iy)):
        if leaf is not None and leaf.grad is not None:
            out["d" + name] = leaf.grad.numpy(); grads.append(name)
    assert all(q.grad is None for q in psl)
    return out, grads


def features(rng, K, n, d):
    return rng.uniform(0.1, 2.0, size=(K, n, d)).astype(np.float32)


def graphs(rng, K, n, dens=0.35, directed=False):
    A = (rng.random_sample((K, n, n)) < dens) & ~np.eye(n, dtype=bool)
    if not directed:
        A = np.triu(A, 1); A = A | A.transpose(0, 2, 1)
    return A.astype(np.float32)


def case(seed, K, n, d, N=None, sizes=None, p=False, lambdas=False, directed=False, fixed_C=False, fixed_Y=False):
    rng = np.random.RandomState(seed)
    sizes = sizes or [n] * K
    n_max = max(sizes)
    N = N or n
    Ys = np.zeros((K, n_max, d), np.float32)
    Cs = np.zeros((K, n_max, n_max), np.float32)
    for s, ns in enumerate(sizes):
        Ys[s, :ns] = features(rng, 1, ns, d)[0]
        Cs[s, :ns, :ns] = graphs(rng, 1, ns, directed=directed)[0]
    inp = dict(Ys=Ys, Cs=Cs, sizes=np.array(sizes, np.int32))
    if p:
        w = rng.uniform(0.5, 1.5, size=N)
        inp["p"] = (w / w.sum()).astype(np.float32)
    if lambdas:
        w = rng.uniform(0.5, 1.5, size=K)
        inp["lambdas"] = (w / w.sum()).astype(np.float32)
    if sizes[0] == N:
        inp["init_C"] = Cs[0, :N, :N].copy()
    else:
        x = rng.normal(size=(N, 2))
        inp["init_C"] = (((x[:, None] - x[None]) ** 2).sum(-1)).astype(np.float32)
    if fixed_C:
        inp["init_C"] = graphs(rng, 1, N)[0] + np.eye(N, dtype=np.float32) * 0.5
    if fixed_Y:
        inp["init_Y"] = features(rng, 1, N, d)[0]
    return inp, N


CASES = [
    # name, solver, inputs, overrides
    ("pgd_k5_n9_d3", "PGD", lambda: case(51, 5, 9, 3), {}),
    ("pgd_k5_n33_d8_plam", "PGD", lambda: case(52, 5, 33, 8, p=True, lambdas=True), dict(epsilon=0.5)),
    ("pgd_k2_n66_d4_plam", "PGD", lambda: case(53, 2, 66, 4, p=True, lambdas=True), dict(epsilon=0.5)),
    ("pgd_kl_k3_n10_d4_adj", "PGD", lambda: case(54, 3, 10, 4, p=True, lambdas=True), dict(loss_fun="kl_loss")),
    ("ppa_k3_n10_d4", "PPA", lambda: case(55, 3, 10, 4, p=True, lambdas=True), {}),
    ("bapg_k3_n10_d4", "BAPG", lambda: case(56, 3, 10, 4, p=True, lambdas=True), dict(epsilon=1.0)),
    ("pgd_k3_n10_d4_dir", "PGD", lambda: case(57, 3, 10, 4, p=True, lambdas=True, directed=True), dict(symmetric=False)),
    ("pgd_k3_n10_d4_fixedC", "PGD", lambda: case(58, 3, 10, 4, p=True, lambdas=True, fixed_C=True), dict(fixed_structure=True)),
    ("pgd_k3_n10_d4_fixedY", "PGD", lambda: case(59, 3, 10, 4, p=True, lambdas=True, fixed_Y=True), dict(fixed_features=True)),
    ("pgd_rect_N7", "PGD", lambda: case(60, 3, 0, 3, N=7, sizes=[9, 6, 8], p=True, lambdas=True), {}),
]


def save(name, solver, inp, N, over):
    r64, g64 = run_ref(inp, N, torch.float64, solver, over)
    for k, v in r64.items():
        assert np.isfinite(v).all(), (name, k, "the fp64 reference is not finite: not a fixture")
    r32, g32 = run_ref(inp, N, torch.float32, solver, over)
    assert g32 == g64, (g32, g64)
    prm = dict(PROD); prm.update(over)
    rec = dict(inp)
    rec["Cs"] = inp["Cs"].astype(np.uint8)
    rec.update(N=np.int32(N), solver=np.array(solver), symmetric=np.int32(SYM_CODE[prm["symmetric"]]),
               alpha=np.float64(prm["alpha"]), epsilon=np.float64(prm["epsilon"]), max_iter=np.int32(prm["max_iter"]), tol=np.float64(prm["tol"]),
               num_iter_max=np.int32(prm["numItermax"]), stop_thr=np.float64(prm["stopThr"]), warmstart=np.int32(prm["warmstartT"]),
               fixed_structure=np.int32(prm["fixed_structure"]), fixed_features=np.int32(prm["fixed_features"]),
               loss_fun=np.array(prm["loss_fun"]), gw_seed=np.int32(GW_SEED), gc_seed=np.int32(GC_SEED), grads=np.array(g64))
    for tag, rr in (("r32", r32), ("r64", r64)):
        for k, v in rr.items():
            rec[f"{tag}_{k}"] = v.astype(np.float32) if tag == "r32" else v
    path = os.path.join(HERE, f"fgw_grad_{name}.npz")
    np.savez_compressed(path, **rec)
    rel = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    print(f"{name}: {os.path.getsize(path) // 1024} KB grads={g64} " +
          " ".join(f"{k}={rel(r32[k], r64[k]):.1e}" for k in r64))


def main():
    only = sys.argv[1:]
    for name, solver, make, over in CASES:
        if only and name not in only:
            continue
        inp, N = make()
        save(name, solver, inp, N, over)


if __name__ == "__main__":
    main()
