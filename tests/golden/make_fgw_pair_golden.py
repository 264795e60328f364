"""Generates tests/golden/fgw_pair_*.npz: the reference's pairwise coupling solve fgw(M, C1, C2, p, q, ...) (bregman.py:8-67 -> fgw_projected
:70-167 / fgw_bregman :170-279) called directly, with log=True.

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).  Like make_fgw_sym_golden.py it imports the reference's own solver (through
make_fgw_golden's helpers) and records the inputs (M, C1, C2 — uint8 where 0/1 —, p, q, G0, the parameters) plus the reference's T, err list
and fgw_dist in fp32 ("r32") and fp64 ("r64"), with the fp64 run's iteration and Sinkhorn counts (make_fgw_solver_golden's Counter: Sinkhorn
calls and iterations for PGD / PPA, pairs of torch.exp calls for BAPG; sk_last: the iterations of the last Sinkhorn call).  No reference source is copied.  Asserted per case: the fp64 run is
finite, the fp32 run took the same counts, and the second recorded err of every multi-check case is above 1e-12 (the plan still moved).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_pair_golden.py [name ...]
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

from make_fgw_golden import ref_bary, ref_breg  # noqa: E402  (imports the reference; ref_bary.fgw is bregman.fgw, the name Counter wraps)
from make_fgw_solver_golden import Counter  # noqa: E402

SYM_CODE = {True: 1, False: 0, None: -1}
BASE = dict(loss_fun="square_loss", epsilon=0.1, symmetric=True, alpha=0.5, max_iter=100, tol=1e-5, solver="PGD", numItermax=100, stopThr=1e-5)
MODEL = dict(alpha=0.1, epsilon=0.1, max_iter=5, tol=1e-4, numItermax=5, stopThr=1e-2)      # the model's literals (schnet_no_sum.py:281-306)


def undirected(rng, n, dens=0.3):
    a = np.triu(rng.random_sample((n, n)) < dens, 1)
    return (a | a.T).astype(np.float32)


def directed(rng, n, dens=0.3):
    return ((rng.random_sample((n, n)) < dens) & ~np.eye(n, dtype=bool)).astype(np.float32)


def sym_float(rng, n):
    c = rng.uniform(0.05, 1.0, size=(n, n))
    return (0.5 * (c + c.T)).astype(np.float32)


def inputs(n1, n2, graph, seed=1, dens=0.3):
    """M ~ U(0, 2), p, q ~ U(0.5, 1.5) normalised, C1 / C2 from `graph`."""
    rng = np.random.RandomState(seed)
    M = rng.uniform(0.0, 2.0, size=(n1, n2)).astype(np.float32)
    p = rng.uniform(0.5, 1.5, size=n1); q = rng.uniform(0.5, 1.5, size=n2)
    p = (p / p.sum()).astype(np.float32); q = (q / q.sum()).astype(np.float32)
    mk = (lambda n: graph(rng, n, dens)) if graph is not sym_float else (lambda n: graph(rng, n))
    return dict(M=M, C1=mk(n1), C2=mk(n2), p=p, q=q)


def projected_start(d):
    """G0: p q^T * exp(-M), Sinkhorn-projected onto the marginals (100 scaling sweeps in fp64, stored fp32)."""
    p, q = d["p"].astype(np.float64), d["q"].astype(np.float64)
    G = np.outer(p, q) * np.exp(-d["M"].astype(np.float64))
    for _ in range(100):
        G *= (p / G.sum(1))[:, None]
        G *= (q / G.sum(0))[None, :]
    return G.astype(np.float32)


CASES = [
    # name, (n1, n2), graph, overrides, G0?
    ("pgd_n10", (10, 10), undirected, {}, False),
    ("pgd_rect_7x12", (7, 12), undirected, {}, False),
    ("pgd_n10_cap25", (10, 10), undirected, dict(max_iter=25, tol=1e-12), False),
    ("pgd_n10_g0", (10, 10), undirected, {}, True),
    ("pgd_kl_n10_float", (10, 10), sym_float, dict(loss_fun="kl_loss"), False),
    ("ppa_n10", (10, 10), undirected, dict(solver="PPA"), False),
    ("bapg_n12", (12, 12), undirected, dict(solver="BAPG", epsilon=1.0), False),
    ("pgd_dir_n12_false", (12, 12), directed, dict(symmetric=False), False),
    ("pgd_dir_n12_none", (12, 12), directed, dict(symmetric=None), False),
    ("pgd_undir_n12_none", (12, 12), undirected, dict(symmetric=None), False),
    ("bapg_dir_n12_false", (12, 12), directed, dict(solver="BAPG", symmetric=False, epsilon=1.0), False),
    ("bapg_rect_7x12", (7, 12), undirected, dict(solver="BAPG", epsilon=1.0), False),
    ("pgd_1x5", (1, 5), undirected, {}, False),
    ("pgd_model_n20", (20, 20), undirected, dict(MODEL), False),
    ("pgd_n33", (33, 33), undirected, {}, False),
    ("pgd_n80", (80, 80), undirected, dict(alpha=0.9, epsilon=0.05, max_iter=30), False),
    ("ppa_dir_n80_false", (80, 80), directed, dict(solver="PPA", symmetric=False, alpha=0.9, epsilon=0.05, max_iter=20), False),
    ("pgd_n140", (140, 140), undirected, dict(alpha=0.9, epsilon=0.05, max_iter=30), False),
    ("bapg_n140", (140, 140), undirected, dict(solver="BAPG", alpha=0.9, epsilon=0.5, max_iter=30), False),
]


def run_ref(d, G0, prm, dtype):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    kw = {} if prm["solver"] == "BAPG" else dict(numItermax=prm["numItermax"], stopThr=prm["stopThr"])
    per_call = []                                               # Sinkhorn iterations of every call (the last one tells whether it stopped on stopThr)
    with Counter() as cnt:
        counted = ref_breg.sinkhorn

        def sinkhorn(*a, **k):
            before = cnt.calls[-1][1]
            out = counted(*a, **k)
            per_call.append(cnt.calls[-1][1] - before)
            return out

        ref_breg.sinkhorn = sinkhorn                            # (Counter restores the reference's own on exit)
        T, log = ref_bary.fgw(t(d["M"]), t(d["C1"]), t(d["C2"]), t(d["p"]), t(d["q"]), loss_fun=prm["loss_fun"], epsilon=prm["epsilon"],
                              symmetric=prm["symmetric"], alpha=prm["alpha"], G0=None if G0 is None else t(G0), max_iter=prm["max_iter"],
                              tol=prm["tol"], solver=prm["solver"], log=True, **kw)
    (c,) = cnt.calls
    it = c[2] // 2 if prm["solver"] == "BAPG" else c[0]
    sk = 0 if prm["solver"] == "BAPG" else c[1]
    return dict(T=T.numpy(), err=np.array([float(e) for e in log["err"]]), fgw_dist=np.array(float(log["fgw_dist"])), it=np.int64(it), sk=np.int64(sk),
                sk_last=np.int64(per_call[-1] if per_call else 0))


def save(name, shape, graph, over, with_g0):
    prm = dict(BASE); prm.update(over)
    d = inputs(*shape, graph)
    G0 = projected_start(d) if with_g0 else None
    r64 = run_ref(d, G0, prm, torch.float64)
    assert np.isfinite(r64["T"]).all() and np.isfinite(r64["err"]).all() and np.isfinite(r64["fgw_dist"]), (name, "the fp64 reference is not finite")
    r32 = run_ref(d, G0, prm, torch.float32)
    assert (int(r32["it"]), int(r32["sk"])) == (int(r64["it"]), int(r64["sk"])), (name, "fp32 and fp64 counts differ", r32["it"], r64["it"], r32["sk"], r64["sk"])
    assert len(r64["err"]) == -(-int(r64["it"]) // 10), name
    if len(r64["err"]) > 1:
        assert r64["err"][1] > 1e-12, (name, "the plan no longer moves at the second check")
    is01 = lambda a: bool(np.all((a == 0) | (a == 1)))
    rec = dict(M=d["M"], C1=d["C1"].astype(np.uint8) if is01(d["C1"]) else d["C1"], C2=d["C2"].astype(np.uint8) if is01(d["C2"]) else d["C2"],
               p=d["p"], q=d["q"], G0=G0 if G0 is not None else np.zeros((0, 0), np.float32), solver=np.array(prm["solver"]),
               symmetric=np.int32(SYM_CODE[prm["symmetric"]]), loss_fun=np.array(prm["loss_fun"]), alpha=np.float64(prm["alpha"]),
               epsilon=np.float64(prm["epsilon"]), max_iter=np.int32(prm["max_iter"]), tol=np.float64(prm["tol"]),
               num_iter_max=np.int32(prm["numItermax"]), stop_thr=np.float64(prm["stopThr"]))
    for tag, rr in (("r32", r32), ("r64", r64)):
        for k, v in rr.items():
            if tag == "r32" and k in ("it", "sk", "sk_last"):
                continue
            rec[f"{tag}_{k}"] = v.astype(np.float32) if (tag == "r32" and v.dtype.kind == "f") else v
    path = os.path.join(HERE, f"fgw_pair_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 512 * 1024, (name, os.path.getsize(path))
    rel = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    print(f"{name}: {os.path.getsize(path) // 1024} KB it={int(r64['it'])} sk={int(r64['sk'])} errs={len(r64['err'])} relT={rel(r32['T'], r64['T']):.2e} "
          f"reldist={abs(float(r32['fgw_dist']) - float(r64['fgw_dist'])) / abs(float(r64['fgw_dist'])):.2e} sumT={r64['T'].sum():.8f}")


def main():
    only = sys.argv[1:]
    for case in CASES:
        if not only or case[0] in only:
            save(*case)


if __name__ == "__main__":
    main()
