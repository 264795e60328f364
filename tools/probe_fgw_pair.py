"""What does the pair form of the general coupling kernels cost next to the register-resident barycenter path?

    python tools/probe_fgw_pair.py [--runs 25] [--warmup 5] [--json OUT.json]

Three shapes with the model's literals (alpha 0.1, epsilon 0.1, max_iter 5, tol 1e-4, numItermax 5, stopThr 1e-2), HIP events around the call
after warm-up, median of --runs (>= 20) runs:

    ops.fgw_pair_batched           B = 1280, N = 33
    ops.fgw_pair_batched           B = 120,  N = 83
    fgw.fgw_pairwise_distances     G = 64,   N = 33   (2016 pairs; "solve only" is the one batched call inside it, without forming the costs)

Beside each, the SAME couplings through the entry point that existed before the pair form: ops.fgw_barycenter_batched with K = 1, init_C = C1,
init_Y = Y0, fixed_structure and fixed_features, max_iter 5 — its first outer iteration is the coupling solve with M = dist(Y0, Z); the update
finds nothing moved and the other four iterations' launches exit at once.  At N <= 64 it is the register-resident path, at N = 83
k_fgw_coupling_big; neither contains the general solve the pair form runs.  The plans of the two
columns are compared (relative Frobenius error, printed) so that the timings are known to be of the same problem."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd import fgw as pfgw  # noqa: E402
from conan_fgw_amd import ops  # noqa: E402

MODEL = dict(alpha=0.1, epsilon=0.1, max_iter=5, tol=1e-4, num_iter_max=5, stop_thr=1e-2)


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def problem(B, N, d, seed, dev):
    rng = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)

    def adjacency():
        a = np.triu(rng.random_sample((B, N, N)) < 0.1, 1)
        return t(a | a.transpose(0, 2, 1))
    return t(rng.uniform(0.1, 2.0, size=(B, N, d))), t(rng.uniform(0.1, 2.0, size=(B, N, d))), adjacency(), adjacency()


def batched_case(B, N, runs, warmup, dev):
    Y0, Z, C1, C2 = problem(B, N, 8, 10 + N, dev)
    M = torch.stack([pfgw.feature_cost(Y0[b], Z[b]) for b in range(B)])
    pair = lambda: ops.fgw_pair_batched(M, C1, C2, symmetric=True, **MODEL)
    bary = lambda: ops.fgw_barycenter_batched(Z[:, None], C2[:, None], init_C=C1, init_Y=Y0, fixed_structure=True, fixed_features=True,
                                              warmstart=False, cs_small_int=True, alpha=0.1, epsilon=0.1, max_iter=5, tol=1e-2, inner_tol=1e-4,
                                              num_iter_max=5, stop_thr=1e-2)
    Tp, Tb = pair()[0], bary()[2][:, 0]
    err = float((Tp - Tb).norm() / Tb.norm())
    (pm, plo, phi), (bm, blo, bhi) = timed(pair, runs, warmup), timed(bary, runs, warmup)
    return dict(case=f"fgw_pair_batched B={B} N={N}", pair_ms=pm, pair_min_max=[plo, phi], barycenter_ms=bm, barycenter_min_max=[blo, bhi],
                ratio=pm / bm, plans_rel_err=err)


def pairwise_case(G, N, runs, warmup, dev):
    Y, _, C, _ = problem(G, N, 8, 77, dev)
    Ys, Cs = list(Y), list(C)
    kw = dict(alpha=0.1, epsilon=0.1, max_iter=5, tol=1e-4, numItermax=5, stopThr=1e-2, symmetric=True)
    whole = lambda: pfgw.fgw_pairwise_distances(Ys, Cs, **kw)
    ia, ib = torch.triu_indices(G, G, 1)
    M = torch.stack([pfgw.feature_cost(Ys[a], Ys[b]) for a, b in zip(ia.tolist(), ib.tolist())])
    C1, C2, Y0, Z = C[ia.to(dev)], C[ib.to(dev)], Y[ia.to(dev)], Y[ib.to(dev)]
    solve = lambda: ops.fgw_pair_batched(M, C1, C2, symmetric=True, **MODEL)
    bary = lambda: ops.fgw_barycenter_batched(Z[:, None], C2[:, None], init_C=C1, init_Y=Y0, fixed_structure=True, fixed_features=True,
                                              warmstart=False, cs_small_int=True, alpha=0.1, epsilon=0.1, max_iter=5, tol=1e-2, inner_tol=1e-4,
                                              num_iter_max=5, stop_thr=1e-2)
    err = float((solve()[0] - bary()[2][:, 0]).norm() / bary()[2][:, 0].norm())
    (wm, wlo, whi), (sm, slo, shi), (bm, blo, bhi) = timed(whole, runs, warmup), timed(solve, runs, warmup), timed(bary, runs, warmup)
    return dict(case=f"fgw_pairwise_distances G={G} N={N} ({len(ia)} pairs)", whole_ms=wm, whole_min_max=[wlo, whi], pair_ms=sm, pair_min_max=[slo, shi],
                barycenter_ms=bm, barycenter_min_max=[blo, bhi], ratio=sm / bm, plans_rel_err=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.runs >= 20, "a median of at least 20 runs"
    dev = torch.device("cuda:0")
    rows = [batched_case(1280, 33, a.runs, a.warmup, dev), batched_case(120, 83, a.runs, a.warmup, dev), pairwise_case(64, 33, a.runs, a.warmup, dev)]
    for r in rows:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), runs=a.runs, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
