"""Generates tests/golden/fgw_ppa_*.npz and tests/golden/fgw_bapg_*.npz: the reference's fgw_barycenters with solver="PPA" and
solver="BAPG" (barycenter.py:7-225 -> bregman.py:8-67 -> fgw_projected / fgw_bregman).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).  Like make_fgw_golden.py it imports the reference's own FGW solver and records
inputs plus the reference's outputs in fp32 ("r32") and in fp64 ("r64"); no reference source is copied.  Inner iterations are counted by
wrapping the reference's call sites: one fgw() call per coupling solve, per call the Sinkhorn calls (PPA) or the pairs of torch.exp calls
(BAPG: two per iteration, nothing else in fgw_bregman calls it).  A fixture is only written where the fp64 result is finite (asserted): BAPG's
multiplicative iteration underflows to NaN on 64-wide features at small epsilon, in the reference as here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_solver_golden.py
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

from make_fgw_golden import make_inputs, ref_bary, ref_breg  # noqa: E402  (imports the reference)

PROD = dict(warmstartT=True, symmetric=True, method="sinkhorn_log", alpha=0.1, fixed_structure=False, fixed_features=False, epsilon=0.1,
            loss_fun="square_loss", max_iter=5, tol=1e-2, numItermax=5, stopThr=1e-2, verbose=False, log=True)   # schnet_no_sum.py:281-306


class Counter:
    def __init__(self):
        self.calls = []          # one entry per fgw() call: [inner iterations, Sinkhorn iterations]
        self._o = (torch.logsumexp, torch.exp, ref_breg.sinkhorn, ref_bary.fgw)

    def __enter__(self):
        c = self
        lse0, exp0, sk0, fgw0 = self._o
        state = {"lse": 0}

        def lse(*a, **k):
            state["lse"] += 1
            return lse0(*a, **k)

        def exp(*a, **k):
            if c.calls:
                c.calls[-1][2] += 1
            return exp0(*a, **k)

        def sinkhorn(*a, **k):
            state["lse"] = 0
            out = sk0(*a, **k)
            c.calls[-1][0] += 1
            c.calls[-1][1] += state["lse"] // 2
            return out

        def fgw(*a, **k):
            c.calls.append([0, 0, 0])
            return fgw0(*a, **k)

        torch.logsumexp, torch.exp, ref_breg.sinkhorn, ref_bary.fgw = lse, exp, sinkhorn, fgw
        return self

    def __exit__(self, *exc):
        torch.logsumexp, torch.exp, ref_breg.sinkhorn, ref_bary.fgw = self._o


def run_ref(Ys, Cs, sizes, N, dtype, solver, **over):
    """Ys [K,n_max,d] / Cs [K,n_max,n_max] zero-padded, sizes[s] = rows of graph s the reference sees."""
    K = len(sizes)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    args = dict(PROD); args.update(over)
    Ysl = [t(Ys[s, :sizes[s]]).requires_grad_(True) for s in range(K)]
    Csl = [t(Cs[s, :sizes[s], :sizes[s]]) for s in range(K)]
    ps = [torch.ones(n, dtype=dtype) / n for n in sizes]
    lambdas = torch.ones(K, dtype=dtype) / K
    init_C = Csl[0] if sizes[0] == N else None
    with Counter() as cnt:
        Y, C, log = ref_bary.fgw_barycenters(N=N, Ys=Ysl, Cs=Csl, ps=ps, lambdas=lambdas, init_C=init_C, solver=solver, **args)
    outer = len(log["err_feature"])
    inner = sum(c[0] if solver == "PPA" else c[2] // 2 for c in cnt.calls)
    sk = sum(c[1] for c in cnt.calls) if solver == "PPA" else 0
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


CASES = [
    # name, solver, seed, K, n_real, n_pad, d, r, overrides
    ("ppa_k5_n9_d3", "PPA", 11, 5, 9, 0, 3, 10.0, {}),
    ("ppa_k5_n20_d64_cold", "PPA", 12, 5, 20, 0, 64, 10.0, dict(warmstartT=False)),
    ("ppa_k10_n18p2_d64", "PPA", 17, 10, 18, 2, 64, 10.0, {}),
    ("ppa_k3_n15p5_d64_fixedC", "PPA", 16, 3, 15, 5, 64, 10.0, dict(fixed_structure=True)),
    ("ppa_kl_k3_n15p5_d64", "PPA", 16, 3, 15, 5, 64, 10.0, dict(loss_fun="kl_loss")),
    ("ppa_k3_n70_d16", "PPA", 23, 3, 70, 0, 16, 10.0, dict(epsilon=1.0)),
    ("ppa_k4_n12_d8_default", "PPA", 24, 4, 12, 0, 8, 10.0, dict(max_iter=100, tol=1e-9, numItermax=100, stopThr=1e-5, warmstartT=False)),
    ("bapg_k5_n9_d3", "BAPG", 11, 5, 9, 0, 3, 10.0, dict(epsilon=0.2)),
    ("bapg_k5_n9_d3_cold", "BAPG", 11, 5, 9, 0, 3, 10.0, dict(epsilon=0.2, warmstartT=False)),
    ("bapg_k5_n18p2_d64", "BAPG", 17, 5, 18, 2, 64, 10.0, dict(epsilon=1.0)),
    ("bapg_k3_n20_d64_fixedC", "BAPG", 12, 3, 20, 0, 64, 10.0, dict(epsilon=1.0, fixed_structure=True)),
    ("bapg_k3_n80_d64", "BAPG", 25, 3, 80, 0, 64, 5.0, dict(epsilon=2.0)),
    ("bapg_kl_k5_n9_d3", "BAPG", 11, 5, 9, 0, 3, 10.0, dict(loss_fun="kl_loss", epsilon=1.0)),
    ("bapg_k4_n12_d8_default", "BAPG", 24, 4, 12, 0, 8, 10.0, dict(max_iter=100, tol=1e-9, epsilon=0.5, warmstartT=False)),
]
# input graphs of different sizes around a barycenter of N nodes (barycenter.py:50-67; fgw.py embeds them with massless nodes)
RAGGED = [("ppa_ragged_N7", "PPA", 31, 7, [9, 6, 8], 3, {}), ("bapg_ragged_N7", "BAPG", 31, 7, [9, 6, 8], 3, dict(epsilon=2.0))]


def ragged_inputs(seed, sizes, d):
    rng = np.random.RandomState(seed)
    n_max = max(sizes)
    Ys = np.zeros((len(sizes), n_max, d), np.float32)
    Cs = np.zeros((len(sizes), n_max, n_max), np.float32)
    for s, n in enumerate(sizes):
        Ys[s, :n] = rng.uniform(0.1, 2.0, size=(n, d))
        a = np.triu(rng.random_sample((n, n)) < 0.4, 1)
        Cs[s, :n, :n] = a | a.T
    return Ys, Cs


def save(name, solver, Ys, Cs, sizes, N, over):
    r64 = run_ref(Ys, Cs, sizes, N, torch.float64, solver, **over)
    for k in ("Y", "C", "T", "dYs"):
        assert np.isfinite(r64[k]).all(), (name, k, "the fp64 reference is not finite: not a fixture")
    r32 = run_ref(Ys, Cs, sizes, N, torch.float32, solver, **over)
    prm = dict(PROD); prm.update(over)
    rec = dict(Ys=Ys, Cs=Cs.astype(np.uint8), sizes=np.array(sizes, np.int32), N=np.int32(N), solver=np.array(solver),
               alpha=np.float64(prm["alpha"]), epsilon=np.float64(prm["epsilon"]), max_iter=np.int32(prm["max_iter"]), tol=np.float64(prm["tol"]),
               num_iter_max=np.int32(prm["numItermax"]), stop_thr=np.float64(prm["stopThr"]), warmstart=np.int32(prm["warmstartT"]),
               fixed_structure=np.int32(prm["fixed_structure"]), loss_fun=np.array(prm["loss_fun"]))
    for tag, rr in (("r32", r32), ("r64", r64)):
        for k, v in rr.items():
            if tag == "r64" and k == "grad_w":
                continue
            rec[f"{tag}_{k}"] = v.astype(np.float32) if (tag == "r32" and v.dtype.kind == "f") else v
    np.savez_compressed(os.path.join(HERE, f"fgw_{name}.npz"), **rec)
    rel = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    print(f"{name}: outer64={len(r64['err_feature'])} outer32={len(r32['err_feature'])} inner64={int(r64['inner'])} inner32={int(r32['inner'])} "
          f"sk64={int(r64['sinkhorn'])} relY={rel(r32['Y'], r64['Y']):.2e} relC={rel(r32['C'], r64['C']):.2e} relT={rel(r32['T'], r64['T']):.2e}")


def main():
    only = sys.argv[1:]
    for name, solver, seed, K, n_real, n_pad, d, r, over in CASES:
        if only and name not in only:
            continue
        Ys, Cs = make_inputs(seed, K, n_real, n_pad, d, r)
        N = n_real + n_pad
        save(name, solver, Ys, Cs, [N] * K, N, over)
    for name, solver, seed, N, sizes, d, over in RAGGED:
        if only and name not in only:
            continue
        Ys, Cs = ragged_inputs(seed, sizes, d)
        save(name, solver, Ys, Cs, sizes, N, over)


if __name__ == "__main__":
    main()
