"""Generates tests/golden/fgw_bregman_unrollgrad_*.npz: torch autograd through the reference's own fgw_bregman (bregman.py:170-279, BAPG), in
fp64, on fp32-rounded inputs: the yardstick of the unrolled BAPG pairwise FGW gradient (csrc/fgw_bregman_grad.hip, ops.fgw_bregman_unrolled).

RUNS ONLY IN THE BUILD CONTAINER (needs the reference).  It imports the reference's function (through make_fgw_golden's helpers); no reference
source is copied.  One file per case, data only.  REUSED cases take the inputs of tests/golden/fgw_pair_<src>.npz (src = that name; the
parameters are that file's, overridden by what this file stores) and store the gradients only; NEW cases store their inputs under the same keys
as those files.  Every file holds the parameters, W (standard normal, fp32), iters (the iterations the reference ran: torch.exp calls / 2), errs
(every evaluated ||T - Tprev||), dist, T, tmin (the smallest plan entry with mass) and, with every input a leaf, the gradients of
    gT_*:  sum(W * T)            gd_*:  log["fgw_dist"]            gl_*:  log["loss"]  (LOSS cases only)
to M, C1, C2, p, q and, where a start is given, G0.

Every finite fixture must be DETERMINED: a second reference run on the relabelled problem (a seeded permutation of each graph: every sum then
runs in another order) takes the same iterations and reproduces the gradients, relabelled back, to 1e-10
(tests/fgw_acc_grad_ref.grad_error).  And because the forward's error check reads the previous plan from an fp32 copy (the error moves by about
1e-8 ||T||): tol is either so small that the solve runs to max_iter or at least 1e-6, and no evaluated error lies within a factor 2 of tol.  A
new case that fails either is replaced by the next seed's (+100); a reused one that fails stops the script.

Zero weight (zerop_9x11, p[3] = 0): the reference's 0 / 0 scaling makes its plan NaN.  The project treats the node as absent: the yardstick
stored is the reference run on the problem WITHOUT that node, embedded with exact zeros at the node's rows / columns.  What the reference gives
on the full problem is kept beside it: ref_full_T (NaN).

NaN (nan_n10): M >= 1 everywhere, alpha = 0.5, epsilon = 5e-4: every factor of the first half-step is exp(x) with x < -900 (first_x_max,
asserted), an exact zero under any exp, never a denormal; every row sum is 0 and the reference's plan and gradients are NaN.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_bregman_unrolled_golden.py [name ...]
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
warnings.filterwarnings("ignore")

from make_fgw_golden import ref_breg  # noqa: E402  (imports the reference)
from make_fgw_pair_golden import SYM_CODE, directed, inputs, projected_start, sym_float, undirected  # noqa: E402
from fgw_acc_grad_ref import grad_error  # noqa: E402

W_SEED = 2525
ZERO_AT = 3
SYM = {1: True, 0: False, -1: None}
LIMIT = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("fgw_unrollgrad_") and f.endswith(".npz"))
BASE = dict(loss_fun="square_loss", epsilon=1.0, symmetric=True, alpha=0.5, max_iter=100, tol=1e-5)


def dir_float(rng, n, dens=None):
    return rng.uniform(0.05, 1.0, size=(n, n)).astype(np.float32)


REUSED = [
    # name, src, overrides
    ("n12", "bapg_n12", {}),
    ("rect_7x12", "bapg_rect_7x12", {}),
    ("dir_n12_false", "bapg_dir_n12_false", {}),
    ("1x5", "pgd_1x5", dict(epsilon=1.0, max_iter=20, tol=1e-6)),
    ("n33", "pgd_n33", dict(epsilon=0.5, max_iter=30, tol=1e-12)),
    ("n80", "pgd_n80", dict(epsilon=0.5, max_iter=12, tol=1e-12)),
]
NEW = [
    # name, seed, (n1, n2), graph, overrides, G0?
    ("kl_n10", 41, (10, 10), sym_float, dict(loss_fun="kl_loss", epsilon=0.5, max_iter=30, tol=1e-12), False),
    ("kl_dir_n12_false", 42, (12, 12), dir_float, dict(loss_fun="kl_loss", symmetric=False, epsilon=0.5, max_iter=30, tol=1e-12), False),
    ("dir_n12_none", 43, (12, 12), directed, dict(symmetric=None, max_iter=30, tol=1e-12), False),
    ("undir_n12_none", 44, (12, 12), undirected, dict(symmetric=None, max_iter=30, tol=1e-12), False),
    ("n10_g0", 45, (10, 10), undirected, dict(max_iter=30, tol=1e-12), True),
    ("eps002_n12", 46, (12, 12), undirected, dict(epsilon=0.02, max_iter=40, tol=1e-12), False),
    ("stop_n12", 47, (12, 12), undirected, dict(epsilon=0.3, max_iter=100, tol=1e-3), False),
    ("zerop_9x11", 48, (9, 11), undirected, dict(max_iter=20, tol=1e-12), False),
]
LOSS = ("n12", "kl_n10")
NAN = "nan_n10"
KEYS = ("dM", "dC1", "dC2", "dp", "dq", "dG0")
GRADS = [f"{tag}_{k}" for tag in ("gT", "gd", "gl") for k in KEYS]


class ExpCount:
    def __enter__(self):
        self.n, self._o = 0, torch.exp

        def exp(*a, **k):
            self.n += 1
            return self._o(*a, **k)

        torch.exp = exp
        return self

    def __exit__(self, *exc):
        torch.exp = self._o


def run(d, prm, W, with_loss=False):
    """d: M, C1, C2, p, q, optional G0 (numpy); prm: the reference's keywords -> T, dist, iters, errs, tmin and the gradients."""
    leaf = lambda v: torch.from_numpy(np.asarray(v)).to(torch.float64).requires_grad_(True)
    M, C1, C2, p, q = (leaf(d[k]) for k in ("M", "C1", "C2", "p", "q"))
    G0 = leaf(d["G0"]) if d.get("G0") is not None else None
    with ExpCount() as cnt:
        T, log = ref_breg.fgw_bregman(M, C1, C2, p, q, loss_fun=prm["loss_fun"], epsilon=prm["epsilon"], symmetric=prm["symmetric"], alpha=prm["alpha"],
                                      G0=G0, max_iter=prm["max_iter"], tol=prm["tol"], log=True)
    Wt = torch.from_numpy(np.asarray(W)).to(torch.float64)
    ins = [M, C1, C2, p, q] + ([] if G0 is None else [G0])
    Tn = T.detach().numpy()
    mass = (np.asarray(d["p"])[:, None] > 0) & (np.asarray(d["q"])[None, :] > 0)
    out = dict(T=Tn, dist=np.float64(log["fgw_dist"].item()), iters=np.int32(cnt.n // 2), errs=np.array([float(e) for e in log["err"]]),
               tmin=np.float64(Tn[mass].min()) if np.isfinite(Tn).all() else np.float64(np.nan))
    objs = [("gT", (Wt * T).sum()), ("gd", log["fgw_dist"])] + ([("gl", log["loss"])] if with_loss else [])
    for tag, obj in objs:
        gs = torch.autograd.grad(obj, ins, retain_graph=True)
        for k, g in zip(KEYS, gs):
            out[f"{tag}_{k}"] = g.numpy()
    return out


def relabelled(d, prm, W, r, seed, with_loss):
    """The largest grad_error between the run r and a run on the relabelled problem (None when that run counts differently)."""
    n1, n2 = d["M"].shape
    g = np.random.default_rng(977 + seed)
    p1, p2 = g.permutation(n1), g.permutation(n2)
    e = dict(M=d["M"][p1][:, p2], C1=d["C1"][p1][:, p1], C2=d["C2"][p2][:, p2], p=d["p"][p1], q=d["q"][p2])
    if d.get("G0") is not None:
        e["G0"] = d["G0"][p1][:, p2]
    r2 = run(e, prm, W[p1][:, p2], with_loss)
    if int(r2["iters"]) != int(r["iters"]):
        return None
    idx = dict(dM=(p1, p2), dC1=(p1, p1), dC2=(p2, p2), dp=(p1,), dq=(p2,), dG0=(p1, p2))
    worst = 0.0
    for k in GRADS:
        if k in r:
            ix = idx[k[3:]]
            u = np.empty_like(r[k])
            if len(ix) == 2:
                u[np.ix_(*ix)] = r2[k]
            else:
                u[ix[0]] = r2[k]
            worst = max(worst, grad_error(u, r[k], W if k[:2] == "gT" else 1.0))
    return worst


def tol_rule(prm, r):
    """tol so small that the solve ran to max_iter, or at least 1e-6; and no evaluated error within a factor 2 of it."""
    tol, e = prm["tol"], r["errs"]
    clear = bool(np.all((e > 2 * tol) | (e < tol / 2)))
    return clear and ((int(r["iters"]) == prm["max_iter"] and bool(np.all(e > 2 * tol))) or tol >= 1e-6)


def determined(d, prm, W, r, seed, with_loss=False):
    moved = relabelled(d, prm, W, r, seed, with_loss)
    finite = all(np.isfinite(r[k]).all() for k in GRADS if k in r) and np.isfinite(r["T"]).all()
    return finite and moved is not None and moved <= 1e-10 and tol_rule(prm, r), moved


def weights(shape):
    return np.random.default_rng(W_SEED).standard_normal(shape).astype(np.float32)


def write(name, rec):
    path = os.path.join(HERE, f"fgw_bregman_unrollgrad_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= LIMIT, (name, os.path.getsize(path), LIMIT)
    return os.path.getsize(path) // 1024


def prm_record(prm):
    return dict(symmetric=np.int32(SYM_CODE[prm["symmetric"]]), loss_fun=np.array(prm["loss_fun"]), alpha=np.float64(prm["alpha"]),
                epsilon=np.float64(prm["epsilon"]), max_iter=np.int32(prm["max_iter"]), tol=np.float64(prm["tol"]))


def load_pair(src, over):
    g = np.load(os.path.join(HERE, f"fgw_pair_{src}.npz"))
    d = dict(M=g["M"], C1=g["C1"].astype(np.float32), C2=g["C2"].astype(np.float32), p=g["p"], q=g["q"], G0=g["G0"] if g["G0"].size else None)
    prm = dict(loss_fun=str(g["loss_fun"]), epsilon=float(g["epsilon"]), symmetric=SYM[int(g["symmetric"])], alpha=float(g["alpha"]),
               max_iter=int(g["max_iter"]), tol=float(g["tol"]))
    prm.update(over)
    return g, d, prm


def save_reused(name, src, over):
    g, d, prm = load_pair(src, over)
    W = weights(d["M"].shape)
    r = run(d, prm, W.astype(np.float64), name in LOSS)
    if not over:
        assert float(r["dist"]) == float(g["r64_fgw_dist"]) and int(r["iters"]) == int(g["r64_it"]), name
    ok, moved = determined(d, prm, W.astype(np.float64), r, 0, name in LOSS)
    assert ok, (name, "not determined", moved, r["errs"])
    kb = write(name, dict(src=np.array(src), W=W, **prm_record(prm), **r))
    print(f"{name}: {kb} KB iters {int(r['iters'])} errs {r['errs'][-2:]} relabelled {moved:.1e} tmin {float(r['tmin']):.3g} |gd_dM| {np.linalg.norm(r['gd_dM']):.3g}")


def save_new(name, seed, shape, graph, over, with_g0):
    prm = dict(BASE); prm.update(over)
    for seed in range(seed, seed + 3000, 100):
        d = inputs(*shape, graph, seed=seed)
        if graph in (sym_float, dir_float):
            rng = np.random.RandomState(seed + 7)
            d["C1"], d["C2"] = graph(rng, shape[0]), graph(rng, shape[1])
        if with_g0:
            d["G0"] = projected_start(d)
        W = weights(d["M"].shape)
        extra = {}
        if name.startswith("zerop"):
            p = d["p"].astype(np.float64); p[ZERO_AT] = 0.0
            d["p"] = (p / p.sum()).astype(np.float32)
            keep = np.array([i for i in range(shape[0]) if i != ZERO_AT])
            e = dict(M=d["M"][keep], C1=d["C1"][keep][:, keep], C2=d["C2"], p=d["p"][keep], q=d["q"])
            rr = run(e, prm, W.astype(np.float64)[keep])
            ok, moved = determined(e, prm, W.astype(np.float64)[keep], rr, seed)
            r = dict(rr)
            for k in GRADS + ["T"]:                                        # embed: exact zeros at the absent node
                if k not in rr:
                    continue
                kind = k.split("_")[-1]
                if kind in ("dM", "T"):
                    u = np.zeros(shape); u[keep] = rr[k]
                elif kind == "dC1":
                    u = np.zeros((shape[0], shape[0])); u[np.ix_(keep, keep)] = rr[k]
                elif kind == "dp":
                    u = np.zeros(shape[0]); u[keep] = rr[k]
                else:
                    u = rr[k]
                r[k] = u
            full = run(d, prm, W.astype(np.float64))
            assert np.isnan(full["T"]).all(), "the reference's plan on the full problem is expected to be NaN"
            extra = dict(ref_full_T=full["T"])
        else:
            r = run(d, prm, W.astype(np.float64), name in LOSS)
            ok, moved = determined(d, prm, W.astype(np.float64), r, seed, name in LOSS)
        if name.startswith("eps002"):
            ok = ok and bool((r["T"] == 0).any())
        if name.startswith("stop"):
            ok = ok and int(r["iters"]) in (11, 21)
        print(f"   {name} seed {seed}: ok {ok} (relabelled {moved}, iters {int(r['iters'])}, errs {r['errs'][-3:]}, zeros {int((r['T'] == 0).sum())})")
        if ok:
            break
    else:
        raise AssertionError((name, "no finite and determined case found"))
    is01 = lambda a: bool(np.all((a == 0) | (a == 1)))
    small = lambda a: a.astype(np.uint8) if is01(a) else a
    kb = write(name, dict(src=np.array(""), input_seed=np.int32(seed), W=W, M=d["M"], C1=small(d["C1"]), C2=small(d["C2"]), p=d["p"], q=d["q"],
                          G0=d["G0"] if with_g0 else np.zeros((0, 0), np.float32), **prm_record(prm), **extra, **r))
    print(f"{name} (seed {seed}): {kb} KB iters {int(r['iters'])} tmin {float(r['tmin']):.3g} zeros {int((r['T'] == 0).sum())}")


def save_nan():
    prm = dict(BASE); prm.update(epsilon=5e-4, max_iter=20, tol=1e-12)
    seed = 51
    d = inputs(10, 10, undirected, seed=seed)
    d["M"] = (d["M"] + np.float32(1.5)).astype(np.float32)
    W = weights(d["M"].shape)
    f = lambda k: d[k].astype(np.float64)
    T0 = np.outer(f("p"), f("q"))
    x = -(-2 * prm["alpha"] * (f("C1") @ T0 @ (2 * f("C2")).T) + (1 - prm["alpha"]) * f("M")) / prm["epsilon"]
    assert d["M"].min() >= 1.0 and x.max() < -900.0, (d["M"].min(), x.max())
    r = run(d, prm, W.astype(np.float64))
    assert np.isnan(r["T"]).all() and all(np.isnan(r[k]).all() for k in GRADS if k in r)
    kb = write(NAN, dict(src=np.array(""), input_seed=np.int32(seed), W=W, M=d["M"], C1=d["C1"].astype(np.uint8), C2=d["C2"].astype(np.uint8), p=d["p"],
                         q=d["q"], G0=np.zeros((0, 0), np.float32), **prm_record(prm), T=r["T"], dist=r["dist"], iters=r["iters"], errs=r["errs"],
                         first_x_max=np.float64(x.max())))
    print(f"{NAN} (seed {seed}): {kb} KB iters {int(r['iters'])} largest exponent of the first half-step {x.max():.1f}")


def main():
    only = sys.argv[1:]
    for case in REUSED:
        if not only or case[0] in only:
            save_reused(*case)
    for case in NEW:
        if not only or case[0] in only:
            save_new(*case)
    if not only or NAN in only:
        save_nan()


if __name__ == "__main__":
    main()
