"""Generates tests/golden/fgw_unrollgrad_*.npz: torch autograd through the reference's own fgw (bregman.py:8-167, PGD / PPA around
sinkhorn_log), in fp64, on fp32-rounded inputs: the yardstick of the unrolled pairwise FGW gradient (csrc/fgw_pair_grad.hip,
ops.fgw_pair_unrolled).

RUNS ONLY IN THE BUILD CONTAINER (needs the reference).  It imports the reference's function (through make_fgw_golden's helpers); no reference
source is copied.  One file per case, data only.  REUSED cases take the inputs and parameters of tests/golden/fgw_pair_<name>.npz (src = that
name; asserted: the reference reproduces its r64_fgw_dist exactly) and store the gradients only; NEW cases store their inputs under the same
keys as those files.  Every file holds W (standard normal, fp32), iters (the outer iterations the reference ran), sweeps (the Sinkhorn sweeps
of every outer iteration: torch.logsumexp calls / 2), sk_errs (every evaluated Sinkhorn error), dist, T and, with every input a leaf, the
gradients of two objectives,
    gT_*:  sum(W * T)            gd_*:  log["fgw_dist"]
to M, C1, C2, p, q and, where a start is given, G0.

Every finite fixture must be DETERMINED: a second reference run on the relabelled problem (a seeded permutation of each graph: every sum then
runs in another order) takes the same iterations and sweeps and reproduces the gradients, relabelled back, to 1e-10
(tests/fgw_acc_grad_ref.grad_error), and no evaluated Sinkhorn error lies within 1e-6 relative of stopThr.  A new case that fails either is
replaced by the next seed's (+100); a reused one that fails stops the script.

Zero weight (zerop_9x11, p[3] = 0): the reference's log(0) potential makes its dp[3] NaN (0 * inf), and its first half-sweep of every Sinkhorn
call still counts the massless row.  The project treats the node as absent: the yardstick stored is the reference run on the problem WITHOUT
that node, embedded with exact zeros at the node's rows / columns.  What the reference gives on the full problem is kept beside it: ref_full_dp
(its dp, NaN at the node) and ref_full_gap (the largest grad_error of its other gradients against the stored ones: the difference of convention).

NaN (nan_ppa_n10: a new 10 x 10 PPA pair at epsilon = 0.01, 30 iterations): entries of the plan underflow to exact zero in fp64 and log(T)
of the next iteration makes every gradient NaN in the reference.  The inputs of fgw_pair_ppa_n10 (71 iterations) do that too, but their one
offending entry crosses the border in steps of 10 in the log domain: -744 (a denormal) after iteration 57, -754.7 after iteration 58.  A NaN
case that hangs on a denormal is worthless, so the stored case is searched by seed for: in the first input plan that holds an exact zero, every
zero entry has its log-domain value Mr + f + g below -800 (exp underflows to zero at -745.13; log_zero_max), and no entry of an earlier plan
lies below -700 (denormals begin at -708.4; log_lowest_before).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_pair_unrolled_golden.py [name ...]
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

from make_fgw_golden import ref_bary, ref_breg  # noqa: E402  (imports the reference)
from make_fgw_pair_golden import SYM_CODE, inputs, undirected  # noqa: E402
from fgw_acc_grad_ref import grad_error  # noqa: E402
import fgw_pair_unrolled_ref as R  # noqa: E402

W_SEED = 2424
ZERO_AT = 3
SYM = {1: True, 0: False, -1: None}
REUSED = ["pgd_1x5", "pgd_model_n20", "pgd_n10", "pgd_n10_cap25", "pgd_n10_g0", "pgd_rect_7x12", "pgd_dir_n12_false", "pgd_dir_n12_none",
          "pgd_undir_n12_none", "pgd_n33", "pgd_n80", "ppa_dir_n80_false"]
BASE = dict(loss_fun="square_loss", epsilon=0.1, symmetric=True, alpha=0.5, max_iter=100, tol=1e-5, solver="PGD", numItermax=100, stopThr=1e-5)
NEW = [
    # name, seed, (n1, n2), graph, overrides
    ("ppa_12x9", 21, (12, 9), undirected, dict(solver="PPA", max_iter=20)),
    ("zerop_9x11", 22, (9, 11), undirected, dict(max_iter=20)),
]
NAN = "nan_ppa_n10"


class Trace:
    """Per Sinkhorn call of the reference: its sweeps (torch.logsumexp calls / 2) and every error it evaluated (its torch.norm calls)."""
    def __enter__(self):
        self.sweeps, self.errs = [], []
        self._o = (torch.logsumexp, torch.norm, ref_breg.sinkhorn)
        lse0, norm0, sk0 = self._o
        st = {"lse": 0, "in": False}

        def lse(*a, **k):
            st["lse"] += 1
            return lse0(*a, **k)

        def norm(*a, **k):
            out = norm0(*a, **k)
            if st["in"]:
                self.errs.append(float(out))
            return out

        def sinkhorn(*a, **k):
            st["lse"], st["in"] = 0, True
            out = sk0(*a, **k)
            st["in"] = False
            self.sweeps.append(st["lse"] // 2)
            return out

        torch.logsumexp, torch.norm, ref_breg.sinkhorn = lse, norm, sinkhorn
        return self

    def __exit__(self, *exc):
        torch.logsumexp, torch.norm, ref_breg.sinkhorn = self._o


def run(d, prm, W):
    """d: M, C1, C2, p, q, optional G0 (numpy); prm: the reference's keywords -> T, dist, iters, sweeps, sk_errs and the gradients."""
    leaf = lambda v: torch.from_numpy(np.asarray(v)).to(torch.float64).requires_grad_(True)
    M, C1, C2, p, q = (leaf(d[k]) for k in ("M", "C1", "C2", "p", "q"))
    G0 = leaf(d["G0"]) if d.get("G0") is not None else None
    with Trace() as tr:
        T, log = ref_bary.fgw(M, C1, C2, p, q, loss_fun=prm["loss_fun"], epsilon=prm["epsilon"], symmetric=prm["symmetric"], alpha=prm["alpha"], G0=G0,
                              max_iter=prm["max_iter"], tol=prm["tol"], solver=prm["solver"], log=True, numItermax=prm["numItermax"],
                              stopThr=prm["stopThr"])
    Wt = torch.from_numpy(np.asarray(W)).to(torch.float64)
    ins = [M, C1, C2, p, q] + ([] if G0 is None else [G0])
    out = dict(T=T.detach().numpy(), dist=np.float64(log["fgw_dist"].item()), iters=np.int32(len(tr.sweeps)), sweeps=np.array(tr.sweeps, np.int32),
               sk_errs=np.array(tr.errs))
    for tag, obj in (("gT", (Wt * T).sum()), ("gd", log["fgw_dist"])):
        gs = torch.autograd.grad(obj, ins, retain_graph=True)
        for k, g in zip(("dM", "dC1", "dC2", "dp", "dq", "dG0"), gs):
            out[f"{tag}_{k}"] = g.numpy()
    return out


GRADS = [f"{tag}_{k}" for tag in ("gT", "gd") for k in ("dM", "dC1", "dC2", "dp", "dq", "dG0")]


def relabelled(d, prm, W, r, seed):
    """The largest grad_error between the run r and a run on the relabelled problem (None when that run counts differently)."""
    n1, n2 = d["M"].shape
    g = np.random.default_rng(977 + seed)
    p1, p2 = g.permutation(n1), g.permutation(n2)
    e = dict(M=d["M"][p1][:, p2], C1=d["C1"][p1][:, p1], C2=d["C2"][p2][:, p2], p=d["p"][p1], q=d["q"][p2])
    if d.get("G0") is not None:
        e["G0"] = d["G0"][p1][:, p2]
    r2 = run(e, prm, W[p1][:, p2])
    if list(r2["sweeps"]) != list(r["sweeps"]):
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


def determined(d, prm, W, r, seed):
    moved = relabelled(d, prm, W, r, seed)
    margin = np.abs(r["sk_errs"] - prm["stopThr"]).min() / prm["stopThr"] if len(r["sk_errs"]) else 1.0
    finite = all(np.isfinite(r[k]).all() for k in GRADS if k in r)
    return finite and moved is not None and moved <= 1e-10 and margin > 1e-6, moved, margin


def weights(shape):
    return np.random.default_rng(W_SEED).standard_normal(shape).astype(np.float32)


def write(name, rec):
    path = os.path.join(HERE, f"fgw_unrollgrad_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 512 * 1024, (name, os.path.getsize(path))
    return os.path.getsize(path) // 1024


def prm_record(prm):
    return dict(solver=np.array(prm["solver"]), symmetric=np.int32(SYM_CODE[prm["symmetric"]]), loss_fun=np.array(prm["loss_fun"]),
                alpha=np.float64(prm["alpha"]), epsilon=np.float64(prm["epsilon"]), max_iter=np.int32(prm["max_iter"]), tol=np.float64(prm["tol"]),
                num_iter_max=np.int32(prm["numItermax"]), stop_thr=np.float64(prm["stopThr"]))


def load_pair(name):
    g = np.load(os.path.join(HERE, f"fgw_pair_{name}.npz"))
    d = dict(M=g["M"], C1=g["C1"].astype(np.float32), C2=g["C2"].astype(np.float32), p=g["p"], q=g["q"], G0=g["G0"] if g["G0"].size else None)
    prm = dict(loss_fun=str(g["loss_fun"]), epsilon=float(g["epsilon"]), symmetric=SYM[int(g["symmetric"])], alpha=float(g["alpha"]),
               max_iter=int(g["max_iter"]), tol=float(g["tol"]), solver=str(g["solver"]), numItermax=int(g["num_iter_max"]), stopThr=float(g["stop_thr"]))
    return g, d, prm


def save_reused(name):
    g, d, prm = load_pair(name)
    W = weights(d["M"].shape)
    r = run(d, prm, W.astype(np.float64))
    assert float(r["dist"]) == float(g["r64_fgw_dist"]) and int(r["iters"]) == int(g["r64_it"]) and int(r["sweeps"].sum()) == int(g["r64_sk"]), name
    ok, moved, margin = determined(d, prm, W.astype(np.float64), r, 0)
    assert ok, (name, "not determined", moved, margin)
    kb = write(name, dict(src=np.array(name), W=W, **r))
    print(f"{name}: {kb} KB iters {int(r['iters'])} sweeps {list(r['sweeps'])} relabelled {moved:.1e} margin {margin:.1e} |gd_dM| {np.linalg.norm(r['gd_dM']):.3g}")


def save_new(name, seed, shape, graph, over):
    prm = dict(BASE); prm.update(over)
    for seed in range(seed, seed + 1000, 100):
        d = inputs(*shape, graph, seed=seed)
        W = weights(d["M"].shape)
        extra = {}
        if name.startswith("zerop"):
            p = d["p"].astype(np.float64); p[ZERO_AT] = 0.0
            d["p"] = (p / p.sum()).astype(np.float32)
            keep = np.array([i for i in range(shape[0]) if i != ZERO_AT])
            e = dict(M=d["M"][keep], C1=d["C1"][keep][:, keep], C2=d["C2"], p=d["p"][keep], q=d["q"])
            rr = run(e, prm, W.astype(np.float64)[keep])
            ok, moved, margin = determined(e, prm, W.astype(np.float64)[keep], rr, seed)
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
            gap = 0.0
            for k in GRADS:
                if k in r and not k.endswith("dp"):
                    f = np.array(full[k])
                    if k.endswith("dM"):
                        f[ZERO_AT] = 0.0
                    if k.endswith("dC1"):
                        f[ZERO_AT] = 0.0; f[:, ZERO_AT] = 0.0
                    gap = max(gap, grad_error(np.nan_to_num(f, nan=1e300), r[k], W if k[:2] == "gT" else 1.0))
            extra = dict(ref_full_dp=np.stack([full["gT_dp"], full["gd_dp"]]), ref_full_gap=np.float64(gap), ref_full_sweeps=full["sweeps"])
        else:
            r = run(d, prm, W.astype(np.float64))
            ok, moved, margin = determined(d, prm, W.astype(np.float64), r, seed)
        print(f"   {name} seed {seed}: determined {ok} (relabelled {moved}, margin {margin:.1e})")
        if ok:
            break
    else:
        raise AssertionError((name, "no finite and determined case found"))
    kb = write(name, dict(src=np.array(""), input_seed=np.int32(seed), W=W, M=d["M"], C1=d["C1"].astype(np.uint8), C2=d["C2"].astype(np.uint8), p=d["p"],
                          q=d["q"], G0=np.zeros((0, 0), np.float32), **prm_record(prm), **extra, **r))
    print(f"{name} (seed {seed}): {kb} KB iters {int(r['iters'])} sweeps {list(r['sweeps'])} " + " ".join(f"{k} {v}" for k, v in extra.items() if np.ndim(v) == 0))


def zero_entries(d, prm, r):
    """The restatement's replay of the run r: (k, largest log-domain value Mr + f + g among the entries that are exactly zero) for the first
    input plan T_k, k < iters, that has one, and the smallest log-domain value of a non-zero entry of the plans before it (None: no zero)."""
    t = lambda v: torch.from_numpy(np.asarray(v)).to(torch.float64)
    M, C1, C2, p, q = (t(d[k]) for k in ("M", "C1", "C2", "p", "q"))
    live = (p[:, None] > 0) & (q[None, :] > 0)
    const = R._consts(C1, C2, p, q, prm["alpha"], True)
    T, low = p[:, None] * q[None, :], 0.0
    for k in range(int(r["iters"]) - 1):                                   # the plans that are inputs of a later iteration's log
        tens = R._tens(M, C1, C2, T, const, prm["alpha"], prm["epsilon"], True, True, live)
        Mr = -tens / prm["epsilon"]
        ref = Mr.max(0).values
        us, vs = R.sinkhorn_sweeps(R._kernel(tens, prm["epsilon"], live), p, q, prm["numItermax"], prm["stopThr"], int(r["sweeps"][k]))
        logT = Mr - ref[None, :] + torch.log(us[-1])[:, None] + torch.log(vs[-1])[None, :]
        T = torch.exp(logT)
        if (T == 0).any():
            return k, float(logT[T == 0].max()), low
        low = min(low, float(logT.min()))
    return None


def save_nan():
    """A 10 x 10 PPA pair at epsilon = 0.01: the plan loses about a hundred in the log domain per iteration at its smallest entries."""
    prm = dict(BASE); prm.update(solver="PPA", epsilon=0.01, max_iter=30, tol=1e-12)
    g, d0, prm0 = load_pair("ppa_n10")
    r0 = run(d0, prm0, weights(d0["M"].shape).astype(np.float64))
    print(f"   (fgw_pair_ppa_n10, the issue's candidate: first zero (iteration, log, lowest before) = {zero_entries(d0, prm0, r0)}: at the border, not used)")
    for seed in range(31, 1031, 100):
        d = inputs(10, 10, undirected, seed=seed)
        W = weights(d["M"].shape)
        r = run(d, prm, W.astype(np.float64))
        z = zero_entries(d, prm, r)
        nan = all(np.isnan(r[k]).all() for k in GRADS if k in r)
        print(f"   {NAN} seed {seed}: all NaN {nan}, first zero (iteration, log, lowest before) {z}")
        # every entry that is zero in the first plan with a zero is far below the border (-745.13), every entry before it is a normal number (> -708.4)
        if nan and np.isfinite(r["T"]).all() and z is not None and z[1] < -800.0 and z[2] > -700.0:
            break
    else:
        raise AssertionError((NAN, "no case found"))
    kb = write(NAN, dict(src=np.array(""), input_seed=np.int32(seed), W=W, M=d["M"], C1=d["C1"].astype(np.uint8), C2=d["C2"].astype(np.uint8), p=d["p"],
                         q=d["q"], G0=np.zeros((0, 0), np.float32), **prm_record(prm), T=r["T"], dist=r["dist"], iters=r["iters"], sweeps=r["sweeps"],
                         sk_errs=r["sk_errs"], first_zero_iter=np.int32(z[0]), log_zero_max=np.float64(z[1]), log_lowest_before=np.float64(z[2])))
    print(f"{NAN} (seed {seed}): {kb} KB iters {int(r['iters'])} first exact zero after iteration {z[0]}, its largest log {z[1]:.1f}, lowest log before {z[2]:.1f}")


def main():
    only = sys.argv[1:]
    for name in REUSED:
        if not only or name in only:
            save_reused(name)
    for case in NEW:
        if not only or case[0] in only:
            save_new(*case)
    if not only or NAN in only:
        save_nan()


if __name__ == "__main__":
    main()
