"""Generates tests/golden/mixup_grad_*.npz: gradients of the FGWMixup barycenter (the reference's fgw_barycenters_BAPG, barycenter.py:259-390)
in the fixed-plan convention, for the loss  sum(Y * gw) + sum(C * gc)  (gw, gc: normal draws of the recorded seeds).

The reference runs fused_ACC_torch with autograd on, so its own .backward() unrolls every epoch of every coupling solve.  The project holds the
couplings of the last outer iteration constant, as the reference's fgw_barycenters does (barycenter.py:120).  That gradient is taken from the
reference's own functions: per case and precision
    1. run the reference's fgw_barycenters_BAPG(log=True) on plain tensors and take T = [t.detach() for t in log["T"]];
    2. with every input a fresh leaf, recompute Y and C with the reference's update_feature_matrix and update_square_loss / update_kl_loss at
       that T (or take init_Y / init_C under fixed_features / fixed_structure), the last steps of its loop (barycenter.py:352-362);
    3. assert that these are the run's returned Y and C, bit for bit;
    4. back-propagate the loss; the names of the inputs whose .grad is filled are recorded in `grads`, the others stay None.

RUNS ONLY IN THE BUILD CONTAINER (needs the reference).  It imports the reference's own functions (through make_fgw_golden's helpers) and records
inputs plus T, Y, C and the gradients in fp32 ("r32") and fp64 ("r64").  No reference source is copied.

Every fixture is asserted FINITE, FAIR in the sense of tests/fgw_mixup_ref.fair (no relative objective change near eps, no outer error near tol,
in both precisions, and the same number of outer iterations in both) and STABLE as make_fgw_mixup_golden.py has it (the fp32 run within 1e-3 of
the fp64 run in Y and C).  A case that is not is replaced by the next seed's (+100), never exempted.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_mixup_grad_golden.py [name ...]
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

from make_fgw_golden import ref_bary  # noqa: E402  (imports the reference)
from make_fgw_grad_golden import case  # noqa: E402
from make_fgw_mixup_golden import EPS, Counter, rel_changes  # noqa: E402
from fgw_mixup_ref import fair  # noqa: E402

GW_SEED, GC_SEED = 7, 8
DEFAULTS = dict(alpha=0.5, rho=1.0, max_iter=100, tol=1e-9, loss_fun="square_loss", fixed_structure=False, fixed_features=False)


def run_ref(inp, N, dtype, prm):
    sizes = [int(n) for n in inp["sizes"]]
    K = len(sizes)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)

    def inputs():
        Ysl = [t(inp["Ys"][s, :sizes[s]]) for s in range(K)]
        Csl = [t(inp["Cs"][s, :sizes[s], :sizes[s]]) for s in range(K)]
        psl = [t(inp["ps"][s, :sizes[s]]) for s in range(K)]
        opt = lambda k: t(inp[k]) if k in inp else None
        return Ysl, Csl, psl, opt("p"), opt("lambdas"), t(inp["init_C"]), opt("init_Y")

    Ysl, Csl, psl, p, lam, ic, iy = inputs()
    with Counter() as cnt:
        Y0, C0, log = ref_bary.fgw_barycenters_BAPG(N, Ysl, Csl, ps=psl, p=p, lambdas=lam, init_C=ic, init_Y=iy, log=True, **prm)
    T = [x.detach() for x in log["T"]]
    outer = len(log["err_feature"])
    compared = [v for c in cnt.calls for v in rel_changes(c[1])]
    errs = [float(e) for k, fixed in (("err_feature", prm["fixed_features"]), ("err_structure", prm["fixed_structure"])) if not fixed for e in log[k]]

    # the last update steps on fresh leaves, at the run's couplings
    Ysl, Csl, psl, p, lam, ic, iy = [[x.requires_grad_(True) for x in v] if isinstance(v, list) else (None if v is None else v.requires_grad_(True))
                                     for v in inputs()]
    pp = p if p is not None else torch.ones(N, dtype=dtype) / N
    ll = lam if lam is not None else [1.0 / K] * K
    if prm["fixed_features"]:
        Y = iy
    else:
        Y = ref_bary.update_feature_matrix(ll, [y.T for y in Ysl], T, pp).T
    if prm["fixed_structure"]:
        C = ic
    else:
        C = (ref_bary.update_square_loss if prm["loss_fun"] == "square_loss" else ref_bary.update_kl_loss)(pp, ll, T, Csl)
    assert torch.equal(Y.detach(), Y0.detach()) and torch.equal(C.detach(), C0.detach()), "the recomputed last steps are not the run's Y, C"
    gw = torch.from_numpy(np.random.RandomState(GW_SEED).normal(size=tuple(Y.shape))).to(dtype)
    gc = torch.from_numpy(np.random.RandomState(GC_SEED).normal(size=tuple(C.shape))).to(dtype)
    ((Y * gw).sum() + (C * gc).sum()).backward()

    n_max = inp["Ys"].shape[1]
    Tn = np.zeros((K, N, n_max))
    for s in range(K):
        Tn[s, :, :sizes[s]] = T[s].numpy()
    out = dict(Y=Y.detach().numpy(), C=C.detach().numpy(), T=Tn)
    grads = []
    if Ysl[0].grad is not None:
        dYs = np.zeros(inp["Ys"].shape)
        for s in range(K):
            dYs[s, :sizes[s]] = Ysl[s].grad.numpy()
        out["dYs"] = dYs; grads.append("Ys")
    if Csl[0].grad is not None:
        dCs = np.zeros(inp["Cs"].shape)
        for s in range(K):
            dCs[s, :sizes[s], :sizes[s]] = Csl[s].grad.numpy()
        out["dCs"] = dCs; grads.append("Cs")
    for name, leaf in (("p", p), ("lambdas", lam), ("init_C", ic), ("init_Y", iy)):
        if leaf is not None and leaf.grad is not None:
            out["d" + name] = leaf.grad.numpy(); grads.append(name)
    assert all(q.grad is None for q in psl)
    return out, grads, outer, compared, errs


def with_ps(inp, seed, given):
    """ps [K,n_max] zero-padded: uniform over each graph's own nodes, or (given) seeded positive weights."""
    sizes = [int(n) for n in inp["sizes"]]
    rng = np.random.RandomState(seed + 7)
    ps = np.zeros((len(sizes), max(sizes)), np.float32)
    for s, n in enumerate(sizes):
        w = rng.uniform(0.5, 1.5, n) if given else np.ones(n)
        ps[s, :n] = w / w.sum()
    inp["ps"] = ps
    return inp


CASES = [
    # name, seed, arguments of make_fgw_grad_golden.case, given ps, the reference's keywords
    # (max_iter: with the default 100 and tol 1e-9 the fp32 run never meets tol on these inputs and takes all 100 outer iterations where the
    # fp64 run takes about 20: not fair.  Every case caps the outer loop, as most mixup_bary_* fixtures do; the rest of the first is default.)
    ("k3_n10_d4", 71, dict(K=3, n=10, d=4), False, dict(max_iter=5)),
    ("kl_k3_n10_d4", 72, dict(K=3, n=10, d=4), False, dict(loss_fun="kl_loss", rho=4.0, max_iter=5)),          # (rho 1.0: checks near eps at seeds 72 and 272, not stable at 172)
    ("k3_n10_d4_dir", 73, dict(K=3, n=10, d=4, directed=True), False, dict(rho=4.0, max_iter=5)),
    ("k3_n10_d4_fixedC", 174, dict(K=3, n=10, d=4, fixed_C=True), False, dict(fixed_structure=True, rho=4.0, max_iter=5)),          # (seed 74 passes at 6e-4 in Y: a wide yardstick)
    ("k3_n10_d4_fixedY", 75, dict(K=3, n=10, d=4, fixed_Y=True), False, dict(fixed_features=True, rho=4.0, max_iter=5)),
    ("k5_n33_d8_weights", 76, dict(K=5, n=33, d=8, p=True, lambdas=True), True, dict(rho=4.0, max_iter=5)),
    ("ragged_N7", 77, dict(K=3, n=0, d=3, N=7, sizes=[9, 6, 8], p=True, lambdas=True), False, dict(rho=4.0, max_iter=5)),
    ("k2_n66_d4", 78, dict(K=2, n=66, d=4, p=True, lambdas=True), False, dict(rho=4.0, max_iter=3)),
]


def save(name, inp, N, seed, over):
    prm = dict(DEFAULTS); prm.update(over)
    r64, g64, outer64, cmp64, errs64 = run_ref(inp, N, torch.float64, prm)
    r32, g32, outer32, cmp32, errs32 = run_ref(inp, N, torch.float32, prm)
    for r in (r32, r64):
        if not all(np.isfinite(v).all() for v in r.values()):
            return False
    if outer32 != outer64 or not (fair(cmp64, EPS) and fair(cmp32, EPS) and fair(errs64, prm["tol"]) and fair(errs32, prm["tol"])):
        return False          # not FAIR: counts could not be compared (the caller replaces the case)
    rel = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    if max(rel(r32["Y"], r64["Y"]), rel(r32["C"], r64["C"])) > 1e-3:
        return False          # not STABLE
    assert g32 == g64, (g32, g64)
    rec = dict(inp)
    rec["Cs"] = inp["Cs"].astype(np.uint8)
    rec.update(N=np.int32(N), input_seed=np.int32(seed), alpha=np.float64(prm["alpha"]), rho=np.float64(prm["rho"]), max_iter=np.int32(prm["max_iter"]),
               tol=np.float64(prm["tol"]), fixed_structure=np.int32(prm["fixed_structure"]), fixed_features=np.int32(prm["fixed_features"]),
               loss_fun=np.array(prm["loss_fun"]), gw_seed=np.int32(GW_SEED), gc_seed=np.int32(GC_SEED), grads=np.array(g64), outer=np.int32(outer64))
    for tag, rr in (("r32", r32), ("r64", r64)):
        for k, v in rr.items():
            rec[f"{tag}_{k}"] = v.astype(np.float32) if tag == "r32" else v
    path = os.path.join(HERE, f"mixup_grad_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 256 * 1024, (name, os.path.getsize(path))
    print(f"{name} (seed {seed}): {os.path.getsize(path) // 1024} KB outer={outer64} grads={g64} " + " ".join(f"{k}={rel(r32[k], r64[k]):.1e}" for k in r64))
    return True


def main():
    only = sys.argv[1:]
    for name, seed, kw, given_ps, over in CASES:
        if only and name not in only:
            continue
        for seed in range(seed, seed + 1000, 100):          # a case that is not finite, fair and stable is replaced by the next seed's
            kw_ = dict(kw)
            inp, N = case(seed, kw_.pop("K"), kw_.pop("n"), kw_.pop("d"), **kw_)
            if save(name, with_ps(inp, seed, given_ps), N, seed, over):
                break
        else:
            raise AssertionError((name, "no finite, fair and stable case found"))


if __name__ == "__main__":
    main()
