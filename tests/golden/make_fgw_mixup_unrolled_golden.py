"""Generates tests/golden/grad_mixup_unrolled_*.npz: the reference's OWN gradient of the FGWMixup barycenter — torch autograd through its
fgw_barycenters_BAPG (barycenter.py:259-390), i.e. through every epoch of every fused_ACC_torch call of every outer iteration — which
fgw.fgw_barycenters_BAPG_unrolled delivers (the mixup_grad_* fixtures hold the fixed-plan gradient of fgw_barycenters_BAPG instead).

RUNS ONLY IN THE BUILD CONTAINER (needs the reference).  It imports the reference's own function (through make_fgw_golden's helpers) and
copies no reference source.  Per case: fp32-rounded inputs, then ONE fp64 run with every input a leaf (ps, and uniform p / lambdas, are passed
explicitly, as the fp32 values of 1 / N and 1 / K, and their gradients stored).  Stored: Y, C, the last T, the outer count, every solve's epoch count [outer,K], and for the three
losses  sum(Y * gw)  ("gY_"),  sum(C * gc)  ("gC_")  and their sum ("gB_") the gradients to Ys, Cs, ps, p, lambdas, init_C and init_Y.

Every fixture is asserted FINITE, FAIR (fgw_mixup_ref.fair on every compared objective change against eps and on every outer error against
tol) and DETERMINED: a second run on the problem with every graph's nodes and the barycenter's nodes relabelled reproduces all gradients,
relabelled back, to 1e-10 in grad_error.  A case that fails one of the three is replaced by the next seed's (+100), never exempted.

The zero-weight case (`zero_ps`): node ZERO_AT of graph 0 has ps = 0, is isolated in Cs[0] and sits far away in feature space, so that the
reference's 1e-10 lift of its column (the project never lifts a massless entry) reaches the other entries only through factors below
e^-40.  What remains is the node's own entries: the reference gives dps there a finite value and 1e-10-sized rows of dYs / dCs (3e-10 of
the gradient's norm, asserted below 1e-9).  The fixture stores the project's exact zeros at that node and keeps the reference's values
aside (ref_at_zero_weight, ref_max_abs_zeroed).
The tol case (`tol_stop`): the maker picks tol between two outer errors of a run without tol, so that the loop leaves before max_iter.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_mixup_unrolled_golden.py [name ...]
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
from make_fgw_mixup_grad_golden import with_ps  # noqa: E402
from fgw_mixup_ref import fair  # noqa: E402
from fgw_acc_grad_ref import grad_error  # noqa: E402

GW_SEED, GC_SEED = 7, 8
ZERO_AT = 2
DEFAULTS = dict(alpha=0.5, rho=4.0, max_iter=3, tol=1e-9, loss_fun="square_loss", fixed_structure=False, fixed_features=False)
TAGS = ("gY", "gC", "gB")

CASES = [
    # name, seed, arguments of make_fgw_grad_golden.case, given ps, the reference's keywords
    ("k3_n10_d4", 71, dict(K=3, n=10, d=4), False, dict(rho=1.0)),
    ("k3_n10_d4_dir", 73, dict(K=3, n=10, d=4, directed=True), False, {}),
    ("ragged_N7", 77, dict(K=3, n=0, d=3, N=7, sizes=[9, 6, 8], p=True, lambdas=True), False, {}),
    ("k5_n33_d8_weights", 76, dict(K=5, n=33, d=8, p=True, lambdas=True), False, {}),
    ("k2_n66_d4", 78, dict(K=2, n=66, d=4, p=True, lambdas=True), False, dict(max_iter=2)),      # above the backward's LDS bound (61): streamed
    ("fixedC", 174, dict(K=3, n=10, d=4, fixed_C=True), False, dict(fixed_structure=True)),
    ("fixedY", 75, dict(K=3, n=10, d=4, fixed_Y=True), False, dict(fixed_features=True)),
    ("kl", 72, dict(K=3, n=10, d=4), False, dict(loss_fun="kl_loss")),
    ("given_ps", 79, dict(K=3, n=10, d=4, p=True), True, {}),
    ("zero_ps", 80, dict(K=3, n=9, d=4, p=True), True, {}),
    ("tol_stop", 81, dict(K=3, n=10, d=4), False, dict(max_iter=6)),
]


def run(inp, N, prm, gw=None, gc=None):
    sizes = [int(n) for n in inp["sizes"]]
    K = len(sizes)
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64).requires_grad_(True)
    Ysl = [leaf(inp["Ys"][s, :sizes[s]]) for s in range(K)]
    Csl = [leaf(inp["Cs"][s, :sizes[s], :sizes[s]]) for s in range(K)]
    psl = [leaf(inp["ps"][s, :sizes[s]]) for s in range(K)]
    p = leaf(inp["p"] if "p" in inp else np.full(N, 1.0 / N, np.float32))          # (uniform weights too are fp32 values: what the GPU is given)
    lam = leaf(inp["lambdas"] if "lambdas" in inp else np.full(K, 1.0 / K, np.float32))
    ic = leaf(inp["init_C"])
    iy = leaf(inp["init_Y"]) if "init_Y" in inp else None
    with Counter() as cnt:
        Y, C, log = ref_bary.fgw_barycenters_BAPG(N, Ysl, Csl, ps=psl, p=p, lambdas=lam, init_C=ic, init_Y=iy, log=True, **prm)
    outer = len(log["err_feature"])
    assert len(cnt.calls) == outer * K
    epochs = np.array([c[0] // 2 for c in cnt.calls], np.int32).reshape(outer, K)          # (kl: the update's own exp rounds away)
    compared = [v for c in cnt.calls for v in rel_changes(c[1])]
    errs = [float(e) for k, fixed in (("err_feature", prm["fixed_features"]), ("err_structure", prm["fixed_structure"])) if not fixed for e in log[k]]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)          # the cotangents are stored, and used, as fp32 values
    gw = f32(np.random.RandomState(GW_SEED).normal(size=tuple(Y.shape))) if gw is None else gw
    gc = f32(np.random.RandomState(GC_SEED).normal(size=tuple(C.shape))) if gc is None else gc
    n_max = inp["Ys"].shape[1]
    T = np.zeros((K, N, n_max))
    for s in range(K):
        T[s, :, :sizes[s]] = log["T"][s].detach().numpy()
    out = dict(Y=Y.detach().numpy(), C=C.detach().numpy(), T=T, gw=gw, gc=gc, epochs=epochs)
    lY, lC = (Y * torch.from_numpy(gw)).sum(), (C * torch.from_numpy(gc)).sum()
    ins = Ysl + Csl + psl + [p, lam, ic] + ([] if iy is None else [iy])
    for tag, loss in zip(TAGS, (lY, lC, lY + lC)):
        gs = torch.autograd.grad(loss, ins, retain_graph=True, allow_unused=True)
        gs = [torch.zeros_like(x) if g is None else g for g, x in zip(gs, ins)]
        dYs, dCs, dps = np.zeros(inp["Ys"].shape), np.zeros(inp["Cs"].shape), np.zeros(inp["ps"].shape)
        for s in range(K):
            dYs[s, :sizes[s]] = gs[s].numpy()
            dCs[s, :sizes[s], :sizes[s]] = gs[K + s].numpy()
            dps[s, :sizes[s]] = gs[2 * K + s].numpy()
        out.update({f"{tag}_dYs": dYs, f"{tag}_dCs": dCs, f"{tag}_dps": dps, f"{tag}_dp": gs[3 * K].numpy(), f"{tag}_dlambdas": gs[3 * K + 1].numpy(),
                    f"{tag}_dinit_C": gs[3 * K + 2].numpy()})
        if iy is not None:
            out[f"{tag}_dinit_Y"] = gs[3 * K + 3].numpy()
    return out, outer, compared, errs


def relabelled(inp, N, prm, r, seed):
    """The largest grad_error between the run r and a run on the relabelled problem (None when that run counts differently)."""
    sizes = [int(n) for n in inp["sizes"]]
    K = len(sizes)
    g = np.random.default_rng(977 + seed)
    pb = g.permutation(N)
    pg = [g.permutation(n) for n in sizes]
    q = {k: np.array(v) for k, v in inp.items()}
    for s, n in enumerate(sizes):
        q["Ys"][s, :n] = inp["Ys"][s, :n][pg[s]]
        q["Cs"][s, :n, :n] = inp["Cs"][s, :n, :n][pg[s]][:, pg[s]]
        q["ps"][s, :n] = inp["ps"][s, :n][pg[s]]
    if "p" in inp:
        q["p"] = inp["p"][pb]
    q["init_C"] = inp["init_C"][pb][:, pb]
    if "init_Y" in inp:
        q["init_Y"] = inp["init_Y"][pb]
    r2, outer2, _, _ = run(q, N, prm, gw=r["gw"][pb], gc=r["gc"][pb][:, pb])
    if r2["epochs"].shape != r["epochs"].shape or not np.array_equal(r2["epochs"], r["epochs"]):
        return None
    worst = 0.0
    for tag in TAGS:
        cot = np.sqrt((np.linalg.norm(r["gw"]) ** 2 if tag != "gC" else 0.0) + (np.linalg.norm(r["gc"]) ** 2 if tag != "gY" else 0.0))
        for k in ("dYs", "dCs", "dps", "dp", "dlambdas", "dinit_C", "dinit_Y"):
            if f"{tag}_{k}" not in r:
                continue
            v, v2 = r[f"{tag}_{k}"], r2[f"{tag}_{k}"]
            u = np.zeros_like(v)
            if k in ("dYs", "dps"):
                for s, n in enumerate(sizes):
                    u[s, :n][pg[s]] = v2[s, :n]
            elif k == "dCs":
                for s, n in enumerate(sizes):
                    u[s, :n, :n][np.ix_(pg[s], pg[s])] = v2[s, :n, :n]
            elif k in ("dp", "dinit_Y"):
                u[pb] = v2
            elif k == "dinit_C":
                u[np.ix_(pb, pb)] = v2
            else:
                u = v2
            worst = max(worst, grad_error(u, v, cot))
    return worst


def pick_tol(inp, N, prm):
    """tol between two outer errors of a run without tol: the loop then leaves after k + 1 < max_iter iterations (None: no fair choice)."""
    free = dict(prm); free["tol"] = 0.0
    _, outer, _, errs = run(inp, N, free)
    ef, es = errs[:outer], errs[outer:]
    m = [max(a, b) for a, b in zip(ef, es)]
    for k in range(1, outer - 1):
        tol = 2.0 * m[k]
        if all(v >= 1.5 * tol for v in m[:k]) and fair(ef[:k + 1] + es[:k + 1], tol):
            return tol, k + 1
    return None


def save(name, seed0, kw, given_ps, over):
    prm = dict(DEFAULTS); prm.update(over)
    for seed in range(seed0, seed0 + 1000, 100):
        kw_ = dict(kw)
        inp, N = case(seed, kw_.pop("K"), kw_.pop("n"), kw_.pop("d"), **kw_)
        inp = with_ps(inp, seed, given_ps)
        want_outer = prm["max_iter"]
        if name == "zero_ps":
            ps = inp["ps"].astype(np.float64)
            ps[0, ZERO_AT] = 0.0
            inp["ps"] = (ps / ps.sum(1, keepdims=True)).astype(np.float32)
            inp["Cs"][0, ZERO_AT, :] = 0.0
            inp["Cs"][0, :, ZERO_AT] = 0.0
            inp["Ys"][0, ZERO_AT, :] = 10.0
        if name == "tol_stop":
            picked = pick_tol(inp, N, prm)
            if picked is None:
                continue
            prm["tol"], want_outer = picked
        r, outer, compared, errs = run(inp, N, prm)
        finite = all(np.isfinite(v).all() for v in r.values())
        if not (finite and outer == want_outer and fair(compared, EPS) and fair(errs, prm["tol"])):
            print(f"   {name} seed {seed}: finite {finite}, outer {outer} (wanted {want_outer}), not fair or not finite")
            continue
        moved = relabelled(inp, N, prm, r, seed)
        print(f"   {name} seed {seed}: relabelled run moves the gradients by {moved}")
        if moved is not None and moved <= 1e-10:
            break
    else:
        raise AssertionError((name, "no finite, fair and determined case found"))
    ref_at_zero, ref_small = np.zeros(len(TAGS)), 0.0
    if name == "zero_ps":
        for n_, tag in enumerate(TAGS):
            ref_at_zero[n_] = r[f"{tag}_dps"][0, ZERO_AT]
            r[f"{tag}_dps"][0, ZERO_AT] = 0.0
            # the node's own entries of dYs and dCs: 1e-10-sized in the reference (its lifted column times the cotangent), exactly 0 in the
            # project: dCs[0][ZERO_AT, :] = (C_t X)[:, ZERO_AT]^T dG meets the lifted column itself at every row half-step, whatever M is.
            # Measured against the whole gradient they must stay below the 1e-9 the restatement is held to.
            for k, at in (("dYs", (0, ZERO_AT)), ("dCs", (0, ZERO_AT)), ("dCs", (0, slice(None), ZERO_AT))):
                v = r[f"{tag}_{k}"]
                ref_small = max(ref_small, float(np.linalg.norm(v[at]) / np.linalg.norm(v)))
                v[at] = 0.0
        assert ref_small < 1e-9, ref_small
    rec = dict(inp)
    rec["Cs"] = inp["Cs"].astype(np.uint8)
    rec.update(N=np.int32(N), input_seed=np.int32(seed), alpha=np.float64(prm["alpha"]), rho=np.float64(prm["rho"]), max_iter=np.int32(prm["max_iter"]),
               tol=np.float64(prm["tol"]), fixed_structure=np.int32(prm["fixed_structure"]), fixed_features=np.int32(prm["fixed_features"]),
               loss_fun=np.array(prm["loss_fun"]), outer=np.int32(outer), ref_at_zero_weight=ref_at_zero, ref_max_abs_zeroed=np.float64(ref_small),
               zero_at=np.int32(ZERO_AT if name == "zero_ps" else -1), relabelled=np.float64(moved))
    rec.update(r)
    rec["gw"], rec["gc"] = r["gw"].astype(np.float32), r["gc"].astype(np.float32)
    path = os.path.join(HERE, f"grad_mixup_unrolled_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 512 * 1024, (name, os.path.getsize(path))
    print(f"{name} (seed {seed}, relabelled {moved:.1e}): outer {outer} of {prm['max_iter']}, tol {prm['tol']:.3g}, epochs {r['epochs'].tolist()}, "
          f"|dYs| {np.linalg.norm(r['gB_dYs']):.3g} |dCs| {np.linalg.norm(r['gB_dCs']):.3g} |dps| {np.linalg.norm(r['gB_dps']):.3g} "
          f"ref dps at zero weight {ref_at_zero} (zeroed entries: {ref_small:.1e} of their gradient) {os.path.getsize(path) // 1024} KB")


def main():
    only = sys.argv[1:]
    for c in CASES:
        if not only or c[0] in only:
            save(*c)


if __name__ == "__main__":
    main()
