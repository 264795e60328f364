"""Generates tests/golden/grad_acc_*.npz: torch autograd through the reference's own fused_ACC_torch (barycenter.py:228-256), in fp64, on fp32-rounded
inputs: the yardstick of the unrolled FGWMixup gradient (csrc/fgw_acc_grad.hip, ops.fgw_acc_pair_unrolled).

RUNS ONLY IN THE BUILD CONTAINER (needs the reference).  It imports the reference's function (through make_fgw_mixup_golden's helpers, which also
build the inputs and count the epochs); no reference source is copied.  One file per case, data only: the inputs, alpha, rho, epoch, eps, the
epochs the reference ran, len(obj_list), the plan X, and with every input a leaf the gradients of two objectives,
    gX_*:  sum(W * X), W standard normal rounded to fp32 (stored)            gd_*:  the FGWMixup distance of X,
        (1 - alpha) <M, X> + alpha (<c1, X> - 2 <A X B, X>),   c1 = (A o A) a 1^T + 1 b^T (B o B)   (barycenter.py:348-350),
to M, A, B, a, b and, where a start is given, X0.  Uniform weights are passed to the reference explicitly (it forms a dot product for None)
and their gradients are stored too.

Every fixture must give a FINITE plan and finite gradients, a FAIR run (tests/fgw_mixup_ref.fair: no relative objective change near eps, so
that two fp64 implementations count the same epochs) and a DETERMINED yardstick: the reference is run a second time on the same problem with
its nodes relabelled (a seeded permutation of each graph: every sum then runs in another order) and the gradients, relabelled back, must agree
with the first run's to 1e-10 (tests/fgw_acc_grad_ref.grad_error).  The CPU test holds an fp64 restatement to these files at 1e-9: that cap
means something only where the yardstick's own fp64 rounding sits well below it.  (It does not everywhere: at rho = 0.1 the plan of a 5 x 7
pair runs into a vertex, the gradients of sum(W * X) shrink to 1e-7 of the cotangent and what is left of them is cancellation: seed 4 there
moves by 5e-8 under relabelling.)  A case that fails one of the three is replaced by the next seed's (+100), never exempted.

Zero weight (9x11_zeroa, a[3] = 0): the reference lifts the entries of that row by 1e-10 every epoch and its da[3] is a finite number, the
mean of the row's cotangent; the project treats the node as absent and delivers 0.  The fixture stores 0 there (the project's convention, as
grad_sinkhorn_zeroa does) and keeps the reference's value in ref_da_at_zero_weight; the node's row of dM and its row and column of dA, 1e-10-sized
in the reference (its lifted row times the cotangent; the largest is kept in ref_max_abs_zeroed), are stored as the project's exact 0 too.  The
node has no edges in A.  With edges the reference's
lifted row reaches the other rows through A X, 1e-8 relative in the plan's neighbourhood and in every gradient (measured: 1e-9 in X, 8e-9 in
dM): that is the documented difference of convention (ops.fgw_acc_pair_batched: a zero weight means "absent"), not arithmetic, and it would
sit above the CPU test's cap.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_acc_grad_golden.py [name ...]
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

from make_fgw_mixup_golden import EPS, Counter, pair_inputs, ref_bary, rel_changes  # noqa: E402  (imports the reference)
from fgw_mixup_ref import fair  # noqa: E402
from fgw_acc_grad_ref import grad_error  # noqa: E402

W_SEED = 4242
ZERO_AT = 3

CASES = [
    # name, seed, n1, n2, inputs, alpha, rho, epoch
    ("1x5", 3, 1, 5, {}, 0.5, 1.0, 25),
    ("5x7", 4, 5, 7, dict(weights=True), 0.5, 0.5, 25),                       # rectangular, runs out its 25 epochs
    ("5x7_stop", 4, 5, 7, dict(weights=True), 0.5, 0.1, 200),                 # small rho: stops on the objective, a data-dependent epoch count
    ("12x9_directed", 5, 12, 9, dict(directed=True, weights=True), 0.6, 0.5, 35),
    ("7x7_start", 6, 7, 7, dict(weights=True, start=True), 0.5, 0.5, 25),
    ("9x11_zeroa", 7, 9, 11, dict(weights=True), 0.5, 0.5, 25),
    ("33x33", 8, 33, 33, {}, 0.5, 1.0, 30),
    ("62x62", 9, 62, 62, dict(d=8), 0.5, 4.0, 12),                            # just above conan_fgw_acc_pair_bwd_lds_resident's bound (61): streamed
]


def distance(M, A, B, a, b, X, alpha):
    c1 = ((A * A) @ a)[:, None] + (b @ (B * B))[None, :]
    return (1 - alpha) * (M * X).sum() + alpha * ((c1 * X).sum() - 2 * (((A @ X) @ B) * X).sum())


def run(rec, alpha, rho, epoch, W=None):
    n1, n2 = rec["M"].shape
    leaf = lambda v: torch.from_numpy(np.asarray(v)).to(torch.float64).requires_grad_(True)
    M, A, B = leaf(rec["M"]), leaf(rec["A"]), leaf(rec["B"])
    a = leaf(rec["a"] if "a" in rec else np.full(n1, 1.0 / n1))
    b = leaf(rec["b"] if "b" in rec else np.full(n2, 1.0 / n2))
    X0 = leaf(rec["X0"]) if "X0" in rec else None
    with Counter() as cnt:
        X, objs = ref_bary.fused_ACC_torch(M, A, B, a, b, X0, alpha=alpha, epoch=epoch, eps=EPS, rho=rho)
    (nexp, checks), = cnt.calls
    assert nexp % 2 == 0
    W = torch.from_numpy(np.random.default_rng(W_SEED).standard_normal((n1, n2)).astype(np.float32) if W is None else W).to(torch.float64)
    ins = [M, A, B, a, b] + ([] if X0 is None else [X0])
    out = dict(X=X.detach().numpy(), W=W.numpy().astype(np.float32), epochs=np.int32(nexp // 2), stored=np.int32(len(objs)), checks=np.array(checks))
    for tag, obj in (("gX", (W * X).sum()), ("gd", distance(M, A, B, a, b, X, alpha))):
        gs = torch.autograd.grad(obj, ins, retain_graph=True)
        for k, g in zip(("dM", "dA", "dB", "da", "db", "dX0"), gs):
            out[f"{tag}_{k}"] = g.numpy()
    out["dist"] = np.float64(distance(M, A, B, a, b, X, alpha).item())
    return out


def relabelled(rec, r, alpha, rho, epoch, seed):
    """The largest grad_error between the run r and a run on the relabelled problem (None when that run counts other epochs)."""
    n1, n2 = rec["M"].shape
    g = np.random.default_rng(977 + seed)
    p1, p2 = g.permutation(n1), g.permutation(n2)
    q = dict(M=rec["M"][p1][:, p2], A=rec["A"][p1][:, p1], B=rec["B"][p2][:, p2])
    if "a" in rec:
        q["a"], q["b"] = rec["a"][p1], rec["b"][p2]
    if "X0" in rec:
        q["X0"] = rec["X0"][p1][:, p2]
    w = r["W"].astype(np.float64)
    r2 = run(q, alpha, rho, epoch, W=w[p1][:, p2])
    if int(r2["epochs"]) != int(r["epochs"]):
        return None
    back = dict(dM=lambda v: (p1, p2), dA=lambda v: (p1, p1), dB=lambda v: (p2, p2), da=lambda v: (p1,), db=lambda v: (p2,), dX0=lambda v: (p1, p2))
    worst = 0.0
    for k, v in r.items():
        if k[:3] in ("gX_", "gd_"):
            idx = back[k[3:]](v)
            u = np.empty_like(v)
            if len(idx) == 2:
                u[np.ix_(*idx)] = r2[k]
            else:
                u[idx[0]] = r2[k]
            worst = max(worst, grad_error(u, v, w if k[:2] == "gX" else 1.0))
    return worst


def save(name, seed, n1, n2, kw, alpha, rho, epoch):
    for seed in range(seed, seed + 1000, 100):
        rec = pair_inputs(seed, n1, n2, **kw)
        if name == "9x11_zeroa":
            a = rec["a"].astype(np.float64)
            a[ZERO_AT] = 0.0
            rec["a"] = (a / a.sum()).astype(np.float32)
            rec["A"][ZERO_AT, :] = 0.0
            rec["A"][:, ZERO_AT] = 0.0
        r = run(rec, alpha, rho, epoch)
        finite = all(np.isfinite(v).all() for v in r.values())
        stopped = int(r["epochs"]) < epoch
        wanted = {"5x7": False, "5x7_stop": True}.get(name, stopped)        # the pair of 5x7 cases: one runs into its cap, one leaves on the objective
        if not (finite and fair(rel_changes(list(r["checks"])), EPS) and stopped == wanted):
            continue
        moved = relabelled(rec, r, alpha, rho, epoch, seed)
        print(f"   {name} seed {seed}: relabelled run moves the gradients by {moved}")
        if moved is not None and moved <= 1e-10:
            break
    else:
        raise AssertionError((name, "no finite, fair and determined case found"))
    ref_at_zero, ref_small = np.zeros(2), 0.0
    if name == "9x11_zeroa":
        ref_at_zero = np.array([r["gX_da"][ZERO_AT], r["gd_da"][ZERO_AT]])
        for tag in ("gX", "gd"):
            # the node's own entries of dM and dA: 1e-10-sized in the reference (its lifted row times the cotangent), exactly 0 in the project
            ref_small = max(ref_small, np.abs(r[tag + "_dM"][ZERO_AT]).max(), np.abs(r[tag + "_dA"][ZERO_AT]).max(), np.abs(r[tag + "_dA"][:, ZERO_AT]).max())
            r[tag + "_da"][ZERO_AT] = 0.0
            r[tag + "_dM"][ZERO_AT] = 0.0
            r[tag + "_dA"][ZERO_AT] = 0.0
            r[tag + "_dA"][:, ZERO_AT] = 0.0
        assert ref_small < 1e-8, ref_small
    out = dict(rec, alpha=np.float64(alpha), rho=np.float64(rho), epoch=np.int32(epoch), eps=np.float64(EPS), input_seed=np.int32(seed),
               ref_da_at_zero_weight=ref_at_zero, ref_max_abs_zeroed=np.float64(ref_small), **{k: v for k, v in r.items() if k != "checks"})
    out["A"], out["B"] = rec["A"].astype(np.uint8), rec["B"].astype(np.uint8)                   # 0 / 1 adjacency
    path = os.path.join(HERE, f"grad_acc_{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 512 * 1024, (name, os.path.getsize(path))
    print(f"{name} (seed {seed}, relabelled {moved:.1e}): epochs {int(r['epochs'])} of {epoch}, stored {int(r['stored'])}, |gX_dM| {np.linalg.norm(r['gX_dM']):.3g} "
          f"|gd_dM| {np.linalg.norm(r['gd_dM']):.3g} ref da at zero weight {ref_at_zero} {os.path.getsize(path) // 1024} KB")


def main():
    only = sys.argv[1:]
    for case in CASES:
        if not only or case[0] in only:
            save(*case)


if __name__ == "__main__":
    main()
