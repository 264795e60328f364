"""Regenerates tests/golden/hists_sinkhorn_*.npz from the reference's own fgw/sinkhorn.py (imported, never copied):

    python tests/golden/make_sinkhorn_hists_golden.py --reference /path/to/conan_fgw/src/model/fgw/sinkhorn.py

Needs only torch and numpy on the CPU.  One file per case, data only: the reference's sinkhorn_knopp with b [n2,H] (one M, one a, H target
histograms, solved jointly).  Per case: M, a, b (and the warm start) rounded to fp32 first, reg (an fp32 value too), numItermax, stopThr, and
the reference's fp64 run on the widened fp32 inputs: r64_loss [H], r64_u [n1,H], r64_v [n2,H], r64_err, r64_niter, r64_warn ("" / "noconv" /
"numerr").  The joint-stop case also stores r64_niter_cols [H], the iteration counts of the H columns solved alone (1-D calls of the same
function), and early_col, a column that alone stops fairly at an earlier check than the joint run.

The fairness rule is make_sinkhorn_golden.py's, unchanged: stopped on the threshold -> last err <= 0.6 stopThr and every earlier check >=
1.5 stopThr; ran out -> last err >= 1.5 stopThr.  A seed that misses this (or the case's planned iteration count) is skipped for the next one;
the condition is never loosened.  With fp32-rounded columns the error plateaus near 3e-9 (the column masses differ from sum(a) by fp32
rounding), so every threshold here is 1e-5 or 1e-6."""
import argparse
import importlib.util
import os
import warnings

import numpy as np
import torch

from make_sinkhorn_golden import fair, problem

HERE = os.path.dirname(os.path.abspath(__file__))

# name, n1, n2, H, reg, stopThr, numItermax, planned r64 niter (None: any), variant
CASES = [
    ("1x5_h2", 1, 5, 2, 0.01, 1e-5, 100, 0, ""),
    ("7x12_h3", 7, 12, 3, 0.01, 1e-5, 100, 99, ""),                 # runs to numItermax
    ("20x25_h1", 20, 25, 1, 0.05, 1e-5, 100, None, ""),
    ("33x33_h5", 33, 33, 5, 0.05, 1e-5, 100, None, ""),
    ("33x33_h16", 33, 33, 16, 0.05, 1e-5, 100, None, ""),           # an exact MFMA tile of histograms
    ("33x33_h17", 33, 33, 17, 0.05, 1e-5, 100, None, ""),           # and one past it
    ("64x80_h33", 64, 80, 33, 0.05, 1e-6, 1000, None, "joint"),     # at least one column alone stops at an earlier check
    ("257x65_h4", 257, 65, 4, 0.02, 1e-6, 1000, None, ""),          # more rows than threads
    ("65x257_h4", 65, 257, 4, 0.02, 1e-6, 1000, None, ""),
    ("zeroa", 20, 25, 3, 0.05, 1e-5, 100, None, "zeroa"),           # one entry of a is zero
    ("warm", 33, 33, 5, 0.05, 1e-5, 100, 0, "warm"),                # warm start from a converged solve
    ("numerr", 9, 11, 3, 0.1, 1e-5, 100, 0, "bigcol"),              # one column of M at 900 reg: K^T u is zero there, in every histogram
]


def hists(n2, H, seed):
    g = np.random.default_rng(seed + 104729)
    b = g.random((n2, H)) + 0.1
    return (b / b.sum(0, keepdims=True)).astype(np.float32)


def run(ref, a, b, M, reg, it, thr, warm=None):
    t = lambda v: torch.from_numpy(np.asarray(v)).to(torch.float64)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res, log = ref.sinkhorn_knopp(t(a), t(b), t(M), reg, numItermax=it, stopThr=thr, log=True, warmstart=None if warm is None else (t(warm[0]), t(warm[1])))
    msgs = [str(x.message) for x in w]
    warn = "numerr" if any("numerical errors" in m for m in msgs) else ("noconv" if any("did not converge" in m for m in msgs) else "")
    return dict(res=res.numpy(), err=np.array([float(e) for e in log["err"]], dtype=np.float64), niter=int(log["niter"]), warn=warn,
                u=log["u"].numpy(), v=log["v"].numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's fgw/sinkhorn.py")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_sinkhorn", args.reference)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    for name, n1, n2, H, reg, thr, it, planned, variant in CASES:
        reg = float(np.float32(reg))
        for seed in range(400):
            M, a, _ = problem(n1, n2, 1000 * n1 + n2 + 7919 * seed)
            b = hists(n2, H, 1000 * n1 + n2 + 7919 * seed)
            if variant == "bigcol":
                M[:, 4] = np.float32(900.0 * reg)
            if variant == "zeroa":
                a[3] = 0.0
                a = (a / a.sum()).astype(np.float32)
            warm, extra = None, {}
            if variant == "warm":
                first = run(ref, a, b, M, reg, it, thr)
                if not (fair(first, thr, it) and first["warn"] == "" and first["niter"] < it - 1):
                    continue
                warm = (np.log(first["u"]).astype(np.float32), np.log(first["v"]).astype(np.float32))
            r = run(ref, a, b, M, reg, it, thr, warm)
            ok = fair(r, thr, it) and (planned is None or r["niter"] == planned)
            if variant == "bigcol":
                ok = ok and r["warn"] == "numerr"
            elif planned is None:
                ok = ok and r["warn"] == "" and r["niter"] > 0
            if variant == "zeroa":
                ok = ok and np.isfinite(r["res"]).all() and (r["u"][3] == 0).all()
            if ok and variant == "joint":
                cols = [run1(ref, a, b[:, k], M, reg, it, thr) for k in range(H)]
                ncols = np.array([c["niter"] for c in cols], dtype=np.int32)
                early = [k for k in range(H) if ncols[k] < r["niter"] and fair(cols[k], thr, it)]
                ok = bool(early)
                if ok:
                    assert ncols.min() < r["niter"]
                    extra = dict(r64_niter_cols=ncols, early_col=np.int32(early[0]))
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed in range gives a fair case")
        d = dict(M=M, a=a, b=b, reg=np.float32(reg), numItermax=np.int32(it), stopThr=np.float64(thr), r64_loss=r["res"], r64_u=r["u"], r64_v=r["v"],
                 r64_err=r["err"], r64_niter=np.int32(r["niter"]), r64_warn=np.array(r["warn"]), **extra)
        if warm is not None:
            d["warm_u"], d["warm_v"] = warm
        path = os.path.join(HERE, f"hists_sinkhorn_{name}.npz")
        np.savez(path, **d)
        e = r["err"]
        print(f"{name:10s} seed {seed:3d} niter {r['niter']:3d} warn '{r['warn']}' last/thr {e[-1] / thr if len(e) else float('nan'):.3g} "
              f"prev/thr {e[-2] / thr if len(e) > 1 else float('nan'):.3g} {extra.get('r64_niter_cols', '')} {os.path.getsize(path) // 1024} KB")
        assert os.path.getsize(path) < 512 * 1024


def run1(ref, a, bk, M, reg, it, thr):
    """One column alone: the reference's 1-D sinkhorn_knopp."""
    t = lambda v: torch.from_numpy(np.asarray(v)).to(torch.float64)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        _T, log = ref.sinkhorn_knopp(t(a), t(bk), t(M), reg, numItermax=it, stopThr=thr, log=True)
    msgs = [str(x.message) for x in w]
    warn = "numerr" if any("numerical errors" in m for m in msgs) else ("noconv" if any("did not converge" in m for m in msgs) else "")
    return dict(err=np.array([float(e) for e in log["err"]], dtype=np.float64), niter=int(log["niter"]), warn=warn)


if __name__ == "__main__":
    main()
