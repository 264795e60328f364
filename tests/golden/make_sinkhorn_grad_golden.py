"""Regenerates tests/golden/grad_sinkhorn_*.npz from the reference's own fgw/sinkhorn.py (imported, never copied):

    python tests/golden/make_sinkhorn_grad_golden.py --reference /path/to/conan_fgw/src/model/fgw/sinkhorn.py

Needs only torch and numpy on the CPU.  One file per case and method, data only: the reference's fp64 run on fp32-rounded inputs with
requires_grad on M, a, b and the warm start, and torch autograd's gradients of two objectives,
    g1_*:  sum(M * T)                      g2_*:  sum(M * T) + sum(dT * T),   dT standard normal rounded to fp32 (stored),
to M, a, b and warmstart[0] (dwu; zeros without a warm start), with niter, the err list and the warning of the run.  The inputs are those of
the forward fixtures (sinkhorn_<case>_<method>.npz, written by make_sinkhorn_golden.py from problem()); the row case is built here.  Every case
must pass make_sinkhorn_golden.fair(), which is never loosened.  (The files are grad_sinkhorn_*: the forward fixtures own the prefix
sinkhorn_*, and tests/test_sinkhorn_cpu.py holds that list complete.)

Zero weight (zeroa): the reference's sinkhorn_log gives NaN at exactly a.grad[3]; the fixture stores 0 there (the project's convention) and
records the fact in ref_nan_at_zero_weight.  Knopp gives NaN everywhere on that problem: no fixture.  Knopp on the underflowing column leaves at
iteration 0 on numerical errors: its plan is u0 K v0, a.grad / b.grad are None: zeros are stored."""
import argparse
import importlib.util
import os
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# name, forward fixture (None: built here), methods
CASES = [
    ("1x5", "1x5", ("log", "knopp")),
    ("7x12", "7x12", ("log", "knopp")),                 # reg 0.01: runs out its 100 sweeps
    ("33x33", "33x33", ("log", "knopp")),
    ("64x80", "64x80", ("log", "knopp")),               # more than 64 rows ... columns: lanes take two trips
    ("zeroa", "zeroa", ("log",)),                       # 20 x 25, a[3] = 0
    ("warm", "warm", ("log", "knopp")),                 # 33 x 33 warm-started: stores d warmstart[0]
    ("9x11col", "9x11col", ("log", "knopp")),           # a column at 900 reg; Knopp leaves at iteration 0 (S = 0)
    ("9x11row", None, ("log",)),                        # a ROW at 900 reg: the forward takes the exact log-domain path
]
METHOD = {"log": "sinkhorn_log", "knopp": "sinkhorn"}


def load_module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, method, a, b, M, reg, it, thr, warm, dT):
    t = lambda v: torch.from_numpy(np.asarray(v)).to(torch.float64).requires_grad_(True)
    a_, b_, M_ = t(a), t(b), t(M)
    w_ = None if warm is None else (t(warm[0]), t(warm[1]))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        T, log = ref.sinkhorn(a_, b_, M_, reg, method=method, numItermax=it, stopThr=thr, log=True, warmstart=w_)
    msgs = [str(x.message) for x in w]
    warn = "numerr" if any("numerical errors" in m for m in msgs) else ("noconv" if any("did not converge" in m for m in msgs) else "")
    r = dict(T=T.detach().numpy(), err=np.array([float(e) for e in log["err"]], dtype=np.float64), niter=int(log["niter"]), warn=warn)
    ins = [M_, a_, b_] + ([] if w_ is None else [w_[0], w_[1]])
    dTt = torch.from_numpy(dT).to(torch.float64)
    for tag, obj in (("g1", (M_ * T).sum()), ("g2", (M_ * T).sum() + (dTt * T).sum())):
        gs = torch.autograd.grad(obj, ins, retain_graph=True, allow_unused=True)
        if w_ is not None:
            assert gs[4] is None or not gs[4].any()                        # warmstart[1] gets no gradient
        z = lambda g, like: np.zeros(like.shape) if g is None else g.numpy()
        r[tag + "_dM"], r[tag + "_da"], r[tag + "_db"] = z(gs[0], M_), z(gs[1], a_), z(gs[2], b_)
        r[tag + "_dwu"] = np.zeros(a_.shape) if w_ is None else z(gs[3], a_)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's fgw/sinkhorn.py")
    args = ap.parse_args()
    ref = load_module(args.reference, "reference_sinkhorn")
    fwd = load_module(os.path.join(HERE, "make_sinkhorn_golden.py"), "make_sinkhorn_golden")

    for name, src, tags in CASES:
        for tag in tags:
            method = METHOD[tag]
            if src is not None:
                z = np.load(os.path.join(HERE, f"sinkhorn_{src}_{tag}.npz"))
                M, a, b, reg, it, thr = z["M"], z["a"], z["b"], float(z["reg"]), int(z["numItermax"]), float(z["stopThr"])
                warm = (z["warm_u"], z["warm_v"]) if "warm_u" in z.files else None
                seeds = [0]
            else:
                reg, it, thr, warm, seeds = float(np.float32(0.1)), 100, 1e-5, None, range(400)
            for seed in seeds:
                if src is None:
                    M, a, b = fwd.problem(9, 11, 1000 * 9 + 11 + 7919 * seed)
                    M[4, :] = np.float32(900.0 * reg)
                dT = np.random.default_rng(4242 + seed).standard_normal(M.shape).astype(np.float32)      # an fp32 input like M, a, b
                r = run(ref, method, a, b, M, reg, it, thr, warm, dT)
                if fwd.fair(r, thr, it):
                    break
            else:
                raise SystemExit(f"{name}: no seed in range gives a fair case")
            nan_at = False
            if name == "zeroa":
                for k in ("g1_da", "g2_da"):
                    bad = np.isnan(r[k])
                    assert bad[3] and bad.sum() == 1, (k, bad)
                    r[k][3] = 0.0
                nan_at = True
            for k, v in r.items():
                if k.startswith("g"):
                    assert np.isfinite(v).all(), (name, tag, k)
            d = dict(M=M, a=a, b=b, reg=np.float32(reg), method=np.array(method), numItermax=np.int32(it), stopThr=np.float64(thr), dT=dT,
                     r64_T=r["T"], r64_err=r["err"], r64_niter=np.int32(r["niter"]), r64_warn=np.array(r["warn"]),
                     ref_nan_at_zero_weight=np.bool_(nan_at), **{k: v for k, v in r.items() if k.startswith("g")})
            if warm is not None:
                d["warm_u"], d["warm_v"] = warm
            path = os.path.join(HERE, f"grad_sinkhorn_{name}_{tag}.npz")
            np.savez(path, **d)
            print(f"{name:8s} {tag:5s} niter {r['niter']:3d} warn '{r['warn']}' max|da| {np.abs(r['g1_da']).max():.3g} "
                  f"max|dwu| {np.abs(r['g2_dwu']).max():.3g} {os.path.getsize(path) // 1024} KB")
            assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
