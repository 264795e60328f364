"""Regenerates tests/golden/sinkhorn_*.npz from the reference's own fgw/sinkhorn.py (imported, never copied):

    python tests/golden/make_sinkhorn_golden.py --reference /path/to/conan_fgw/src/model/fgw/sinkhorn.py

Needs only torch and numpy on the CPU.  One file per case and method, data only.  Per case: M, a, b (and the warm start) rounded to fp32 first,
reg (an fp32 value too: the C entry point takes a float), method, numItermax, stopThr; the reference's fp32 run (r32_T, r32_err, r32_niter) and
its fp64 run on the widened fp32 inputs (r64_T, r64_err, r64_niter, r64_loss, r64_log_u, r64_log_v, r64_warn: "" / "noconv" / "numerr").

The iteration count is a fair yardstick only away from the threshold, so every case must satisfy, in its fp64 run: stopped on the threshold ->
last err <= 0.6 stopThr and every earlier check >= 1.5 stopThr; ran out -> last err >= 1.5 stopThr.  A seed that misses this (or the
case's planned iteration count) is skipped for the next one; the condition is never loosened."""
import argparse
import importlib.util
import os
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# name, n1, n2, reg, stopThr, numItermax, planned r64 niter, variant
CASES = [
    ("1x5", 1, 5, 0.01, 1e-5, 100, 0, ""),
    ("7x12", 7, 12, 0.01, 1e-5, 100, 99, ""),
    ("33x33", 33, 33, 0.05, 1e-5, 100, 10, ""),
    ("64x80", 64, 80, 0.05, 1e-9, 1000, 20, ""),
    ("257x65", 257, 65, 0.02, 1e-9, 1000, 50, ""),
    ("140x140", 140, 140, 0.02, 1e-5, 100, 20, ""),
    ("9x11col", 9, 11, 0.1, 1e-5, 100, None, "bigcol"),       # one column of M at 900 reg: exp(-M / reg) underflows fp64 for that column
    ("zeroa", 20, 25, 0.05, 1e-5, 100, 20, "zeroa"),          # one entry of a is zero
    ("warm", 33, 33, 0.05, 1e-5, 100, 0, "warm"),             # warm start from a converged solve's potentials
    ("65x257", 65, 257, 0.02, 1e-9, 1000, None, "transpose"),  # the transpose of 257x65
]
METHODS = {"sinkhorn_log": "log", "sinkhorn": "knopp"}


def problem(n1, n2, seed):
    g = np.random.default_rng(seed)
    x, y = g.standard_normal((n1, 3)), g.standard_normal((n2, 3)) + 0.5
    M = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    M = (M / M.max()).astype(np.float32)
    a, b = g.random(n1) + 0.1, g.random(n2) + 0.1
    return M, (a / a.sum()).astype(np.float32), (b / b.sum()).astype(np.float32)


def run(ref, method, a, b, M, reg, it, thr, dtype, warm=None):
    t = lambda v: torch.from_numpy(np.asarray(v)).to(dtype)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        T, log = ref.sinkhorn(t(a), t(b), t(M), reg, method=method, numItermax=it, stopThr=thr, log=True,
                              warmstart=None if warm is None else (t(warm[0]), t(warm[1])))
    msgs = [str(x.message) for x in w]
    warn = "numerr" if any("numerical errors" in m for m in msgs) else ("noconv" if any("did not converge" in m for m in msgs) else "")
    lu = log["log_u"] if "log_u" in log else torch.log(log["u"])
    lv = log["log_v"] if "log_v" in log else torch.log(log["v"])
    return dict(T=T.numpy(), err=np.array([float(e) for e in log["err"]], dtype=np.float64), niter=int(log["niter"]), warn=warn,
                log_u=lu.numpy(), log_v=lv.numpy())


def fair(r, thr, it):
    e = r["err"]
    if r["warn"] == "numerr":
        return True
    if r["niter"] < it - 1 or (len(e) and e[-1] < thr):          # stopped on the threshold
        return len(e) > 0 and e[-1] <= 0.6 * thr and bool(np.all(e[:-1] >= 1.5 * thr))
    return len(e) > 0 and e[-1] >= 1.5 * thr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's fgw/sinkhorn.py")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_sinkhorn", args.reference)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    chosen = {}
    for name, n1, n2, reg, thr, it, planned, variant in CASES:
        reg = float(np.float32(reg))
        for seed in range(400):
            if variant == "transpose":
                M, a, b = chosen["257x65"]
                M, a, b = np.ascontiguousarray(M.T), b, a
            else:
                M, a, b = problem(n1, n2, 1000 * n1 + n2 + 7919 * seed)
            if variant == "bigcol":
                M[:, 4] = np.float32(900.0 * reg)
            if variant == "zeroa":
                a[3] = 0.0
                a = (a / a.sum()).astype(np.float32)
            out, ok = {}, True
            for method, tag in METHODS.items():
                warm = None
                if variant == "warm":
                    first = run(ref, method, a, b, M, reg, it, thr, torch.float64)
                    ok = ok and fair(first, thr, it) and first["niter"] < it - 1
                    warm = (first["log_u"].astype(np.float32), first["log_v"].astype(np.float32))
                r64 = run(ref, method, a, b, M, reg, it, thr, torch.float64, warm)
                ok = ok and fair(r64, thr, it)
                if ok and name == "257x65":                      # its transpose is a case too: the seed must be fair for both
                    ok = fair(run(ref, method, b, a, np.ascontiguousarray(M.T), reg, it, thr, torch.float64), thr, it)
                if not ok:
                    break
                r32 = run(ref, method, a, b, M, reg, it, thr, torch.float32, warm)
                if variant == "bigcol":
                    ok = ok and (r64["warn"] == "numerr" and r64["niter"] == 0 and r32["niter"] == 0 if tag == "knopp" else r64["niter"] == 10)
                elif planned is not None:
                    ok = ok and r64["niter"] == planned
                if variant == "zeroa":
                    ok = ok and not np.isnan(r64["T"]).any()
                out[tag] = (r64, r32, warm)
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed in range gives a fair case")
        chosen[name] = (M, a, b)
        for tag, (r64, r32, warm) in out.items():
            method = [m for m, t in METHODS.items() if t == tag][0]
            d = dict(M=M, a=a, b=b, reg=np.float32(reg), method=np.array(method), numItermax=np.int32(it), stopThr=np.float64(thr),
                     r32_T=r32["T"].astype(np.float32), r32_err=r32["err"], r32_niter=np.int32(r32["niter"]),
                     r64_T=r64["T"], r64_err=r64["err"], r64_niter=np.int32(r64["niter"]), r64_loss=np.float64((M.astype(np.float64) * r64["T"]).sum()),
                     r64_log_u=r64["log_u"], r64_log_v=r64["log_v"], r64_warn=np.array(r64["warn"]))
            if warm is not None:
                d["warm_u"], d["warm_v"] = warm
            path = os.path.join(HERE, f"sinkhorn_{name}_{tag}.npz")
            np.savez(path, **d)
            e = r64["err"]
            print(f"{name:9s} {tag:5s} seed {seed:3d} r64 niter {r64['niter']:3d} r32 niter {r32['niter']:3d} warn '{r64['warn']}' "
                  f"last/thr {e[-1] / thr if len(e) else float('nan'):.3g} prev/thr {e[-2] / thr if len(e) > 1 else float('nan'):.3g} "
                  f"{os.path.getsize(path) // 1024} KB")
            assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
