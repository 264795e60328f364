"""Regenerates tests/golden/ext_sinkhorn_*.npz from the reference's own fgw/sinkhorn.py (imported, never copied): its greenkhorn,
sinkhorn_stabilized and sinkhorn_epsilon_scaling.

    python tests/golden/make_sinkhorn_ext_golden.py --reference /path/to/conan_fgw/src/model/fgw/sinkhorn.py

(The files are not called sinkhorn_ext_*: tests/test_sinkhorn_cpu.py takes every sinkhorn_*.npz for a fixture of the first two methods.)
Needs only torch and numpy on the CPU.  One file per case, data only.  Per case: M, a, b (and the warm start) rounded to fp32 first; reg, tau and
epsilon0 fp32-representable; the reference's fp32 run (r32_T, r32_niter) and its fp64 run on the widened fp32 inputs (r64_*: plan, iteration
index, warning, loss, and the solver's log).  What the reference does not report is counted around it: absorptions as the pairs of torch.full
calls it makes beyond the initial one, the inner solves of epsilon scaling by wrapping its sinkhorn_stabilized at call time.

Iteration counts are a fair yardstick only away from the thresholds, so a seed is taken only if, in its fp64 run,
  (a) every error list (stabilized, every inner solve of epsilon scaling, and the outer list) keeps a factor 1.5 from stopThr: the stopping check
      <= 0.6 stopThr, every other one >= 1.5 stopThr;
  (b) a converged greenkhorn run leaves at a stopping value <= stopThr / 1.001 with every earlier one >= 1.001 stopThr (stopThr is CHOSEN that
      way from the recorded values of a longer run: the geometric mean of a new minimum and the smallest value before it);
  (c) every arg-max of a greenkhorn run is decided by a relative gap >= 1e-9.
The conditions are never loosened; a seed that misses one is skipped for the next."""
import argparse
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from sinkhorn_ext_ref import greenkhorn_fair, greenkhorn_ref      # noqa: E402  (the recorded stopping values and gaps come from the restatement)

SHAPES = [(1, 5), (7, 12), (33, 33), (64, 80), (65, 257), (257, 65), (140, 140)]
# name, n1, n2, reg, stopThr, numItermax, extra arguments, variant
STAB = [(f"stab_{n1}x{n2}", n1, n2, 0.1, 1e-9, 1000, {}, "noabs") for n1, n2 in SHAPES] + [
    ("stab_7x12_r01", 7, 12, 0.01, 1e-6, 1000, {}, "abs"),
    ("stab_33x33_r01", 33, 33, 0.01, 1e-6, 1000, {}, "abs"),
    ("stab_64x80_r01", 64, 80, 0.01, 1e-6, 1000, {}, "abs"),
    ("stab_tau10", 7, 12, 0.01, 1e-6, 1000, {"tau": 10.0}, "manyabs"),
    ("stab_pp7", 33, 33, 0.1, 1e-9, 1000, {"print_period": 7}, "noabs"),
    ("stab_cap", 33, 33, 0.01, 1e-9, 15, {}, "cap"),
    ("stab_warm", 33, 33, 0.01, 1e-6, 1000, {}, "warm"),
    ("stab_zeroa", 20, 25, 0.01, 1e-6, 1000, {}, "zeroa"),
    ("stab_bigcol", 9, 11, 0.1, 1e-6, 1000, {}, "bigcol"),
]
EPS = [
    ("eps_7x12", 7, 12, 0.1, 1e-9, 100, {"numInnerItermax": 30}, ""),
    ("eps_33x33", 33, 33, 0.1, 1e-9, 100, {"numInnerItermax": 30}, ""),
    ("eps_33x33_r01", 33, 33, 0.01, 1e-6, 100, {"numInnerItermax": 40}, ""),
    ("eps_140x140", 140, 140, 0.1, 1e-6, 100, {"numInnerItermax": 20}, ""),
    ("eps_warm", 33, 33, 0.01, 1e-6, 100, {"numInnerItermax": 40, "epsilon0": 100.0}, "warm"),
    ("eps_clamp", 7, 12, 0.1, 1e-9, 10, {"numInnerItermax": 30}, "clamp"),
]
GK = [(f"gk_{n1}x{n2}", n1, n2, 0.1, None, 400, {}, "") for n1, n2 in SHAPES] + [
    ("gk_warm", 33, 33, 0.1, None, 400, {}, "warm"),
    ("gk_zeroa", 20, 25, 0.1, None, 400, {}, "zeroa"),
    ("gk_cap", 33, 33, 0.1, 1e-9, 300, {}, "cap"),
]
NOCONV, NUMERR = "did not converge", "Numerical errors at iteration"


def problem(n1, n2, seed):
    g = np.random.default_rng(seed)
    M = g.random((n1, n2)).astype(np.float32)
    a, b = g.random(n1) + 0.1, g.random(n2) + 0.1
    return M, (a / a.sum()).astype(np.float32), (b / b.sum()).astype(np.float32)


def kind(msgs):
    return "numerr" if any(NUMERR in m for m in msgs) else ("noconv" if any(NOCONV in m for m in msgs) else "")


def fair_list(errs, thr, stopped):
    e = np.asarray(errs, dtype=np.float64)
    if len(e) == 0:
        return False
    if stopped:
        return e[-1] <= 0.6 * thr and bool(np.all(e[:-1] >= 1.5 * thr))
    return bool(np.all(e[~np.isnan(e)] >= 1.5 * thr))


def call(ref, fn, a, b, M, reg, dtype, warm=None, **kw):
    """One run of the reference -> (plan, log, warning kind, absorptions of a stabilized run, records of the inner solves of epsilon scaling)."""
    t = lambda v: torch.from_numpy(np.asarray(v)).to(dtype)
    inner, fulls, real_stab, real_full = [], [0], ref.sinkhorn_stabilized, torch.full

    def counting_full(*args, **kwargs):
        fulls[0] += 1
        return real_full(*args, **kwargs)

    def recording_stab(*args, **kwargs):
        n0 = fulls[0]
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            G, log = real_stab(*args, **kwargs)
        inner.append(dict(n_iter=int(log["n_iter"]), err=[float(e) for e in log["err"]], warn=kind([str(x.message) for x in w]),
                          absorptions=(fulls[0] - n0 - 2) // 2))
        return G, log

    torch.full = counting_full
    if fn == "sinkhorn_epsilon_scaling":
        ref.sinkhorn_stabilized = recording_stab
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            T, log = getattr(ref, fn)(t(a), t(b), t(M), reg, log=True, warmstart=None if warm is None else (t(warm[0]), t(warm[1])), **kw)
    finally:
        torch.full = real_full
        ref.sinkhorn_stabilized = real_stab
    return T.numpy(), log, kind([str(x.message) for x in w]), (fulls[0] - 2) // 2, inner


def variant_inputs(variant, n1, n2, reg, seed):
    M, a, b = problem(n1, n2, 1000 * n1 + n2 + 7919 * seed)
    if variant == "bigcol":
        M[:, 4] = np.float32(900.0 * reg)
    if variant == "zeroa":
        a[3] = 0.0
        a = (a / a.sum()).astype(np.float32)
    return M, a, b


def common(M, a, b, reg, method, it, thr, r64, r32, warm, niter_key):
    T64, log64, warn64, _, _ = r64
    d = dict(M=M, a=a, b=b, reg=np.float32(reg), method=np.array(method), numItermax=np.int32(it), stopThr=np.float64(thr),
             r64_T=T64, r64_niter=np.int32(log64[niter_key]), r64_warn=np.array(warn64), r64_loss=np.float64(np.nansum(M.astype(np.float64) * T64)),
             r32_T=r32[0].astype(np.float32), r32_niter=np.int32(r32[1][niter_key]))
    if warm is not None:
        d["warm_u"], d["warm_v"] = warm
    return d


def f32(x):
    return float(np.float32(x))


def make_stab(ref, case):
    name, n1, n2, reg, thr, it, kw, variant = case
    reg = f32(reg)
    kw = dict(kw, tau=f32(kw.get("tau", 1e3)), print_period=kw.get("print_period", 20))
    for seed in range(200):
        M, a, b = variant_inputs(variant, n1, n2, reg, seed)
        warm = None
        if variant == "warm":
            first = call(ref, "sinkhorn_stabilized", a, b, M, reg, torch.float64, numItermax=it, stopThr=1e-3, **kw)
            if first[2] != "" or not fair_list(first[1]["err"], 1e-3, True):
                continue
            warm = (first[1]["alpha"].numpy().astype(np.float32), first[1]["beta"].numpy().astype(np.float32))
        r64 = call(ref, "sinkhorn_stabilized", a, b, M, reg, torch.float64, warm, numItermax=it, stopThr=thr, **kw)
        T, log, warn, nabs, _ = r64
        errs = [float(e) for e in log["err"]]
        if warn != "numerr" and not fair_list(errs, thr, warn == ""):
            continue
        want = {"noabs": warn == "" and nabs == 0, "abs": warn == "" and nabs >= 1, "manyabs": warn == "" and nabs >= 5, "cap": warn == "noconv",
                "warm": warn == "", "zeroa": True, "bigcol": True}[variant]
        if not want:
            continue
        r32 = call(ref, "sinkhorn_stabilized", a, b, M, reg, torch.float32, warm, numItermax=it, stopThr=thr, **kw)
        d = common(M, a, b, reg, "sinkhorn_stabilized", it, thr, r64, r32, warm, "n_iter")
        d.update(tau=np.float32(kw["tau"]), print_period=np.int32(kw["print_period"]), r64_err=np.array(errs, dtype=np.float64),
                 r64_absorptions=np.int32(nabs), r64_logu=log["logu"].numpy(), r64_logv=log["logv"].numpy(), r64_alpha=log["alpha"].numpy(),
                 r64_beta=log["beta"].numpy())
        print(f"{name:16s} seed {seed:3d} n_iter {int(log['n_iter']):4d} absorptions {nabs:3d} warn '{warn}' checks {len(errs)} "
              f"last/thr {errs[-1] / thr:.3g} NaN in plan {int(np.isnan(T).sum())}")
        return name, d
    raise SystemExit(f"{name}: no seed in range gives a fair case")


def make_eps(ref, case):
    name, n1, n2, reg, thr, it, kw, variant = case
    reg = f32(reg)
    kw = dict(kw, tau=f32(kw.get("tau", 1e3)), print_period=kw.get("print_period", 10), epsilon0=f32(kw.get("epsilon0", 1e4)))
    for seed in range(200):
        M, a, b = variant_inputs(variant, n1, n2, reg, seed)
        warm = None
        if variant == "warm":
            first = call(ref, "sinkhorn_stabilized", a, b, M, f32(1.0), torch.float64, numItermax=1000, stopThr=1e-6, tau=kw["tau"])
            warm = (first[1]["alpha"].numpy().astype(np.float32), first[1]["beta"].numpy().astype(np.float32))
        r64 = call(ref, "sinkhorn_epsilon_scaling", a, b, M, reg, torch.float64, warm, numItermax=it, stopThr=thr, **kw)
        T, log, warn, _, inner = r64
        errs = np.array([float(e) for e in log["err"]], dtype=np.float64)
        if not all(x["warn"] == "numerr" or fair_list(x["err"], thr, x["warn"] == "") for x in inner):
            continue
        if np.any((errs > 0.6 * thr) & (errs < 1.5 * thr)) or np.isnan(T).any():
            continue
        if (variant == "clamp") != (warn == "noconv") or (variant == "clamp" and int(log["niter"]) != 34):
            continue
        r32 = call(ref, "sinkhorn_epsilon_scaling", a, b, M, reg, torch.float32, warm, numItermax=it, stopThr=thr, **kw)
        d = common(M, a, b, reg, "sinkhorn_epsilon_scaling", it, thr, r64, r32, warm, "niter")
        width = max(len(x["err"]) for x in inner)
        ierr = np.full((len(inner), width), np.nan)
        for k, x in enumerate(inner):
            ierr[k, :len(x["err"])] = x["err"]
        d.update(tau=np.float32(kw["tau"]), print_period=np.int32(kw["print_period"]), epsilon0=np.float32(kw["epsilon0"]),
                 numInnerItermax=np.int32(kw["numInnerItermax"]), r64_err=errs, r64_alpha=log["alpha"].numpy(), r64_beta=log["beta"].numpy(),
                 r64_inner_niter=np.array([x["n_iter"] for x in inner], dtype=np.int32), r64_inner_err=ierr,
                 r64_inner_noconv=np.array([x["warn"] == "noconv" for x in inner]), r64_inner_numerr=np.array([x["warn"] == "numerr" for x in inner]),
                 r64_inner_absorptions=np.array([x["absorptions"] for x in inner], dtype=np.int32))
        print(f"{name:16s} seed {seed:3d} niter {int(log['niter']):3d} warn '{warn}' inner solves {len(inner)} capped {int(d['r64_inner_noconv'].sum())} "
              f"sweeps {int((d['r64_inner_niter'] + 1).sum())} absorptions {int(d['r64_inner_absorptions'].sum())} errs/thr {errs / thr}")
        return name, d
    raise SystemExit(f"{name}: no seed in range gives a fair case")


def pick_threshold(stop_vals, lo, hi):
    """(step, stopThr): the latest step in [lo, hi) whose stopping value is a new minimum by more than 1 %, stopThr between it and the smallest
    value before it (fp32-representable)."""
    s = np.asarray(stop_vals)
    for k in range(min(hi, len(s)) - 1, lo - 1, -1):
        before = s[:k].min() if k else np.inf
        if s[k] > 1e-12 and s[k] * 1.01 < before:
            thr = f32(np.sqrt(s[k] * before)) if np.isfinite(before) else f32(2.0 * s[k])
            if s[k] <= thr / 1.001 and before >= 1.001 * thr:
                return k, thr
    return None


def make_gk(ref, case):
    name, n1, n2, reg, thr, it, kw, variant = case
    reg = f32(reg)
    for seed in range(200):
        M, a, b = variant_inputs(variant, n1, n2, reg, seed)
        warm = None
        if variant == "warm":
            first = call(ref, "greenkhorn", a, b, M, reg, torch.float64, numItermax=150, stopThr=0.0)
            warm = (torch.log(first[1]["u"]).numpy().astype(np.float32), torch.log(first[1]["v"]).numpy().astype(np.float32))
        case_thr = thr
        if variant != "cap":
            _, probe = greenkhorn_ref(a, b, M, reg, 320, 0.0, warm)
            got = pick_threshold(probe["stop_vals"], 0 if n1 == 1 else 100, 320)
            if got is None:
                continue
            planned, case_thr = got
        _, rl = greenkhorn_ref(a, b, M, reg, it, case_thr, warm)
        if not greenkhorn_fair(rl["stop_vals"], rl["gaps"], rl["n_iter"], it, case_thr, variant != "cap"):
            continue
        r64 = call(ref, "greenkhorn", a, b, M, reg, torch.float64, warm, numItermax=it, stopThr=case_thr)
        T, log, warn, _, _ = r64
        if int(log["n_iter"]) != (it - 1 if variant == "cap" else planned) or (warn == "noconv") != (variant == "cap"):
            continue
        r32 = call(ref, "greenkhorn", a, b, M, reg, torch.float32, warm, numItermax=it, stopThr=case_thr)
        d = common(M, a, b, reg, "greenkhorn", it, case_thr, r64, r32, warm, "n_iter")
        d.update(r64_u=log["u"].numpy(), r64_v=log["v"].numpy())
        print(f"{name:16s} seed {seed:3d} n_iter {int(log['n_iter']):4d} r32 n_iter {int(r32[1]['n_iter']):4d} warn '{warn}' stopThr {case_thr:.4g} "
              f"smallest gap {min(rl['gaps']):.2g}")
        return name, d
    raise SystemExit(f"{name}: no seed in range gives a fair case")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's fgw/sinkhorn.py")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_sinkhorn", args.reference)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for maker, cases in ((make_stab, STAB), (make_eps, EPS), (make_gk, GK)):
        for case in cases:
            name, d = maker(ref, case)
            path = os.path.join(HERE, f"ext_sinkhorn_{name}.npz")
            np.savez_compressed(path, **d)
            assert os.path.getsize(path) < 512 * 1024, (name, os.path.getsize(path))


if __name__ == "__main__":
    main()
