"""The reference's other three Sinkhorn solvers (greenkhorn, sinkhorn_stabilized, sinkhorn_epsilon_scaling), what needs no GPU: the stored fixtures
(tests/golden/ext_sinkhorn_*.npz, written by tests/golden/make_sinkhorn_ext_golden.py) are complete, the fp64 restatement
tests/sinkhorn_ext_ref.py reproduces every one of them (counts equal, plans to 1e-10 relative), every fixture satisfies the conditions under
which iteration counts can be compared between two implementations, the C entry points are declared, answer their host-side queries and refuse
bad arguments before any launch, and the public functions refuse what they do not build."""
import ctypes
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, ops
from conan_fgw_amd import sinkhorn as sk

from sinkhorn_ext_ref import epsilon_scaling_ref, greenkhorn_fair, greenkhorn_ref, stabilized_ref
from sinkhorn_ref import fair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ["1x5", "7x12", "33x33", "64x80", "65x257", "257x65", "140x140"]
STAB = [f"stab_{s}" for s in SHAPES] + ["stab_7x12_r01", "stab_33x33_r01", "stab_64x80_r01", "stab_tau10", "stab_pp7", "stab_cap", "stab_warm",
                                        "stab_zeroa", "stab_bigcol"]
EPS = ["eps_7x12", "eps_33x33", "eps_33x33_r01", "eps_140x140", "eps_warm", "eps_clamp"]
GK = [f"gk_{s}" for s in SHAPES] + ["gk_warm", "gk_zeroa", "gk_cap"]
NAMES = STAB + EPS + GK


def load(name):
    z = np.load(os.path.join(GOLDEN, f"ext_sinkhorn_{name}.npz"))
    return {k: z[k] for k in z.files}


def restate(f):
    """The restatement's run of a fixture -> (T, log)."""
    warm = (f["warm_u"], f["warm_v"]) if "warm_u" in f else None
    method, it, thr, reg = str(f["method"]), int(f["numItermax"]), float(f["stopThr"]), float(f["reg"])
    if method == "greenkhorn":
        return greenkhorn_ref(f["a"], f["b"], f["M"], reg, it, thr, warm)
    if method == "sinkhorn_stabilized":
        return stabilized_ref(f["a"], f["b"], f["M"], reg, it, float(f["tau"]), thr, warm, int(f["print_period"]))
    return epsilon_scaling_ref(f["a"], f["b"], f["M"], reg, it, float(f["epsilon0"]), int(f["numInnerItermax"]), float(f["tau"]), thr, warm,
                               int(f["print_period"]))


def test_fixture_list_is_complete():
    have = sorted(os.path.basename(p)[len("ext_sinkhorn_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "ext_sinkhorn_*.npz")))
    assert have == sorted(NAMES)
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, f"ext_sinkhorn_{name}.npz")) < 512 * 1024
        f = load(name)
        assert f["M"].dtype == f["a"].dtype == f["b"].dtype == f["r32_T"].dtype == f["reg"].dtype == np.float32 and f["r64_T"].dtype == np.float64
        for key in ("tau", "epsilon0"):
            assert key not in f or f[key].dtype == np.float32
    # what the cases are there for
    assert all(int(load(f"stab_{s}")["r64_absorptions"]) == 0 for s in SHAPES)
    assert all(int(load(n)["r64_absorptions"]) >= 1 for n in ("stab_7x12_r01", "stab_33x33_r01", "stab_64x80_r01"))
    assert int(load("stab_tau10")["r64_absorptions"]) >= 5 and int(load("stab_pp7")["print_period"]) == 7
    assert str(load("stab_cap")["r64_warn"]) == "noconv" and int(load("stab_cap")["r64_niter"]) == int(load("stab_cap")["numItermax"]) - 1
    assert load("stab_zeroa")["a"][3] == 0 and load("gk_zeroa")["a"][3] == 0
    assert int(load("eps_clamp")["numItermax"]) < 35 and int(load("eps_clamp")["r64_niter"]) == 34 and str(load("eps_clamp")["r64_warn"]) == "noconv"
    assert all(int(load(n)["r64_niter"]) == 36 for n in EPS if n != "eps_clamp")
    assert str(load("gk_cap")["r64_warn"]) == "noconv" and int(load("gk_cap")["r64_niter"]) == int(load("gk_cap")["numItermax"]) - 1
    assert all(str(load(n)["r64_warn"]) == "" and int(load(n)["r64_niter"]) < 400 for n in GK if n != "gk_cap")


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_fp64_run(name):
    f = load(name)
    T, log = restate(f)
    method = str(f["method"])
    assert log["n_iter" if method != "sinkhorn_epsilon_scaling" else "niter"] == int(f["r64_niter"]) and log["warn"] == str(f["r64_warn"])
    ref = f["r64_T"]
    mask = np.isnan(ref)
    assert np.array_equal(np.isnan(T), mask)
    if not mask.all():
        assert np.linalg.norm((T - ref)[~mask]) <= 1e-10 * np.linalg.norm(ref[~mask])
        assert abs(log["loss"] - float(f["r64_loss"])) <= 1e-10 * abs(float(f["r64_loss"]))
    if method == "greenkhorn":
        np.testing.assert_allclose(log["u"], f["r64_u"], rtol=1e-10)
        np.testing.assert_allclose(log["v"], f["r64_v"], rtol=1e-10)
        return
    # An error is a norm of differences between marginals and sums of n positive entries of Gamma, each the exp of an argument of magnitude up to
    # ~50 (M / reg, alpha / reg, log u) and so carrying up to 50 eps relative; the sums add n eps in an order that depends on the machine.  Two
    # correct fp64 evaluations of a norm therefore differ by up to 64 n eps (||a|| + ||b||).  The outer error of epsilon scaling is a sum of two
    # squared norms: d(e^2) = 2 e de.
    floor = 64 * max(f["M"].shape) * np.finfo(np.float64).eps * float(np.linalg.norm(f["a"].astype(np.float64)) + np.linalg.norm(f["b"].astype(np.float64)))
    floor = 2 * np.sqrt(f["r64_err"]) * floor + floor ** 2 if method == "sinkhorn_epsilon_scaling" else floor
    assert len(log["err"]) == len(f["r64_err"])
    got, want = np.array(log["err"]), f["r64_err"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    with np.errstate(invalid="ignore"):
        assert np.all(np.isnan(want) | (np.abs(got - want) <= 1e-7 * np.abs(want) + floor)), (got, want)
    with np.errstate(invalid="ignore"):
        for key in ("alpha", "beta"):
            x, y = log[key], f["r64_" + key]
            ok = np.isfinite(y)
            assert np.array_equal(x[~ok], y[~ok], equal_nan=True) and np.allclose(x[ok], y[ok], rtol=0, atol=1e-10)
    if method == "sinkhorn_stabilized":
        assert log["absorptions"] == int(f["r64_absorptions"])
    else:
        assert [x["n_iter"] for x in log["inner"]] == list(f["r64_inner_niter"])
        assert [x["absorptions"] for x in log["inner"]] == list(f["r64_inner_absorptions"])
        assert [x["warn"] == "noconv" for x in log["inner"]] == list(f["r64_inner_noconv"]) and log["ncap"] == int(f["r64_inner_noconv"].sum())
        assert log["sweeps"] == int((f["r64_inner_niter"] + 1).sum())


@pytest.mark.parametrize("name", STAB + EPS)
def test_error_lists_stay_away_from_the_threshold(name):
    """Condition (a): sinkhorn_ref.fair on the error list of a stabilized run and of every inner solve of epsilon scaling."""
    f = load(name)
    thr = float(f["stopThr"])
    if name in STAB:
        assert fair(list(f["r64_err"]), int(f["r64_niter"]), int(f["numItermax"]), thr, str(f["r64_warn"]))
        if str(f["r64_warn"]) == "":
            assert f["r64_err"][-1] <= thr
        return
    cap = int(f["numInnerItermax"])
    for k in range(len(f["r64_inner_niter"])):
        errs = [e for e in f["r64_inner_err"][k] if not np.isnan(e)]
        assert fair(errs, int(f["r64_inner_niter"][k]), cap, thr, "numerr" if f["r64_inner_numerr"][k] else ""), (k, errs)
        assert (errs[-1] >= thr) == bool(f["r64_inner_noconv"][k])
    e = f["r64_err"]
    assert not np.any((e > 0.6 * thr) & (e < 1.5 * thr))                  # the outer list decides the exit at ii = 36


@pytest.mark.parametrize("name", GK)
def test_greenkhorn_decisions_have_margin(name):
    """Conditions (b) and (c), on the restatement's record of the run (held to the reference's run above)."""
    f = load(name)
    _, log = restate(f)
    thr, it = float(f["stopThr"]), int(f["numItermax"])
    s, g = log["stop_vals"], log["gaps"]
    assert len(s) == len(g) == log["n_iter"] + 1 and min(g) >= 1e-9
    if str(f["r64_warn"]) == "":
        assert s[-1] <= thr / 1.001 and min(s[:-1]) >= 1.001 * thr
    else:
        assert log["n_iter"] == it - 1 and min(s) >= 1.001 * thr
    assert greenkhorn_fair(s, g, log["n_iter"], it, thr, str(f["r64_warn"]) == "")


def test_signatures_and_host_queries():
    for name in ("conan_sinkhorn_ext_workspace_bytes", "conan_sinkhorn_ext_lds_resident", "conan_sinkhorn_ext_nerr", "conan_sinkhorn_ext_fwd"):
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.conan_abi_version() == 6
    assert L.conan_sinkhorn_ext_lds_resident(33, 33) == 1 and L.conan_sinkhorn_ext_lds_resident(257, 65) == 1 and L.conan_sinkhorn_ext_lds_resident(65, 257) == 1
    assert L.conan_sinkhorn_ext_lds_resident(140, 140) == 0 and L.conan_sinkhorn_ext_lds_resident(0, 5) == 0 and L.conan_sinkhorn_ext_lds_resident(5, -1) == 0
    for n1, n2 in ((140, 139), (140, 138), (140, 140), (64, 300), (64, 305), (7, 2800)):      # the documented limit
        assert L.conan_sinkhorn_ext_lds_resident(n1, n2) == int((16 + 4 * n1 + 4 * n2 + n1 * (n2 | 1)) * 8 <= 160 * 1024)
    w = [L.conan_sinkhorn_ext_workspace_bytes(B, 200, 300) for B in (1, 2, 7)]
    assert w[0] >= 200 * 301 * 8 and w[0] < w[1] < w[2]                   # streamed: a copy of the matrix per problem
    assert all(L.conan_sinkhorn_ext_workspace_bytes(B, 33, 33) > 0 for B in (1, 64))
    for bad in ((0, 5, 5), (-1, 5, 5), (1, 0, 5), (1, 5, 0)):
        assert L.conan_sinkhorn_ext_workspace_bytes(*bad) == 0
    assert L.conan_sinkhorn_ext_nerr(2, 10000, 20) == 0 and L.conan_sinkhorn_ext_nerr(3, 1000, 20) == 50 and L.conan_sinkhorn_ext_nerr(3, 15, 7) == 3
    assert L.conan_sinkhorn_ext_nerr(4, 10, 10) == 4 and L.conan_sinkhorn_ext_nerr(4, 100, 10) == 10           # numItermax = max(35, numItermax)
    assert L.conan_sinkhorn_ext_nerr(1, 10, 10) == -1 and L.conan_sinkhorn_ext_nerr(3, 0, 10) == -1 and L.conan_sinkhorn_ext_nerr(3, 10, 0) == -1


def ext_rc(L, good, **kw):
    a = dict(good, **kw)
    return L.conan_sinkhorn_ext_fwd(a["M"], None, None, None, None, None, None, a["B"], a["N1"], a["N2"], a["stride"], a["reg"], a["method"], a["it"],
                                    a["thr"], a["tau"], a["pp"], a["eps0"], a["inner"], a["T"], None, None, None, None, None, None, None, None, a["ws"],
                                    a.get("stream"))


BAD_ARGUMENTS = [dict(M=None), dict(T=None), dict(ws=None), dict(B=0), dict(B=-1), dict(N1=0), dict(N2=-3), dict(it=0), dict(it=-5), dict(reg=0.0),
                 dict(reg=-1.0), dict(reg=float("inf")), dict(reg=float("nan")), dict(method=1), dict(method=0), dict(method=5), dict(method=-1),
                 dict(stride=-1), dict(thr=float("nan")), dict(method=3, tau=0.0), dict(method=3, tau=float("nan")), dict(method=4, tau=-1.0),
                 dict(method=3, pp=0), dict(method=4, pp=-2), dict(method=4, inner=0), dict(method=4, eps0=float("inf")),
                 dict(method=4, eps0=float("nan"))]


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(M=p, B=1, N1=4, N2=4, stride=16, reg=0.1, method=3, it=10, thr=1e-9, tau=1e3, pp=20, eps0=1e4, inner=100, T=p, ws=p)
    for kw in BAD_ARGUMENTS:
        assert ext_rc(L, good, **kw) == -1, kw
    assert L.conan_sinkhorn_fwd(p, None, None, None, None, None, None, 1, 4, 4, 16, 0.1, 2, 10, 1e-5, p, None, None, None, None, None, p, None) == -1


def test_public_signatures_are_the_references():
    want = {"greenkhorn": dict(numItermax=10000, stopThr=1e-9, verbose=False, log=False, warn=True, warmstart=None),
            "sinkhorn_stabilized": dict(numItermax=1000, tau=1e3, stopThr=1e-9, warmstart=None, verbose=False, print_period=20, log=False, warn=True),
            "sinkhorn_epsilon_scaling": dict(numItermax=100, epsilon0=1e4, numInnerItermax=100, tau=1e3, stopThr=1e-9, warmstart=None, verbose=False,
                                             print_period=10, log=False, warn=True)}
    for name, defaults in want.items():
        ps = inspect.signature(getattr(sk, name)).parameters
        assert list(ps)[:4] == ["a", "b", "M", "reg"]
        public = [k for k, p in ps.items() if p.default is not inspect.Parameter.empty and not k.startswith("_")]
        assert public == list(defaults) and all(ps[k].default == v for k, v in defaults.items()), name
    assert set(ops.SINKHORN_EXT_METHODS) == set(want) and set(ops.SINKHORN_METHODS) == {"sinkhorn_log", "sinkhorn"}


def test_public_refusals_touch_no_tensor():
    a, b, M = torch.ones(3) / 3, torch.ones(4) / 4, torch.rand(3, 4)
    fns = (sk.greenkhorn, sk.sinkhorn_stabilized, sk.sinkhorn_epsilon_scaling)
    for fn in fns:
        with pytest.raises(NotImplementedError, match="several histograms"):
            fn(a, torch.ones(4, 2) / 4, M, 0.1)
        with pytest.raises(NotImplementedError, match="not implemented for CPU tensors.*runs on the GPU only"):
            fn(a, b, M, 0.1)
    for m in ("greenkhorn", "sinkhorn_stabilized", "sinkhorn_epsilon_scaling", "GREENKHORN", "Sinkhorn_Epsilon_Scaling"):
        with pytest.raises(NotImplementedError, match="not implemented"):
            sk.sinkhorn(a, b, M, 0.1, method=m)
        with pytest.raises(NotImplementedError, match="several histograms"):
            sk.sinkhorn(a, torch.ones(4, 2) / 4, M, 0.1, method=m)
    with pytest.raises(NotImplementedError, match="not implemented"):
        sk.sinkhorn2(a, b, M, 0.1, method="Sinkhorn_Stabilized")
    for m in ("greenkhorn", "sinkhorn_epsilon_scaling"):                   # as the reference's sinkhorn2
        with pytest.raises(ValueError, match="Unknown method"):
            sk.sinkhorn2(a, b, M, 0.1, method=m)
    for fn in (ops.sinkhorn_ext_batched, ops.sinkhorn_ext_loss):
        with pytest.raises(NotImplementedError, match="runs on the GPU only"):
            fn(M[None], reg=0.1, method="greenkhorn")
        for m in ("sinkhorn", "sinkhorn_log", "nope"):
            with pytest.raises(ValueError, match="Unknown method"):
                fn(M[None], reg=0.1, method=m)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.sinkhorn_ext_list([M], reg=0.1, method="sinkhorn_stabilized")
