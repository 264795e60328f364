"""The unrolled gradient of the FGWMixup barycenter, what needs no GPU: the fp64 restatement tests/fgw_mixup_unrolled_ref.py (a hand reverse
pass: the chain over outer iterations composed with fgw_acc_grad_ref.acc_grad_ref, no autograd) reproduces torch autograd through the
reference's own fgw_barycenters_BAPG on every stored fixture (tests/golden/grad_mixup_unrolled_*.npz, written by
tests/golden/make_fgw_mixup_unrolled_golden.py) to 1e-9 in grad_error, the project's cap for restatements, which pins both the restatement and
the conditioning of the chosen cases; a central finite difference of fgw_mixup_ref.mixup_ref at fixed counts; the fixed-plan gradient is a
different quantity; the new header agrees with its _lib.EXT_TABLES entry and the library; the host-side queries answer; bad arguments are
refused before any launch; the public functions have their signatures."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

from conan_fgw_amd import _lib, fgw, ops
from conan_fgw_amd._lib import FgwParams

import fgw_mixup_unrolled_ref as R
from fgw_mixup_ref import fair, mixup_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INCLUDE = os.path.join(ROOT, "include")
NAMES = ["k3_n10_d4", "k3_n10_d4_dir", "ragged_N7", "k5_n33_d8_weights", "k2_n66_d4", "fixedC", "fixedY", "kl", "given_ps", "zero_ps", "tol_stop"]
HEADER = "conan_fgw_hip_mixup_grad.h"
EXPORTS = ("conan_fgw_mixup_barycenter_fwd_record", "conan_fgw_mixup_barycenter_bwd_lds_resident", "conan_fgw_mixup_barycenter_bwd_workspace_bytes",
           "conan_fgw_mixup_barycenter_bwd")
load = lambda name: np.load(os.path.join(GOLDEN, f"grad_mixup_unrolled_{name}.npz"))


def test_fixture_list_is_complete_and_every_fixture_is_finite_fair_and_determined():
    have = sorted(os.path.basename(p)[len("grad_mixup_unrolled_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "grad_mixup_unrolled_*.npz")))
    assert have == sorted(NAMES)
    for name in NAMES:
        g = load(name)
        assert os.path.getsize(os.path.join(GOLDEN, f"grad_mixup_unrolled_{name}.npz")) < 512 * 1024
        assert all(np.isfinite(g[k]).all() for k in g.files if g[k].dtype.kind == "f") and float(g["relabelled"]) <= 1e-10
        assert all(g[k].dtype == np.float32 for k in ("Ys", "ps", "init_C", "gw", "gc")) and g["Cs"].dtype == np.uint8
        assert g["epochs"].shape == (int(g["outer"]), len(g["sizes"])) and int(g["outer"]) <= int(g["max_iter"])
        assert all(f"{tag}_{k}" in g.files for tag in R.TAGS for k in R.GRADS[:6]) and ("gB_dinit_Y" in g.files) == ("init_Y" in g.files)
    assert load("k3_n10_d4")["epochs"].min() == 51                           # a data-dependent epoch count: the replay has to stop there too
    assert int(load("tol_stop")["outer"]) < int(load("tol_stop")["max_iter"]) and float(load("tol_stop")["tol"]) > 1e-3
    z = load("zero_ps")
    assert z["ps"][0, int(z["zero_at"])] == 0 and np.abs(z["ref_at_zero_weight"]).min() > 1.0 and float(z["ref_max_abs_zeroed"]) < 1e-9
    assert load("k2_n66_d4")["Ys"].shape[1] == 66 and load("ragged_N7")["sizes"].tolist() == [9, 6, 8]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_autograd(name):
    g = load(name)
    args, kw, N, sizes = R.fixture_problem(g)
    Np, n_max = args[0].shape[1], g["Ys"].shape[1]
    tags = R.TAGS if Np <= 12 else ("gB",)                                   # (the 33- and 66-node cases: the cotangents together, a few seconds)
    for tag in tags:
        gY, gC = R.embed_cotangents(g, tag, Np)
        r = R.mixup_unrolled_ref(*args, gY=gY, gC=gC, **kw)
        assert R.grad_error(r["Y"][:N], g["Y"]) <= 1e-12 and R.grad_error(r["C"][:N, :N], g["C"]) <= 1e-12
        assert R.grad_error(r["T"][:, :N, :n_max], g["T"]) <= 1e-12
        got = R.cut(r, N, sizes, n_max)
        for k, v in got.items():
            e = R.grad_error(v, g[f"{tag}_{k}"], R.cotangent_norm(g, tag))
            print(f"{name} {tag} {k}: {e:.2e}")
            assert e <= 1e-9, (name, tag, k, e)
        if name == "zero_ps":                                                # the massless rule: exact zeros, no division by the zero weight
            z = int(g["zero_at"])
            assert got["dps"][0, z] == 0 and not got["dYs"][0, z].any() and not got["dCs"][0, z].any() and not got["dCs"][0, :, z].any()
        if name == "ragged_N7":
            assert not r["dp"][N:].any() and not r["dinit_C"][N:].any() and all(not r["dps"][s, n:].any() for s, n in enumerate(sizes))


def test_the_restatements_counts_are_the_stopping_rules_own():
    """mixup_ref (the forward's restatement, with the stopping rules) counts what the fixtures record, on a case that stops on the objective
    and on one that stops on tol."""
    for name in ("k3_n10_d4", "tol_stop"):
        g = load(name)
        (Ys, Cs, ps, p, lam, init_C, init_Y), kw, N, sizes = R.fixture_problem(g)
        _, _, lg = mixup_ref(N, list(Ys), list(Cs), list(ps), p, lam, init_C=init_C, init_Y=init_Y, alpha=kw["alpha"], rho=kw["rho"],
                             max_iter=int(g["max_iter"]), tol=float(g["tol"]))
        assert lg["epochs"] == g["epochs"].tolist() and fair(lg["rel"], 1e-5) and fair(lg["err_feature"] + lg["err_structure"], float(g["tol"]))


def test_restatement_against_a_central_finite_difference():
    """L = sum(gw * Y) + sum(gc * C) of mixup_ref on K = 2 graphs of 5 and 4 nodes embedded in N = 5, directed, given weights and both starts,
    2 outer iterations (tol = 0) of 12 epochs each (the first objective check, at epoch 11, only stores: the counts are fixed):
    <gradient, V> against (L(x + h V) - L(x - h V)) / 2h for a random direction V of every input, h = 1e-6.  The error of a difference quotient
    is ABSOLUTE: the rounding term eps |L| / h = 2.2e-10 |L| and the truncation term h^2 L''' / 6.  Bound: 10 eps |L| / h, with every
    directional derivative required above 1e-4, orders more than the bound: a missing or mis-signed term of the chain cannot hide under it."""
    rng = np.random.default_rng(17)
    K, N, d, sizes = 2, 5, 3, [5, 4]
    for kl in (False, True):
        Ys, Cs, ps = np.zeros((K, N, d)), np.zeros((K, N, N)), np.zeros((K, N))
        for s, n in enumerate(sizes):
            Ys[s, :n] = rng.uniform(0.1, 1.5, (n, d))
            Cs[s, :n, :n] = (rng.random((n, n)) < 0.5) + 0.2 + 0.1 * rng.random((n, n))
            ps[s, :n] = rng.uniform(0.5, 1.5, n)
            ps[s] /= ps[s].sum()
        p = rng.uniform(0.5, 1.5, N); p /= p.sum()
        lam = rng.uniform(0.5, 1.5, K); lam /= lam.sum()
        ins = dict(Ys=Ys, Cs=Cs, ps=ps, p=p, lam=lam, init_C=rng.uniform(0.2, 1.0, (N, N)), init_Y=rng.uniform(0.1, 1.5, (N, d)))
        gw, gc = rng.standard_normal((N, d)), rng.standard_normal((N, N))
        run = dict(alpha=0.5, rho=2.0, max_iter=2, tol=0.0, epoch=12, loss_fun="kl_loss" if kl else "square_loss")

        def loss(v):
            Y, C, lg = mixup_ref(N, [v["Ys"][s, :n] for s, n in enumerate(sizes)], [v["Cs"][s, :n, :n] for s, n in enumerate(sizes)],
                                 [v["ps"][s, :n] for s, n in enumerate(sizes)], v["p"], v["lam"], init_C=v["init_C"], init_Y=v["init_Y"], **run)
            assert lg["epochs"] == [[12, 12], [12, 12]]
            return float((gw * Y).sum() + (gc * C).sum())

        r = R.mixup_unrolled_ref(Ys, Cs, ps, p, lam, ins["init_C"], ins["init_Y"], alpha=0.5, rho=2.0, counts=[[12, 12]] * 2, gY=gw, gC=gc, kl=kl)
        h = 1e-6
        for k, gk in (("Ys", "dYs"), ("Cs", "dCs"), ("ps", "dps"), ("p", "dp"), ("lam", "dlam"), ("init_C", "dinit_C"), ("init_Y", "dinit_Y")):
            V = rng.standard_normal(ins[k].shape) * np.abs(ins[k]).mean() * (ins[k] != 0)           # (the embedding's zeros stay zeros)
            fd = (loss(dict(ins, **{k: ins[k] + h * V})) - loss(dict(ins, **{k: ins[k] - h * V}))) / (2 * h)
            an = float((r[gk] * V).sum())
            print(f"kl={kl} {k}: analytic {an:+.9e} finite difference {fd:+.9e}")
            assert abs(an) > 1e-4 and abs(fd - an) <= 10 * np.finfo(np.float64).eps * abs(loss(ins)) / h, (kl, k, an, fd)


def test_fixed_plan_gradient_is_a_different_quantity():
    """The gradient of the last update steps at the last couplings held constant (what fgw_barycenters_BAPG delivers): the restatement's chain
    cut after step (a) of the last outer iteration."""
    for name in ("k3_n10_d4", "k5_n33_d8_weights"):
        g = load(name)
        (Ys, Cs, ps, p, lam, init_C, init_Y), kw, N, sizes = R.fixture_problem(g)
        T = g["T"]
        pinv = 1.0 / p
        U, V = g["gw"] * pinv[:, None], g["gc"] * (pinv[:, None] * pinv[None, :])
        dYs = np.stack([lam[s] * (T[s].T @ U) for s in range(len(sizes))])
        dCs = np.stack([lam[s] * (T[s].T @ V @ T[s]) for s in range(len(sizes))])
        for k, v in (("dYs", dYs), ("dCs", dCs)):
            e = R.grad_error(v, g[f"gB_{k}"])
            print(f"{name}: fixed-plan {k} against the unrolled gradient: {e:.3f}")
            assert e > 0.5, (name, k, e)
        assert np.linalg.norm(g["gB_dps"]) > 1.0 and np.linalg.norm(g["gB_dinit_C"]) > 0.1      # which the fixed-plan convention sets to none


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return {m.group(2): len(m.group(3).split(",")) for m in re.finditer(r"\b(int|long long)\s+(conan_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_the_header_agrees_with_its_table_and_the_library():
    assert list(_lib.EXT_TABLES)[-1] == HEADER and set(_lib.EXT_TABLES[HEADER]) == set(EXPORTS)
    d, raw = _declared(HEADER), ctypes.CDLL(_lib.library_path())
    assert set(d) == set(EXPORTS)
    others = "".join(open(os.path.join(INCLUDE, h)).read() for h in os.listdir(INCLUDE) if h != HEADER)
    for name, (_res, args) in _lib.EXT_TABLES[HEADER].items():
        assert len(args) == d[name] and hasattr(raw, name) and not re.search(r"\b" + name + r"\b", others), name
        assert getattr(_lib.lib(), name).argtypes == args
    I, LL, P, D, PR = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(FgwParams)
    assert _lib.EXT_TABLES[HEADER]["conan_fgw_mixup_barycenter_fwd_record"] == (I, [P] * 7 + [I, I, I, I, PR, D, I, D] + [P] * 9)
    assert _lib.EXT_TABLES[HEADER]["conan_fgw_mixup_barycenter_bwd"] == (I, [P] * 6 + [I, I, I, I, PR, D, I, D] + [P] * 15)
    assert _lib.EXT_TABLES[HEADER]["conan_fgw_mixup_barycenter_bwd_workspace_bytes"] == (LL, [I] * 5)
    assert _lib.EXT_TABLES[HEADER]["conan_fgw_mixup_barycenter_bwd_lds_resident"] == (I, [I])
    assert _lib.lib().conan_abi_version() == _lib.ABI_VERSION == 6


def test_every_export_is_named_by_the_gpu_test_file():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_fgw_mixup_unrolled.py")).read()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\b", gpu_tests), f"{name}: no GPU test names it"


def test_queries_need_no_gpu():
    L = _lib.lib()
    al = lambda doubles: (doubles * 8 + 255) // 256 * 256
    for B, K, N, d, ep in ((1, 3, 10, 4, 100), (256, 5, 33, 8, 100), (64, 3, 90, 64, 100), (3, 2, 61, 4, 12), (2, 2, 62, 4, 12), (1, 1, 1, 1, 1)):
        res = ((8 + 8) * N + 16) * 8 + N * (N | 1) * 40 <= 160 * 1024
        assert L.conan_fgw_mixup_barycenter_bwd_lds_resident(N) == int(res)
        BK, NN, Nd = B * K, N * N, N * d
        want = (al(B * NN) + al(B * Nd) + al(B * N) + 2 * (al(BK * NN) + al(BK * Nd) + al(BK * N)) + al(BK) + 2 * al(BK * NN) + al(BK * 2 * ep * NN)
                + (0 if res else al(BK * 5 * N * (N | 1))))
        assert L.conan_fgw_mixup_barycenter_bwd_workspace_bytes(B, K, N, d, ep) == want
    assert L.conan_fgw_mixup_barycenter_bwd_lds_resident(61) == 1 and L.conan_fgw_mixup_barycenter_bwd_lds_resident(62) == 0
    assert 2.2e9 < 1280 * 2 * 100 * 33 * 33 * 8 < L.conan_fgw_mixup_barycenter_bwd_workspace_bytes(256, 5, 33, 8, 100) < 2.3e9      # the docstring's figure
    assert L.conan_fgw_mixup_barycenter_bwd_lds_resident(0) == 0 and L.conan_fgw_mixup_barycenter_bwd_lds_resident(-4) == 0
    for bad in ((0, 3, 5, 4, 10), (-1, 3, 5, 4, 10), (1, 0, 5, 4, 10), (1, 3, 0, 4, 10), (1, 3, -3, 4, 10), (1, 3, 5, 0, 10), (1, 3, 5, 4, 0), (1, 3, 5, 4, -2),
                (1, 3, 5000, 4, 10)):
        assert L.conan_fgw_mixup_barycenter_bwd_workspace_bytes(*bad) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """Every pointer is a HOST buffer filled with 7: a launch would fault on it, a refusal leaves it as it is."""
    L = _lib.lib()
    buf = (ctypes.c_float * 256)(*([7.0] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(Ys=p, Cs=p, ps=p, p=p, lam=p, iY=p, B=1, K=2, N=4, d=2, mi=3, loss=0, fs=0, ff=0, prm=True, rho=1.0, epoch=10, eps=1e-5, info=p, rec=p,
                dY=p, dC=p, dYs=p, dCs=p, dps=p, dp=p, dlam=p, dic=p, diy=p, chk=p, ep=p, ws=p)

    def rc(**kw):
        v = dict(good, **kw)
        prm = FgwParams(0.5, 0.0, v["mi"], 1e-9, 0.0, 1, 0.0, v["fs"], v["ff"], 0, v["loss"], 0)
        return L.conan_fgw_mixup_barycenter_bwd(v["Ys"], v["Cs"], v["ps"], v["p"], v["lam"], v["iY"], v["B"], v["K"], v["N"], v["d"],
                                                ctypes.byref(prm) if v["prm"] else None, v["rho"], v["epoch"], v["eps"], v["info"], v["rec"], v["dY"],
                                                v["dC"], v["dYs"], v["dCs"], v["dps"], v["dp"], v["dlam"], v["dic"], v["diy"], v["chk"], v["ep"], v["ws"], None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(Ys=None), dict(Cs=None), dict(prm=False), dict(info=None), dict(rec=None), dict(ws=None), dict(dY=None, dC=None), dict(ps=None),
               dict(p=None), dict(lam=None), dict(iY=None), dict(iY=None, diy=None, ff=1), dict(B=0), dict(B=-2), dict(K=0), dict(N=0), dict(N=-1), dict(d=0),
               dict(mi=0), dict(mi=-5), dict(epoch=0), dict(epoch=-1), dict(rho=0.0), dict(rho=-1.0), dict(rho=inf), dict(rho=nan), dict(eps=nan),
               dict(loss=2), dict(loss=-1)):
        assert rc(**kw) == -1, kw                                          # (ps / p / lambdas / init_Y null with their gradient wanted: refused too)
    assert rc(N=5000) == -3                                                # the vectors alone exceed the LDS
    assert L.conan_fgw_mixup_barycenter_fwd_record(p, p, None, None, None, None, None, 1, 2, 4, 2, ctypes.byref(FgwParams(0.5, 0.0, 3, 1e-9, 0.0, 1, 0.0, 0, 0, 0, 0, 0)),
                                                   1.0, 10, 1e-5, p, p, p, None, p, p, None, p, None) == -1            # no record
    assert all(v == 7.0 for v in buf)


def test_python_signatures_and_docstrings():
    assert str(inspect.signature(ops.fgw_mixup_barycenter_unrolled)) == str(inspect.signature(ops.fgw_mixup_barycenter_batched))
    assert str(inspect.signature(fgw.fgw_barycenters_BAPG_unrolled)) == str(inspect.signature(fgw.fgw_barycenters_BAPG))
    doc = ops.fgw_mixup_barycenter_unrolled.__doc__
    assert "B * K * 2 epoch * N^2 * 8 bytes" in doc and "2.2 GB" in doc and "2 max_iter + 1 launches" in doc
    assert "fgw_barycenters_BAPG_unrolled" in fgw.__doc__ and "fgw_barycenters_BAPG_unrolled" in fgw.fgw_barycenters_BAPG.__doc__
    assert "fgw_mixup_barycenter_unrolled" in ops.fgw_mixup_barycenter_batched.__doc__
    import torch
    Ys, Cs = [torch.rand(4, 2) for _ in range(3)], [torch.zeros(4, 4) for _ in range(3)]
    with pytest.raises(ValueError, match="Unknown `loss_fun='abs'`"):
        fgw.fgw_barycenters_BAPG_unrolled(4, Ys, Cs, loss_fun="abs")
    with pytest.raises(ValueError, match="If C is fixed it must be initialized"):
        fgw.fgw_barycenters_BAPG_unrolled(4, Ys, Cs, fixed_structure=True)
    with pytest.raises(ValueError, match="If Y is fixed it must be initialized"):
        fgw.fgw_barycenters_BAPG_unrolled(4, Ys, Cs, fixed_features=True)
    with pytest.raises(NotImplementedError, match="fgw_barycenters_BAPG_unrolled runs on the GPU only"):
        fgw.fgw_barycenters_BAPG_unrolled(4, Ys, Cs)
    with pytest.raises(NotImplementedError, match="fgw_barycenters_BAPG runs on the GPU only"):          # the existing name keeps its message
        fgw.fgw_barycenters_BAPG(4, Ys, Cs)
