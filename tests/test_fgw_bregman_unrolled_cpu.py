"""The unrolled BAPG pairwise FGW gradient, what needs no GPU: the fp64 restatement tests/fgw_bregman_unrolled_ref.py reproduces torch autograd
through the reference's own fgw_bregman on every stored fixture (tests/golden/fgw_bregman_unrollgrad_*.npz, written by
tests/golden/make_fgw_bregman_unrolled_golden.py) to 1e-9 (grad_error: the Frobenius norm of the difference over that of the yardstick), which
pins both the restatement and the conditioning of the chosen cases; the fixed-plan gradient is a different quantity; the header, the table and
the library agree; the host-side queries answer; bad arguments are refused before any launch; the public functions have their signatures and
their refusals hold on CPU tensors; the PGD / PPA unrolled names still refuse BAPG and kl_loss."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, fgw, ops

from fgw_bregman_unrolled_ref import fixed_plan, grad_error, unrolled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INCLUDE = os.path.join(ROOT, "include")
REUSED = {"n12": "bapg_n12", "rect_7x12": "bapg_rect_7x12", "dir_n12_false": "bapg_dir_n12_false", "1x5": "pgd_1x5", "n33": "pgd_n33", "n80": "pgd_n80"}
NEW = ["kl_n10", "kl_dir_n12_false", "dir_n12_none", "undir_n12_none", "n10_g0", "eps002_n12", "stop_n12", "zerop_9x11"]
FINITE = list(REUSED) + NEW
LOSS = ("n12", "kl_n10")
NAN = "nan_n10"
SYM = {1: True, 0: False, -1: None}
HEADER = "conan_fgw_hip_bregman_grad.h"
EXPORTS = ("conan_fgw_bregman_bwd_lds_resident", "conan_fgw_bregman_bwd_workspace_bytes", "conan_fgw_bregman_bwd")
KEYS = ("dM", "dC1", "dC2", "dp", "dq", "dG0")


def load(name):
    """The fixture (it holds the parameters) and the file that holds its inputs (a reused case: tests/golden/fgw_pair_<src>.npz)."""
    z = np.load(os.path.join(GOLDEN, f"fgw_bregman_unrollgrad_{name}.npz"))
    f = {k: z[k] for k in z.files}
    src = str(f["src"])
    g = np.load(os.path.join(GOLDEN, f"fgw_pair_{src}.npz")) if src else f
    return f, g


def problem(g):
    return (g["M"], g["C1"].astype(np.float32), g["C2"].astype(np.float32), g["p"], g["q"], g["G0"] if g["G0"].size else None)


def ref_kw(f):
    return dict(alpha=float(f["alpha"]), epsilon=float(f["epsilon"]), loss_fun=str(f["loss_fun"]), symmetric=SYM[int(f["symmetric"])], iters=int(f["iters"]))


def test_fixture_list_is_complete():
    have = sorted(os.path.basename(p)[len("fgw_bregman_unrollgrad_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "fgw_bregman_unrollgrad_*.npz")))
    assert have == sorted(FINITE + [NAN])
    limit = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "fgw_unrollgrad_*.npz")))
    for name in have:
        assert os.path.getsize(os.path.join(GOLDEN, f"fgw_bregman_unrollgrad_{name}.npz")) <= limit
    for name, src in REUSED.items():
        assert str(load(name)[0]["src"]) == src


@pytest.mark.parametrize("name", FINITE)
def test_restatement_reproduces_the_reference_autograd(name):
    f, g = load(name)
    M, C1, C2, p, q, G0 = problem(g)
    assert all(v.dtype == np.float32 for v in (M, p, q, f["W"]))
    tol, errs, iters, cap = float(f["tol"]), f["errs"], int(f["iters"]), int(f["max_iter"])
    # the fixture rule: no evaluated error within a factor 2 of tol; tol at least 1e-6 unless the solve ran to the cap
    assert ((errs > 2 * tol) | (errs < tol / 2)).all() and (tol >= 1e-6 or (iters == cap and (errs > 2 * tol).all())) and len(errs) == (iters + 9) // 10
    assert ("gT_dG0" in f) == (G0 is not None) == (name == "n10_g0") and ("gl_dM" in f) == (name in LOSS)
    if name.startswith("kl"):
        assert str(f["loss_fun"]) == "kl_loss" and (C1 > 0).all() and (C2 > 0).all() and (name != "kl_dir_n12_false" or ((C2 != C2.T).any() and int(f["symmetric"]) == 0))
    if name in ("dir_n12_none", "undir_n12_none"):
        assert int(f["symmetric"]) == -1 and bool((C1 == C1.T).all() and (C2 == C2.T).all()) == (name == "undir_n12_none")
    if name == "n80":
        assert M.shape == (80, 80) and cap == 12
    if name == "eps002_n12":
        assert float(f["epsilon"]) == 0.02 and (f["T"] == 0).any() and float(f["tmin"]) == 0
    if name == "stop_n12":
        assert iters in (11, 21) and iters < cap and tol >= 1e-6
    if name == "zerop_9x11":
        assert p[3] == 0 and (p > 0).sum() == 8 and np.isnan(f["ref_full_T"]).all()      # the reference's 0 / 0 on the full problem
    objs = [("gT", dict(dT=f["W"]), f["W"]), ("gd", dict(ddist=1.0), 1.0)]
    for tag, kw, cot in objs:
        r = unrolled(M, C1, C2, p, q, G0, **ref_kw(f), **kw)
        assert not r["flagged"]
        assert grad_error(r["T"], f["T"]) <= 1e-12 and abs(r["dist"] - float(f["dist"])) <= 1e-12 * abs(float(f["dist"]))
        for k in KEYS:
            if f"{tag}_{k}" in f:
                e = grad_error(r[k], f[f"{tag}_{k}"], cot)
                print(f"{name} {tag} {k}: {e:.2e}")
                assert e <= 1e-9, (name, tag, k, e)
        if name == "zerop_9x11":                                           # the massless rule: exact zeros, no division by the zero weight
            assert r["dp"][3] == 0 and not r["dM"][3].any() and not r["dC1"][3].any() and not r["dC1"][:, 3].any() and not r["T"][3].any()
            assert all(np.isfinite(r[k]).all() for k in KEYS[:5])


@pytest.mark.parametrize("name", LOSS)
def test_loss_gradient_by_composition(name):
    """log["loss"] = fgw_dist - alpha sum(constC o T): the restatement's walk with cotangents ddist = 1, dT = -alpha constC, plus the direct
    partials of constC in C1, C2, p, q, reproduces the reference's gradient of log["loss"]: what fgw.fgw_bregman_unrolled composes in torch."""
    f, g = load(name)
    M, C1, C2, p, q, G0 = problem(g)
    alpha, kl = float(f["alpha"]), str(f["loss_fun"]) == "kl_loss"
    a, b, pw, qw, T = (torch.from_numpy(np.asarray(v, dtype=np.float64)).requires_grad_(True) for v in (C1, C2, p, q, f["T"]))
    f1, f2 = (a * torch.log(a + 1e-15) - a, b) if kl else (a * a, b * b)
    constC = (f1 @ pw)[:, None] + (f2 @ qw)[None, :]
    direct = torch.autograd.grad(-alpha * (constC * T).sum(), [a, b, pw, qw, T])
    r = unrolled(M, C1, C2, p, q, G0, **ref_kw(f), dT=direct[4].numpy(), ddist=1.0)
    for k, extra in (("dM", 0.0), ("dC1", direct[0].numpy()), ("dC2", direct[1].numpy()), ("dp", direct[2].numpy()), ("dq", direct[3].numpy())):
        e = grad_error(r[k] + extra, f[f"gl_{k}"])
        print(f"{name} gl {k}: {e:.2e}")
        assert e <= 1e-9, (name, k, e)


def test_nan_fixture():
    """Every factor of the first half-step underflows to an exact zero (exponents below -900): every row sum is 0, the reference's plan and
    gradients are NaN, and the restatement names the cause (a zero sum on a node with mass)."""
    f, g = load(NAN)
    assert float(f["first_x_max"]) < -900.0 and (f["M"] >= 1).all() and float(f["alpha"]) == 0.5 and float(f["epsilon"]) == 5e-4
    assert np.isnan(f["T"]).all() and not any(k.startswith(("gT_", "gd_")) for k in f)      # (the reference's gradients: all NaN, not stored)
    r = unrolled(*problem(g), **ref_kw(f), dT=f["W"], ddist=1.0)
    assert r["flagged"] and "dM" not in r


def test_fixed_plan_gradient_is_a_different_quantity():
    f, g = load("rect_7x12")
    M, C1, C2, p, q, _ = problem(g)
    fixed = fixed_plan(M, C1, C2, p, q, f["T"], alpha=float(f["alpha"]), loss_fun=str(f["loss_fun"]))
    for k, v in fixed.items():
        e = grad_error(v, f[f"gd_{k}"])
        print(f"fixed-plan {k} against the unrolled gradient: {e:.3f}")
        assert e > 1e-3, (k, e)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return {m.group(2): len(m.group(3).split(",")) for m in re.finditer(r"\b(int|long long)\s+(conan_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_table_and_library_agree():
    keys = list(_lib.EXT_TABLES)
    assert keys.index(HEADER) == 1 and keys[0] == "conan_fgw_hip_pair_grad.h" and keys[-1] == "conan_fgw_hip_mixup_grad.h"
    table, d = _lib.EXT_TABLES[HEADER], _declared(HEADER)
    assert set(table) == set(EXPORTS) == set(d)
    raw = ctypes.CDLL(_lib.library_path())
    first = open(os.path.join(INCLUDE, "conan_fgw_hip.h")).read()
    for name, (_res, args) in table.items():
        assert len(args) == d[name] and hasattr(raw, name) and not re.search(r"\b" + name + r"\b", first)
        assert getattr(_lib.lib(), name).argtypes == args
    assert _lib.lib().conan_abi_version() == _lib.ABI_VERSION == 6          # an added export does not change the version
    I, LL, P, D = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_double
    assert table["conan_fgw_bregman_bwd"] == (I, [P] * 6 + [I, I, D, D, I, I, I] + [P] * 13)
    assert table["conan_fgw_bregman_bwd_workspace_bytes"] == (LL, [I, I, I])
    assert table["conan_fgw_bregman_bwd_lds_resident"] == (I, [I])


def test_every_entry_is_named_by_the_gpu_test_file():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_fgw_bregman_unrolled.py")).read()
    for name in _lib.EXT_TABLES[HEADER]:
        assert re.search(r"\b" + name + r"\b", gpu_tests), f"{name}: no GPU test names it"


def test_queries_need_no_gpu():
    L = _lib.lib()
    al = lambda v: (v + 255) // 256 * 256
    for B, N, mi in ((1, 33, 100), (1, 33, 1000), (1280, 33, 5), (3, 61, 12), (2, 62, 12), (1, 1, 1), (2, 200, 10), (192, 90, 100)):
        res = (11 + 8) * N * 8 + N * (N | 1) * 40 <= 160 * 1024
        assert L.conan_fgw_bregman_bwd_lds_resident(N) == int(res)
        per = (2 * mi + 4) * N * N * 8 + (0 if res else 5 * N * (N | 1) * 8)
        assert L.conan_fgw_bregman_bwd_workspace_bytes(B, N, mi) == B * al(per)
    assert L.conan_fgw_bregman_bwd_lds_resident(61) == 1 and L.conan_fgw_bregman_bwd_lds_resident(62) == 0
    assert 1.75e6 < L.conan_fgw_bregman_bwd_workspace_bytes(1, 33, 100) < 1.85e6 and 17.4e6 < L.conan_fgw_bregman_bwd_workspace_bytes(1, 33, 1000) < 17.6e6      # the docstrings' figures
    assert L.conan_fgw_bregman_bwd_lds_resident(0) == 0 and L.conan_fgw_bregman_bwd_lds_resident(-4) == 0
    for bad in ((0, 5, 10), (-1, 5, 10), (1, 0, 10), (1, -3, 10), (1, 5, 0), (1, 5, -2), (1, 5000, 10)):
        assert L.conan_fgw_bregman_bwd_workspace_bytes(*bad) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """Every pointer is a HOST buffer filled with 7: a launch would fault on it, a refusal leaves it as it is."""
    L = _lib.lib()
    buf = (ctypes.c_float * 256)(*([7.0] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(M=p, C1=p, C2=p, p=p, q=p, G0=p, B=1, N=4, alpha=0.5, eps=0.1, mi=10, loss=0, sym=1, info=p, dT=p, dd=p, dM=p, dC1=p, dC2=p, dp=p, dq=p,
                dG0=p, chk=p, binfo=p, ws=p)

    def rc(**kw):
        v = dict(good, **kw)
        return L.conan_fgw_bregman_bwd(v["M"], v["C1"], v["C2"], v["p"], v["q"], v["G0"], v["B"], v["N"], v["alpha"], v["eps"], v["mi"], v["loss"], v["sym"],
                                       v["info"], v["dT"], v["dd"], v["dM"], v["dC1"], v["dC2"], v["dp"], v["dq"], v["dG0"], v["chk"], v["binfo"], v["ws"], None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(M=None), dict(C1=None), dict(C2=None), dict(info=None), dict(dM=None), dict(dC1=None), dict(dC2=None), dict(ws=None),
               dict(dT=None, dd=None), dict(p=None), dict(q=None), dict(G0=None), dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(mi=0), dict(mi=-5),
               dict(eps=0.0), dict(eps=-1.0), dict(eps=inf), dict(eps=nan), dict(alpha=nan), dict(loss=2), dict(loss=-1), dict(sym=2), dict(sym=-2)):
        assert rc(**kw) == -1, kw                                          # (p / q / G0 null with dp / dq / dG0 wanted: refused too)
    assert rc(N=5000) == -3                                                # unsupported: the vectors alone exceed the LDS
    assert all(v == 7.0 for v in buf)


def test_python_signatures():
    assert str(inspect.signature(fgw.fgw_bregman_unrolled)) == str(inspect.signature(fgw.fgw_bregman))
    assert str(inspect.signature(fgw.fgw_bregman_distance_unrolled)) == str(inspect.signature(fgw.fgw_bregman))
    sig = inspect.signature(ops.fgw_bregman_unrolled)
    assert list(sig.parameters) == ["M", "C1", "C2", "p", "q", "G0", "alpha", "epsilon", "max_iter", "tol", "loss_fun", "symmetric"]
    assert sig.parameters["max_iter"].default == 1000 and sig.parameters["tol"].default == 1e-9
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("alpha", "epsilon", "max_iter", "tol", "loss_fun", "symmetric"))
    for doc in (ops.fgw_bregman_unrolled.__doc__, fgw.fgw_bregman_unrolled.__doc__, fgw.fgw_bregman_distance_unrolled.__doc__):
        assert "(2 max_iter + 4) N^2 * 8 bytes" in doc and "1.8 MB" in doc and "17.5 MB" in doc
    assert 'log["err"]' in fgw.fgw_bregman_unrolled.__doc__
    assert "fgw_bregman_unrolled" in fgw.__doc__ and "fgw_bregman_distance_unrolled" in fgw.__doc__


def test_refusals_hold_on_cpu_tensors():
    M, C1, C2 = torch.rand(3, 4), torch.zeros(3, 3), torch.zeros(4, 4)
    for fn in (fgw.fgw_bregman_unrolled, fgw.fgw_bregman_distance_unrolled):
        with pytest.raises(NotImplementedError, match="marginal_loss=True is not implemented"):
            fn(M, C1, C2, marginal_loss=True)
        with pytest.raises(ValueError, match="Unknown `loss_fun='abs'`"):
            fn(M, C1, C2, loss_fun="abs")
        with pytest.raises(NotImplementedError, match=fn.__name__ + " runs on the GPU only: pass CUDA .ROCm. tensors .M is not one."):
            fn(M, C1, C2)
        with pytest.raises(NotImplementedError, match=fn.__name__ + " runs on the GPU only: pass CUDA .ROCm. tensors .M is not one."):
            fn(M, C1, C2, loss_fun="kl_loss", symmetric=False)
    with pytest.raises(ValueError, match="Unknown `loss_fun='abs'`"):
        ops.fgw_bregman_unrolled(M[None], C1[None], C2[None], loss_fun="abs")
    with pytest.raises(NotImplementedError, match="runs on the GPU only: M is a CPU tensor"):
        ops.fgw_bregman_unrolled(M[None], C1[None], C2[None])
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.fgw_bregman_unrolled_list([M], [C1], [C2])


def test_the_pinned_names_still_refuse_bapg_and_kl():
    M, C1, C2 = torch.rand(3, 4), torch.zeros(3, 3), torch.zeros(4, 4)
    Ys, Cs = [torch.rand(4, 2) for _ in range(3)], [torch.zeros(4, 4) for _ in range(3)]
    calls = [lambda **kw: fgw.fgw_unrolled(M, C1, C2, **kw), lambda **kw: fgw.fgw_distance_unrolled(M, C1, C2, **kw),
             lambda **kw: fgw.fgw_pairwise_distances_unrolled(Ys, Cs, **kw), lambda **kw: ops.fgw_pair_unrolled(M[None], C1[None], C2[None], **kw),
             lambda **kw: ops.fgw_pair_unrolled_list([M], [C1], [C2], **kw)]
    for call in calls:
        with pytest.raises(NotImplementedError, match="'BAPG' is not implemented"):
            call(solver="BAPG")
        with pytest.raises(NotImplementedError, match="'kl_loss'"):
            call(loss_fun="kl_loss")
