"""Sinkhorn-Knopp for several histograms at once (a 2-D b), what needs no GPU: the fp64 restatement tests/sinkhorn_hists_ref.py reproduces every
stored run of the reference (tests/golden/hists_sinkhorn_*.npz, written by tests/golden/make_sinkhorn_hists_golden.py: niter and warning equal;
err, loss, u, v to 1e-12 relative); the fixtures keep the generator's fairness rule; the header, the table and the library agree; the host
queries answer and match the header's formula; bad arguments are refused before any launch; the CPU refusals hold; ot_ops lists the new
names."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, ops, ot_ops
from conan_fgw_amd import sinkhorn as sk

from sinkhorn_hists_ref import knopp_hists, loss_grad_M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INCLUDE = os.path.join(ROOT, "include")
HEADER = "conan_fgw_hip_sinkhorn_hists.h"
EXPORTS = ("conan_sinkhorn_hists_max_hists", "conan_sinkhorn_hists_lds_resident", "conan_sinkhorn_hists_workspace_bytes",
           "conan_sinkhorn_hists_fwd", "conan_sinkhorn_hists_loss_bwd")
CASES = {"1x5_h2": (1, 5, 2), "7x12_h3": (7, 12, 3), "20x25_h1": (20, 25, 1), "33x33_h5": (33, 33, 5), "33x33_h16": (33, 33, 16),
         "33x33_h17": (33, 33, 17), "64x80_h33": (64, 80, 33), "257x65_h4": (257, 65, 4), "65x257_h4": (65, 257, 4), "zeroa": (20, 25, 3),
         "warm": (33, 33, 5), "numerr": (9, 11, 3)}
LDS = 160 * 1024


def load(name):
    z = np.load(os.path.join(GOLDEN, f"hists_sinkhorn_{name}.npz"))
    return {k: z[k] for k in z.files}


def relerr(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = np.linalg.norm(y)
    return float(np.linalg.norm(x - y) / n) if n > 0 else float(np.linalg.norm(x - y))


def test_fixture_list_is_complete():
    have = sorted(os.path.basename(p)[len("hists_sinkhorn_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "hists_sinkhorn_*.npz")))
    assert have == sorted(CASES)
    for name in have:
        assert os.path.getsize(os.path.join(GOLDEN, f"hists_sinkhorn_{name}.npz")) < 128 * 1024


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_fair_and_what_it_says(name):
    f = load(name)
    n1, n2, H = CASES[name]
    assert f["M"].shape == (n1, n2) and f["a"].shape == (n1,) and f["b"].shape == (n2, H) and f["r64_u"].shape == (n1, H) and f["r64_v"].shape == (n2, H)
    assert all(f[k].dtype == np.float32 for k in ("M", "a", "b", "reg")) and f["r64_loss"].shape == (H,) and f["r64_loss"].dtype == np.float64
    thr, it, e, niter, warn = float(f["stopThr"]), int(f["numItermax"]), f["r64_err"], int(f["r64_niter"]), str(f["r64_warn"])
    assert thr >= 1e-6                                                     # well above the 3e-9 plateau of fp32-rounded columns
    if warn == "":                                                         # stopped on the threshold
        assert niter < it - 1 and len(e) == niter // 10 + 1 and e[-1] <= 0.6 * thr and (e[:-1] >= 1.5 * thr).all()
    elif warn == "noconv":
        assert niter == it - 1 and len(e) == (it + 9) // 10 and e[-1] >= 1.5 * thr
    else:
        assert warn == "numerr" and name == "numerr" and niter == 0 and len(e) == 0
        assert (f["M"][:, 4] == np.float32(900.0) * f["reg"]).all() and (np.exp(f["M"][:, 4].astype(np.float64) / -float(f["reg"])) == 0).all()
        assert (f["r64_u"] == 1.0 / n1).all() and (f["r64_v"] == 1.0 / n2).all()        # the start values, restored for ALL histograms
    assert (name == "7x12_h3") == (warn == "noconv") and ("warm_u" in f) == (name == "warm") and ("r64_niter_cols" in f) == (name == "64x80_h33")
    if name == "zeroa":
        assert f["a"][3] == 0 and (f["a"] > 0).sum() == n1 - 1 and (f["r64_u"][3] == 0).all() and np.isfinite(f["r64_loss"]).all()
    if name == "warm":
        assert niter == 0 and f["warm_u"].shape == (n1, H) and f["warm_v"].shape == (n2, H) and f["warm_u"].dtype == np.float32
    if name == "64x80_h33":                                                # the joint stop shows: a column alone stops at an earlier check
        cols, k = f["r64_niter_cols"], int(f["early_col"])
        assert cols.shape == (H,) and cols.min() < niter and cols[k] < niter


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    f = load(name)
    warm = (f["warm_u"], f["warm_v"]) if "warm_u" in f else None
    r = knopp_hists(f["M"], f["a"], f["b"], float(f["reg"]), int(f["numItermax"]), float(f["stopThr"]), warm)
    assert r["niter"] == int(f["r64_niter"]) and r["warn"] == str(f["r64_warn"]) and len(r["err"]) == len(f["r64_err"])
    figures = dict(err=relerr(r["err"], f["r64_err"]) if len(r["err"]) else 0.0, loss=float(np.max(np.abs(r["loss"] - f["r64_loss"]) / np.abs(f["r64_loss"]))),
                   u=relerr(r["u"], f["r64_u"]), v=relerr(r["v"], f["r64_v"]))
    print(name, {k: f"{v:.1e}" for k, v in figures.items()})
    if len(r["err"]):
        # entry by entry as well; an err is the norm of a difference of marginals of size <= 1, which two fp64 summation orders (torch's and
        # numpy's matmul) reproduce to a few 1e-17 absolute, not to 1e-12 of a 6e-8 residual: hence the absolute term
        assert np.all(np.abs(r["err"] - f["r64_err"]) <= 1e-12 * np.abs(f["r64_err"]) + 1e-15)
    assert all(v <= 1e-12 for v in figures.values()), figures


def test_joint_stop_differs_from_the_columns_alone():
    f = load("64x80_h33")
    k = int(f["early_col"])
    alone = knopp_hists(f["M"], f["a"], f["b"][:, k:k + 1], float(f["reg"]), int(f["numItermax"]), float(f["stopThr"]))
    assert alone["niter"] == int(f["r64_niter_cols"][k]) < int(f["r64_niter"])
    assert relerr(alone["u"][:, 0], f["r64_u"][:, k]) > 1e-9               # so stacking the columns gives other u, v than the joint solve


def test_restatement_gradient_is_the_derivative_at_constant_u_v():
    f = load("7x12_h3")
    M, u, v, reg = f["M"].astype(np.float64), f["r64_u"], f["r64_v"], float(f["reg"])
    g = np.array([0.5, -1.25, 2.0])
    dM = loss_grad_M(M, u, v, g, reg)
    Mt = torch.from_numpy(M).requires_grad_(True)
    K = torch.exp(torch.from_numpy(M) / -reg)                              # the plan u K v is a constant of the backward: only the explicit M moves
    (torch.einsum("ik,ij,jk,ij->k", torch.from_numpy(u), K, torch.from_numpy(v), Mt) * torch.from_numpy(g)).sum().backward()
    assert relerr(dM, Mt.grad.numpy()) <= 1e-14


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return {m.group(2): len(m.group(3).split(",")) for m in re.finditer(r"\b(int|long long)\s+(conan_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_table_and_library_agree():
    keys = list(_lib.EXT_TABLES)
    assert HEADER in keys and keys.index(HEADER) == len(keys) - 2 and keys[0] == "conan_fgw_hip_pair_grad.h" and keys[-1] == "conan_fgw_hip_mixup_grad.h"
    table, d = _lib.EXT_TABLES[HEADER], _declared(HEADER)
    assert set(table) == set(EXPORTS) == set(d)
    raw = ctypes.CDLL(_lib.library_path())
    first = open(os.path.join(INCLUDE, "conan_fgw_hip.h")).read()
    for name, (_res, args) in table.items():
        assert len(args) == d[name] and hasattr(raw, name) and not re.search(r"\b" + name + r"\b", first)
        assert getattr(_lib.lib(), name).argtypes == args
    assert _lib.lib().conan_abi_version() == _lib.ABI_VERSION == 6          # an added export does not change the version
    assert len(_lib.SIGNATURES) == 141 and not any("hists" in n for n in list(_lib.SIGNATURES) + list(_lib.EXT_SIGNATURES))
    I, LL, P, D = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_double
    assert table["conan_sinkhorn_hists_fwd"] == (I, [P] * 8 + [I] * 4 + [LL, D, I, D] + [P] * 7)      # reg and stop_thr are doubles
    assert table["conan_sinkhorn_hists_loss_bwd"] == (I, [P] * 7 + [I] * 4 + [LL, D] + [P] * 2)
    assert table["conan_sinkhorn_hists_workspace_bytes"] == (LL, [I] * 4)
    assert table["conan_sinkhorn_hists_lds_resident"] == (I, [I] * 3) and table["conan_sinkhorn_hists_max_hists"] == (I, [I] * 2)


def test_every_entry_is_named_by_the_gpu_test_file():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_sinkhorn_hists.py")).read()
    for name in _lib.EXT_TABLES[HEADER]:
        assert re.search(r"\b" + name + r"\b", gpu_tests), f"{name}: no GPU test names it"


def vec_bytes(N1, N2, H):
    return (16 + N1 + (2 * N1 + 3 * N2) * (H | 1)) * 8                     # the header's formula


def test_queries_need_no_gpu_and_match_the_headers_formula():
    L = _lib.lib()
    header = open(os.path.join(INCLUDE, HEADER)).read()
    assert "(16 + N1 + (2 N1 + 3 N2) (H | 1)) * 8 <= 160 KiB" in header
    al = lambda v: (v + 255) // 256 * 256
    for N1, N2 in ((1, 5), (7, 12), (33, 33), (64, 80), (257, 65), (65, 257), (83, 83), (140, 140), (1, 1), (2000, 10), (10, 2000)):
        hmax = L.conan_sinkhorn_hists_max_hists(N1, N2)
        assert hmax >= 1 and vec_bytes(N1, N2, hmax) <= LDS and vec_bytes(N1, N2, hmax + 1) > LDS and vec_bytes(N1, N2, hmax + 2) > LDS
        for H in (1, 2, 5, 16, 17, 33, 64, hmax):
            if H > hmax:
                continue
            mat = N1 * (N2 | 1) * 8
            res = vec_bytes(N1, N2, H) + mat <= LDS
            assert L.conan_sinkhorn_hists_lds_resident(N1, N2, H) == int(res)
            for B in (1, 3, 256):
                assert L.conan_sinkhorn_hists_workspace_bytes(B, N1, N2, H) == (256 if res else B * al(mat))
        # one past the vector bound: not resident, no workspace, and the entry points refuse it (test_bad_arguments...)
        assert L.conan_sinkhorn_hists_lds_resident(N1, N2, hmax + 1) == 0 and L.conan_sinkhorn_hists_workspace_bytes(1, N1, N2, hmax + 1) == 0
    hc = (LDS // 8 - 16 - 33) // (5 * 33)                                  # 33 x 33: the largest H | 1, so the largest H is the odd one at or below it
    assert L.conan_sinkhorn_hists_max_hists(33, 33) == (hc if hc % 2 else hc - 1) == 123
    assert L.conan_sinkhorn_hists_lds_resident(33, 33, 64) == 1 and L.conan_sinkhorn_hists_lds_resident(257, 65, 4) == 0 and L.conan_sinkhorn_hists_lds_resident(65, 257, 4) == 0
    assert L.conan_sinkhorn_hists_max_hists(4000, 4000) == 0 and L.conan_sinkhorn_hists_max_hists(0, 5) == 0 and L.conan_sinkhorn_hists_max_hists(5, -1) == 0
    for bad in ((0, 5, 5, 2), (-1, 5, 5, 2), (1, 0, 5, 2), (1, 5, 0, 2), (1, 5, 5, 0), (1, 5, 5, -3), (1, 4000, 4000, 1)):
        assert L.conan_sinkhorn_hists_workspace_bytes(*bad) == 0
        assert L.conan_sinkhorn_hists_lds_resident(*bad[1:]) == int(bad[0] <= 0)       # (the first two are bad in B alone)


def test_bad_arguments_are_refused_before_any_launch():
    """Every pointer is a HOST buffer filled with 7: a launch would fault on it, a refusal leaves it as it is."""
    L = _lib.lib()
    buf = (ctypes.c_float * 256)(*([7.0] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(M=p, a=p, b=p, wu=p, wv=p, n1=p, n2=p, nh=p, B=1, N1=4, N2=5, H=3, ms=20, reg=0.1, it=10, thr=1e-9, loss=p, lu=p, lv=p, info=p, errs=p, ws=p)

    def fwd(**kw):
        v = dict(good, **kw)
        return L.conan_sinkhorn_hists_fwd(v["M"], v["a"], v["b"], v["wu"], v["wv"], v["n1"], v["n2"], v["nh"], v["B"], v["N1"], v["N2"], v["H"], v["ms"],
                                          v["reg"], v["it"], v["thr"], v["loss"], v["lu"], v["lv"], v["info"], v["errs"], v["ws"], None)

    def bwd(**kw):
        v = dict(good, **kw)
        return L.conan_sinkhorn_hists_loss_bwd(v["M"], v["lu"], v["lv"], v["loss"], v["n1"], v["n2"], v["nh"], v["B"], v["N1"], v["N2"], v["H"], v["ms"],
                                               v["reg"], v["ws"], None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(M=None), dict(b=None), dict(loss=None), dict(lu=None), dict(lv=None), dict(ws=None), dict(wu=None), dict(wv=None), dict(B=0), dict(B=-2),
               dict(N1=0), dict(N2=-1), dict(H=0), dict(H=-4), dict(it=0), dict(it=-5), dict(ms=-1), dict(reg=0.0), dict(reg=-1.0), dict(reg=inf),
               dict(reg=nan), dict(thr=nan)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(M=None), dict(lu=None), dict(lv=None), dict(loss=None), dict(ws=None), dict(B=0), dict(N1=0), dict(N2=0), dict(H=0), dict(ms=-1),
               dict(reg=0.0), dict(reg=nan), dict(reg=inf)):
        assert bwd(**kw) == -1, kw
    hmax = L.conan_sinkhorn_hists_max_hists(33, 33)
    assert fwd(N1=33, N2=33, H=hmax + 1) == -3 and bwd(N1=33, N2=33, H=hmax + 1) == -3      # past the vector bound: never launched
    assert fwd(N1=4000, N2=4000, H=1) == -3
    assert all(v == 7.0 for v in buf)


def test_cpu_refusals_hold():
    a, b, M = torch.ones(3) / 3, torch.ones(4, 2) / 4, torch.rand(3, 4)
    for fn in (sk.sinkhorn, sk.sinkhorn2, sk.sinkhorn_log, sk.sinkhorn_knopp):
        for kw in ({}, dict(grad="unrolled")):
            with pytest.raises(NotImplementedError, match=r"several histograms at once \(a 2-D b\) run on the GPU only"):
                fn(a, b, M, 0.1, **kw)
    for m in ("sinkhorn", "sinkhorn_log"):
        for fn in (sk.sinkhorn, sk.sinkhorn2):
            with pytest.raises(NotImplementedError, match="several histograms"):
                fn(a, b, M, 0.1, method=m)
    for fn in (sk.greenkhorn, sk.sinkhorn_stabilized, sk.sinkhorn_epsilon_scaling):
        with pytest.raises(NotImplementedError, match="several histograms at once .a 2-D b. are not implemented"):
            fn(a, b, M, 0.1)
    with pytest.raises(ValueError, match="grad must be"):
        sk.sinkhorn2(a, b, M, 0.1, grad="nope")
    with pytest.raises(NotImplementedError, match="the Sinkhorn solve runs on the GPU only: M is a CPU tensor"):
        ops.sinkhorn_hists_batched(M[None], a[None], b[None], reg=0.1)
    with pytest.raises(NotImplementedError, match="the Sinkhorn solve runs on the GPU only: M is a CPU tensor"):
        ops.sinkhorn_hists_loss(M, None, b[None], reg=0.1)


def test_ot_ops_lists_the_new_names():
    for name in ("sinkhorn_hists_batched", "sinkhorn_hists_loss"):
        assert name in ot_ops.__all__ and getattr(ops, name) is getattr(ot_ops, name)
    sig = inspect.signature(ot_ops.sinkhorn_hists_batched)
    assert list(sig.parameters) == ["M", "a", "b", "reg", "num_iter_max", "stop_thr", "warmstart", "n1", "n2", "nh"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
    assert list(inspect.signature(ot_ops.sinkhorn_hists_loss).parameters)[:10] == list(sig.parameters)
