"""CPU-side checks of the pair distance's backward (conan_fgw_pair_dist_bwd, fgw_distance): the export is declared, exported and in the ctypes table
with its documented argument list; its refusals come before any launch; the closed form the kernel implements (the table of DESIGN.md 3.3, "Pair
form: backward") reproduces the reference's autograd gradients stored in tests/golden/fgw_distgrad_*.npz (make_fgw_pair_grad_golden.py); and every
such file belongs to a fgw_pair_ fixture."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fgw_pair_grad_ref import fgw_dist_grads
from helpers import GOLDEN, golden_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADS = golden_files("fgw_distgrad_")
ids = lambda ps: [os.path.basename(p)[len("fgw_distgrad_"):-4] for p in ps]
NAMES = ("dM", "dC1", "dC2", "dp", "dq")
EPS = 1e-15


def pair_of(path):
    return os.path.join(GOLDEN, "fgw_pair_" + os.path.basename(path)[len("fgw_distgrad_"):])


def closed_form(M, C1, C2, p, q, T, alpha, loss_fun, g=1.0):
    """The five gradients of fgw_dist at the fixed plan T, as conan_fgw_pair_dist_bwd forms them (numpy, in the dtype of the inputs)."""
    r, c = T.sum(1), T.sum(0)
    if loss_fun == "square_loss":
        dC1 = 2 * C1 * np.outer(r, p) - 2 * T @ C2 @ T.T
        dC2 = 2 * C2 * np.outer(c, q) - 2 * T.T @ C1 @ T
        dp, dq = (C1 * C1).T @ r, (C2 * C2).T @ c
    else:
        dC1 = (np.log(C1 + EPS) + C1 / (C1 + EPS) - 1) * np.outer(r, p) - T @ np.log(C2 + EPS) @ T.T
        dC2 = np.outer(c, q) - (T.T @ C1 @ T) / (C2 + EPS)
        dp, dq = (C1 * np.log(C1 + EPS) - C1).T @ r, C2.T @ c
    return dict(dM=(1 - alpha) * g * T, dC1=alpha * g * dC1, dC2=alpha * g * dC2, dp=alpha * g * dp, dq=alpha * g * dq)


def test_there_are_the_seventeen_cases_up_to_80_nodes():
    want = sorted(os.path.basename(p)[len("fgw_pair_"):-4] for p in golden_files("fgw_pair_") if max(np.load(p)["M"].shape) <= 80)
    assert ids(GRADS) == want and len(want) == 17


@pytest.mark.parametrize("path", GRADS, ids=ids(GRADS))
def test_every_gradient_file_names_a_pair_fixture(path):
    g = np.load(path)
    assert os.path.getsize(path) < 512 * 1024
    assert os.path.exists(pair_of(path)) and str(g["case"]) == os.path.basename(path)[len("fgw_distgrad_"):-4]
    f = np.load(pair_of(path))
    n1, n2 = f["M"].shape
    assert sorted(g.files) == sorted(["case"] + [f"{tag}_{k}" for tag in ("r32", "r64") for k in NAMES])          # the inputs are not duplicated
    for tag, dt in (("r32", np.float32), ("r64", np.float64)):
        shapes = [g[f"{tag}_{k}"].shape for k in NAMES]
        assert shapes == [(n1, n2), (n1, n1), (n2, n2), (n1,), (n2,)] and all(g[f"{tag}_{k}"].dtype == dt for k in NAMES)
    assert all(np.isfinite(g[f"r64_{k}"]).all() for k in NAMES)


@pytest.mark.parametrize("path", GRADS, ids=ids(GRADS))
def test_closed_form_reproduces_the_references_autograd(path):
    g, f = np.load(path), np.load(pair_of(path))
    d = lambda k: f[k].astype(np.float64)
    got = closed_form(d("M"), d("C1"), d("C2"), d("p"), d("q"), f["r64_T"], float(f["alpha"]), str(f["loss_fun"]))
    for k in NAMES:
        want = g[f"r64_{k}"]
        err = np.linalg.norm(got[k] - want) / max(np.linalg.norm(want), 1e-300)
        assert err <= 1e-12, (k, err)


@pytest.mark.parametrize("path", GRADS, ids=ids(GRADS))
def test_torch_expression_of_the_gpu_tests_reproduces_the_references_autograd(path):
    g, f = np.load(path), np.load(pair_of(path))
    d = lambda k: torch.from_numpy(f[k].astype(np.float64))[None]
    got = fgw_dist_grads(d("M"), d("C1"), d("C2"), d("p"), d("q"), d("r64_T"), float(f["alpha"]), str(f["loss_fun"]))
    for k, x in zip(NAMES, got):
        want = g[f"r64_{k}"]
        err = np.linalg.norm(x[0].numpy() - want) / max(np.linalg.norm(want), 1e-300)
        assert err <= 1e-12, (k, err)


def _argument_list(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_export_is_declared_exported_and_in_the_ctypes_table():
    want = ["const float *C1", "const float *C2", "const float *p", "const float *q", "const float *T", "const float *gout", "int B", "int N",
            "float alpha", "int loss_fun", "float *dM", "float *dC1", "float *dC2", "float *dp", "float *dq", "void *stream"]
    assert _argument_list(open(os.path.join(ROOT, "include", "conan_fgw_hip.h")).read(), "conan_fgw_pair_dist_bwd") == want
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["conan_fgw_pair_dist_bwd"] == (I, [P] * 6 + [I, I, F, I] + [P] * 6)
    assert hasattr(ctypes.CDLL(_lib.library_path()), "conan_fgw_pair_dist_bwd")
    assert _lib.ABI_VERSION == 6                                          # (this added export left it at 5; 6 came with the barycenter signatures)


def test_bad_arguments_are_refused_without_a_gpu():
    """Every row returns CONAN_E_BADARG before any launch: the pointers are never dereferenced on the host, and there is no device here."""
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    L = _lib.lib()
    x = 256                                                                # a non-null pointer value that no code path may touch
    good = dict(C1=x, C2=x, p=x, q=x, T=x, gout=x, B=2, N=6, loss=0, dM=x, dC1=x, dC2=x, dp=x, dq=x)
    table = [dict(C1=None), dict(C2=None), dict(T=None), dict(gout=None), dict(dM=None, dC1=None, dC2=None, dp=None, dq=None), dict(p=None),
             dict(q=None), dict(p=None, dq=None, dM=None, dC1=None, dC2=None), dict(B=0), dict(B=-1), dict(N=0), dict(loss=2), dict(loss=-1)]
    for bad in table:
        a = dict(good); a.update(bad)
        rc = L.conan_fgw_pair_dist_bwd(a["C1"], a["C2"], a["p"], a["q"], a["T"], a["gout"], a["B"], a["N"], 0.5, a["loss"], a["dM"], a["dC1"], a["dC2"],
                                       a["dp"], a["dq"], None)
        assert rc == -1, bad
