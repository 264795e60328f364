"""CPU-side checks of the pairwise FGW solve (fgw, fgw_projected, fgw_bregman, fgw_pairwise_distances): the fixtures tests/golden/fgw_pair_*.npz
(written by make_fgw_pair_golden.py from the reference's own fgw()) are self-consistent, and the three functions refuse what they do not
run — with the reference's messages where it raises too — before any tensor is touched or the library does any work."""
import math
import os

import numpy as np
import pytest
import torch

from helpers import golden_files
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops, ot_ops
from oracle import fgw as ofgw

ALL = golden_files("fgw_pair_")
ids = lambda ps: [os.path.basename(p)[9:-4] for p in ps]
# the 19 cases of make_fgw_pair_golden.py
NAMES = ["bapg_dir_n12_false", "bapg_n12", "bapg_n140", "bapg_rect_7x12", "pgd_1x5", "pgd_dir_n12_false", "pgd_dir_n12_none", "pgd_kl_n10_float",
         "pgd_model_n20", "pgd_n10", "pgd_n10_cap25", "pgd_n10_g0", "pgd_n140", "pgd_n33", "pgd_n80", "pgd_rect_7x12", "pgd_undir_n12_none",
         "ppa_dir_n80_false", "ppa_n10"]


def test_every_case_has_its_fixture():
    assert ids(ALL) == NAMES


@pytest.mark.parametrize("path", ALL, ids=ids(ALL))
def test_fixture_is_self_consistent(path):
    g = np.load(path)
    assert os.path.getsize(path) < 512 * 1024
    n1, n2 = g["M"].shape
    assert g["C1"].shape == (n1, n1) and g["C2"].shape == (n2, n2) and g["r64_T"].shape == (n1, n2) and g["r32_T"].shape == (n1, n2)
    assert g["r32_T"].dtype == np.float32 and g["r64_T"].dtype == np.float64
    it = int(g["r64_it"])
    assert 1 <= it <= int(g["max_iter"])
    assert len(g["r64_err"]) == len(g["r32_err"]) == math.ceil(it / 10)
    assert (int(g["r64_sk"]) == 0) == (str(g["solver"]) == "BAPG")
    if len(g["r64_err"]) > 1:
        assert g["r64_err"][1] > 1e-12                          # the plan still moved at the second check
    assert np.isfinite(g["r64_T"]).all() and np.isfinite(g["r64_err"]).all() and np.isfinite(g["r64_fgw_dist"])
    # marginals to the Sinkhorn threshold (sinkhorn.py:418-433 stops on the column-sum violation)
    T, p, q = g["r64_T"], g["p"].astype(np.float64), g["q"].astype(np.float64)
    thr = float(g["stop_thr"])
    if str(g["solver"]) == "BAPG":      # no Sinkhorn: each half-step projects onto ONE marginal, the last onto the columns; the rows stay off at a finite epsilon
        np.testing.assert_allclose(T.sum(0), q, rtol=1e-12, atol=0)
    else:
        # the last Sinkhorn update is the rows' (sinkhorn.py:415-416): exact; the columns are within stopThr where the last call stopped on it
        # rather than at numItermax
        np.testing.assert_allclose(T.sum(1), p, rtol=1e-9, atol=0)
        assert 1 <= int(g["r64_sk_last"]) <= int(g["num_iter_max"])
        if int(g["r64_sk_last"]) < int(g["num_iter_max"]):
            assert np.linalg.norm(T.sum(0) - q) < thr
    if str(g["loss_fun"]) == "square_loss":
        d = ofgw.fgw_dist(g["M"], g["C1"], g["C2"], T, float(g["alpha"]), p, q, np.float64)
        assert abs(d - float(g["r64_fgw_dist"])) <= 1e-6 * abs(float(g["r64_fgw_dist"]))


def _cpu_pair(n=4):
    return torch.rand(n, n), torch.zeros(n, n), torch.zeros(n, n), torch.ones(n) / n, torch.ones(n) / n


@pytest.fixture
def no_library(monkeypatch):
    """The refusals below must come before the library is touched: any C call fails the test."""
    def boom(*a, **k):
        raise AssertionError("the library was called")
    for mod in (ops, ot_ops):          # the solver code binds them in ot_ops
        monkeypatch.setattr(mod, "call", boom)
        monkeypatch.setattr(mod, "lib", boom)


def test_unknown_solver_is_the_references_value_error(no_library):
    M, C1, C2, p, q = _cpu_pair()
    with pytest.raises(ValueError, match=r"Unknown solver 'XYZ'. Pick one in \['PGD', 'PPA', 'BAPG'\]."):
        pfgw.fgw(M, C1, C2, p, q, solver="XYZ")
    with pytest.raises(ValueError, match=r"Unknown solver 'BAPG'. Pick one in \['PGD', 'PPA'\]."):
        pfgw.fgw_projected(M, C1, C2, p, q, solver="BAPG")
    with pytest.raises(ValueError, match=r"Unknown solver 'XYZ'"):
        pfgw.fgw(None, None, None, solver="XYZ")                 # before any tensor is touched
    with pytest.raises(ValueError, match=r"Unknown solver 'XYZ'"):
        ops.fgw_pair_batched(M[None], C1[None], C2[None], solver="XYZ")


@pytest.mark.parametrize("fn", [pfgw.fgw, pfgw.fgw_projected, pfgw.fgw_bregman], ids=["fgw", "fgw_projected", "fgw_bregman"])
def test_unknown_loss_is_the_references_value_error(fn, no_library):
    with pytest.raises(ValueError, match=r"Unknown `loss_fun='cube_loss'`. Use one of: \('square_loss', 'kl_loss'\)."):
        fn(None, None, None, loss_fun="cube_loss")
    with pytest.raises(ValueError, match=r"Unknown `loss_fun='cube_loss'`"):
        pfgw.fgw(None, None, None, loss_fun="cube_loss", solver="BAPG")


def test_not_implemented_paths(no_library):
    M, C1, C2, p, q = _cpu_pair()
    with pytest.raises(NotImplementedError, match="warmstart"):
        pfgw.fgw(M, C1, C2, p, q, warmstart=True)
    with pytest.raises(NotImplementedError, match="sinkhorn_log"):
        pfgw.fgw(M, C1, C2, p, q, method="sinkhorn")
    with pytest.raises(NotImplementedError, match="marginal_loss"):
        pfgw.fgw_bregman(M, C1, C2, p, q, marginal_loss=True)
    for kw in (dict(), dict(solver="PPA"), dict(solver="BAPG"), dict(log=True)):
        with pytest.raises(NotImplementedError, match="GPU only"):
            pfgw.fgw(M, C1, C2, p, q, **kw)
    with pytest.raises(NotImplementedError, match="GPU only"):
        pfgw.fgw_bregman(M, C1, C2)
    with pytest.raises(NotImplementedError, match="GPU only"):
        pfgw.fgw_pairwise_distances([torch.rand(4, 3)] * 3, [C1] * 3)
    with pytest.raises(NotImplementedError, match="GPU only"):
        ops.fgw_pair_batched(M[None], C1[None], C2[None])
    with pytest.raises(NotImplementedError, match="GPU only"):
        ops.fgw_pair_list([M], [C1], [C2])


def test_defaults_are_the_references():
    import inspect
    want = dict(p=None, q=None, loss_fun="square_loss", epsilon=0.1, symmetric=None, alpha=0.5, G0=None, max_iter=100, tol=1e-5, solver="PGD",
                method="sinkhorn_log", warmstart=False, verbose=False, log=False)
    for fn in (pfgw.fgw, pfgw.fgw_projected):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:3] == ["M", "C1", "C2"]
        assert {k: sig.parameters[k].default for k in want} == want
    sig = inspect.signature(pfgw.fgw_bregman)
    assert (sig.parameters["max_iter"].default, sig.parameters["tol"].default, sig.parameters["marginal_loss"].default) == (1000, 1e-9, False)


def test_pair_exports_refuse_bad_codes_and_sizes_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    L = _lib.lib()
    assert L.conan_fgw_pair_workspace_bytes(3, 33, 0, 1) > 0
    assert L.conan_fgw_pair_workspace_bytes(3, 140, 2, 0) > L.conan_fgw_pair_workspace_bytes(3, 140, 2, 1) > 0
    for bad in ((0, 33, 0, 1), (3, 0, 0, 1), (3, 33, 3, 1), (3, 33, 0, 2), (3, 33, -1, 1), (3, 33, 0, -2)):
        assert L.conan_fgw_pair_workspace_bytes(*bad) == 0, bad
    assert L.conan_fgw_pair_fwd(None, None, None, None, None, None, 1, 4, None, 0, 1, None, None, None, None, None, None) == -1
    assert L.conan_fgw_pair_dist(None, None, None, None, None, None, 1, 4, 0.5, 0, None, None) == -1
