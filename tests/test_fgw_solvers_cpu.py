"""CPU-side checks of the PPA / BAPG coupling solvers: the C ABI exports them, the ctypes table declares them, and fgw_barycenters validates
its arguments like the reference (barycenter.py:33-44, 55-72) before refusing CPU tensors (GPU only)."""
import ctypes
import os
import re

import pytest
import torch

from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("conan_fgw_barycenter_fwd_solver", "conan_fgw_barycenter_fwd_ragged_solver")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    return _lib


def test_solver_exports_are_declared_and_exported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "conan_fgw_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(built.library_path())
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} not declared"
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[-1] == "int solver"
        assert hasattr(L, name)
        assert len(built.SIGNATURES[name][1]) == len(args)
    # the PGD entry points are unchanged: the solver exports take exactly one argument more
    assert len(built.SIGNATURES[NEW[0]][1]) == len(built.SIGNATURES["conan_fgw_barycenter_fwd"][1]) + 1
    assert len(built.SIGNATURES[NEW[1]][1]) == len(built.SIGNATURES["conan_fgw_barycenter_fwd_ragged"][1]) + 1


def test_solver_exports_refuse_bad_arguments_without_launching(built):
    L = built.lib()
    for solver in (0, 1, 2, 3, -1):
        assert L.conan_fgw_barycenter_fwd_solver(None, None, None, None, None, None, None, 1, 1, 1, 1, None, None, None, None, None, None,
                                                 None, None, None, solver) == -1
        assert L.conan_fgw_barycenter_fwd_ragged_solver(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, None, None,
                                                        None, None, None, None, None, None, None, solver) == -1


@pytest.mark.parametrize("solver", ["PPA", "BAPG"])
def test_fgw_barycenters_solver_argument_checks(solver):
    Ys = [torch.zeros(3, 2)]; Cs = [torch.zeros(3, 3)]
    with pytest.raises(ValueError, match="loss_fun"):
        pfgw.fgw_barycenters(3, Ys, Cs, loss_fun="nope", solver=solver)
    with pytest.raises(ValueError, match="stop_criterion"):
        pfgw.fgw_barycenters(3, Ys, Cs, stop_criterion="nope", solver=solver)
    with pytest.raises(ValueError, match="fixed"):
        pfgw.fgw_barycenters(3, Ys, Cs, fixed_structure=True, solver=solver)
    with pytest.raises(ValueError, match="fixed"):
        pfgw.fgw_barycenters(3, Ys, Cs, fixed_features=True, init_C=Cs[0], solver=solver)
    with pytest.raises(NotImplementedError):                  # still refused: broken in the reference / reached by no caller
        pfgw.fgw_barycenters(3, Ys, Cs, stop_criterion="loss", init_C=Cs[0], solver=solver)
    with pytest.raises(NotImplementedError):
        pfgw.fgw_barycenters(3, Ys, Cs, symmetric=False, init_C=Cs[0], solver=solver)
    # accepted arguments, CPU tensors: refused as GPU only (NotImplementedError, a RuntimeError)
    with pytest.raises(NotImplementedError, match="GPU only"):
        pfgw.fgw_barycenters(3, Ys, Cs, init_C=Cs[0], solver=solver)
    with pytest.raises(RuntimeError, match="GPU only"):
        pfgw.fgw_barycenters(3, Ys, Cs, init_C=Cs[0], solver=solver, loss_fun="kl_loss", warmstartT=True)


def test_bapg_ignores_the_sinkhorn_keywords():
    """fgw_bregman takes no Sinkhorn keywords (bregman.py:52-67): method / numItermax / stopThr are accepted and unused; PPA refuses a method
    other than sinkhorn_log like PGD."""
    Ys = [torch.zeros(3, 2)]; Cs = [torch.zeros(3, 3)]
    with pytest.raises(NotImplementedError, match="GPU only"):
        pfgw.fgw_barycenters(3, Ys, Cs, init_C=Cs[0], solver="BAPG", method="sinkhorn", numItermax=3, stopThr=1e-3)
    with pytest.raises(NotImplementedError, match="sinkhorn_log"):
        pfgw.fgw_barycenters(3, Ys, Cs, init_C=Cs[0], solver="PPA", method="sinkhorn")


def test_batched_entry_rejects_unknown_solver():
    with pytest.raises(ValueError, match="solver"):
        ops.fgw_barycenter_batched(torch.zeros(1, 1, 3, 2), torch.zeros(1, 1, 3, 3), solver="nope")
    assert ops.FGW_SOLVERS == {"PGD": 0, "PPA": 1, "BAPG": 2}
