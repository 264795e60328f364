"""CPU-side checks of the PPA / BAPG coupling solvers: the two forward entry points take the solver code, and fgw_barycenters validates
its arguments like the reference (barycenter.py:33-44, 55-72) before refusing CPU tensors (GPU only)."""
import ctypes
import os
import re

import pytest
import torch

from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ("conan_fgw_barycenter_fwd", "conan_fgw_barycenter_fwd_ragged")
REMOVED = tuple("conan_fgw_barycenter_fwd" + s for s in ("_solver", "_ragged_solver", "_sym", "_ragged_sym"))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    return _lib


def _args(hdr, name):
    m = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{name} not declared"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_solver_exports_are_declared_and_exported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "conan_fgw_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(built.library_path())
    # the two forward entry points take `int solver, int symmetric` right after `params`, where conan_fgw_pair_fwd has them
    for name in FWD:
        args, table = _args(hdr, name), built.SIGNATURES[name][1]
        at = args.index("const conan_fgw_params *params")
        assert args[at + 1:at + 3] == ["int solver", "int symmetric"], name
        assert table[at] == ctypes.POINTER(built.FgwParams) and table[at + 1:at + 3] == [ctypes.c_int, ctypes.c_int] and len(table) == len(args)
        assert hasattr(L, name)
    # the layered variants are gone (the size query: tests/test_fgw_sym_cpu.py)
    for name in REMOVED:
        assert not re.search(r"\b" + name + r"\b", hdr) and name not in built.SIGNATURES and not hasattr(L, name), name


def test_solver_exports_refuse_bad_arguments_without_launching(built):
    L = built.lib()
    for solver in (0, 1, 2, 3, -1):
        assert L.conan_fgw_barycenter_fwd(None, None, None, None, None, None, None, 1, 1, 1, 1, None, solver, 1, None, None, None, None, None,
                                          None, None, None) == -1
        assert L.conan_fgw_barycenter_fwd_ragged(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, None, solver, 1, None,
                                                 None, None, None, None, None, None, None) == -1


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
