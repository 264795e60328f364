"""CPU-side checks of fgw_barycenters(symmetric=False | None): the one size query is declared with both codes and follows them, the two
forward entry points refuse bad (solver, symmetric) codes without launching, and the Python layers validate `symmetric` before refusing CPU
tensors (GPU only).  (The forward declarations: tests/test_fgw_solvers_cpu.py.)"""
import ctypes
import os
import re

import pytest
import torch

from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY = "conan_fgw_workspace_bytes"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    return _lib


def test_sym_exports_are_declared_and_exported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "conan_fgw_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(built.library_path())
    m = re.search(r"\blong long\s+" + QUERY + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{QUERY} not declared"
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == ["int B", "int K", "int N", "int d", "int ragged", "int solver",
                                                                             "int symmetric"]
    assert built.SIGNATURES[QUERY] == (ctypes.c_longlong, [ctypes.c_int] * 7) and hasattr(L, QUERY)
    for name in (QUERY + "_ragged", QUERY + "_sym", QUERY + "_ragged_sym"):      # the one query replaced these
        assert not re.search(r"\b" + name + r"\b", hdr) and name not in built.SIGNATURES and not hasattr(L, name), name


def test_sym_exports_refuse_bad_arguments_without_launching(built):
    L = built.lib()
    for solver, symmetric in ((0, 1), (1, 0), (2, -1), (0, 2), (1, -2), (3, 0), (-1, 1)):
        assert L.conan_fgw_barycenter_fwd(None, None, None, None, None, None, None, 1, 1, 1, 1, None, solver, symmetric, None, None, None, None,
                                          None, None, None, None) == -1
        assert L.conan_fgw_barycenter_fwd_ragged(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, None, solver, symmetric,
                                                 None, None, None, None, None, None, None, None) == -1


def test_sym_workspace_queries(built):
    query = built.lib().conan_fgw_workspace_bytes
    for B, K, N, d in ((256, 5, 33, 64), (4, 3, 90, 64), (1, 2, 7, 3)):
        base, ragged = query(B, K, N, d, 0, 0, 1), query(B, K, N, d, 1, 0, 1)
        for solver in (0, 1, 2):
            # symmetric = True, and every PGD / PPA solve: the workspace of the models' solve
            assert query(B, K, N, d, 0, solver, 1) == base
            assert query(B, K, N, d, 1, solver, 1) == ragged
            for symmetric in (0, -1):
                w, wr = query(B, K, N, d, 0, solver, symmetric), query(B, K, N, d, 1, solver, symmetric)
                if solver < 2 or N <= 64:
                    assert (w, wr) == (base, ragged)
                else:           # asymmetric BAPG outside LDS: 36 bytes per N x P entry and coupling behind the regular workspace
                    assert w - base == wr - ragged >= B * K * N * (N | 1) * 36
        assert query(B, K, N, d, 0, 0, 2) == 0
        assert query(B, K, N, d, 1, 3, 0) == 0


@pytest.mark.parametrize("solver", ["PGD", "PPA", "BAPG"])
@pytest.mark.parametrize("symmetric", [False, None])
def test_fgw_barycenters_symmetric_on_cpu_tensors_is_gpu_only(solver, symmetric):
    Ys = [torch.zeros(3, 2)]; Cs = [torch.zeros(3, 3)]
    with pytest.raises(NotImplementedError, match="GPU only"):
        pfgw.fgw_barycenters(3, Ys, Cs, init_C=Cs[0], solver=solver, symmetric=symmetric)
    with pytest.raises(NotImplementedError, match="GPU only"):
        pfgw.fgw_barycenters(3, Ys, Cs, init_C=Cs[0], solver=solver, symmetric=symmetric, loss_fun="kl_loss")
    # argument errors still come first (barycenter.py:33-44)
    with pytest.raises(ValueError, match="loss_fun"):
        pfgw.fgw_barycenters(3, Ys, Cs, loss_fun="nope", solver=solver, symmetric=symmetric)


def test_batched_entry_rejects_unknown_symmetric():
    for bad in ("x", 1, 0, 2.0):
        with pytest.raises(ValueError, match="symmetric"):
            ops.fgw_barycenter_batched(torch.zeros(1, 1, 3, 2), torch.zeros(1, 1, 3, 3), symmetric=bad)
