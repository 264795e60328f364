"""CPU-side checks of fgw_barycenters(symmetric=False | None): the C ABI exports the `_sym` pair and its size queries, the ctypes table
declares them with the `_solver` pair's arguments plus `int symmetric`, bad codes are refused without launching, and the Python layers
validate `symmetric` before refusing CPU tensors (GPU only)."""
import ctypes
import os
import re

import pytest
import torch

from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("conan_fgw_barycenter_fwd_sym", "conan_fgw_barycenter_fwd_solver"),
         ("conan_fgw_barycenter_fwd_ragged_sym", "conan_fgw_barycenter_fwd_ragged_solver"))


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


def test_sym_exports_are_declared_and_exported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "conan_fgw_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(built.library_path())
    for new, old in PAIRS:
        args, base = _args(hdr, new), _args(hdr, old)
        assert args == base + ["int symmetric"], new
        assert hasattr(L, new)
        assert built.SIGNATURES[new][1] == built.SIGNATURES[old][1] + [ctypes.c_int]
    for name in ("conan_fgw_workspace_bytes_sym", "conan_fgw_workspace_bytes_ragged_sym"):
        assert _args(hdr, name) == ["int B", "int K", "int N", "int d", "int solver", "int symmetric"]
        assert hasattr(L, name) and name in built.SIGNATURES


def test_sym_exports_refuse_bad_arguments_without_launching(built):
    L = built.lib()
    for solver, symmetric in ((0, 1), (1, 0), (2, -1), (0, 2), (1, -2), (3, 0), (-1, 1)):
        assert L.conan_fgw_barycenter_fwd_sym(None, None, None, None, None, None, None, 1, 1, 1, 1, None, None, None, None, None, None,
                                              None, None, None, solver, symmetric) == -1
        assert L.conan_fgw_barycenter_fwd_ragged_sym(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, None, None,
                                                     None, None, None, None, None, None, None, solver, symmetric) == -1


def test_sym_workspace_queries(built):
    L = built.lib()
    for B, K, N, d in ((256, 5, 33, 64), (4, 3, 90, 64), (1, 2, 7, 3)):
        base, ragged = L.conan_fgw_workspace_bytes(B, K, N, d), L.conan_fgw_workspace_bytes_ragged(B, K, N, d)
        for solver in (0, 1, 2):
            # symmetric = True, and every PGD / PPA solve: the workspace of today's entry points
            assert L.conan_fgw_workspace_bytes_sym(B, K, N, d, solver, 1) == base
            assert L.conan_fgw_workspace_bytes_ragged_sym(B, K, N, d, solver, 1) == ragged
            for symmetric in (0, -1):
                w, wr = L.conan_fgw_workspace_bytes_sym(B, K, N, d, solver, symmetric), L.conan_fgw_workspace_bytes_ragged_sym(B, K, N, d, solver, symmetric)
                if solver < 2 or N <= 64:
                    assert (w, wr) == (base, ragged)
                else:           # asymmetric BAPG outside LDS: 36 bytes per N x P entry and coupling behind the regular workspace
                    assert w - base == wr - ragged >= B * K * N * (N | 1) * 36
        assert L.conan_fgw_workspace_bytes_sym(B, K, N, d, 0, 2) == 0
        assert L.conan_fgw_workspace_bytes_ragged_sym(B, K, N, d, 3, 0) == 0


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
