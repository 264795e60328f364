"""fgw_barycenters(..., solver="PPA" | "BAPG") on the GPU against the reference's own fp32 / fp64 runs (tests/golden/fgw_ppa_*.npz,
fgw_bapg_*.npz, written by make_fgw_solver_golden.py).  Same yardsticks as test_gpu_fgw.py::test_golden_vectors: outer, inner and Sinkhorn
iteration counts of r64, errs within rtol 2e-3, Y and C within 1e-4 of r64, T within 1e-4 of r32 or no further from r64 than r32 is."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import golden_files, rel
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops
from conan_fgw_amd._lib import FgwParams, call, lib, ptr, stream_ptr
from conan_fgw_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
ALL = golden_files("fgw_ppa_") + golden_files("fgw_bapg_")
DENSE = [p for p in ALL if "ragged" not in p]
RAGGED = [p for p in ALL if "ragged" in p]
ids = lambda ps: [os.path.basename(p)[4:-4] for p in ps]


def _kw(g):
    return dict(alpha=float(g["alpha"]), epsilon=float(g["epsilon"]), max_iter=int(g["max_iter"]), tol=float(g["tol"]), inner_tol=1e-4,
                num_iter_max=int(g["num_iter_max"]), stop_thr=float(g["stop_thr"]), warmstart=bool(g["warmstart"]),
                fixed_structure=bool(g["fixed_structure"]), loss_fun=str(g["loss_fun"]), solver=str(g["solver"]))


def _check_matrices(g, Y, C, T):
    for key, val in (("Y", Y), ("C", C), ("T", T)):
        yard = rel(g["r32_" + key], g["r64_" + key])
        e32, e64 = rel(val, g["r32_" + key]), rel(val, g["r64_" + key])
        assert e32 <= 1e-4 or e64 <= yard, (key, e32, e64, yard)
        if key != "T":
            assert e64 <= 1e-4, (key, e64)


@pytest.mark.parametrize("small_int", [False, True], ids=["cs_f32", "cs_u8"])
@pytest.mark.parametrize("path", DENSE, ids=ids(DENSE))
def test_solver_golden_vectors(path, small_int):
    g = np.load(path)
    Yt = torch.from_numpy(g["Ys"]).to(dev)[None]
    Ct = torch.from_numpy(g["Cs"].astype(np.float32)).to(dev)[None]
    Y, C, T, info, errs = ops.fgw_barycenter_batched(Yt, Ct, cs_small_int=small_int, **_kw(g))
    assert int(info[0, 3]) == 0                                         # no padded-node merge, no zero row / column sum
    outer = int(info[0, 0])
    assert outer == len(g["r64_err_feature"])
    assert int(info[0, 1]) == int(g["r64_inner"]) and int(info[0, 2]) == int(g["r64_sinkhorn"])
    np.testing.assert_allclose(errs[0, 0, :outer].cpu().numpy(), g["r64_err_feature"], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(errs[0, 1, :outer].cpu().numpy(), g["r64_err_structure"], rtol=2e-3, atol=1e-6)
    _check_matrices(g, Y[0].cpu().numpy(), C[0].cpu().numpy(), T[0].cpu().numpy())


@pytest.mark.parametrize("path", RAGGED, ids=ids(RAGGED))
def test_solver_ragged_sizes_through_fgw_barycenters(path):
    """Input graphs of 9, 6 and 8 nodes around a barycenter of 7 (the reference's rectangular problems; fgw.py embeds them with massless
    nodes), with the reference's random init_C."""
    g = np.load(path)
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ys = [t(g["Ys"][s, :n]) for s, n in enumerate(sizes)]
    Cs = [t(g["Cs"][s, :n, :n].astype(np.float32)) for s, n in enumerate(sizes)]
    ps = [torch.ones(n, device=dev) / n for n in sizes]
    kw = _kw(g)
    Y, C, log = pfgw.fgw_barycenters(N, Ys, Cs, ps=ps, lambdas=[1.0 / len(sizes)] * len(sizes), alpha=kw["alpha"], epsilon=kw["epsilon"],
                                     max_iter=kw["max_iter"], tol=kw["tol"], solver=kw["solver"], warmstartT=kw["warmstart"], log=True,
                                     numItermax=kw["num_iter_max"], stopThr=kw["stop_thr"])
    assert log["n_outer"] == len(g["r64_err_feature"])
    assert log["n_pgd"] == int(g["r64_inner"]) and log["n_sinkhorn"] == int(g["r64_sinkhorn"])
    T = np.zeros_like(g["r64_T"])
    for s, n in enumerate(sizes):
        T[s, :, :n] = log["T"][s].cpu().numpy()
    _check_matrices(g, Y.cpu().numpy(), C.cpu().numpy(), T)


@pytest.mark.parametrize("path", [p for p in DENSE if "n9_d3" in p and "kl" not in p and "cold" not in p] +
                         [p for p in DENSE if "n18p2" in p], ids=lambda p: os.path.basename(p)[4:-4])
def test_solver_backward_matches_reference_autograd(path):
    """Gradient through the final couplings held constant (barycenter.py:120), as for PGD."""
    g = np.load(path)
    Yt = torch.from_numpy(g["Ys"]).to(dev)[None].requires_grad_(True)
    Ct = torch.from_numpy(g["Cs"].astype(np.float32)).to(dev)[None]
    Y, *_ = ops.fgw_barycenter_batched(Yt, Ct, **_kw(g))
    (Y[0] * torch.from_numpy(g["r32_grad_w"]).to(dev)).sum().backward()
    yard = rel(g["r32_dYs"], g["r64_dYs"])
    e = rel(Yt.grad[0].cpu().numpy(), g["r64_dYs"])
    assert e <= max(1e-4, yard), (e, yard)


def _model_batch(shape, B, K, seed=77):
    b = make_batch(shape, B, K, seed=seed)
    pos = torch.from_numpy(b.pos).to(dev); batch = torch.from_numpy(b.batch).to(dev)
    gp = ops.graph_ptr_from_batch(batch, b.num_graphs)
    graph = ops.RadiusGraph(pos, gp, b.num_graphs, 10.0 if shape == "esol" else 5.0, 32)
    torch.manual_seed(3)
    feat = torch.nn.functional.softplus(torch.randn(len(b.z), 64, device=dev))
    Ys, Cs = ops.fgw_densify(feat, graph, b.max_nodes, 0.5)
    N = b.max_nodes
    return Ys.view(B, K, N, 64), Cs.view(B, K, N, N), graph


@pytest.mark.parametrize("solver,kw", [("PPA", {}), ("PPA", {"loss_fun": "kl_loss"}), ("BAPG", {"epsilon": 2.0})], ids=["ppa", "ppa_kl", "bapg"])
@pytest.mark.parametrize("shape,B,K", [("esol", 6, 5), ("bace", 4, 3)], ids=["n_le_64", "n_gt_64"])
def test_solver_adjacency_path_equals_the_dense_path(shape, B, K, solver, kw):
    """`adjacency=graph`: the ragged neighbour lists are expanded into the dense scratch, then the same solve — bit for bit."""
    Ys, Cs, graph = _model_batch(shape, B, K)
    dense = ops.fgw_barycenter_batched(Ys, Cs, cs_small_int=True, solver=solver, **kw)
    ragged = ops.fgw_barycenter_batched(Ys, None, adjacency=graph, solver=solver, **kw)
    assert bool(torch.isfinite(dense[0]).all())
    for a, b, name in zip(dense, ragged, ("Y", "C", "T", "info", "errs")):
        assert torch.equal(a, b) or (name == "errs" and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))), name   # (errs: NaN where not run)


def test_bapg_zero_row_sum_raises_the_flag_and_the_warning():
    """64-wide features at epsilon = 0.1: a whole row / column of BAPG's multiplicative iterate underflows to zero (the reference's NaN case,
    where it only warns).  The solve finishes, flags bit 2 is raised and fgw_barycenters emits the reference's warning."""
    rng = np.random.RandomState(3)                  # (the reference, fp64, is NaN on this input after 2 outer iterations)
    K, N, d = 3, 12, 64
    Ys = rng.random_sample((K, N, d)).astype(np.float32)
    A = np.triu(rng.random_sample((K, N, N)) < 0.4, 1); Cs = (A | A.transpose(0, 2, 1)).astype(np.float32)
    Yt, Ct = torch.from_numpy(Ys).to(dev)[None], torch.from_numpy(Cs).to(dev)[None]
    Y, C, T, info, errs = ops.fgw_barycenter_batched(Yt, Ct, solver="BAPG", epsilon=0.1)
    torch.cuda.synchronize()
    assert int(info[0, 3]) & 4 == 4
    assert int(info[0, 2]) == 0
    with pytest.warns(UserWarning, match="Solver failed to produce a transport plan"):
        pfgw.fgw_barycenters(N, list(Yt[0].unbind(0)), list(Ct[0].unbind(0)), init_C=Ct[0, 0], solver="BAPG", epsilon=0.1, alpha=0.1,
                             max_iter=5, tol=1e-2)
    # the device is still usable: a finite solve right after
    Y2, *_ = ops.fgw_barycenter_batched(Yt, Ct, solver="BAPG", epsilon=2.0)
    assert bool(torch.isfinite(Y2).all())


def _fwd_entry(Ys, Cs, graph, solver, symmetric, **params):
    """conan_fgw_barycenter_fwd (graph is None) / _ragged called directly through ctypes, with the size query's numbers."""
    prm_d = dict(ops.PROD_FGW); prm_d.update(params)
    B, K, N, d = Ys.shape
    prm = FgwParams(float(prm_d["alpha"]), float(prm_d["epsilon"]), int(prm_d["max_iter"]), float(prm_d["tol"]), float(prm_d["inner_tol"]),
                    int(prm_d["num_iter_max"]), float(prm_d["stop_thr"]), 0, 0, int(bool(prm_d["warmstart"])), 0, 1)
    Y = torch.empty(B, N, d, device=dev); C = torch.empty(B, N, N, device=dev); T = torch.empty(B, K, N, N, device=dev)
    info = torch.empty(B, 4, dtype=torch.int32, device=dev); errs = torch.empty(B, 2, prm.max_iter, device=dev)
    ws = torch.empty(int(lib().conan_fgw_workspace_bytes(B, K, N, d, int(graph is not None), solver, symmetric)), dtype=torch.uint8, device=dev)
    structure = (ptr(Cs.contiguous()),) if graph is None else (ptr(graph.graph_ptr), ptr(graph.rowptr), ptr(graph.col), ptr(graph.tgt))
    call("conan_fgw_barycenter_fwd" if graph is None else "conan_fgw_barycenter_fwd_ragged", ptr(Ys.contiguous()), *structure, None, None, None,
         None, None, B, K, N, d, ctypes.byref(prm), solver, symmetric, ptr(Y), ptr(C), ptr(T), None, ptr(info), ptr(errs), ptr(ws), stream_ptr())
    return Y, C, T, info, errs


def _same(direct, through_ops):
    for a, b, name in zip(direct, through_ops, ("Y", "C", "T", "info", "errs")):
        if name == "errs":                          # NaN where not run
            assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), name
        else:                                       # bit for bit, the NaN of a BAPG molecule with flags bit 2 included
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), name


@pytest.mark.parametrize("code,solver,eps", [(0, "PGD", 0.1), (1, "PPA", 0.1), (2, "BAPG", 2.0)], ids=["pgd", "ppa", "bapg"])
@pytest.mark.parametrize("shape,B,K", [("esol", 256, 5), ("lipo", 104, 5)], ids=["cfg2", "lipophilicity"])
def test_the_entry_points_called_directly_are_the_ops_solve(shape, B, K, code, solver, eps):
    """Both entry points with (solver code, symmetric 1) against ops.fgw_barycenter_batched(solver=<name>, symmetric=True), ragged and dense:
    ops sends the right codes and asks the right size for every solver, and its default is the models' solve (PGD, symmetric)."""
    Ys, Cs, graph = _model_batch(shape, B, K)
    ragged, dense = _fwd_entry(Ys, None, graph, code, 1, epsilon=eps), _fwd_entry(Ys, Cs, None, code, 1, epsilon=eps)
    _same(ragged, ops.fgw_barycenter_batched(Ys, None, adjacency=graph, solver=solver, symmetric=True, epsilon=eps))
    _same(dense, ops.fgw_barycenter_batched(Ys, Cs, cs_small_int=True, solver=solver, symmetric=True, epsilon=eps))
    if code == 0:
        _same(ragged, ops.fgw_barycenter_batched(Ys, None, adjacency=graph))
        _same(dense, ops.fgw_barycenter_batched(Ys, Cs, cs_small_int=True))
