"""fgw_barycenters(..., symmetric=False | None) on the GPU against the reference's own fp32 / fp64 runs (tests/golden/fgw_sym_*.npz, written
by make_fgw_sym_golden.py): directed graphs and asymmetric float matrices, square and KL loss, PGD / PPA / BAPG, N <= 64 and N > 64.  Same
yardsticks as test_gpu_fgw_solvers.py: outer, inner and Sinkhorn iteration counts of r64, errs within rtol 2e-3, Y and C within 1e-4 of r64,
T within 1e-4 of r32 or no further from r64 than r32 is.  Further: symmetric=None against False / True, the adjacency path, the backward
and the notebook call (notebooks/fgw.ipynb on cfm_log)."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, golden_files, rel
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops
from conan_fgw_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
ALL = golden_files("fgw_sym_")
DENSE = [p for p in ALL if "ragged" not in p and "notebook" not in p]
RAGGED = [p for p in ALL if "ragged" in p]
NONE = [p for p in ALL if "_none_" in p]
ids = lambda ps: [os.path.basename(p)[8:-4] for p in ps]
SYM = {1: True, 0: False, -1: None}
NAMES = ("Y", "C", "T", "info", "errs")


def _kw(g):
    return dict(alpha=float(g["alpha"]), epsilon=float(g["epsilon"]), max_iter=int(g["max_iter"]), tol=float(g["tol"]), inner_tol=1e-4,
                num_iter_max=int(g["num_iter_max"]), stop_thr=float(g["stop_thr"]), warmstart=bool(g["warmstart"]),
                fixed_structure=bool(g["fixed_structure"]), loss_fun=str(g["loss_fun"]), solver=str(g["solver"]),
                symmetric=SYM[int(g["symmetric"])])


def _check_matrices(g, Y, C, T):
    for key, val in (("Y", Y), ("C", C), ("T", T)):
        yard = rel(g["r32_" + key], g["r64_" + key])
        e32, e64 = rel(val, g["r32_" + key]), rel(val, g["r64_" + key])
        assert e32 <= 1e-4 or e64 <= yard, (key, e32, e64, yard)
        if key != "T":
            assert e64 <= 1e-4, (key, e64)


def _same(a_out, b_out):
    """Bit for bit, NaN included (errs is NaN where not run; BAPG at N = 90 leaves NaN molecules, flags bit 2, in the reference as here)."""
    for a, b, name in zip(a_out, b_out, NAMES):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), name


def _dense(g):
    Yt = torch.from_numpy(g["Ys"]).to(dev)[None]
    Ct = torch.from_numpy(g["Cs"].astype(np.float32)).to(dev)[None]
    return Yt, Ct, g["Cs"].dtype == np.uint8


@pytest.mark.parametrize("path", DENSE, ids=ids(DENSE))
def test_sym_golden_vectors(path):
    g = np.load(path)
    Yt, Ct, small_int = _dense(g)
    Y, C, T, info, errs = ops.fgw_barycenter_batched(Yt, Ct, cs_small_int=small_int, **_kw(g))
    assert int(info[0, 3]) == 0                                         # no padded-node merge, no zero row / column sum
    outer = int(info[0, 0])
    assert outer == len(g["r64_err_feature"])
    assert int(info[0, 1]) == int(g["r64_inner"]) and int(info[0, 2]) == int(g["r64_sinkhorn"])
    np.testing.assert_allclose(errs[0, 0, :outer].cpu().numpy(), g["r64_err_feature"], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(errs[0, 1, :outer].cpu().numpy(), g["r64_err_structure"], rtol=2e-3, atol=1e-6)
    _check_matrices(g, Y[0].cpu().numpy(), C[0].cpu().numpy(), T[0].cpu().numpy())


def _through_fgw_barycenters(g, ps=None, p=None, lambdas=None, init_C=None, **over):
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    Ys = [t(g["Ys"][s, :n]) for s, n in enumerate(sizes)]
    Cs = [t(g["Cs"][s, :n, :n]) for s, n in enumerate(sizes)]
    ps = [torch.ones(n, device=dev) / n for n in sizes] if ps is None else ps
    kw = _kw(g)
    args = dict(ps=ps, p=p, lambdas=[1.0 / len(sizes)] * len(sizes) if lambdas is None else lambdas, alpha=kw["alpha"], epsilon=kw["epsilon"],
                max_iter=kw["max_iter"], tol=kw["tol"], solver=kw["solver"], warmstartT=kw["warmstart"], log=True, numItermax=kw["num_iter_max"],
                stopThr=kw["stop_thr"], loss_fun=kw["loss_fun"], symmetric=kw["symmetric"], init_C=init_C)
    args.update(over)
    return (sizes, N) + tuple(pfgw.fgw_barycenters(N, Ys, Cs, **args))


@pytest.mark.parametrize("path", RAGGED, ids=ids(RAGGED))
def test_sym_rectangular_through_fgw_barycenters(path):
    """Directed input graphs of 9, 6 and 8 nodes around a barycenter of 7 (the reference's rectangular problems; fgw.py embeds them with
    massless nodes), with the reference's random init_C: outputs, and the log (T, Ts_iter, n_outer)."""
    g = np.load(path)
    sizes, N, Y, C, log = _through_fgw_barycenters(g)
    assert log["n_outer"] == len(g["r64_err_feature"])
    assert log["n_pgd"] == int(g["r64_inner"]) and log["n_sinkhorn"] == int(g["r64_sinkhorn"])
    T = np.zeros_like(g["r64_T"])
    for s, n in enumerate(sizes):
        assert tuple(log["T"][s].shape) == (N, n)
        T[s, :, :n] = log["T"][s].cpu().numpy()
    _check_matrices(g, Y.cpu().numpy(), C.cpu().numpy(), T)
    assert len(log["Ts_iter"]) == log["n_outer"] and all(len(ts) == len(sizes) for ts in log["Ts_iter"])
    assert all(torch.equal(a, b) for a, b in zip(log["Ts_iter"][-1], log["T"]))      # the last snapshot IS the returned coupling
    np.testing.assert_allclose([float(e) for e in log["err_feature"]], g["r64_err_feature"], rtol=2e-3, atol=1e-6)


@pytest.mark.parametrize("path", NONE, ids=ids(NONE))
def test_symmetric_none_on_asymmetric_input_is_symmetric_false(path):
    g = np.load(path)
    Yt, Ct, small_int = _dense(g)
    kw = _kw(g)
    assert kw.pop("symmetric") is None
    none = ops.fgw_barycenter_batched(Yt, Ct, cs_small_int=small_int, symmetric=None, **kw)
    false = ops.fgw_barycenter_batched(Yt, Ct, cs_small_int=small_int, symmetric=False, **kw)
    _same(none, false)


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


SOLVERS = [("PGD", {}), ("PPA", {}), ("PPA", {"loss_fun": "kl_loss"}), ("BAPG", {"epsilon": 2.0})]
SOLVER_IDS = ["pgd", "ppa", "ppa_kl", "bapg"]


@pytest.mark.parametrize("solver,kw", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("shape,B,K", [("esol", 6, 5), ("bace", 4, 3)], ids=["n_le_64", "n_gt_64"])
def test_symmetric_none_on_symmetric_input_matches_true(shape, B, K, solver, kw):
    """Symmetric input graphs give symmetric barycenters: symmetric=None takes the symmetric form in every coupling solve (PGD: on the general
    kernel, where True takes the model path).  The radius graphs are symmetrised first: with more than 32 atoms within the cutoff the
    neighbour cap (max_num_neighbors = 32) drops edges of one direction only, and such a graph is rightly solved as a directed one."""
    Ys, Cs, _ = _model_batch(shape, B, K)
    Cs = torch.maximum(Cs, Cs.transpose(-1, -2)).contiguous()
    true = ops.fgw_barycenter_batched(Ys, Cs, cs_small_int=True, solver=solver, **kw)
    none = ops.fgw_barycenter_batched(Ys, Cs, cs_small_int=True, solver=solver, symmetric=None, **kw)
    assert bool(torch.isfinite(none[0]).all())
    for a, b, name in zip(true[:3], none[:3], NAMES):
        assert rel(b.cpu().numpy(), a.cpu().numpy()) <= 1e-5, name
    assert torch.equal(true[3][:, :3], none[3][:, :3])                   # outer, inner and Sinkhorn iteration counts
    assert int((none[3][:, 3] & 2).sum()) == 0                           # (no padded-node merge off the model path)


@pytest.mark.parametrize("solver,kw", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("shape,B,K", [("esol", 6, 5), ("bace", 4, 3)], ids=["n_le_64", "n_gt_64"])
def test_sym_false_adjacency_path_equals_the_dense_path(shape, B, K, solver, kw):
    """`adjacency=graph` with symmetric=False: the ragged neighbour lists are expanded into the dense scratch, then the same solve — bit for bit."""
    Ys, Cs, graph = _model_batch(shape, B, K)
    dense = ops.fgw_barycenter_batched(Ys, Cs, cs_small_int=True, solver=solver, symmetric=False, **kw)
    ragged = ops.fgw_barycenter_batched(Ys, None, adjacency=graph, solver=solver, symmetric=False, **kw)
    assert bool(torch.isfinite(dense[0]).all())
    _same(dense, ragged)


@pytest.mark.parametrize("path", [p for p in DENSE if "_n12_" in p and "none" not in p], ids=lambda p: os.path.basename(p)[8:-4])
def test_sym_backward_matches_reference_autograd(path):
    """Gradient through the final couplings held constant (barycenter.py:120), as for symmetric=True."""
    g = np.load(path)
    Yt, Ct, small_int = _dense(g)
    Yt.requires_grad_(True)
    Y, *_ = ops.fgw_barycenter_batched(Yt, Ct, cs_small_int=small_int, **_kw(g))
    (Y[0] * torch.from_numpy(g["r32_grad_w"]).to(dev)).sum().backward()
    yard = rel(g["r32_dYs"], g["r64_dYs"])
    e = rel(Yt.grad[0].cpu().numpy(), g["r64_dYs"])
    assert e <= max(1e-4, yard), (e, yard)


def _notebook(max_iter):
    g = np.load(os.path.join(GOLDEN, "cfm_log.npz"))
    N = int(g["N"])
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
    return pfgw.fgw_barycenters(N=N, Ys=[t(y) for y in g["Ys"]], Cs=[t(c) for c in g["Cs"]], ps=[t(p) for p in g["ps"]], lambdas=t(g["lambdas"]),
                                p=torch.ones(N, device=dev) / N, warmstartT=True, symmetric=False, method="sinkhorn_log", alpha=0.5, solver="PGD",
                                fixed_structure=False, fixed_features=False, epsilon=0.05, loss_fun="kl_loss", max_iter=max_iter, tol=1e-5,
                                numItermax=50, stopThr=5e-2, verbose=False, log=True, init_C=None), g


def test_notebook_call_first_iterations_match_the_reference():
    """notebooks/fgw.ipynb's call truncated to 3 outer iterations, entry by entry against the reference's fp64 run (its own fp32 run is
    already far away there: the call amplifies rounding)."""
    r = np.load(os.path.join(GOLDEN, "fgw_sym_notebook_cfm_it3.npz"))
    (Y, C, log), _ = _notebook(3)
    assert log["n_outer"] == len(r["r64_err_feature"]) == 3
    assert log["n_pgd"] == int(r["r64_inner"]) and log["n_sinkhorn"] == int(r["r64_sinkhorn"])
    assert np.abs(Y.cpu().numpy() - r["r64_Y"]).max() <= 1e-4
    assert np.abs(C.cpu().numpy() - r["r64_C"]).max() <= 1e-4
    assert np.abs(torch.stack(log["T"]).cpu().numpy() - r["r64_T"]).max() <= 1e-4


def test_notebook_call_full_length_invariants():
    """The 50-iteration notebook call: finite, and its outputs are the barycenter update of its own couplings (utils.py:76-95)."""
    (Y, C, log), g = _notebook(50)
    T = torch.stack(log["T"]).double().cpu()
    for v in (Y, C, T):
        assert bool(torch.isfinite(v).all())
    lam = torch.from_numpy(g["lambdas"]).double()
    Cs = torch.from_numpy(g["Cs"]).double(); Ys = torch.from_numpy(g["Ys"]).double()
    p = torch.ones(int(g["N"]), dtype=torch.float64) / int(g["N"])
    logsum = sum(lam[s] * (T[s] @ torch.log(torch.clamp(Cs[s], min=1e-15)) @ T[s].T) for s in range(len(T)))
    C_upd = torch.exp(logsum / torch.outer(p, p))
    Y_upd = sum(lam[s] * (T[s] @ Ys[s]) for s in range(len(T))) / p[:, None]
    assert rel(C.double().cpu().numpy(), C_upd.numpy()) <= 1e-4
    assert rel(Y.double().cpu().numpy(), Y_upd.numpy()) <= 1e-4
