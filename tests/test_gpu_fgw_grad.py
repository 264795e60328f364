"""The full backward of the FGW barycenter block on the GPU (conan_fgw_barycenter_bwd_full): gradients for Ys, Cs, p, lambdas, init_C and
init_Y.  Against the reference's own fp32 / fp64 autograd (tests/golden/fgw_grad_*.npz, written by make_fgw_grad_golden.py) through
fgw_barycenters; against fp64 autograd of the three update formulas on the kernel's own couplings over every LDS / tiling branch; the model
path (only Ys requires grad) launching exactly conan_fgw_barycenter_bwd; determinism and the edge cases (massless nodes, zero KL entries,
an underflowed KL barycenter)."""
import os

import numpy as np
import pytest
import torch

from helpers import golden_files, rel
from conan_fgw_amd import _lib
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops
from conan_fgw_amd._lib import call, ptr, stream_ptr
from conan_fgw_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
ALL = golden_files("fgw_grad_")
ids = lambda ps: [os.path.basename(p)[9:-4] for p in ps]
SYM = {1: True, 0: False, -1: None}


# ---------------------------------------------------------------------------------------------- 1. the reference's autograd
@pytest.mark.parametrize("path", ALL, ids=ids(ALL))
def test_gradients_match_the_reference(path):
    g = np.load(path)
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
    Ys = [leaf(g["Ys"][s, :n]) for s, n in enumerate(sizes)]
    Cs = [leaf(g["Cs"][s, :n, :n]) for s, n in enumerate(sizes)]
    ps = [leaf(np.ones(n) / n) for n in sizes]
    p = leaf(g["p"]) if "p" in g.files else None
    lam = leaf(g["lambdas"]) if "lambdas" in g.files else None
    init_C = leaf(g["init_C"])
    init_Y = leaf(g["init_Y"]) if "init_Y" in g.files else None
    Y, C = pfgw.fgw_barycenters(N, Ys, Cs, ps=ps, p=p, lambdas=lam, loss_fun=str(g["loss_fun"]), epsilon=float(g["epsilon"]),
                                symmetric=SYM[int(g["symmetric"])], alpha=float(g["alpha"]), max_iter=int(g["max_iter"]), tol=float(g["tol"]),
                                solver=str(g["solver"]), warmstartT=bool(g["warmstart"]), init_C=init_C, init_Y=init_Y,
                                fixed_structure=bool(g["fixed_structure"]), fixed_features=bool(g["fixed_features"]),
                                numItermax=int(g["num_iter_max"]), stopThr=float(g["stop_thr"]))
    gw = torch.from_numpy(np.random.RandomState(int(g["gw_seed"])).normal(size=tuple(Y.shape))).float().to(dev)
    gc = torch.from_numpy(np.random.RandomState(int(g["gc_seed"])).normal(size=tuple(C.shape))).float().to(dev)
    ((Y * gw).sum() + (C * gc).sum()).backward()
    grads = [str(x) for x in g["grads"]]

    def padded(ts, shape):
        out = np.zeros(shape, np.float32)
        for s, t in enumerate(ts):
            out[(s,) + tuple(slice(0, k) for k in t.shape)] = t.grad.cpu().numpy()
        return out

    got = {}
    for name, ts, shape in (("Ys", Ys, g["Ys"].shape), ("Cs", Cs, g["Cs"].shape)):
        if name in grads:
            assert all(t.grad is not None for t in ts), name
            got[name] = padded(ts, shape)
        else:
            assert all(t.grad is None for t in ts), name
    for name, t in (("p", p), ("lambdas", lam), ("init_C", init_C), ("init_Y", init_Y)):
        if t is None:
            continue
        if name in grads:
            assert t.grad is not None, name
            got[name] = t.grad.cpu().numpy()
        else:
            assert t.grad is None, name
    assert all(q.grad is None for q in ps)
    for name, val in got.items():
        assert np.isfinite(val).all(), name
        yard = rel(g["r32_d" + name], g["r64_d" + name])
        e = rel(val, g["r64_d" + name])
        assert e <= max(1e-4, yard), (name, e, yard)


# ---------------------------------------------------------------------------------------------- 2. exact adjoint on the kernel's own T
def _formulas(T, Ys, Cs, p, lam, init_C, init_Y, kl, fs, ff):
    """The reference's three update steps (utils.py:67-95) in fp64 on the couplings T [B,K,N,N]."""
    pinv = 1.0 / p
    if ff:
        Y = init_Y
    else:
        Y = pinv[:, :, None] * torch.einsum("k,bkij,bkjc->bic", lam, T, Ys)
    if fs:
        C = init_C
    else:
        X = torch.log(torch.clamp(Cs, min=1e-15)) if kl else Cs
        S = torch.einsum("k,bkij,bkjl,bkml->bim", lam, T, X, T) * pinv[:, :, None] * pinv[:, None, :]
        C = torch.exp(S) if kl else S
    return Y, C


def _inputs(B, K, N, d, kl, seed):
    g = torch.Generator().manual_seed(seed)
    Ys = torch.rand(B, K, N, d, generator=g) * 1.9 + 0.1
    if kl:
        Cs = torch.rand(B, K, N, N, generator=g) * 0.95 + 0.05
    else:
        A = (torch.rand(B, K, N, N, generator=g) < 0.3).float()
        Cs = torch.triu(A, 1) + torch.triu(A, 1).transpose(-1, -2)
    w = torch.rand(B, N, generator=g) + 0.5
    p = w / w.sum(1, keepdim=True)
    lam = torch.rand(K, generator=g) + 0.5
    lam = lam / lam.sum()
    init_C = Cs[:, 0].clone()
    init_Y = torch.rand(B, N, d, generator=g) + 0.1
    return Ys, Cs, p, lam, init_C, init_Y


ADJ = [(K, N) for N in (9, 33, 64, 65, 83, 130) for K in ((1, 5) if N in (33, 83, 130) else (5,))]


@pytest.mark.parametrize("fixed", ["none", "fixed_structure", "fixed_features"])
@pytest.mark.parametrize("loss", ["square_loss", "kl_loss"])
@pytest.mark.parametrize("K,N", ADJ, ids=[f"k{k}_n{n}" for k, n in ADJ])
def test_exact_adjoint_on_the_kernels_couplings(K, N, loss, fixed):
    B, d = 3, 16
    kl, fs, ff = loss == "kl_loss", fixed == "fixed_structure", fixed == "fixed_features"
    host = _inputs(B, K, N, d, kl, seed=N * 10 + K)
    leaves = [t.to(dev).requires_grad_(True) for t in host]
    Ys, Cs, p, lam, init_C, init_Y = leaves
    Y, C, T, info, errs = ops.fgw_barycenter_batched(Ys, Cs, p=p, lambdas=lam, init_C=init_C, init_Y=init_Y, loss_fun=loss,
                                                     fixed_structure=fs, fixed_features=ff, epsilon=0.5)
    gen = torch.Generator().manual_seed(1)
    gw = torch.rand(B, N, d, generator=gen) + 0.5          # positive: the sums behind dlambdas and dp do not cancel
    gc = torch.rand(B, N, N, generator=gen) + 0.5
    ((Y * gw.to(dev)).sum() + (C * gc.to(dev)).sum()).backward()

    ref = [t.double().requires_grad_(True) for t in host]
    Yr, Cr = _formulas(T.detach().cpu().double(), *ref, kl, fs, ff)
    ((Yr * gw.double()).sum() + (Cr * gc.double()).sum()).backward()
    for name, ours, r in zip(("Ys", "Cs", "p", "lambdas", "init_C", "init_Y"), leaves, ref):
        if r.grad is None:
            assert ours.grad is None, name
            continue
        assert ours.grad is not None, name
        e = rel(ours.grad.cpu().numpy(), r.grad.numpy())
        assert e <= 1e-5, (name, e)


# ---------------------------------------------------------------------------------------------- 3. the model path is untouched
def _model_batch(shape, B, K, seed=77):
    b = make_batch(shape, B, K, seed=seed)
    pos = torch.from_numpy(b.pos).to(dev); batch = torch.from_numpy(b.batch).to(dev)
    gp = ops.graph_ptr_from_batch(batch, b.num_graphs)
    graph = ops.RadiusGraph(pos, gp, b.num_graphs, 10.0 if shape == "esol" else 5.0, 32)
    torch.manual_seed(3)
    feat = torch.nn.functional.softplus(torch.randn(len(b.z), 64, device=dev))
    Ys, Cs = ops.fgw_densify(feat, graph, b.max_nodes, 0.5)
    N = b.max_nodes
    return Ys.view(B, K, N, 64).detach().contiguous(), Cs.view(B, K, N, N), graph


def _direct_bwd(T, dY, B, K, N, d, p=None, lam=None):
    dYs = torch.empty(B, K, N, d, device=dev)
    call("conan_fgw_barycenter_bwd", ptr(T), ptr(dY.contiguous()), ptr(p), ptr(lam), B, K, N, d, ptr(dYs), stream_ptr())
    return dYs


@pytest.mark.parametrize("adjacency", [False, True], ids=["dense", "adjacency"])
@pytest.mark.parametrize("shape,B,K", [("esol", 6, 5), ("bace", 4, 3)], ids=["n_le_64", "n_gt_64"])
def test_model_path_launches_only_the_ys_backward(shape, B, K, adjacency):
    Ys, Cs, graph = _model_batch(shape, B, K)
    N, d = Ys.shape[2], Ys.shape[3]
    Ys.requires_grad_(True)
    if adjacency:
        Y, C, T, info, errs = ops.fgw_barycenter_batched(Ys, None, adjacency=graph)
    else:
        Y, C, T, info, errs = ops.fgw_barycenter_batched(Ys, Cs, cs_small_int=True)
    assert not C.requires_grad
    gw = torch.randn(B, N, d, device=dev)
    names = []

    def trace(name, fn, args):
        names.append(name)
        return fn(*args)

    prev = _lib.set_call_trace(trace)
    try:
        (Y * gw).sum().backward()
        torch.cuda.synchronize()
    finally:
        _lib.set_call_trace(prev)
    assert names == ["conan_fgw_barycenter_bwd"]
    assert torch.equal(Ys.grad, _direct_bwd(T, gw, B, K, N, d))


@pytest.mark.parametrize("N", [33, 83, 130])
def test_full_path_dys_equals_the_ys_backward_bit_for_bit(N):
    """With more gradients asked for, dYs comes out of the full kernel: the same fma chains as conan_fgw_barycenter_bwd."""
    B, K, d = 3, 5, 64 if N < 100 else 16
    Ys, Cs, p, lam, _, _ = (t.to(dev) for t in _inputs(B, K, N, d, False, seed=3))
    Ys.requires_grad_(True); Cs.requires_grad_(True); lam.requires_grad_(True)
    Y, C, T, info, errs = ops.fgw_barycenter_batched(Ys, Cs, p=p, lambdas=lam)
    assert C.requires_grad
    gw = torch.randn(B, N, d, device=dev)
    names = []

    def trace(name, fn, args):
        names.append(name)
        return fn(*args)

    prev = _lib.set_call_trace(trace)
    try:
        (Y * gw).sum().backward()
        torch.cuda.synchronize()
    finally:
        _lib.set_call_trace(prev)
    assert names == ["conan_fgw_barycenter_bwd_full"]
    assert torch.equal(Ys.grad, _direct_bwd(T, gw, B, K, N, d, p, lam.detach()))


# ---------------------------------------------------------------------------------------------- 4. determinism and edge cases
def _all_grads(B, K, N, d, loss, p_zero=(), seed=11, Cs_override=None, massless_seed=0.0):
    Ys, Cs, p, lam, _, _ = _inputs(B, K, N, d, loss == "kl_loss", seed)
    if Cs_override is not None:
        Cs = Cs_override
    for i in p_zero:
        p[:, i] = 0.0
        Ys[:, :, i] = 0.0
        Cs[:, :, i, :] = 0.0; Cs[:, :, :, i] = 0.0
    p = p / p.sum(1, keepdim=True)
    leaves = [t.to(dev).requires_grad_(True) for t in (Ys, Cs, p, lam)]
    Y, C, T, info, errs = ops.fgw_barycenter_batched(leaves[0], leaves[1], p=leaves[2], lambdas=leaves[3], loss_fun=loss, epsilon=0.5)
    gen = torch.Generator().manual_seed(2)
    gw, gc = torch.randn(B, N, d, generator=gen).to(dev), torch.randn(B, N, N, generator=gen).to(dev)
    for i in p_zero:                                # the output gradient at a massless barycenter node
        gw[:, i] = massless_seed; gc[:, i, :] = massless_seed; gc[:, :, i] = massless_seed
    ((Y * gw).sum() + (C * gc).sum()).backward()
    return [t.grad for t in leaves], C.detach(), leaves[1].detach()


@pytest.mark.parametrize("N", [20, 83, 130])
@pytest.mark.parametrize("loss", ["square_loss", "kl_loss"])
def test_two_backward_passes_are_bit_identical(N, loss):
    a, _, _ = _all_grads(4, 5, N, 16, loss)
    b, _, _ = _all_grads(4, 5, N, 16, loss)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("N", [20, 83, 130])
@pytest.mark.parametrize("loss", ["square_loss", "kl_loss"])
def test_massless_nodes_carry_no_gradient(N, loss):
    """p_i = 0: dp_i = 0, every gradient finite, and the output gradient at node i (row i of dY, row / column i of dC) reaches nothing."""
    zero = (3, N - 1)
    a, _, _ = _all_grads(3, 4, N, 8, loss, p_zero=zero)
    b, _, _ = _all_grads(3, 4, N, 8, loss, p_zero=zero, massless_seed=1e3)
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x).all())
        assert torch.equal(x, y)
    for i in zero:
        assert bool((a[2][:, i] == 0).all())


def test_kl_zero_structure_entries_get_zero_gradient():
    B, K, N = 3, 4, 12
    A = (torch.rand(B, K, N, N, generator=torch.Generator().manual_seed(4)) < 0.4).float()
    Cs = torch.triu(A, 1) + torch.triu(A, 1).transpose(-1, -2)
    (dYs, dCs, dp, dlam), _, C2 = _all_grads(B, K, N, 8, "kl_loss", Cs_override=Cs)
    for t in (dYs, dCs, dp, dlam):
        assert bool(torch.isfinite(t).all())
    assert bool((dCs[C2 == 0] == 0).all())
    assert bool((dCs[C2 != 0] != 0).any())


def test_kl_underflowed_barycenter_gives_finite_dp():
    B, K, N = 2, 3, 16
    Cs = torch.full((B, K, N, N), 1e-30)            # log clamps at 1e-15; the massless rows / columns of C are exactly 0
    (dYs, dCs, dp, dlam), C, _ = _all_grads(B, K, N, 8, "kl_loss", p_zero=(2, 9), Cs_override=Cs)
    assert bool((C == 0).any())
    for t in (dYs, dCs, dp, dlam):
        assert bool(torch.isfinite(t).all())
