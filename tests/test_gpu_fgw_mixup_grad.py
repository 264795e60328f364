"""The differentiable FGWMixup pair on the GPU: fgw.fgw_barycenters_BAPG / ops.fgw_mixup_barycenter_batched with gradients for Ys, Cs, p,
lambdas, init_C and init_Y, and fgw.fgw_mixup_distance / ops.fgw_acc_pair_distance, in the fixed-plan convention (the couplings of the last outer
iteration are constants).  Against the reference's own update steps differentiated at its couplings (tests/golden/mixup_grad_*.npz, written by
make_fgw_mixup_grad_golden.py) through the public function; against fp64 autograd of the plain formulas (tests/fgw_mixup_grad_ref.py, held to every
fixture by test_fgw_mixup_grad_cpu.py) on the kernel's own couplings over every LDS / tiling branch of the forward and the backward; which C-ABI calls
are issued with which leaves; determinism and the edge cases (massless nodes, zero KL entries, tensor-valued lambdas); the distance on the
mixup_acc_* fixtures' inputs.  Yardsticks: against the fixtures max(1e-4, rel(r32, r64)), as test_gpu_fgw_grad.py; against the formulas at the
kernel's own couplings 1e-5 (fp32 fma chains over at most 130 terms against fp64), the value of the distance 1e-5 as test_gpu_fgw_pair.py has it."""
import os

import numpy as np
import pytest
import torch

from fgw_mixup_grad_ref import mixup_distance, update_steps
from helpers import golden_files, rel
from conan_fgw_amd import _lib
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops
from conan_fgw_amd._lib import call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GRAD, PAIRS = golden_files("mixup_grad_"), golden_files("mixup_acc_")
bits = lambda x: x.contiguous().view(torch.int32)
KW = dict(alpha=0.5, rho=8.0, max_iter=2, epoch=20)          # (rho 8: the feature costs of d = 16 uniform features reach about 50; no exp underflows)


class Trace:
    """Records the name of every C-ABI call issued inside the block."""

    def __enter__(self):
        self.names = []

        def trace(name, fn, args):
            self.names.append(name)
            return fn(*args)
        self._prev = _lib.set_call_trace(trace)
        return self.names

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _lib.set_call_trace(self._prev)


# ---------------------------------------------------------------------------------------------- 1. the reference's update steps at its couplings
@pytest.mark.parametrize("path", GRAD, ids=[os.path.basename(p)[11:-4] for p in GRAD])
def test_gradients_match_the_reference(path):
    g = np.load(path)
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
    Ys = [leaf(g["Ys"][s, :n]) for s, n in enumerate(sizes)]
    Cs = [leaf(g["Cs"][s, :n, :n]) for s, n in enumerate(sizes)]
    ps = [leaf(g["ps"][s, :n]) for s, n in enumerate(sizes)]
    p = leaf(g["p"]) if "p" in g.files else None
    lam = leaf(g["lambdas"]) if "lambdas" in g.files else None
    init_C = leaf(g["init_C"])
    init_Y = leaf(g["init_Y"]) if "init_Y" in g.files else None
    Y, C, log = pfgw.fgw_barycenters_BAPG(N, Ys, Cs, ps=ps, p=p, lambdas=lam, loss_fun=str(g["loss_fun"]), alpha=float(g["alpha"]),
                                          max_iter=int(g["max_iter"]), tol=float(g["tol"]), rho=float(g["rho"]), init_C=init_C, init_Y=init_Y,
                                          fixed_structure=bool(g["fixed_structure"]), fixed_features=bool(g["fixed_features"]), log=True)
    assert log["n_outer"] == int(g["outer"]) and Y.shape == g["r64_Y"].shape and C.shape == g["r64_C"].shape
    assert not any(x.requires_grad for x in log["T"] + log["Ms"] + [x for it in log["Ts_iter"] for x in it])
    assert rel(Y.detach().cpu().numpy(), g["r64_Y"]) <= 1e-4 and rel(C.detach().cpu().numpy(), g["r64_C"]) <= 1e-4
    gw = torch.from_numpy(np.random.RandomState(int(g["gw_seed"])).normal(size=tuple(Y.shape))).float().to(dev)
    gc = torch.from_numpy(np.random.RandomState(int(g["gc_seed"])).normal(size=tuple(C.shape))).float().to(dev)
    ((Y * gw).sum() + (C * gc).sum()).backward()
    grads = [str(x) for x in g["grads"]]

    def padded(ts, shape):
        out = np.zeros(shape, np.float32)
        for s, t in enumerate(ts):
            assert t.grad.shape == t.shape                       # the caller's own shapes
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
            assert t.grad is not None and t.grad.shape == t.shape, name
            got[name] = t.grad.cpu().numpy()
        else:
            assert t.grad is None, name
    assert all(q.grad is None for q in ps)
    assert sorted(got) == sorted(grads)
    for name, val in got.items():
        assert np.isfinite(val).all(), name
        yard = rel(g["r32_d" + name], g["r64_d" + name])
        e = rel(val, g["r64_d" + name])
        print(f"{name}: rel(ours, r64) {e:.2e}  rel(r32, r64) {yard:.2e}")
        assert e <= max(1e-4, yard), (name, e, yard)


# ---------------------------------------------------------------------------------------------- 2. exact adjoint on the kernel's own T
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


def _acc_lds_edge():
    """The largest N whose matrices the coupling solve keeps in LDS, found from the library's own answer."""
    N = 1
    while lib().conan_fgw_acc_lds_resident(N + 1):
        N += 1
        assert N < 400
    return N


# 16-wide tile edges of the backward's MFMA products; 112 | 113: its LDS-to-scratch boundary; both sides of the forward's LDS residency
ADJ = [(K, str(N)) for N in (9, 16, 17, 33) for K in (1, 5)] + [(2, str(N)) for N in (112, 113, 130)] + [(2, "acc_lds_max"), (2, "acc_streamed_min")]


@pytest.mark.parametrize("fixed", ["none", "fixed_structure", "fixed_features"])
@pytest.mark.parametrize("loss", ["square_loss", "kl_loss"])
@pytest.mark.parametrize("K,size", ADJ, ids=[f"k{k}_n{n}" for k, n in ADJ])
def test_exact_adjoint_on_the_kernels_couplings(K, size, loss, fixed):
    if size.startswith("acc_"):
        edge = _acc_lds_edge()
        N = edge if size == "acc_lds_max" else edge + 1
        assert lib().conan_fgw_acc_lds_resident(N) == (1 if size == "acc_lds_max" else 0)
    else:
        N = int(size)
    B, d = 3, 16
    kl, fs, ff = loss == "kl_loss", fixed == "fixed_structure", fixed == "fixed_features"
    host = _inputs(B, K, N, d, kl, seed=N * 10 + K)
    leaves = [t.to(dev).requires_grad_(True) for t in host]
    Ys, Cs, p, lam, init_C, init_Y = leaves
    Y, C, T, info, errs = ops.fgw_mixup_barycenter_batched(Ys, Cs, p=p, lambdas=lam, init_C=init_C, init_Y=init_Y, loss_fun=loss, fixed_structure=fs,
                                                           fixed_features=ff, **KW)
    assert info[:, 3].tolist() == [0] * B and not T.requires_grad and not info.requires_grad and not errs.requires_grad
    gen = torch.Generator().manual_seed(1)
    gw = torch.rand(B, N, d, generator=gen) + 0.5          # positive: the sums behind dlambdas and dp do not cancel
    gc = torch.rand(B, N, N, generator=gen) + 0.5
    ((Y * gw.to(dev)).sum() + (C * gc.to(dev)).sum()).backward()

    ref = [t.double().requires_grad_(True) for t in host]
    Yr, Cr = update_steps(T.detach().cpu().double(), *ref, kl, fs, ff)
    assert rel(Y.detach().cpu().numpy(), Yr.detach().numpy()) <= 1e-5 and rel(C.detach().cpu().numpy(), Cr.detach().numpy()) <= 1e-5
    ((Yr * gw.double()).sum() + (Cr * gc.double()).sum()).backward()
    for name, ours, r in zip(("Ys", "Cs", "p", "lambdas", "init_C", "init_Y"), leaves, ref):
        if r.grad is None:
            assert ours.grad is None, name
            continue
        assert ours.grad is not None, name
        e = rel(ours.grad.cpu().numpy(), r.grad.numpy())
        assert e <= 1e-5, (name, e)


# ---------------------------------------------------------------------------------------------- 3. which calls are issued
def _direct_bwd(T, dY, B, K, N, d, p=None, lam=None):
    dYs = torch.empty(B, K, N, d, device=dev)
    call("conan_fgw_barycenter_bwd", ptr(T), ptr(dY.contiguous()), ptr(p), ptr(lam), B, K, N, d, ptr(dYs), stream_ptr())
    return dYs


@pytest.mark.parametrize("N", [33, 130])
def test_ys_only_backward_is_the_ys_kernel_alone(N):
    B, K, d = 3, 5, 16
    Ys, Cs, p, lam, _, _ = (t.to(dev) for t in _inputs(B, K, N, d, False, seed=3))
    Ys.requires_grad_(True)
    Y, C, T, info, errs = ops.fgw_mixup_barycenter_batched(Ys, Cs, p=p, lambdas=lam, **KW)
    assert Y.requires_grad and not C.requires_grad
    gw = torch.randn(B, N, d, device=dev)
    with Trace() as names:
        (Y * gw).sum().backward()
    assert names == ["conan_fgw_barycenter_bwd"]
    want = _direct_bwd(T, gw, B, K, N, d, p, lam)
    assert torch.equal(bits(Ys.grad), bits(want))

    # with more leaves dYs comes out of the full kernel: the same fma chains, the same bits
    Ys2, Cs2, lam2 = Ys.detach().clone().requires_grad_(True), Cs.clone().requires_grad_(True), lam.clone().requires_grad_(True)
    Y2, C2, T2, _, _ = ops.fgw_mixup_barycenter_batched(Ys2, Cs2, p=p, lambdas=lam2, **KW)
    assert C2.requires_grad and torch.equal(bits(T2), bits(T)) and torch.equal(bits(Y2.detach()), bits(Y.detach()))
    with Trace() as names:
        (Y2 * gw).sum().backward()
    assert names == ["conan_fgw_barycenter_bwd_full"]
    assert torch.equal(bits(Ys2.grad), bits(want)) and not bool(Cs2.grad.any()) and bool(torch.isfinite(lam2.grad).all())      # (no dC came in: dCs is zero)


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep_iterates"])
def test_no_grad_path_issues_the_forward_call_alone_and_gives_the_same_bits(keep):
    B, K, N, d = 3, 3, 20, 16
    Ys, Cs, p, lam, _, _ = (t.to(dev) for t in _inputs(B, K, N, d, False, seed=5))
    kw = dict(KW, keep_iterates=keep)
    with Trace() as names:
        plain = ops.fgw_mixup_barycenter_batched(Ys, Cs, p=p, lambdas=lam, **kw)
    assert names == ["conan_fgw_mixup_barycenter_fwd"] and not any(t.requires_grad for t in plain) and len(plain) == 5 + keep
    leaves = [t.clone().requires_grad_(True) for t in (Ys, Cs, p, lam)]
    with torch.no_grad(), Trace() as names:
        off = ops.fgw_mixup_barycenter_batched(leaves[0], leaves[1], p=leaves[2], lambdas=leaves[3], **kw)
    assert names == ["conan_fgw_mixup_barycenter_fwd"] and not any(t.requires_grad for t in off)
    with Trace() as names:
        on = ops.fgw_mixup_barycenter_batched(leaves[0], leaves[1], p=leaves[2], lambdas=leaves[3], **kw)
    assert names == ["conan_fgw_mixup_barycenter_fwd"]
    assert on[0].requires_grad and on[1].requires_grad and not any(t.requires_grad for t in on[2:])
    for a, b, c in zip(plain, off, on):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c.detach()))


# ---------------------------------------------------------------------------------------------- 4. determinism and edge cases
def _all_grads(B, K, N, d, loss, p_zero=(), ps_zero=(), seed=11, Cs_override=None, massless_seed=0.0):
    Ys, Cs, p, lam, _, _ = _inputs(B, K, N, d, loss == "kl_loss", seed)
    if Cs_override is not None:
        Cs = Cs_override
    for i in p_zero:
        p[:, i] = 0.0
    p = p / p.sum(1, keepdim=True)
    ps = torch.ones(B, K, N)
    for j in ps_zero:                                   # an absent node of every input graph: no mass, zero features, no edges
        ps[:, :, j] = 0.0
        Ys[:, :, j] = 0.0
        Cs[:, :, j, :] = 0.0; Cs[:, :, :, j] = 0.0
    ps = ps / ps.sum(2, keepdim=True)
    leaves = [t.to(dev).requires_grad_(True) for t in (Ys, Cs, p, lam)]
    Y, C, T, info, errs = ops.fgw_mixup_barycenter_batched(leaves[0], leaves[1], ps=ps.to(dev), p=leaves[2], lambdas=leaves[3], loss_fun=loss, **KW)
    assert info[:, 3].tolist() == [0] * B
    gen = torch.Generator().manual_seed(2)
    gw, gc = torch.randn(B, N, d, generator=gen).to(dev), torch.randn(B, N, N, generator=gen).to(dev)
    for i in p_zero:                                    # the output gradient at a massless barycenter node
        gw[:, i] = massless_seed; gc[:, i, :] = massless_seed; gc[:, :, i] = massless_seed
    ((Y * gw).sum() + (C * gc).sum()).backward()
    return [t.grad for t in leaves], C.detach(), leaves[1].detach()


@pytest.mark.parametrize("N", [20, 130])
@pytest.mark.parametrize("loss", ["square_loss", "kl_loss"])
def test_two_backward_passes_are_bit_identical(N, loss):
    a, _, _ = _all_grads(4, 5, N, 16, loss)
    b, _, _ = _all_grads(4, 5, N, 16, loss)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))


@pytest.mark.parametrize("N", [20, 130])
@pytest.mark.parametrize("loss", ["square_loss", "kl_loss"])
def test_massless_nodes_get_exactly_zero_gradient(N, loss):
    """p_i = 0: dp_i = 0 and the output gradient at node i (row i of dY, row / column i of dC) reaches nothing; ps_j = 0: row j of dYs and row /
    column j of dCs are zero.  Every gradient is finite."""
    pz, qz = (3, N - 1), (0, N - 2)
    a, _, _ = _all_grads(3, 4, N, 8, loss, p_zero=pz, ps_zero=qz)
    b, _, _ = _all_grads(3, 4, N, 8, loss, p_zero=pz, ps_zero=qz, massless_seed=1e3)
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x).all())
        assert torch.equal(x, y)
    dYs, dCs, dp, dlam = a
    for i in pz:
        assert bool((dp[:, i] == 0).all())
    for j in qz:
        assert bool((dYs[:, :, j] == 0).all()) and bool((dCs[:, :, j, :] == 0).all()) and bool((dCs[:, :, :, j] == 0).all())
    assert bool((dYs != 0).any()) and bool((dCs != 0).any()) and bool((dp != 0).any())


def test_kl_zero_structure_entries_get_zero_gradient():
    B, K, N = 3, 4, 12
    A = (torch.rand(B, K, N, N, generator=torch.Generator().manual_seed(4)) < 0.4).float()
    Cs = torch.triu(A, 1) + torch.triu(A, 1).transpose(-1, -2)
    (dYs, dCs, dp, dlam), _, C2 = _all_grads(B, K, N, 8, "kl_loss", Cs_override=Cs)
    for t in (dYs, dCs, dp, dlam):
        assert bool(torch.isfinite(t).all())
    assert bool((dCs[C2 < 1e-15] == 0).all())
    assert bool((dCs[C2 >= 1e-15] != 0).any())


def test_a_list_of_lambdas_tensors_receives_gradients():
    """fgw_barycenters_BAPG with lambdas given as a list of 0-d tensors that require grad (a learnable mixing weight): each receives .grad, the
    one the stacked tensor gets; a list of floats still works and gives the same bits of Y and C."""
    K, N, d = 2, 9, 4
    Ys, Cs, _, _, _, _ = (t.to(dev) for t in _inputs(1, K, N, d, False, seed=8))
    Ys, Cs = list(Ys[0]), list(Cs[0])
    lams = [torch.tensor(0.3, device=dev, requires_grad=True), torch.tensor(0.7, device=dev, requires_grad=True)]
    kw = dict(alpha=0.5, rho=8.0, max_iter=2, init_C=Cs[0])
    Y, C = pfgw.fgw_barycenters_BAPG(N, Ys, Cs, lambdas=lams, **kw)
    assert Y.requires_grad and C.requires_grad
    (Y.sum() + C.sum()).backward()
    assert all(l.grad is not None and l.grad.shape == () and bool(torch.isfinite(l.grad)) and float(l.grad) != 0 for l in lams)
    assert all(t.grad is None for t in Ys + Cs)
    stacked = torch.tensor([0.3, 0.7], device=dev, requires_grad=True)
    Y2, C2 = pfgw.fgw_barycenters_BAPG(N, Ys, Cs, lambdas=stacked, **kw)
    (Y2.sum() + C2.sum()).backward()
    assert torch.equal(bits(torch.stack([l.grad for l in lams])), bits(stacked.grad))
    Y3, C3 = pfgw.fgw_barycenters_BAPG(N, Ys, Cs, lambdas=[0.3, 0.7], **kw)
    assert not Y3.requires_grad and torch.equal(bits(Y3), bits(Y.detach())) and torch.equal(bits(C3), bits(C.detach()))


# ---------------------------------------------------------------------------------------------- 5. the distance
@pytest.mark.parametrize("path", PAIRS, ids=[os.path.basename(p)[10:-4] for p in PAIRS])
def test_mixup_distance_value_plan_and_gradients(path):
    g = np.load(path)
    n1, n2 = g["M"].shape
    alpha = float(g["alpha"])
    kw = dict(alpha=alpha, rho=float(g["rho"]), epoch=int(g["epoch"]), eps=float(g["eps"]))
    host = [g["M"], g["A"], g["B"], g["a"] if "a" in g.files else np.full(n1, 1.0 / n1, np.float32), g["b"] if "b" in g.files else np.full(n2, 1.0 / n2, np.float32)]
    host = [torch.from_numpy(np.ascontiguousarray(v, np.float32)) for v in host]
    X0 = torch.from_numpy(g["X0"]).to(dev) if "X0" in g.files else None
    M, A, Bm, a, b = leaves = [t.to(dev).requires_grad_(True) for t in host]
    dist, log = pfgw.fgw_mixup_distance(M, A, Bm, a, b, X0, log=True, **kw)
    X = log["T"]
    assert dist.shape == () and dist.requires_grad and X.shape == (n1, n2) and not X.requires_grad
    # the plan and the objectives are fused_ACC_torch's, bit for bit
    Xp, obj_list = pfgw.fused_ACC_torch(M, A, Bm, a, b, X0, **kw)
    assert not Xp.requires_grad and torch.equal(bits(X), bits(Xp)) and len(log["obj_list"]) == len(obj_list)
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(log["obj_list"], obj_list))

    # the value: the fp64 formula at the returned plan
    ref = [t.double().requires_grad_(True) for t in host]
    Xd = X.detach().cpu().double()
    want = mixup_distance(*(t[None] for t in ref), Xd[None], alpha)[0]
    print(f"dist {float(dist.detach()):.9g} formula {float(want.detach()):.9g}")
    dist_v, want_v = float(dist.detach()), float(want.detach())
    assert abs(dist_v - want_v) <= 1e-5 * abs(want_v)
    # ... which is the solve's final objective plus alpha <c1, X>: where the solve stopped on a check, that check's objective is of the returned plan
    _, _, objs, info = ops.fgw_acc_pair_distance(M[None], A[None], Bm[None], a[None], b[None], None if X0 is None else X0[None], return_plan=True, **kw)
    epochs, stored = int(info[0, 0]), int(info[0, 1])
    if epochs < kw["epoch"]:
        Ad, Bd, ad, bd = (t.detach() for t in ref[1:])
        c1 = ((Ad * Ad) @ ad)[:, None] + (bd @ (Bd * Bd))[None, :]
        final = float(objs[0, stored]) + alpha * float((c1 * Xd).sum())
        assert abs(dist_v - final) <= 1e-5 * abs(final), (dist_v, final)
    # a directed B: the untransposed B would give another value
    if not np.array_equal(g["B"], g["B"].T):
        other = mixup_distance(*(t[None].detach() for t in ref[:2]), ref[2].detach().T[None], ref[3].detach()[None], ref[4].detach()[None], Xd[None], alpha)[0]
        assert abs(float(other) - want_v) > 1e-3 * abs(want_v)
        assert abs(dist_v - float(other)) > 1e-3 * abs(want_v)

    # the gradients: fp64 autograd of the formula at that plan
    dist.backward()
    want.backward()
    for name, ours, r in zip(("M", "A", "B", "a", "b"), leaves, ref):
        assert ours.grad is not None and ours.grad.shape == ours.shape, name
        e = rel(ours.grad.cpu().numpy(), r.grad.numpy())
        print(f"d{name}: {e:.2e}")
        assert e <= 1e-5, (name, e)
    assert X0 is None or X0.grad is None


def test_fixture_set_has_the_distance_cases():
    shapes = {tuple(np.load(p)["M"].shape) for p in PAIRS}
    assert {(12, 7), (7, 12), (1, 5), (84, 84)} <= shapes
    assert any(np.load(p)["M"].shape == (12, 7) and not np.array_equal(np.load(p)["B"], np.load(p)["B"].T) for p in PAIRS)


def test_batched_distance_with_own_sizes_and_without_leaves():
    """ops.fgw_acc_pair_distance on a container with per-pair own sizes: each pair's value and gradients are those of its own rectangular problem
    (zero outside its block); with no leaf the value has the same bits and no graph."""
    rng = np.random.RandomState(7)
    Bn, N1, N2 = 3, 12, 7
    n1, n2 = [12, 5, 1], [7, 7, 4]
    M = torch.from_numpy(rng.uniform(0.1, 2.0, size=(Bn, N1, N2)).astype(np.float32))
    A = torch.from_numpy((rng.random_sample((Bn, N1, N1)) < 0.4).astype(np.float32))
    Bm = torch.from_numpy((rng.random_sample((Bn, N2, N2)) < 0.4).astype(np.float32))
    kw = dict(alpha=0.6, rho=0.8, epoch=25, eps=1e-5, n1=torch.tensor(n1), n2=torch.tensor(n2))
    plain = ops.fgw_acc_pair_distance(M.to(dev), A.to(dev), Bm.to(dev), **kw)
    assert not plain.requires_grad
    leaves = [t.to(dev).requires_grad_(True) for t in (M, A, Bm)]
    dist, X, objs, info = ops.fgw_acc_pair_distance(*leaves, return_plan=True, **kw)
    assert torch.equal(bits(dist.detach()), bits(plain)) and X.shape == (Bn, N1, N2) and not X.requires_grad
    dist.sum().backward()
    for i in range(Bn):
        r = [t[i, :n1[i], :n2[i]] if k == 0 else (t[i, :n1[i], :n1[i]] if k == 1 else t[i, :n2[i], :n2[i]]) for k, t in enumerate((M, A, Bm))]
        r = [t.double().clone().requires_grad_(True) for t in r]
        a, b = torch.full((1, n1[i]), 1.0 / n1[i], dtype=torch.float64), torch.full((1, n2[i]), 1.0 / n2[i], dtype=torch.float64)
        want = mixup_distance(r[0][None], r[1][None], r[2][None], a, b, X[i, :n1[i], :n2[i]].cpu().double()[None], 0.6)[0]
        assert abs(float(dist[i].detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
        want.backward()
        for k, (ours, blk) in enumerate(zip(leaves, ((n1[i], n2[i]), (n1[i], n1[i]), (n2[i], n2[i])))):
            got = ours.grad[i].cpu().numpy().copy()
            assert rel(got[:blk[0], :blk[1]], r[k].grad.numpy()) <= 1e-5, (i, k)
            got[:blk[0], :blk[1]] = 0
            assert not got.any(), (i, k)
