"""FGWMixup on the GPU: fgw.fused_ACC_torch / ops.fgw_acc_pair_batched and fgw.fgw_barycenters_BAPG / ops.fgw_mixup_barycenter_batched against
the reference's own fp32 / fp64 runs (tests/golden/mixup_acc_*.npz, mixup_bary_*.npz, written by make_fgw_mixup_golden.py) and, where no fixture
exists, against the fp64 restatement (tests/fgw_mixup_ref.py, held to every fixture by test_fgw_mixup_cpu.py).
Yardsticks: epoch, check and outer-iteration counts equal to the fp64 run's (every fixture is fair: no compared value sits near its
threshold); objectives within 1e-4 relative of r64 or no further from it than r32 is; errs within rtol 2e-3, atol 1e-6; Y and C within 1e-4 of
r64; X / T as test_gpu_fgw_solvers._check_matrices has it: within 1e-4 of r32, or no further from r64 than r32 is.  Against the restatement
(fp32 inputs exact in both, fp64 iteration in both, fp32 outputs: 6e-8 of rounding, amplified by the iteration like every perturbation): the
same 1e-4."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fgw_mixup_ref import acc_ref, fair, mixup_ref
from helpers import golden_files, rel
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops
from conan_fgw_amd._lib import FgwParams, call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
PAIRS, BARY = golden_files("mixup_acc_"), golden_files("mixup_bary_")
DENSE = [p for p in BARY if "ragged" not in p]
ids = lambda ps: [os.path.basename(p)[6:-4] for p in ps]
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
opt = lambda g, k, f=lambda v: v: f(t(g[k])) if k in g else None


def _check_matrix(val, r32, r64, key):
    yard = rel(r32, r64)
    e32, e64 = rel(val, r32), rel(val, r64)
    assert e32 <= 1e-4 or e64 <= yard, (key, e32, e64, yard)


def _check_objectives(objs, g):
    c64, c32 = g["r64_checks"], g["r32_checks"]
    assert np.isnan(objs[len(c64):]).all()
    for k, c in enumerate(c64):
        bound = max(1e-4 * abs(c), abs(float(c32[k]) - c) if k < len(c32) else 0.0)
        assert abs(float(objs[k]) - c) <= bound, (k, float(objs[k]), c, bound)


def _same(a, b):
    """Bit for bit, NaN included."""
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------- pair fixtures
def _pair_kw(g):
    return dict(alpha=float(g["alpha"]), rho=float(g["rho"]), epoch=int(g["epoch"]), eps=float(g["eps"]))


@pytest.mark.parametrize("path", PAIRS, ids=ids(PAIRS))
def test_pair_golden_vectors_ops(path):
    g = np.load(path)
    one = lambda v: v[None]
    X, objs, info = ops.fgw_acc_pair_batched(t(g["M"])[None], t(g["A"])[None], t(g["B"])[None], opt(g, "a", one), opt(g, "b", one), opt(g, "X0", one),
                                             **_pair_kw(g))
    assert X.shape == (1,) + g["M"].shape and objs.shape == (1, (int(g["epoch"]) + 9) // 10)
    assert info[0].tolist() == [int(g["r64_epochs"]), len(g["r64_objs"]), 0, 0]
    _check_objectives(objs[0].cpu().numpy(), g)
    _check_matrix(X[0].cpu().numpy(), g["r32_X"], g["r64_X"], "X")


@pytest.mark.parametrize("path", PAIRS, ids=ids(PAIRS))
def test_pair_golden_vectors_api(path):
    g = np.load(path)
    X, obj_list = pfgw.fused_ACC_torch(t(g["M"]), t(g["A"]), t(g["B"]), opt(g, "a"), opt(g, "b"), opt(g, "X0"), **_pair_kw(g))
    assert isinstance(obj_list, list) and len(obj_list) == len(g["r64_objs"])
    np.testing.assert_allclose([float(o) for o in obj_list], g["r64_objs"], rtol=1e-4)
    assert not X.requires_grad
    _check_matrix(X.cpu().numpy(), g["r32_X"], g["r64_X"], "X")


# ---------------------------------------------------------------------------------------------------------------------- barycenter fixtures
def _bary_kw(g):
    return dict(alpha=float(g["alpha"]), rho=float(g["rho"]), max_iter=int(g["max_iter"]), tol=float(g["tol"]), loss_fun=str(g["loss_fun"]),
                fixed_structure=bool(g["fixed_structure"]), fixed_features=bool(g["fixed_features"]))


def _check_bary(g, Y, C, T, outer, inner, err_f, err_s):
    assert outer == len(g["r64_err_feature"]) and inner == int(g["r64_epochs"].sum())
    np.testing.assert_allclose(err_f, g["r64_err_feature"], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(err_s, g["r64_err_structure"], rtol=2e-3, atol=1e-6)
    assert rel(Y, g["r64_Y"]) <= 1e-4 and rel(C, g["r64_C"]) <= 1e-4, (rel(Y, g["r64_Y"]), rel(C, g["r64_C"]))
    _check_matrix(T, g["r32_T"], g["r64_T"], "T")


@pytest.mark.parametrize("path", DENSE, ids=ids(DENSE))
def test_bary_golden_vectors_ops(path):
    g = np.load(path)
    N, one = int(g["N"]), lambda v: v[None]
    init_C = None if str(g["init"]) == "first" else pfgw._seeded_init_C(N, int(g["seed"]), dev)[None]
    Y, C, T, info, errs = ops.fgw_mixup_barycenter_batched(t(g["Ys"])[None], t(g["Cs"])[None], opt(g, "ps", one), opt(g, "p", one), opt(g, "lambdas"),
                                                           init_C, opt(g, "init_Y", one), **_bary_kw(g))
    outer = int(info[0, 0])
    assert int(info[0, 2]) == 0 and int(info[0, 3]) == 0
    assert np.isnan(errs[0, :, outer:].cpu().numpy()).all()
    _check_bary(g, Y[0].cpu().numpy(), C[0].cpu().numpy(), T[0].cpu().numpy(), outer, int(info[0, 1]), errs[0, 0, :outer].cpu().numpy(),
                errs[0, 1, :outer].cpu().numpy())


@pytest.mark.parametrize("path", BARY, ids=ids(BARY))
def test_bary_golden_vectors_api(path):
    g = np.load(path)
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    K, d = len(sizes), g["Ys"].shape[2]
    Ys = [t(g["Ys"][s, :sizes[s]]) for s in range(K)]
    Cs = [t(g["Cs"][s, :sizes[s], :sizes[s]]) for s in range(K)]
    ps = [t(g["ps"][s, :sizes[s]]) for s in range(K)] if "ps" in g else None
    kw = _bary_kw(g)
    Y, C, log = pfgw.fgw_barycenters_BAPG(N, Ys, Cs, ps=ps, p=opt(g, "p"), lambdas=opt(g, "lambdas"), init_C=Cs[0] if str(g["init"]) == "first" else None,
                                          init_Y=opt(g, "init_Y"), seed=int(g["seed"]), log=True, **kw)
    assert set(log) == {"err_feature", "err_structure", "Ts_iter", "T", "p", "Ms", "n_outer", "n_inner"}
    outer = log["n_outer"]
    assert Y.shape == (N, d) and C.shape == (N, N) and not Y.requires_grad
    assert len(log["err_feature"]) == len(log["err_structure"]) == len(log["Ts_iter"]) == outer
    assert [tuple(x.shape) for x in log["T"]] == [(N, n) for n in sizes] and [tuple(m.shape) for m in log["Ms"]] == [(N, n) for n in sizes]
    assert all([tuple(x.shape) for x in it] == [(N, n) for n in sizes] for it in log["Ts_iter"])
    assert all(torch.equal(a, b) for a, b in zip(log["Ts_iter"][-1], log["T"])) and tuple(log["p"].shape) == (N,)
    T = np.zeros((K, N, max(sizes)), np.float32)
    for s, n in enumerate(sizes):
        T[s, :, :n] = log["T"][s].cpu().numpy()
        y = Y.double().cpu().numpy(); z = g["Ys"][s, :n].astype(np.float64)
        Ms = np.maximum((y * y).sum(1)[:, None] + (z * z).sum(1)[None, :] - 2 * y @ z.T, 0)
        np.testing.assert_allclose(log["Ms"][s].cpu().numpy(), Ms, rtol=1e-4, atol=1e-5)
    _check_bary(g, Y.cpu().numpy(), C.cpu().numpy(), T, outer, log["n_inner"], [float(e) for e in log["err_feature"]], [float(e) for e in log["err_structure"]])
    Y2, C2 = pfgw.fgw_barycenters_BAPG(N, Ys, Cs, ps=ps, p=opt(g, "p"), lambdas=opt(g, "lambdas"), init_C=Cs[0] if str(g["init"]) == "first" else None,
                                       init_Y=opt(g, "init_Y"), seed=int(g["seed"]), **kw)
    _same(Y2, Y); _same(C2, C)


# ---------------------------------------------------------------------------------------------------------------------- against the restatement
def _random_pairs(seed, B, N, d=6):
    rng = np.random.RandomState(seed)
    y, z = rng.uniform(0.1, 1.5, size=(B, N, d)), rng.uniform(0.1, 1.5, size=(B, N, d))
    M = ((y[:, :, None] - z[:, None]) ** 2).sum(-1).astype(np.float32)
    A = (rng.random_sample((B, N, N)) < 0.3).astype(np.float32) * (1 - np.eye(N, dtype=np.float32))
    Bm = (rng.random_sample((B, N, N)) < 0.3).astype(np.float32) * (1 - np.eye(N, dtype=np.float32))          # directed
    a = rng.uniform(0.5, 1.5, size=(B, N)); b = rng.uniform(0.5, 1.5, size=(B, N))
    return M, A, Bm, (a / a.sum(1, keepdims=True)).astype(np.float32), (b / b.sum(1, keepdims=True)).astype(np.float32)


def _lds_edge():
    """The largest N whose matrices are LDS-resident, found from the library's own answer."""
    L = lib()
    N = 1
    while L.conan_fgw_acc_lds_resident(N + 1):
        N += 1
        assert N < 400
    return N


@pytest.mark.parametrize("which", ["lds_max", "streamed_min", "63", "64", "65"])
def test_pair_against_restatement_at_the_size_edges(which):
    edge = _lds_edge()
    N = {"lds_max": edge, "streamed_min": edge + 1}.get(which) or int(which)
    assert lib().conan_fgw_acc_lds_resident(N) == (0 if which == "streamed_min" else 1)
    kw = dict(alpha=0.5, rho=float(N) / 8, epoch=25, eps=1e-5)          # two checks (epochs 11 and 21); rho grows with N as the gradient's entries do
    M, A, Bm, a, b = _random_pairs(1000 + N, 2, N)
    X, objs, info = ops.fgw_acc_pair_batched(t(M), t(A), t(Bm), t(a), t(b), **kw)
    for i in range(2):
        Xr, lg = acc_ref(M[i], A[i], Bm[i], a[i], b[i], **kw)
        assert np.isfinite(Xr).all() and fair(lg["rel"], kw["eps"]), lg["rel"]
        assert info[i].tolist() == [lg["epochs"], len(lg["objs"]), 0, 0]
        np.testing.assert_allclose(objs[i, :len(lg["checks"])].cpu().numpy(), lg["checks"], rtol=1e-4)
        assert rel(X[i].cpu().numpy(), Xr) <= 1e-4


def test_rectangular_and_own_sizes_against_restatement():
    """N1 != N2 containers and per-pair own sizes: the leading block is the rectangular solve, everything else exactly zero."""
    M, A, Bm, _, _ = _random_pairs(77, 3, 12)
    n1, n2 = [12, 5, 1], [7, 7, 4]
    kw = dict(alpha=0.6, rho=0.8, epoch=25, eps=1e-5)
    X, objs, info = ops.fgw_acc_pair_batched(t(M[:, :, :7]), t(A), t(Bm[:, :7, :7]), n1=torch.tensor(n1), n2=torch.tensor(n2), **kw)
    assert X.shape == (3, 12, 7)
    for i in range(3):
        Xr, lg = acc_ref(M[i, :n1[i], :n2[i]], A[i, :n1[i], :n1[i]], Bm[i, :n2[i], :n2[i]], **kw)
        assert fair(lg["rel"], kw["eps"]) and info[i].tolist() == [lg["epochs"], len(lg["objs"]), 0, 0]
        Xi = X[i].cpu().numpy()
        assert rel(Xi[:n1[i], :n2[i]], Xr) <= 1e-4
        Xi[:n1[i], :n2[i]] = 0
        assert not Xi.any()


# ---------------------------------------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize("N", [20, 84], ids=["lds", "streamed"])
def test_pair_alone_and_at_every_batch_position_same_bits(N):
    B = 7
    M, A, Bm, a, b = _random_pairs(5, B, N)
    a[3, N // 2:] = 0; a[3] /= a[3].sum()                     # a mixed batch: one problem has massless nodes
    kw = dict(alpha=0.5, rho=float(N) / 8, epoch=25, eps=1e-5)
    full = ops.fgw_acc_pair_batched(t(M), t(A), t(Bm), t(a), t(b), **kw)
    for i in range(B):
        solo = ops.fgw_acc_pair_batched(t(M[i:i + 1]), t(A[i:i + 1]), t(Bm[i:i + 1]), t(a[i:i + 1]), t(b[i:i + 1]), **kw)
        for x, y in zip(solo, full):
            _same(x[0], y[i])
        perm = np.roll(np.arange(B), i + 1)                  # problem i at another position of another batch
        moved = ops.fgw_acc_pair_batched(t(M[perm]), t(A[perm]), t(Bm[perm]), t(a[perm]), t(b[perm]), **kw)
        for x, y in zip(moved, full):
            _same(x[int(np.where(perm == i)[0][0])], y[i])
    again = ops.fgw_acc_pair_batched(t(M), t(A), t(Bm), t(a), t(b), **kw)
    for x, y in zip(again, full):
        _same(x, y)


def test_molecules_that_stop_at_different_outer_iterations_equal_their_solo_runs():
    g = np.load([p for p in BARY if p.endswith("k4_n12_d8_default.npz")][0])          # stops after 2 outer iterations
    K, N, d = g["Ys"].shape
    rng = np.random.RandomState(9)
    Ys = np.stack([g["Ys"]] + [rng.uniform(0.1, 2.0, size=(K, N, d)).astype(np.float32) for _ in range(3)])
    Cs = [g["Cs"]]
    for _ in range(3):
        u = np.triu(rng.random_sample((K, N, N)) < 0.4, 1)
        Cs.append((u | u.transpose(0, 2, 1)).astype(np.float32))
    Cs = np.stack(Cs)
    kw = dict(alpha=0.5, rho=1.0, max_iter=6, tol=1e-9)
    full = ops.fgw_mixup_barycenter_batched(t(Ys), t(Cs), keep_iterates=True, **kw)
    outers = full[3][:, 0].tolist()
    assert outers[0] == 2 and len(set(outers)) > 1, outers
    for i in range(4):
        solo = ops.fgw_mixup_barycenter_batched(t(Ys[i:i + 1]), t(Cs[i:i + 1]), **kw)
        for x, y in zip(solo, full[:5]):
            _same(x[0], y[i])
    # the snapshots of a molecule stop changing once it has stopped
    assert torch.equal(full[5][1, 0], full[5][5, 0]) and torch.equal(full[5][5, 0], full[2][0])


def test_c_entry_points_called_directly_equal_ops():
    M, A, Bm, a, b = _random_pairs(21, 3, 33)
    kw = dict(alpha=0.5, rho=4.0, epoch=25, eps=1e-5)
    want = ops.fgw_acc_pair_batched(t(M), t(A), t(Bm), t(a), t(b), **kw)
    B, N = 3, 33
    X = torch.empty(B, N, N, device=dev); objs = torch.empty(B, 3, device=dev); info = torch.empty(B, 4, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib().conan_fgw_acc_pair_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)
    ins = [t(v) for v in (M, A, Bm, a, b)]
    call("conan_fgw_acc_pair_fwd", *[ptr(v) for v in ins], None, B, N, 0.5, 4.0, 25, 1e-5, ptr(X), ptr(objs), ptr(info), ptr(ws), stream_ptr())
    for x, y in zip((X, objs, info), want):
        _same(x, y)

    g = np.load([p for p in BARY if p.endswith("k3_n33_d8.npz")][0])
    K, N, d = g["Ys"].shape
    Ys, Cs = t(g["Ys"])[None], t(g["Cs"])[None]
    want = ops.fgw_mixup_barycenter_batched(Ys, Cs, **_bary_kw(g))
    mi = int(g["max_iter"])
    prm = FgwParams(float(g["alpha"]), 0.0, mi, float(g["tol"]), 0.0, 1, 0.0, 0, 0, 0, 0, 0)
    Y = torch.empty(1, N, d, device=dev); C = torch.empty(1, N, N, device=dev); T = torch.empty(1, K, N, N, device=dev)
    info = torch.empty(1, 4, dtype=torch.int32, device=dev); errs = torch.empty(1, 2, mi, device=dev)
    ws = torch.empty(int(lib().conan_fgw_mixup_workspace_bytes(1, K, N, d)), dtype=torch.uint8, device=dev)
    call("conan_fgw_mixup_barycenter_fwd", ptr(Ys), ptr(Cs), None, None, None, None, None, 1, K, N, d, ctypes.byref(prm), float(g["rho"]), 100, 1e-5,
         ptr(Y), ptr(C), ptr(T), None, ptr(info), ptr(errs), ptr(ws), stream_ptr())
    for x, y in zip((Y, C, T, info, errs), want):
        _same(x, y)


# ---------------------------------------------------------------------------------------------------------------------- the NaN case
def test_underflow_gives_the_reference_nan_and_flags_bit_2():
    """64-wide features at rho = 1e-2: (1 - alpha) M / rho is in the thousands, so every exp of the first half-step underflows to 0 in fp64,
    every row sum is 0 and a / 0 * 0 is NaN — the fp64 restatement (asserted below, seed 3) says so, as the reference's fp64 run does.  An
    underflow, not a fault: the solve runs its epochs on NaNs and ends."""
    rng = np.random.RandomState(3)
    K, N, d = 3, 12, 64
    Ys = rng.uniform(0.1, 2.0, size=(2, K, N, d)).astype(np.float32)
    u = np.triu(rng.random_sample((2, K, N, N)) < 0.4, 1)
    Cs = (u | u.transpose(0, 1, 3, 2)).astype(np.float32)
    Yr, Cr, lg = mixup_ref(N, list(Ys[0]), list(Cs[0]), init_C=Cs[0, 0], alpha=0.5, rho=1e-2, max_iter=3)
    assert np.isnan(Yr).all() and np.isnan(Cr).all() and len(lg["err_feature"]) == 1 and lg["epochs"] == [[100] * K]
    before = ops.fgw_mixup_barycenter_batched(t(Ys), t(Cs), alpha=0.5, rho=20.0, max_iter=2)
    Y, C, T, info, errs = ops.fgw_mixup_barycenter_batched(t(Ys), t(Cs), alpha=0.5, rho=1e-2, max_iter=3)
    assert (info[:, 3] & 4).bool().all() and info[:, 0].tolist() == [1, 1] and info[:, 1].tolist() == [100 * K] * 2
    assert torch.isnan(Y).all() and torch.isnan(C).all() and torch.isnan(T).all()
    X, objs, info = ops.fgw_acc_pair_batched(t(Ys[0, :1, :, :N] * 100), t(Cs[0, :1]), t(Cs[0, 1:2]), alpha=0.5, rho=1e-3, epoch=45)
    assert info[0].tolist() == [45, 4, 4, 0] and torch.isnan(X).all() and torch.isnan(objs[0, :4]).all()
    # a finite solve right after succeeds: the same bits as before the NaN solves
    after = ops.fgw_mixup_barycenter_batched(t(Ys), t(Cs), alpha=0.5, rho=20.0, max_iter=2)
    assert after[3][:, 3].tolist() == [0, 0] and torch.isfinite(after[0]).all() and torch.isfinite(after[1]).all()
    for x, y in zip(after, before):
        _same(x, y)
