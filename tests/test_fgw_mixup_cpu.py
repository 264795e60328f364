"""CPU-side checks of the FGWMixup feature (fgw.fused_ACC_torch, fgw.fgw_barycenters_BAPG): the stored fixtures are complete, self-consistent and
fair; the fp64 restatement (tests/fgw_mixup_ref.py) reproduces every fixture's fp64 run, so it can stand in where no fixture exists; the massless
embedding equals the rectangular solve; the C ABI declares the new entry points, answers the size queries and refuses bad arguments before any
launch; the entry points that existed keep their codes.  No compute call: there is no GPU here."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from fgw_mixup_ref import acc_ref, fair, mixup_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PAIRS = sorted(glob.glob(os.path.join(GOLD, "mixup_acc_*.npz")))
BARY = sorted(glob.glob(os.path.join(GOLD, "mixup_bary_*.npz")))
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]
rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))
EPS = 1e-5


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    return _lib.lib()


def seeded_init_C(N, seed):
    """The reference's random start of its fp64 run (barycenter.py:303-306): N x 2 seeded fp32 normal draws, widened, then their squared
    distances in fp64 (clamped at 0, zero diagonal).  conan_fgw_amd.fgw forms the same matrix in fp32."""
    torch.manual_seed(seed)
    x = torch.randn(N, 2).double().numpy()
    c = -2.0 * (x @ x.T)
    c += (x * x).sum(1)[:, None]
    c += (x * x).sum(1)[None, :]
    return np.maximum(c, 0.0) * (1.0 - np.eye(N))


def bary_args(g):
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    K = len(sizes)
    Ys = [g["Ys"][s, :sizes[s]] for s in range(K)]
    Cs = [g["Cs"][s, :sizes[s], :sizes[s]] for s in range(K)]
    ps = [g["ps"][s, :sizes[s]] for s in range(K)] if "ps" in g else None
    kw = dict(alpha=float(g["alpha"]), rho=float(g["rho"]), max_iter=int(g["max_iter"]), tol=float(g["tol"]), loss_fun=str(g["loss_fun"]),
              fixed_structure=bool(g["fixed_structure"]), fixed_features=bool(g["fixed_features"]))
    init_C = Cs[0] if str(g["init"]) == "first" else seeded_init_C(N, int(g["seed"]))
    return N, Ys, Cs, ps, (g["p"] if "p" in g else None), (g["lambdas"] if "lambdas" in g else None), init_C, (g["init_Y"] if "init_Y" in g else None), kw


# ---------------------------------------------------------------------------------------------------------------------- the fixtures
def test_fixture_set_is_complete():
    """What the committed set must contain, by content, not by file name."""
    assert len(PAIRS) >= 6 and len(BARY) >= 10
    pairs = [np.load(p) for p in PAIRS]
    shapes = {tuple(g["M"].shape) for g in pairs}
    assert {(1, 5), (7, 12), (12, 7), (33, 33)} <= shapes
    assert any(g["M"].shape == (12, 7) and not np.array_equal(g["B"], g["B"].T) for g in pairs)
    assert any(g["M"].shape[0] == g["M"].shape[1] and g["M"].shape[0] > 79 for g in pairs)          # above the kernel's LDS limit
    assert any("X0" in g for g in pairs) and any("a" in g for g in pairs)
    assert any(int(g["r64_epochs"]) < int(g["epoch"]) for g in pairs) and any(int(g["r64_epochs"]) == int(g["epoch"]) for g in pairs)
    bary = [np.load(p) for p in BARY]
    mid = [g for g in bary if len({int(e) for e in g["r64_epochs"].ravel() if 21 < e < 100}) >= 2]
    assert mid, "no case whose couplings stop at different counts strictly between 21 and 100"
    assert any((g["r64_epochs"] == 100).all() for g in bary)
    assert any(str(g["loss_fun"]) == "kl_loss" for g in bary)
    assert any(bool(g["fixed_structure"]) for g in bary)
    assert any(bool(g["fixed_features"]) and "init_Y" in g for g in bary)
    assert any("ps" in g and "p" in g and "lambdas" in g for g in bary)
    assert any([int(n) for n in g["sizes"]] == [9, 6, 8] and int(g["N"]) == 7 for g in bary)
    assert any(str(g["init"]) == "random" for g in bary)
    assert any(not np.array_equal(g["Cs"], g["Cs"].transpose(0, 2, 1)) for g in bary)
    assert any(int(g["N"]) > 79 for g in bary)
    for p in PAIRS + BARY:
        assert os.path.getsize(p) < 512 * 1024, p


@pytest.mark.parametrize("path", PAIRS, ids=ids(PAIRS))
def test_pair_fixture_is_consistent_and_fair(path):
    g = np.load(path)
    n1, n2 = g["M"].shape
    assert g["M"].dtype == np.float32 and g["A"].shape == (n1, n1) and g["B"].shape == (n2, n2)
    for tag, dt in (("r32", np.float32), ("r64", np.float64)):
        X, objs, checks, ran = g[tag + "_X"], g[tag + "_objs"], g[tag + "_checks"], int(g[tag + "_epochs"])
        assert X.dtype == dt and X.shape == (n1, n2) and np.isfinite(X).all() and np.isfinite(checks).all()
        stopped = ran < int(g["epoch"])
        assert ran == (10 * len(checks) + 1 if stopped else int(g["epoch"])) and (not stopped or ran >= 21)
        assert len(objs) == len(checks) - (1 if stopped else 0) and np.array_equal(objs, checks[:len(objs)])
        if not stopped:
            assert len(checks) == (int(g["epoch"]) - 1) // 10
    a = g["a"].astype(np.float64) if "a" in g else np.full(n1, 1.0 / n1)
    b = g["b"].astype(np.float64) if "b" in g else np.full(n2, 1.0 / n2)
    np.testing.assert_allclose(g["r64_X"].sum(0), b, rtol=1e-12)                # the last half-step scales the columns: that marginal is exact,
    assert abs(g["r64_X"].sum() - a.sum()) <= 1e-6 and (g["r64_X"] >= 0).all()  # the rows' only as far as the descent has come
    c = g["r64_checks"]
    changes = [abs((c[k] - c[k - 1]) / c[k - 1]) for k in range(1, len(c))]
    assert fair(changes, float(g["eps"])), changes
    assert all(v >= float(g["eps"]) for v in changes[:-1])


@pytest.mark.parametrize("path", BARY, ids=ids(BARY))
def test_bary_fixture_is_consistent_and_fair(path):
    g = np.load(path)
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    K, d = len(sizes), g["Ys"].shape[2]
    for tag, dt in (("r32", np.float32), ("r64", np.float64)):
        outer = len(g[tag + "_err_feature"])
        assert g[tag + "_Y"].shape == (N, d) and g[tag + "_C"].shape == (N, N) and g[tag + "_T"].shape == (K, N, max(sizes))
        assert g[tag + "_Y"].dtype == dt and g[tag + "_epochs"].shape == (outer, K) and 1 <= outer <= int(g["max_iter"])
        assert all(np.isfinite(g[tag + "_" + k]).all() for k in ("Y", "C", "T", "err_feature", "err_structure"))
        assert ((g[tag + "_epochs"] >= 21) & (g[tag + "_epochs"] <= 100) & ((g[tag + "_epochs"] % 10 == 1) | (g[tag + "_epochs"] == 100))).all()
    p = g["p"].astype(np.float64) if "p" in g else np.full(N, 1.0 / N)
    for s, n in enumerate(sizes):
        q = g["ps"][s, :n].astype(np.float64) if "ps" in g else np.full(n, 1.0 / n)
        np.testing.assert_allclose(g["r64_T"][s, :, :n].sum(0), q, rtol=1e-12)
        assert abs(g["r64_T"][s].sum() - p.sum()) <= 1e-6 and (g["r64_T"][s] >= 0).all()
        assert not g["r64_T"][s, :, n:].any()
    assert fair(list(g["r64_rel"]), EPS)
    tol, outer = float(g["tol"]), len(g["r64_err_feature"])
    errs = [e for k, fixed in (("err_feature", g["fixed_features"]), ("err_structure", g["fixed_structure"])) if not fixed for e in g["r64_" + k]]
    assert fair(errs, tol)
    last = max(g["r64_err_feature"][-1], g["r64_err_structure"][-1])
    assert outer == int(g["max_iter"]) or last <= tol                          # the stop rule (barycenter.py:337)


# ---------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("path", PAIRS, ids=ids(PAIRS))
def test_restatement_reproduces_pair_fixture(path):
    g = np.load(path)
    X, lg = acc_ref(g["M"], g["A"], g["B"], g["a"] if "a" in g else None, g["b"] if "b" in g else None, g["X0"] if "X0" in g else None,
                    alpha=float(g["alpha"]), rho=float(g["rho"]), epoch=int(g["epoch"]), eps=float(g["eps"]))
    assert lg["epochs"] == int(g["r64_epochs"]) and len(lg["objs"]) == len(g["r64_objs"])
    np.testing.assert_allclose(lg["checks"], g["r64_checks"], rtol=1e-9)
    assert rel(X, g["r64_X"]) <= 1e-9


@pytest.mark.parametrize("path", BARY, ids=ids(BARY))
def test_restatement_reproduces_bary_fixture(path):
    g = np.load(path)
    N, Ys, Cs, ps, p, lam, init_C, init_Y, kw = bary_args(g)
    Y, C, lg = mixup_ref(N, Ys, Cs, ps, p, lam, init_C=init_C, init_Y=init_Y, **kw)
    assert len(lg["err_feature"]) == len(g["r64_err_feature"])
    assert np.array_equal(np.array(lg["epochs"]), g["r64_epochs"])
    assert rel(Y, g["r64_Y"]) <= 1e-9 and rel(C, g["r64_C"]) <= 1e-9
    for s, n in enumerate(g["sizes"]):
        assert rel(lg["T"][s], g["r64_T"][s, :, :n]) <= 1e-9


def _random_pair(seed, n1, n2, directed=True):
    rng = np.random.RandomState(seed)
    M = rng.uniform(0.0, 2.0, size=(n1, n2))
    A, B = (rng.random_sample((n1, n1)) < 0.4).astype(np.float64), (rng.random_sample((n2, n2)) < 0.4).astype(np.float64)
    if not directed:
        A, B = np.triu(A, 1) + np.triu(A, 1).T, np.triu(B, 1) + np.triu(B, 1).T
    return M, A, B


@pytest.mark.parametrize("n1,n2", [(7, 12), (12, 7), (1, 5), (9, 9)])
def test_massless_embedding_equals_rectangular_solve(n1, n2):
    M, A, B = _random_pair(n1 * 100 + n2, n1, n2)
    N = max(n1, n2) + 2
    Me, Ae, Be = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N))
    Me[:n1, :n2], Ae[:n1, :n1], Be[:n2, :n2] = M, A, B
    a, b = np.zeros(N), np.zeros(N)
    a[:n1], b[:n2] = 1.0 / n1, 1.0 / n2
    X, lg = acc_ref(M, A, B, alpha=0.5, rho=0.5, epoch=60)
    Xe, lge = acc_ref(Me, Ae, Be, a, b, alpha=0.5, rho=0.5, epoch=60)
    assert lge["epochs"] == lg["epochs"]
    np.testing.assert_allclose(Xe[:n1, :n2], X, rtol=1e-13)
    np.testing.assert_allclose(lge["checks"], lg["checks"], rtol=1e-12)
    Xe[:n1, :n2] = 0
    assert not Xe.any()


def test_transposed_B_is_told_apart():
    """B enters the gradient untransposed: the Bregman solve's product with C2^T would give another plan on a directed graph."""
    M, A, B = _random_pair(5, 12, 7)
    X, _ = acc_ref(M, A, B, alpha=0.5, rho=0.5, epoch=30)
    Xt, _ = acc_ref(M, A, B.T, alpha=0.5, rho=0.5, epoch=30)
    assert rel(Xt, X) > 1e-2
    M, A, B = _random_pair(5, 12, 7, directed=False)
    assert rel(acc_ref(M, A, B.T, alpha=0.5, rho=0.5, epoch=30)[0], acc_ref(M, A, B, alpha=0.5, rho=0.5, epoch=30)[0]) == 0.0


def test_earliest_stop_and_nan_objective():
    M, A, B = np.zeros((3, 3)) + 1.0, np.zeros((3, 3)), np.zeros((3, 3))
    X, lg = acc_ref(M, A, B, alpha=0.5, rho=1.0, epoch=200)                      # a fixed point from the start: still 21 epochs
    assert lg["epochs"] == 21 and len(lg["objs"]) == 1 and len(lg["checks"]) == 2
    X, lg = acc_ref(M * 1e6, A, B, np.array([0.5, 0.5, 0.0]), None, alpha=0.0, rho=1e-3, epoch=45)      # every exp underflows: NaN, never a stop
    assert np.isnan(X[:2]).all() and lg["epochs"] == 45 and len(lg["objs"]) == 4


# ---------------------------------------------------------------------------------------------------------------------- the C ABI
NEW = ("conan_fgw_acc_lds_resident", "conan_fgw_acc_pair_workspace_bytes", "conan_fgw_acc_pair_fwd", "conan_fgw_mixup_workspace_bytes",
       "conan_fgw_mixup_barycenter_fwd")


def test_new_symbols_are_declared_and_exported(L):
    from conan_fgw_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "conan_fgw_hip.h")).read()
    raw = ctypes.CDLL(_lib.library_path())
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header and hasattr(raw, name)
    assert L.conan_abi_version() == 6 == _lib.ABI_VERSION


def test_size_queries(L):
    assert L.conan_fgw_acc_lds_resident(33) == 1 and L.conan_fgw_acc_lds_resident(79) == 1
    assert L.conan_fgw_acc_lds_resident(80) == 0 and L.conan_fgw_acc_lds_resident(0) == 0 and L.conan_fgw_acc_lds_resident(-3) == 0
    for N in (1, 33, 79, 80, 200):
        sizes = [L.conan_fgw_acc_pair_workspace_bytes(B, N) for B in (1, 2, 7, 64)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]      # (rounded up to 256 bytes: N = 1 needs no more for B = 7)
        assert sizes[0] >= 24 * N * (N | 1)                                      # the three fp64 matrices of a streamed pair
        sizes = [L.conan_fgw_mixup_workspace_bytes(B, 3, N, 16) for B in (1, 2, 7, 64)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
        assert L.conan_fgw_mixup_workspace_bytes(2, 50, N, 16) > L.conan_fgw_mixup_workspace_bytes(2, 3, N, 16)
    for bad in ((0, 33), (-1, 33), (4, 0), (4, -2)):
        assert L.conan_fgw_acc_pair_workspace_bytes(*bad) == 0
    for bad in ((0, 3, 33, 8), (2, 0, 33, 8), (2, 3, 0, 8), (2, 3, 33, 0), (2, 3, -33, 8)):
        assert L.conan_fgw_mixup_workspace_bytes(*bad) == 0


def test_bad_arguments_return_minus_one_before_any_launch(L):
    from conan_fgw_amd._lib import FgwParams
    # null pointers: refused whatever else is passed (nothing is dereferenced, nothing launched)
    assert L.conan_fgw_acc_pair_fwd(None, None, None, None, None, None, 2, 9, 0.5, 1.0, 100, 1e-5, None, None, None, None, None) == -1
    prm = FgwParams(0.5, 0.0, 5, 1e-9, 0.0, 1, 0.0, 0, 0, 0, 0, 0)
    nul = (None,) * 7
    out = (None,) * 8
    assert L.conan_fgw_mixup_barycenter_fwd(*nul, 2, 3, 9, 4, ctypes.byref(prm), 1.0, 100, 1e-5, *out) == -1
    assert L.conan_fgw_mixup_barycenter_fwd(*nul, 2, 3, 9, 4, None, 1.0, 100, 1e-5, *out) == -1
    # the checks on values come before any launch too: host buffers stand in for device memory, and must never be touched
    buf = (ctypes.c_float * 4096)()
    keep = bytes(buf)
    P = ctypes.cast(buf, ctypes.c_void_p)
    pair = lambda B, N, rho, epoch, eps=1e-5, alpha=0.5: L.conan_fgw_acc_pair_fwd(P, P, P, None, None, None, B, N, alpha, rho, epoch, eps, P, P, P, P, None)
    for args in ((0, 9, 1.0, 100), (2, 0, 1.0, 100), (-1, 9, 1.0, 100), (2, 9, 0.0, 100), (2, 9, -1.0, 100), (2, 9, float("inf"), 100),
                 (2, 9, float("nan"), 100), (2, 9, 1.0, 0), (2, 9, 1.0, -5), (2, 9, 1.0, 100, float("nan"))):
        assert pair(*args) == -1, args

    def bary(B=2, K=3, N=9, d=4, rho=1.0, epoch=100, eps=1e-5, init_Y=None, **f):
        fields = dict(alpha=0.5, epsilon=0.0, max_iter=5, tol=1e-9, inner_tol=0.0, num_iter_max=1, stop_thr=0.0, fixed_structure=0, fixed_features=0,
                      warmstart=0, loss_fun=0, cs_small_int=0)
        fields.update(f)
        pr = FgwParams(*[fields[n] for n, _ in FgwParams._fields_])
        return L.conan_fgw_mixup_barycenter_fwd(P, P, None, None, None, None, init_Y, B, K, N, d, ctypes.byref(pr), rho, epoch, eps, P, P, P, None, P, P, P, None)
    for kw in (dict(B=0), dict(K=0), dict(N=-1), dict(d=0), dict(rho=0.0), dict(rho=-2.0), dict(rho=float("inf")), dict(rho=float("nan")),
               dict(epoch=0), dict(eps=float("nan")), dict(max_iter=0), dict(fixed_features=1), dict(loss_fun=2)):
        assert bary(**kw) == -1, kw
    assert bytes(buf) == keep


def test_old_entry_points_still_refuse_solver_code_3(L):
    from conan_fgw_amd._lib import FgwParams
    for sym in (1, 0, -1):
        assert L.conan_fgw_workspace_bytes(4, 3, 33, 8, 0, 3, sym) == 0
        assert L.conan_fgw_workspace_bytes(4, 3, 33, 8, 1, 3, sym) == 0
    prm = FgwParams(0.5, 0.1, 5, 1e-9, 1e-4, 5, 1e-2, 0, 0, 0, 0, 0)
    buf = (ctypes.c_float * 16)()
    P = ctypes.cast(buf, ctypes.c_void_p)
    common = (None, None, None, None, None, 1, 1, 2, 2, ctypes.byref(prm), 3, 1, P, P, P, None, P, P, P, None)
    assert L.conan_fgw_barycenter_fwd(P, P, *common) == -1
    assert L.conan_fgw_barycenter_fwd_ragged(P, P, P, P, P, *common) == -1


# ---------------------------------------------------------------------------------------------------------------------- the public functions
def test_public_functions_refuse_cpu_tensors_and_unknown_loss():
    from conan_fgw_amd import fgw, ops
    Ys, Cs = [torch.rand(5, 3) for _ in range(2)], [torch.rand(5, 5) for _ in range(2)]
    with pytest.raises(ValueError, match="Unknown `loss_fun='l1'`"):
        fgw.fgw_barycenters_BAPG(5, Ys, Cs, loss_fun="l1")
    with pytest.raises(ValueError, match="If C is fixed it must be initialized"):
        fgw.fgw_barycenters_BAPG(5, Ys, Cs, fixed_structure=True)
    with pytest.raises(ValueError, match="If Y is fixed it must be initialized"):
        fgw.fgw_barycenters_BAPG(5, Ys, Cs, fixed_features=True)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        fgw.fgw_barycenters_BAPG(5, Ys, Cs)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        fgw.fused_ACC_torch(torch.rand(5, 4), torch.rand(5, 5), torch.rand(4, 4), alpha=0.5)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.fgw_acc_pair_batched(torch.rand(1, 5, 4), torch.rand(1, 5, 5), torch.rand(1, 4, 4), alpha=0.5, rho=1.0)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.fgw_mixup_barycenter_batched(torch.rand(1, 2, 5, 3), torch.rand(1, 2, 5, 5))
    with pytest.raises(ValueError, match="Unknown `loss_fun="):
        ops.fgw_mixup_barycenter_batched(torch.rand(1, 2, 5, 3), torch.rand(1, 2, 5, 5), loss_fun="l1")
    with pytest.raises(ValueError, match="rho must be positive"):
        ops.fgw_acc_pair_batched(torch.rand(1, 5, 4), torch.rand(1, 5, 5), torch.rand(1, 4, 4), alpha=0.5, rho=0.0)
