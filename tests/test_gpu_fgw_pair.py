"""The pairwise entropic FGW solve on the GPU — ops.fgw_pair_batched / fgw_pair_list / fgw_pair_dist, fgw / fgw_projected / fgw_bregman and
fgw_pairwise_distances — against the reference's own fgw() in fp32 ("r32") and fp64 ("r64") (tests/golden/fgw_pair_*.npz, written by
make_fgw_pair_golden.py).  Yardsticks, the project's standing ones: iteration and Sinkhorn counts of r64 exactly; errs within rtol 2e-3 /
atol 1e-6 of r64's, NaN beyond; T within 1e-4 of r32 or no further from r64 than r32 is (_check_matrices of test_gpu_fgw_sym.py); fgw_dist
within 1e-4 of r64 (test_gpu_fgw.py).  Further: the stand-alone distance kernel against the fp64 oracle, batching / list form / repeated
calls bit for bit, symmetric=None, G0, the barycenter path on the same couplings, the all-pairs matrix, and the BADARG table."""
import ctypes
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

from helpers import golden_files, rel
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops
from conan_fgw_amd._lib import FgwParams, lib
from conan_fgw_amd.synthetic import make_batch
from oracle import fgw as ofgw

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
ALL = golden_files("fgw_pair_")
ids = lambda ps: [os.path.basename(p)[9:-4] for p in ps]
SQUARE = [p for p in ALL if "_kl_" not in p]
KL = [p for p in ALL if "_kl_" in p]
SYM = {1: True, 0: False, -1: None}
by_name = lambda name: next(p for p in ALL if os.path.basename(p) == f"fgw_pair_{name}.npz")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _inputs(g):
    G0 = t(g["G0"]) if g["G0"].size else None
    return t(g["M"]), t(g["C1"]), t(g["C2"]), t(g["p"]), t(g["q"]), G0


def _kw(g):
    return dict(alpha=float(g["alpha"]), epsilon=float(g["epsilon"]), max_iter=int(g["max_iter"]), tol=float(g["tol"]),
                num_iter_max=int(g["num_iter_max"]), stop_thr=float(g["stop_thr"]), loss_fun=str(g["loss_fun"]), solver=str(g["solver"]),
                symmetric=SYM[int(g["symmetric"])])


def _batched(g, **over):
    M, C1, C2, p, q, G0 = _inputs(g)
    kw = _kw(g); kw.update(over)
    return ops.fgw_pair_batched(M[None], C1[None], C2[None], p[None], q[None], None if G0 is None else G0[None], **kw)


def _check(g, T, dist, it, sk, errs):
    n1, n2 = g["M"].shape
    assert tuple(T.shape) == (n1, n2)
    print(f"it {it}/{int(g['r64_it'])} sk {sk}/{int(g['r64_sk'])} T: e32 {rel(T, g['r32_T']):.2e} e64 {rel(T, g['r64_T']):.2e} "
          f"yard {rel(g['r32_T'], g['r64_T']):.2e} dist {abs(dist - float(g['r64_fgw_dist'])) / abs(float(g['r64_fgw_dist'])):.2e}")
    assert (it, sk) == (int(g["r64_it"]), int(g["r64_sk"]))
    k = math.ceil(it / 10)
    np.testing.assert_allclose(errs[:k], g["r64_err"], rtol=2e-3, atol=1e-6)
    assert np.isnan(errs[k:]).all() and len(errs) >= k
    yard = rel(g["r32_T"], g["r64_T"])
    e32, e64 = rel(T, g["r32_T"]), rel(T, g["r64_T"])
    assert e32 <= 1e-4 or e64 <= yard, (e32, e64, yard)
    assert abs(dist - float(g["r64_fgw_dist"])) <= 1e-4 * abs(float(g["r64_fgw_dist"]))


def _same(a_out, b_out):
    """Bit for bit, NaN included (errs is NaN where not run)."""
    for a, b, name in zip(a_out, b_out, ("T", "fgw_dist", "info", "errs")):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name


@pytest.mark.parametrize("path", ALL, ids=ids(ALL))
def test_golden_through_fgw_pair_batched(path):
    g = np.load(path)
    T, dist, info, errs = _batched(g)
    assert errs.shape == (1, math.ceil(int(g["max_iter"]) / 10)) and info.shape == (1, 4) and dist.shape == (1,)
    assert int(info[0, 2]) == 0                                         # no zero row / column sum at a node with mass
    _check(g, T[0].cpu().numpy(), float(dist[0]), int(info[0, 0]), int(info[0, 1]), errs[0].cpu().numpy())
    _same((T, dist, info, errs), _batched(g))                            # the same call again


@pytest.mark.parametrize("path", ALL, ids=ids(ALL))
def test_golden_through_fgw(path):
    g = np.load(path)
    M, C1, C2, p, q, G0 = _inputs(g)
    kw = _kw(g)
    sink = dict(numItermax=kw.pop("num_iter_max"), stopThr=kw.pop("stop_thr"))
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="Solver failed")        # the reference's warning is for a failed plan: none here
        T, log = pfgw.fgw(M, C1, C2, p, q, G0=G0, log=True, **kw, **(sink if kw["solver"] != "BAPG" else {}))
        T_only = pfgw.fgw(M, C1, C2, p, q, G0=G0, **kw, **(sink if kw["solver"] != "BAPG" else {}))
    assert torch.equal(T, T_only) and not T.requires_grad
    assert log["fgw_dist"].dim() == 0 and isinstance(log["n_iter"], int) and isinstance(log["n_sinkhorn"], int)
    assert len(log["err"]) == math.ceil(log["n_iter"] / 10) and all(e.dim() == 0 for e in log["err"])
    errs = np.array([float(e) for e in log["err"]])
    _check(g, T.cpu().numpy(), float(log["fgw_dist"]), log["n_iter"], log["n_sinkhorn"], errs)
    _same((T[None], log["fgw_dist"][None]), _batched(g)[:2])


def test_fgw_projected_and_fgw_bregman_directly():
    g = np.load(by_name("ppa_n10"))
    M, C1, C2, p, q, _ = _inputs(g)
    T, log = pfgw.fgw_projected(M, C1, C2, p, q, epsilon=0.1, symmetric=True, solver="PPA", log=True)      # defaults: the fixture's parameters
    _check(g, T.cpu().numpy(), float(log["fgw_dist"]), log["n_iter"], log["n_sinkhorn"], np.array([float(e) for e in log["err"]]))
    g = np.load(by_name("bapg_n12"))
    M, C1, C2, p, q, _ = _inputs(g)
    T, log = pfgw.fgw_bregman(M, C1, C2, p, q, epsilon=1.0, symmetric=True, max_iter=100, tol=1e-5, log=True)
    _check(g, T.cpu().numpy(), float(log["fgw_dist"]), log["n_iter"], 0, np.array([float(e) for e in log["err"]]))
    assert log["n_sinkhorn"] == 0


def test_failed_plan_warns_like_the_reference():
    g = np.load(by_name("pgd_n10"))
    M, C1, C2, p, q, _ = _inputs(g)
    with pytest.warns(UserWarning, match="Solver failed to produce a transport plan"):
        pfgw.fgw(M, C1, C2, p * 0.5, q * 0.5, symmetric=True)            # marginals of mass 1/2: sum(T) = 1/2
    with pytest.warns(UserWarning, match="Solver failed to produce a transport plan"):
        T = pfgw.fgw(M * 1e4, C1, C2, p, q, solver="BAPG", epsilon=1e-3, symmetric=True, max_iter=10)      # exp(-1e7) underflows: a zero row sum
    assert torch.isnan(T).any()
    assert int(ops.fgw_pair_batched(M[None] * 1e4, C1[None], C2[None], p[None], q[None], solver="BAPG", epsilon=1e-3, max_iter=10)[2][0, 2]) == 4


@pytest.mark.parametrize("path", SQUARE, ids=ids(SQUARE))
def test_pair_dist_alone_against_the_oracle(path):
    """conan_fgw_pair_dist on the fixture's r32 plan and on a random positive matrix that is no solver output, against the fp64 oracle formula."""
    g = np.load(path)
    n1, n2 = g["M"].shape
    N = max(n1, n2)
    rng = np.random.RandomState(3)
    rand = rng.uniform(0.1, 1.0, size=(n1, n2)); rand /= rand.sum()
    pad = lambda a, *shape: np.pad(np.asarray(a, np.float32), [(0, s - k) for s, k in zip(shape, np.shape(a))])
    for plan in (g["r32_T"], rand.astype(np.float32)):
        out = ops.fgw_pair_dist(t(pad(g["M"], N, N))[None], t(pad(g["C1"], N, N))[None], t(pad(g["C2"], N, N))[None], t(pad(plan, N, N))[None],
                                t(pad(g["p"], N))[None], t(pad(g["q"], N))[None], alpha=float(g["alpha"]))
        want = ofgw.fgw_dist(g["M"], g["C1"], g["C2"], plan, float(g["alpha"]), g["p"], g["q"], np.float64)
        print(f"pair_dist {float(out[0]):.9g} oracle {want:.9g}")
        assert abs(float(out[0]) - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize("path", KL, ids=ids(KL))
def test_pair_dist_alone_kl(path):
    g = np.load(path)
    M, C1, C2, p, q, _ = _inputs(g)
    out = ops.fgw_pair_dist(M[None], C1[None], C2[None], t(g["r64_T"])[None], p[None], q[None], alpha=float(g["alpha"]), loss_fun="kl_loss")
    assert abs(float(out[0]) - float(g["r64_fgw_dist"])) <= 1e-4 * abs(float(g["r64_fgw_dist"]))


def test_pair_dist_is_what_the_solve_returns():
    g = np.load(by_name("pgd_dir_n12_false"))                            # after an asymmetric solve too: the problem itself, not its transpose
    T, dist, _, _ = _batched(g)
    M, C1, C2, p, q, _ = _inputs(g)
    again = ops.fgw_pair_dist(M[None], C1[None], C2[None], T, p[None], q[None], alpha=float(g["alpha"]))
    assert torch.equal(again, dist)
    assert _batched(g, with_dist=False)[1] is None


def test_batch_of_three_is_the_three_single_calls():
    gs = [np.load(by_name(n)) for n in ("pgd_n10", "pgd_n10_g0", "pgd_n10_cap25")]
    kw = _kw(gs[2])                                                      # one parameter set for the batch: max_iter 25, tol 1e-12
    ins = [_inputs(g) for g in gs]
    G0 = torch.stack([i[5] if i[5] is not None else torch.outer(i[3], i[4]) for i in ins])
    stack = lambda k: torch.stack([i[k] for i in ins])
    batch = ops.fgw_pair_batched(stack(0), stack(1), stack(2), stack(3), stack(4), G0, **kw)
    assert batch[0].shape == (3, 10, 10) and batch[1].shape == (3,) and batch[2].shape == (3, 4) and batch[3].shape == (3, 3)
    for b, i in enumerate(ins):
        single = ops.fgw_pair_batched(i[0][None], i[1][None], i[2][None], i[3][None], i[4][None], G0[b][None], **kw)
        _same(tuple(o[b:b + 1] for o in batch), single)
    assert not torch.equal(batch[0][0], batch[0][1])
    _same(batch, ops.fgw_pair_batched(stack(0), stack(1), stack(2), stack(3), stack(4), G0, **kw))
    # non-contiguous inputs (transposed storage, strided batch) are accepted and give the same bits
    nc = lambda x: x.transpose(-1, -2).contiguous().transpose(-1, -2) if x.dim() == 3 else torch.stack([x, x], 1)[:, 0]
    assert not nc(stack(0)).is_contiguous() and not nc(stack(3)).is_contiguous()
    _same(batch, ops.fgw_pair_batched(nc(stack(0)), nc(stack(1)), nc(stack(2)), nc(stack(3)), nc(stack(4)), nc(G0), **kw))


def test_ragged_list_is_the_per_pair_calls():
    """Pairs of 7 x 12, 12 x 12 and 1 x 12 nodes in one launch (embedded in Np = 12) against one call per pair."""
    g7, g12 = np.load(by_name("pgd_rect_7x12")), np.load(by_name("pgd_undir_n12_none"))
    a, b = _inputs(g7), _inputs(g12)
    one = (a[0][:1], a[1][:1, :1], a[2], torch.ones(1, device=dev), a[4], None)
    pairs = [a, b, one]
    kw = _kw(g7)
    Ts, dist, info, errs = ops.fgw_pair_list([x[0] for x in pairs], [x[1] for x in pairs], [x[2] for x in pairs], [x[3] for x in pairs],
                                             [x[4] for x in pairs], **kw)
    assert [tuple(T.shape) for T in Ts] == [(7, 12), (12, 12), (1, 12)]
    for k, x in enumerate(pairs):
        single = ops.fgw_pair_batched(x[0][None], x[1][None], x[2][None], x[3][None], x[4][None], **kw)
        _same((Ts[k][None], dist[k:k + 1], info[k:k + 1], errs[k:k + 1]), single)
    _check(g7, Ts[0].cpu().numpy(), float(dist[0]), int(info[0, 0]), int(info[0, 1]), errs[0].cpu().numpy())
    assert torch.allclose(Ts[2][0], a[4], rtol=1e-6, atol=0)             # one source node: the plan is q
    # a pair smaller than the common size runs with massless nodes, i.e. on the log-domain Sinkhorn: the same plan to rounding
    g10 = np.load(by_name("pgd_n10"))
    c = _inputs(g10)
    Ts2, dist2, info2, errs2 = ops.fgw_pair_list([c[0], b[0]], [c[1], b[1]], [c[2], b[2]], [c[3], b[3]], [c[4], b[4]], **_kw(g10))
    _check(g10, Ts2[0].cpu().numpy(), float(dist2[0]), int(info2[0, 0]), int(info2[0, 1]), errs2[0].cpu().numpy())


def test_symmetric_none_is_decided_in_the_kernel():
    gd, gu = np.load(by_name("pgd_dir_n12_none")), np.load(by_name("pgd_undir_n12_none"))
    for g, decided in ((gd, False), (gu, True)):
        none, fixed = _batched(g, symmetric=None), _batched(g, symmetric=decided)
        _same(none, fixed)
        assert int(none[2][0, 3]) == int(decided) and int(_batched(g, symmetric=not decided)[2][0, 3]) == int(not decided)
    assert not torch.equal(_batched(gd, symmetric=True)[0], _batched(gd, symmetric=False)[0])
    for solver, eps in (("PPA", 0.1), ("BAPG", 1.0)):
        _same(_batched(gd, symmetric=None, solver=solver, epsilon=eps, max_iter=20), _batched(gd, symmetric=False, solver=solver, epsilon=eps, max_iter=20))
        _same(_batched(gu, symmetric=None, solver=solver, epsilon=eps, max_iter=20), _batched(gu, symmetric=True, solver=solver, epsilon=eps, max_iter=20))


@pytest.mark.parametrize("name", ["pgd_n10", "ppa_n10", "bapg_n12", "pgd_n80", "bapg_n140"])
def test_explicit_product_start_is_the_default_start(name):
    g = np.load(by_name(name))
    M, C1, C2, p, q, _ = _inputs(g)
    kw = _kw(g); kw["max_iter"] = min(kw["max_iter"], 20)
    G0 = (p.double()[:, None] * q.double()[None, :]).float()             # the kernels form p q^T in fp64 and round once
    _same(ops.fgw_pair_batched(M[None], C1[None], C2[None], p[None], q[None], G0[None], **kw),
          ops.fgw_pair_batched(M[None], C1[None], C2[None], p[None], q[None], None, **kw))


def _structure(rng, n, dens):
    a = np.triu(rng.random_sample((n, n)) < dens, 1)
    return (a | a.T).astype(np.float32)


def _same_couplings(N, solver, symmetric, eps, m):
    rng = np.random.RandomState(100 + N)
    d = 4
    Y0, Z = t(rng.uniform(0.1, 1.0, size=(N, d))), t(rng.uniform(0.1, 1.0, size=(N, d)))
    C1, C2 = t(_structure(rng, N, 0.3)), t(_structure(rng, N, 0.3))
    _, _, log = pfgw.fgw_barycenters(N, [Z], [C2], init_C=C1, init_Y=Y0, fixed_structure=True, fixed_features=True, max_iter=m, log=True,
                                     solver=solver, symmetric=symmetric, alpha=0.5, epsilon=eps, tol=1e-9)
    T_b = log["Ts_iter"][0][0]
    n_b = log["n_pgd"] // log["n_outer"]                                 # (fixed / fixed: every outer iteration repeats the same solve)
    T, plog = pfgw.fgw(pfgw.feature_cost(Y0, Z), C1, C2, max_iter=m, tol=1e-4, solver=solver, symmetric=symmetric, alpha=0.5, epsilon=eps, log=True)
    print(f"N {N} {solver}: iterations {plog['n_iter']} / {n_b}, rel {rel(T.cpu().numpy(), T_b.cpu().numpy()):.2e}")
    assert plog["n_iter"] == n_b
    assert rel(T.cpu().numpy(), T_b.cpu().numpy()) <= 1e-4


@pytest.mark.parametrize("solver,symmetric,eps", [("PGD", True, 0.1), ("PPA", True, 0.1), ("BAPG", True, 1.0), ("PGD", False, 0.1)])
@pytest.mark.parametrize("N", [12, 33, 80])
def test_same_couplings_as_the_barycenter_path(N, solver, symmetric, eps):
    """One input graph, structure and features of the barycenter held fixed: the first outer iteration of fgw_barycenters IS one coupling solve
    with M = dist(Y0, Z), max_iter = m and tol = 1e-4.  At N <= 64 the PGD / symmetric barycenter runs the register-resident kernels.
    m = 12 puts a second check of ||T - Tprev|| (iteration 10) inside the solve.  Not at N = 80 with PGD / symmetric: there the barycenter runs
    k_fgw_coupling_big, which forms the error against Tprev only at iteration 0 (its later checks compare with zero, so it never stops early
    after the first: built for the models' max_iter = 5, DESIGN.md 3.3 "Pair form") — on this problem the reference's own fp64 run stops at 11
    iterations (error 6.9e-10 at the second check) and so does the pair form, the big kernel runs all 12.  The two paths are the same loop up to
    the first ten iterations, so that case is compared at m = 10."""
    _same_couplings(N, solver, symmetric, eps, 10 if N > 64 and solver == "PGD" and symmetric else 12)


def _smallest_n_with_no_matrix_in_lds():
    """The smallest N at which general_mode (fgw_common.h) returns 0: the vectors, (6 + 2 GEN_NW) N + 16 doubles, and one N x (N | 1) fp64
    matrix pass LDS_LIMIT.  The two constants are read from the header; the lines of the rule are demanded as they stand, so that a change
    of the rule fails here instead of leaving mode 0 untested."""
    with open(os.path.join(os.path.dirname(pfgw.__file__), "csrc", "fgw_common.h")) as f:
        src = f.read()
    nw = int(re.search(r"constexpr int GEN_NW = (\d+);", src).group(1))
    limit = int(re.search(r"constexpr size_t LDS_LIMIT = (\d+) \* 1024;", src).group(1)) * 1024
    for line in ("int fgw_pitch(int N) { return N | 1; }", "vec_c = (size_t)((6 + 2 * GEN_NW) * N + 16) * 8, mr_bytes = (size_t)N * pitch_of(N) * 8;",
                 "mode = lc <= LDS_LIMIT ? 2 : (vec_c + mr_bytes <= LDS_LIMIT ? 1 : 0);"):
        assert line in src, line
    return next(N for N in range(2, 1024) if ((6 + 2 * nw) * N + 16) * 8 + N * (N | 1) * 8 > limit)


@pytest.mark.parametrize("solver,symmetric", [("PPA", True), ("PGD", False)], ids=["ppa", "pgd_asym"])
def test_same_couplings_with_every_matrix_in_the_global_scratch(solver, symmetric):
    """At the smallest size at which the general coupling kernel keeps no matrix in LDS (133 with 8 wavefronts and 160 KiB), in the barycenter
    form and in the pair form: PPA and symmetric=False take that kernel in both (the goldens of the pair form at N = 140 pin PGD / symmetric
    there against the reference)."""
    _same_couplings(_smallest_n_with_no_matrix_in_lds(), solver, symmetric, 0.1, 10)


def _conformers(G=6, n=14, moved=None):
    """G conformers of one synthetic molecule: E(3)-invariant node features (atomic number, the three nearest-neighbour distances), 0/1 contact
    structure.  moved = (index, rotation, shift): that conformer is moved rigidly before its features are formed."""
    cb = make_batch("esol", num_molecules=1, num_conformers=G, seed=5, fixed_atoms=n)
    # contact threshold: the middle of the widest gap between the ensemble's distances in 2 .. 3 A, so that no contact flips under rounding
    every = np.sort(np.concatenate([np.linalg.norm(cb.pos[k * n:(k + 1) * n, None] - cb.pos[None, k * n:(k + 1) * n], axis=-1).ravel() for k in range(G)]))
    every = every[(every > 2.0) & (every < 3.0)]
    gap = int(np.argmax(np.diff(every)))
    cut = 0.5 * float(every[gap] + every[gap + 1])
    assert every[gap + 1] - every[gap] > 1e-3
    Ys, Cs = [], []
    for k in range(G):
        pos = cb.pos[k * n:(k + 1) * n].astype(np.float64)
        if moved is not None and moved[0] == k:
            pos = (pos @ moved[1].T + moved[2]).astype(np.float32).astype(np.float64)      # positions are stored fp32
        dm = np.linalg.norm(pos[:, None] - pos[None, :], axis=-1)
        near = np.sort(dm + np.eye(n) * 1e9, axis=1)[:, :3]
        Ys.append(t(np.concatenate([cb.z[:n, None] / 10.0, near], axis=1)))
        Cs.append(t(((dm < cut) & ~np.eye(n, dtype=bool))))
    return Ys, Cs


def test_pairwise_distances_of_a_conformer_ensemble():
    kw = dict(alpha=0.5, epsilon=0.1, max_iter=30, tol=1e-5)
    Ys, Cs = _conformers()
    D = pfgw.fgw_pairwise_distances(Ys, Cs, **kw)
    assert D.shape == (6, 6) and torch.equal(D, D.T) and torch.equal(D.diagonal(), torch.zeros(6, device=dev))
    assert (D[~torch.eye(6, dtype=torch.bool, device=dev)] > 0).all() and torch.isfinite(D).all()
    for a, b in ((0, 1), (2, 5), (3, 4)):
        _, log = pfgw.fgw(pfgw.feature_cost(Ys[a], Ys[b]), Cs[a], Cs[b], log=True, **kw)
        assert torch.equal(log["fgw_dist"], D[a, b])
    assert torch.equal(D, pfgw.fgw_pairwise_distances(Ys, Cs, **kw))
    c, s = math.cos(0.7), math.sin(0.7)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    Ym, Cm = _conformers(moved=(2, R, np.array([3.0, -1.0, 2.0])))
    assert all(torch.equal(x, y) for x, y in zip(Cs, Cm))
    Dm = pfgw.fgw_pairwise_distances(Ym, Cm, **kw)
    print("rigid motion:", float((Dm - D).abs().max() / D.max()))
    assert torch.allclose(Dm, D, rtol=2e-4, atol=0)
    # conformer sets of different sizes go through the list form
    D3 = pfgw.fgw_pairwise_distances([Ys[0], Ys[1][:9], Ys[2]], [Cs[0], Cs[1][:9, :9], Cs[2]], **kw)
    assert torch.equal(D3, D3.T) and torch.isfinite(D3).all() and abs(float(D3[0, 2]) - float(D[0, 2])) <= 1e-4 * float(D[0, 2])


def test_bad_arguments_are_refused_before_any_launch():
    L = lib()
    N, B = 6, 2
    f = lambda *s: torch.rand(*s, device=dev)
    M, C1, C2, T, errs = f(B, N, N), f(B, N, N), f(B, N, N), torch.full((B, N, N), -7.0, device=dev), torch.full((B, 10), -7.0, device=dev)
    info = torch.full((B, 4), -7, dtype=torch.int32, device=dev)
    dist = torch.full((B,), -7.0, device=dev)
    ws = torch.empty(int(L.conan_fgw_pair_workspace_bytes(B, N, 2, 0)), dtype=torch.uint8, device=dev)
    good = dict(M=M, C1=C1, C2=C2, T=T, info=info, errs=errs, ws=ws, B=B, N=N, max_iter=100, solver=0, symmetric=1, loss=0)

    def fwd(**over):
        a = dict(good); a.update(over)
        prm = FgwParams(0.5, 0.1, a["max_iter"], 1e-5, 1e-5, 100, 1e-5, 0, 0, 0, a["loss"], 0)
        P = lambda x: None if x is None else x.data_ptr()
        return L.conan_fgw_pair_fwd(P(a["M"]), P(a["C1"]), P(a["C2"]), None, None, None, a["B"], a["N"], ctypes.byref(prm) if a.get("prm", 1) else None,
                                    a["solver"], a["symmetric"], P(a["T"]), dist.data_ptr(), P(a["info"]), P(a["errs"]), P(a["ws"]), None)

    table = [dict(M=None), dict(C1=None), dict(C2=None), dict(T=None), dict(info=None), dict(errs=None), dict(ws=None), dict(prm=0), dict(B=0),
             dict(N=0), dict(max_iter=0), dict(solver=3), dict(solver=-1), dict(symmetric=2), dict(symmetric=-2), dict(loss=2)]
    for bad in table:
        assert fwd(**bad) == -1, bad
    P = lambda x: None if x is None else x.data_ptr()
    for bad in (dict(M=None), dict(C1=None), dict(C2=None), dict(T=None), dict(out=None), dict(B=0), dict(N=0), dict(loss=2)):
        a = dict(M=M, C1=C1, C2=C2, T=T, out=dist, B=B, N=N, loss=0); a.update(bad)
        assert L.conan_fgw_pair_dist(P(a["M"]), P(a["C1"]), P(a["C2"]), None, None, P(a["T"]), a["B"], a["N"], 0.5, a["loss"], P(a["out"]), None) == -1, bad
    torch.cuda.synchronize()
    # nothing ran: every output still holds its fill
    assert (T == -7).all() and (errs == -7).all() and (info == -7).all() and (dist == -7).all()
    assert fwd() == 0
    torch.cuda.synchronize()
    assert (info[:, 0] > 0).all() and torch.isfinite(dist).all()
