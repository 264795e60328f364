"""The backward of the pair distance on the GPU — conan_fgw_pair_dist_bwd, ops.fgw_pair_distance / fgw_pair_distance_list / fgw_pair_dist,
fgw_distance and fgw_pairwise_distances — against the reference's autograd of init_matrix / gwloss at a fixed plan (tests/golden/fgw_distgrad_*.npz,
make_fgw_pair_grad_golden.py; inputs and plans in the fgw_pair_ fixture of the same name) and, where there is no fixture, against the fp64 torch
expression of fgw_pair_grad_ref.py, which test_fgw_pair_grad_cpu.py pins to the same fixtures.  Yardsticks: a kernel fed the oracle's plan within
1e-5 (norm-wise) of r64, the bound of test_gpu_fgw_grad.py; quantities that depend on the fp32 solve within max(1e-4, the reference's own fp32
run) of r64, the project's standing one.  The gradient is the one at the solve's plan held constant, so no finite difference checks it."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from fgw_pair_grad_ref import fgw_dist_grads
from helpers import GOLDEN, golden_files, rel
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops
from conan_fgw_amd._lib import call, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GRADS = golden_files("fgw_distgrad_")
ids = lambda ps: [os.path.basename(p)[len("fgw_distgrad_"):-4] for p in ps]
NAMES = ("dM", "dC1", "dC2", "dp", "dq")
SYM = {1: True, 0: False, -1: None}
LOSS = {"square_loss": 0, "kl_loss": 1}
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
pair = lambda name: np.load(os.path.join(GOLDEN, f"fgw_pair_{name}.npz"))
pair_of = lambda path: np.load(os.path.join(GOLDEN, "fgw_pair_" + os.path.basename(path)[len("fgw_distgrad_"):]))
bits = lambda x: x.contiguous().view(torch.int32)


def _fgw_kw(f):
    kw = dict(alpha=float(f["alpha"]), epsilon=float(f["epsilon"]), max_iter=int(f["max_iter"]), tol=float(f["tol"]), loss_fun=str(f["loss_fun"]),
              solver=str(f["solver"]), symmetric=SYM[int(f["symmetric"])])
    if kw["solver"] != "BAPG":
        kw.update(numItermax=int(f["num_iter_max"]), stopThr=float(f["stop_thr"]))
    return kw


def _ops_kw(f):
    return dict(alpha=float(f["alpha"]), epsilon=float(f["epsilon"]), max_iter=int(f["max_iter"]), tol=float(f["tol"]), num_iter_max=int(f["num_iter_max"]),
                stop_thr=float(f["stop_thr"]), loss_fun=str(f["loss_fun"]), solver=str(f["solver"]), symmetric=SYM[int(f["symmetric"])])


def _square(f, plan):
    """The fixture's pair embedded in N = max(n1, n2) with massless nodes, as ops.fgw_pair_batched passes it to the library, B = 1."""
    n1, n2 = f["M"].shape
    N = max(n1, n2)
    pad = lambda a, *shape: t(np.pad(np.asarray(a, np.float32), [(0, s - k) for s, k in zip(shape, np.shape(a))]))[None]
    return pad(f["C1"], N, N), pad(f["C2"], N, N), pad(f["p"], N), pad(f["q"], N), pad(plan, N, N)


def _bwd(C1, C2, p, q, T, gout, alpha, loss_fun="square_loss", want=NAMES):
    """conan_fgw_pair_dist_bwd called directly.  The five outputs are consecutive slices of ONE buffer filled with NaN, so that a write outside a wanted
    output lands in a neighbour and shows; an unwanted output is passed as NULL -> {name: tensor} over all five."""
    B, N, _ = T.shape
    sizes = [B * N * N] * 3 + [B * N] * 2
    flat = torch.full((sum(sizes),), float("nan"), device=dev)
    out = {k: v.view(B, *([N] * d)) for k, v, d in zip(NAMES, flat.split(sizes), (2, 2, 2, 1, 1))}
    ptr = lambda x: None if x is None else x.data_ptr()
    call("conan_fgw_pair_dist_bwd", ptr(C1), ptr(C2), ptr(p), ptr(q), ptr(T), ptr(gout), B, N, float(alpha), LOSS[loss_fun],
         *(out[k].data_ptr() if k in want else None for k in NAMES), stream_ptr())
    torch.cuda.synchronize()
    return out


def _kernel_alone(path):
    f = pair_of(path)
    C1, C2, p, q, T = _square(f, f["r64_T"])
    return f, _bwd(C1, C2, p, q, T, torch.ones(1, device=dev), float(f["alpha"]), str(f["loss_fun"]))


def _block(f, k, x):
    n1, n2 = f["M"].shape
    return x[{"dM": (slice(n1), slice(n2)), "dC1": (slice(n1), slice(n1)), "dC2": (slice(n2), slice(n2)), "dp": (slice(n1),), "dq": (slice(n2),)}[k]]


@pytest.mark.parametrize("path", GRADS, ids=ids(GRADS))
def test_kernel_alone_on_the_references_plan(path):
    """T = fp32(r64_T), g = 1: 1 x 5 and 7 x 12 embedded with massless nodes, 10 / 12 below one tile, 33 one past 32, 80, directed C, KL."""
    g = np.load(path)
    f, out = _kernel_alone(path)
    for k in NAMES:
        got = out[k][0].cpu().numpy()
        err = rel(_block(f, k, got), g[f"r64_{k}"])
        print(f"{k}: {err:.2e}")
        assert np.isfinite(got).all() and err <= 1e-5, (k, err)
        outside = got.copy(); _block(f, k, outside)[...] = 0
        assert not outside.any(), k                                   # a massless node's rows and columns: exactly zero


@pytest.mark.parametrize("path", GRADS, ids=ids(GRADS))
def test_end_to_end_through_fgw_distance(path):
    g, f = np.load(path), pair_of(path)
    leaves = [t(f[k]).requires_grad_(True) for k in ("M", "C1", "C2", "p", "q")]
    G0 = t(f["G0"]) if f["G0"].size else None
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="Solver failed")
        d = pfgw.fgw_distance(*leaves, G0=G0, **_fgw_kw(f))
        _, log = pfgw.fgw(*(x.detach() for x in leaves), G0=G0, log=True, **_fgw_kw(f))
    assert d.dim() == 0 and d.requires_grad and torch.equal(bits(d.detach()), bits(log["fgw_dist"]))
    d.backward()
    for k, x in zip(NAMES, leaves):
        want = g[f"r64_{k}"]
        bound = max(1e-4, rel(g[f"r32_{k}"], want))
        err = rel(x.grad.cpu().numpy(), want)
        print(f"{k}: {err:.2e} (bound {bound:.2e})")
        assert x.grad.shape == x.shape and err <= bound, (k, err, bound)


def _rows_in_lds(N):
    """pair_dist_rows of fgw_pair.hip, which the backward kernel shares with k_fgw_pair_dist: the rows R of the intermediate product held in LDS.
    The constant and the lines of the rule are demanded as they stand, so that a change of the rule fails here instead of leaving R < N untested."""
    base = os.path.join(os.path.dirname(pfgw.__file__), "csrc")
    with open(os.path.join(base, "fgw_common.h")) as fh:
        common = fh.read()
    with open(os.path.join(base, "fgw_pair.hip")) as fh:
        src = fh.read()
    limit = int(re.search(r"constexpr size_t LDS_LIMIT = (\d+) \* 1024;", common).group(1)) * 1024
    for line in ("const size_t vec = (size_t)(4 * N + 16) * 8, row = (size_t)pitch_of(N) * 8;", "const size_t fit = (LDS_LIMIT - vec) / row;",
                 "const int R = fit >= (size_t)N ? N : (int)(fit / 16 * 16);", "const int R = pair_dist_rows(N, &bytes);"):
        assert line in src, line
    assert "int fgw_pitch(int N) { return N | 1; }" in common
    fit = (limit - (4 * N + 16) * 8) // ((N | 1) * 8)
    return N if fit >= N else fit // 16 * 16


def _inputs(n, graph, seed=1, dens=0.3):
    """make_fgw_pair_golden.py's inputs(): M ~ U(0, 2), p, q ~ U(0.5, 1.5) normalised, 0/1 undirected or positive directed float structures."""
    rng = np.random.RandomState(seed)
    M = rng.uniform(0.0, 2.0, size=(n, n))
    p = rng.uniform(0.5, 1.5, size=n); q = rng.uniform(0.5, 1.5, size=n)

    def structure():
        if graph == "directed_float":
            return rng.uniform(0.05, 1.0, size=(n, n))
        a = np.triu(rng.random_sample((n, n)) < dens, 1)
        return (a | a.T)

    return [t(x)[None] for x in (M, structure(), structure(), p / p.sum(), q / q.sum())]


def _against_fp64_torch(M, C1, C2, p, q, T, alpha, loss_fun, gout):
    out = _bwd(C1, C2, p, q, T, gout, alpha, loss_fun)
    want = fgw_dist_grads(M, C1, C2, p, q, T, alpha, loss_fun, gout)
    for k, w in zip(NAMES, want):
        err = rel(out[k].cpu().numpy(), w.cpu().numpy())
        print(f"{k}: {err:.2e}")
        assert err <= 1e-5, (k, err)


def test_n140_against_fp64_torch_at_our_own_plan():
    f = pair("pgd_n140")
    M, C1, C2, p, q = (t(f[k])[None] for k in ("M", "C1", "C2", "p", "q"))
    T = ops.fgw_pair_batched(M, C1, C2, p, q, **_ops_kw(f))[0]
    assert _rows_in_lds(140) == 140
    _against_fp64_torch(M, C1, C2, p, q, T, float(f["alpha"]), "square_loss", torch.ones(1, device=dev))


@pytest.mark.parametrize("loss_fun", ["square_loss", "kl_loss"])
def test_row_blocked_against_fp64_torch(loss_fun):
    """N = 142: the smallest size at which the intermediate product no longer fits in LDS whole (R = 128 < N with 160 KiB), so that the products run
    over two row blocks, the second of 14 rows.  Random inputs in the style of the fixtures' generator, the plan of our own solve (5 iterations);
    the KL case takes positive directed float structures and the same plan (any plan will do: it is a constant)."""
    N = next(n for n in range(2, 1024) if _rows_in_lds(n) < n)
    assert N == 142 and _rows_in_lds(N) == 128
    M, C1, C2, p, q = _inputs(N, "undirected")
    T = ops.fgw_pair_batched(M, C1, C2, p, q, alpha=0.9, epsilon=0.05, max_iter=5, symmetric=True)[0]
    assert abs(float(T.sum()) - 1) < 1e-5
    if loss_fun == "kl_loss":
        _, C1, C2, _, _ = _inputs(N, "directed_float", seed=2)
    _against_fp64_torch(M, C1, C2, p, q, T, 0.9, loss_fun, torch.full((1,), 0.75, device=dev))


def _three_of_one_size():
    """Three 10-node pairs as one batch: the plans of three fixtures, and the KL fixture's float structures on the third (its own loss is not used)."""
    fs = [pair(n) for n in ("pgd_n10", "ppa_n10", "pgd_kl_n10_float")]
    cols = [torch.cat(x) for x in zip(*(_square(f, f["r64_T"]) for f in fs))]
    return fs, cols


def test_gout_scales_every_pair_by_its_own_value():
    _, (C1, C2, p, q, T) = _three_of_one_size()
    gout = torch.tensor([0.5, -3.0, 7.25], device=dev)
    ones, scaled = _bwd(C1, C2, p, q, T, torch.ones(3, device=dev), 0.5), _bwd(C1, C2, p, q, T, gout, 0.5)
    for k in NAMES:
        for b in range(3):
            assert rel(scaled[k][b].cpu().numpy(), float(gout[b]) * ones[k][b].double().cpu().numpy()) <= 1e-6, (k, b)


@pytest.mark.parametrize("loss_fun", ["square_loss", "kl_loss"])
def test_only_the_wanted_outputs_are_written(loss_fun):
    _, (C1, C2, p, q, T) = _three_of_one_size()
    C1, C2 = C1 + 0.1, C2 + 0.1                                          # (positive structures for the KL run)
    gout = torch.tensor([0.5, -3.0, 7.25], device=dev)
    every = _bwd(C1, C2, p, q, T, gout, 0.5, loss_fun)
    assert all(torch.isfinite(every[k]).all() for k in NAMES)
    for want in ("dC2", "dp", "dM", "dC1", "dq"):
        some = _bwd(C1, C2, p, q, T, gout, 0.5, loss_fun, want=(want,))
        for k in NAMES:
            if k == want:
                assert torch.equal(bits(some[k]), bits(every[k])), (want, k)
            else:
                assert torch.isnan(some[k]).all(), (want, k)


def test_only_c2_requires_grad():
    f = pair("pgd_n33")
    M, C1, C2, p, q = (t(f[k]) for k in ("M", "C1", "C2", "p", "q"))
    C2.requires_grad_(True)
    seen = []
    from conan_fgw_amd import _lib
    prev = _lib.set_call_trace(lambda name, fn, args: (seen.append((name, args)), fn(*args))[1])
    try:
        pfgw.fgw_distance(M, C1, C2, p, q, **_fgw_kw(f)).backward()
    finally:
        _lib.set_call_trace(prev)
    assert [n for n, _ in seen] == ["conan_fgw_pair_fwd", "conan_fgw_pair_dist_bwd"]          # the distance kernel does not run a second time
    dM, dC1, dC2, dp, dq = seen[1][1][10:15]
    assert (dM, dC1, dp, dq) == (None, None, None, None) and dC2 is not None
    assert all(x.grad is None for x in (M, C1, p, q))
    assert rel(C2.grad.cpu().numpy(), np.load(os.path.join(GOLDEN, "fgw_distgrad_pgd_n33.npz"))["r64_dC2"]) <= 1e-4


def _grads_of(dist, leaves):
    return torch.autograd.grad(dist.sum(), leaves)


def test_batch_of_three_is_the_three_single_calls():
    fs, (C1, C2, p, q, T) = _three_of_one_size()
    gout = torch.tensor([0.5, -3.0, 7.25], device=dev)
    batch = _bwd(C1, C2, p, q, T, gout, 0.5)
    again = _bwd(C1, C2, p, q, T, gout, 0.5)
    for k in NAMES:
        assert torch.equal(bits(batch[k]), bits(again[k])), k
        for b in range(3):
            single = _bwd(C1[b:b + 1], C2[b:b + 1], p[b:b + 1], q[b:b + 1], T[b:b + 1], gout[b:b + 1], 0.5)
            assert torch.equal(bits(batch[k][b:b + 1]), bits(single[k])), (k, b)
    assert not torch.equal(batch["dC1"][0], batch["dC1"][1])
    # the same through the solve: ops.fgw_pair_distance on a batch against one call per pair
    M = torch.cat([t(f["M"])[None] for f in fs])
    kw = dict(alpha=0.5, epsilon=0.1, max_iter=25, tol=1e-12, symmetric=True)
    leaves = [x.clone().requires_grad_(True) for x in (M, C1, C2, p, q)]
    d = ops.fgw_pair_distance(*leaves, **kw)
    gb = _grads_of(d, leaves)
    for b in range(3):
        one = [x[b:b + 1].detach().clone().requires_grad_(True) for x in leaves]
        d1 = ops.fgw_pair_distance(*one, **kw)
        assert torch.equal(bits(d1.detach()), bits(d[b:b + 1].detach()))
        for k, x, y in zip(NAMES, gb, _grads_of(d1, one)):
            assert torch.equal(bits(x[b:b + 1]), bits(y)), (k, b)


def test_ragged_list_is_the_per_pair_calls():
    """Pairs of 7 x 12, 12 x 12 and 1 x 12 nodes in one launch (embedded in 12 nodes); the gradients come back in every pair's own shapes."""
    f7, f12 = pair("pgd_rect_7x12"), pair("pgd_undir_n12_none")
    a, b = ([t(f[k]) for k in ("M", "C1", "C2", "p", "q")] for f in (f7, f12))
    one = [a[0][:1], a[1][:1, :1], a[2], torch.ones(1, device=dev), a[4]]
    pairs = [[x.clone().requires_grad_(True) for x in pr] for pr in (a, b, one)]
    kw = _ops_kw(f7)
    cols = [[pr[k] for pr in pairs] for k in range(5)]
    d, Ts, info, errs = ops.fgw_pair_distance_list(*cols, return_plan=True, **kw)
    assert [tuple(T.shape) for T in Ts] == [(7, 12), (12, 12), (1, 12)] and not any(x.requires_grad for x in Ts + [info, errs])
    flat = [x for pr in pairs for x in pr]
    got = torch.autograd.grad(d.sum(), flat)
    assert [x.shape for x in got] == [x.shape for x in flat]
    for k, pr in enumerate(pairs):
        single = [x.detach().clone()[None].requires_grad_(True) for x in pr]
        d1 = ops.fgw_pair_distance(*single, **kw)
        assert torch.equal(bits(d1.detach()), bits(d[k:k + 1].detach()))
        for name, x, y in zip(NAMES, got[5 * k:5 * k + 5], _grads_of(d1, single)):
            assert torch.equal(bits(x), bits(y[0])), (k, name)
    want = np.load(os.path.join(GOLDEN, "fgw_distgrad_pgd_rect_7x12.npz"))
    for name, x in zip(NAMES, got[:5]):
        assert rel(x.cpu().numpy(), want[f"r64_{name}"]) <= max(1e-4, rel(want[f"r32_{name}"], want[f"r64_{name}"])), name


@pytest.mark.parametrize("name", ["pgd_n10", "pgd_rect_7x12"])
def test_no_marginals_means_uniform_marginals(name):
    """p = q = None: in the kernel (1 / N formed in fp64 against the caller's fp32(1 / n): 6e-8 apart, bound 1e-6 at the same plan) and through
    fgw_distance, also for a rectangular pair, whose uniform weights are formed over the REAL nodes (the solve moves with them: 1e-4)."""
    f = pair(name)
    n1, n2 = f["M"].shape
    up, uq = torch.full((n1,), 1.0 / n1, device=dev), torch.full((n2,), 1.0 / n2, device=dev)
    if n1 == n2:
        C1, C2, _, _, T = _square(f, f["r64_T"])
        ones = torch.ones(1, device=dev)
        none = _bwd(C1, C2, None, None, T, ones, 0.5, want=("dM", "dC1", "dC2"))
        full = _bwd(C1, C2, up[None], uq[None], T, ones, 0.5)
        for k in ("dM", "dC1", "dC2"):
            assert rel(none[k].cpu().numpy(), full[k].cpu().numpy()) <= 1e-6, k
    res = []
    for p, q in ((None, None), (up, uq)):
        leaves = [t(f[k]).requires_grad_(True) for k in ("M", "C1", "C2")]
        pfgw.fgw_distance(*leaves, p, q, **_fgw_kw(f)).backward()
        res.append([x.grad for x in leaves])
    for k, x, y in zip(NAMES, *res):
        assert x.shape == y.shape and torch.isfinite(x).all() and rel(x.cpu().numpy(), y.cpu().numpy()) <= 1e-4, k


@pytest.mark.parametrize("ragged", [False, True], ids=["one_size", "ragged"])
def test_pairwise_distances_carry_gradients_to_features_and_structures(ragged):
    from test_gpu_fgw_pair import _conformers
    kw = dict(alpha=0.5, epsilon=0.1, max_iter=30, tol=1e-5)
    Ys, Cs = _conformers(G=4)
    if ragged:
        Ys[1], Cs[1] = Ys[1][:9], Cs[1][:9, :9].contiguous()
    D0 = pfgw.fgw_pairwise_distances(Ys, Cs, **kw)
    assert not D0.requires_grad
    Ys = [y.clone().requires_grad_(True) for y in Ys]
    Cs = [c.clone().requires_grad_(True) for c in Cs]
    D = pfgw.fgw_pairwise_distances(Ys, Cs, **kw)
    assert D.requires_grad and torch.equal(bits(D.detach()), bits(D0))
    D.sum().backward()
    # fp64: every pair's distance at the plan our own solve returns for it, differentiated through feature_cost; each pair counts twice in D.sum()
    Y64 = [y.detach().double().requires_grad_(True) for y in Ys]
    C64 = [c.detach().double().requires_grad_(True) for c in Cs]
    total = 0.0
    from fgw_pair_grad_ref import fgw_dist_torch
    for a in range(4):
        for b in range(a + 1, 4):
            T = pfgw.fgw(pfgw.feature_cost(Ys[a].detach(), Ys[b].detach()), Cs[a].detach(), Cs[b].detach(), **kw)
            na, nb = Y64[a].shape[0], Y64[b].shape[0]
            p, q = torch.full((1, na), 1.0 / na, dtype=torch.float64, device=dev), torch.full((1, nb), 1.0 / nb, dtype=torch.float64, device=dev)
            total = total + 2 * fgw_dist_torch(pfgw.feature_cost(Y64[a], Y64[b])[None], C64[a][None], C64[b][None], p, q, T.double()[None], 0.5).sum()
    total.backward()
    for k in range(4):
        ey, ec = rel(Ys[k].grad.cpu().numpy(), Y64[k].grad.cpu().numpy()), rel(Cs[k].grad.cpu().numpy(), C64[k].grad.cpu().numpy())
        print(f"conformer {k}: dY {ey:.2e} dC {ec:.2e}")
        assert Ys[k].grad.shape == Ys[k].shape and Cs[k].grad.shape == Cs[k].shape and ey <= 1e-4 and ec <= 1e-4, (k, ey, ec)


def test_distance_of_a_given_plan_is_differentiable():
    path = os.path.join(GOLDEN, "fgw_distgrad_pgd_dir_n12_false.npz")
    f, alone = _kernel_alone(path)
    M, C1, C2, p, q, T = (t(f[k])[None] for k in ("M", "C1", "C2", "p", "q", "r64_T"))
    plain = ops.fgw_pair_dist(M, C1, C2, T, p, q, alpha=float(f["alpha"]))
    C1.requires_grad_(True)
    d = ops.fgw_pair_dist(M, C1, C2, T, p, q, alpha=float(f["alpha"]))
    assert not plain.requires_grad and d.requires_grad and torch.equal(bits(d.detach()), bits(plain))
    d.sum().backward()
    assert torch.equal(bits(C1.grad), bits(alone["dC1"])) and M.grad is None and T.grad is None


def test_failed_plan_gives_the_warning_and_nonfinite_gradients():
    """The inputs of test_failed_plan_warns_like_the_reference: marginals of mass 1/2 (a finite plan of mass 1/2: finite gradients), and a BAPG run
    whose kernel underflows to a NaN plan: NaN gradients, the warning, and nothing else happens."""
    f = pair("pgd_n10")
    mk = lambda: [t(f[k]).requires_grad_(True) for k in ("M", "C1", "C2", "p", "q")]
    M, C1, C2, p, q = mk()
    with pytest.warns(UserWarning, match="Solver failed to produce a transport plan"):
        d = pfgw.fgw_distance(M, C1, C2, p * 0.5, q * 0.5, symmetric=True)
    d.backward()
    assert all(torch.isfinite(x.grad).all() for x in (M, C1, C2, p, q))
    M, C1, C2, p, q = mk()
    with pytest.warns(UserWarning, match="Solver failed to produce a transport plan"):
        d, log = pfgw.fgw_distance(M * 1e4, C1, C2, p, q, solver="BAPG", epsilon=1e-3, symmetric=True, max_iter=10, log=True)
    assert torch.isnan(log["T"]).any() and not log["T"].requires_grad and not torch.isfinite(d)
    d.backward()
    torch.cuda.synchronize()
    assert all(not torch.isfinite(x.grad).all() for x in (M, C1, C2))
