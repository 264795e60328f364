"""The reference's greenkhorn, sinkhorn_stabilized and sinkhorn_epsilon_scaling on the GPU (csrc/sinkhorn_ext.hip through ops.sinkhorn_ext_batched /
sinkhorn_ext_list / sinkhorn_ext_loss and conan_fgw_amd.sinkhorn).

Yardsticks: the stored runs of the reference (tests/golden/ext_sinkhorn_*.npz: its fp32 run r32 and its fp64 run r64 on the same fp32 inputs) and,
where no fixture exists, the fp64 restatement tests/sinkhorn_ext_ref.py (held to every fixture by tests/test_sinkhorn_ext_cpu.py, which also
asserts that every fixture keeps its decisions away from the thresholds).  The kernels iterate in fp64, so counts are r64's.  Tolerances are those
of tests/test_gpu_sinkhorn.py:
  iteration index, flags, absorptions / inner counts equal; errs within rtol 2e-3 of r64's plus 1e-3 stopThr absolute, NaN beyond the executed checks;
  T: rel(T, r32_T) <= 1e-4 or rel(T, r64_T) <= rel(r32_T, r64_T); where r32 and r64 took different counts only rel(T, r64_T) <= 1e-4; where the
  reference's plan has NaN, the same NaN mask and the finite entries compared;
  loss within 1e-4 relative; logu / logv / log u / log v within 1e-4 absolute on entries with mass; alpha, beta within 1e-4 reg absolute
  (rel = Frobenius norm of the difference over that of the yardstick)."""
import os
import warnings

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, ops
from conan_fgw_amd import sinkhorn as sk

from sinkhorn_ext_ref import epsilon_scaling_ref, greenkhorn_ref, stabilized_ref
from test_sinkhorn_ext_cpu import BAD_ARGUMENTS, EPS, GK, NAMES, STAB, ext_rc, load

pytestmark = pytest.mark.gpu

DEV = "cuda"
METHODS = ["greenkhorn", "sinkhorn_stabilized", "sinkhorn_epsilon_scaling"]
_NOCONV = "Sinkhorn did not converge. You might want to increase the number of iterations `numItermax` or the regularization parameter `reg`."


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


def gpu(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def same_bits(xs, ys):
    return all(torch.equal(bits(x), bits(y)) if x.is_floating_point() else torch.equal(x.cpu(), y.cpu()) for x, y in zip(xs, ys))


def problem(n1, n2, seed):
    """Uniform random costs, random normalised marginals (the fixtures' construction)."""
    g = np.random.default_rng(seed)
    M = g.random((n1, n2)).astype(np.float32)
    a, b = g.random(n1) + 0.1, g.random(n2) + 0.1
    return M, (a / a.sum()).astype(np.float32), (b / b.sum()).astype(np.float32)


def params_of(f):
    """The op's keyword arguments for a fixture."""
    kw = dict(reg=float(f["reg"]), method=str(f["method"]), num_iter_max=int(f["numItermax"]), stop_thr=float(f["stopThr"]))
    for key, name in (("tau", "tau"), ("print_period", "print_period"), ("epsilon0", "epsilon0"), ("numInnerItermax", "num_inner_iter_max")):
        if key in f:
            kw[name] = float(f[key]) if key in ("tau", "epsilon0") else int(f[key])
    return kw


def solve_one(M, a, b, warm=None, **kw):
    """B = 1 through ops.sinkhorn_ext_batched in the problem's own container -> the nine outputs without the batch axis."""
    w = None if warm is None else (gpu(warm[0], torch.float64)[None], gpu(warm[1], torch.float64)[None])
    out = ops.sinkhorn_ext_batched(gpu(M)[None], None if a is None else gpu(a)[None], None if b is None else gpu(b)[None], warmstart=w, **kw)
    return tuple(o[0] for o in out)


def solve_fixture(f):
    return solve_one(f["M"], f["a"], f["b"], (f["warm_u"], f["warm_v"]) if "warm_u" in f else None, **params_of(f))


def close_where_finite(got, want, tol, mass, tag):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isfinite(got)[mass], np.isfinite(want)[mass]), (tag, got, want)
    ok = np.isfinite(want) & mass
    d = float(np.abs(got - want)[ok].max()) if ok.any() else 0.0
    assert d <= tol, (tag, d, tol)
    return d


def check(f, out, tag):
    """The yardsticks of the module docstring; f is a fixture, out the nine outputs of the op for it."""
    T, loss, lu, lv, al, be, info, errs, extra = (o.cpu().numpy() for o in out)
    method, warn, thr, reg = str(f["method"]), str(f["r64_warn"]), float(f["stopThr"]), float(f["reg"])
    niter, flags, nchk, last = (int(x) for x in info)
    assert niter == int(f["r64_niter"]), (tag, niter, int(f["r64_niter"]))
    if method == "greenkhorn":
        assert flags == (1 if warn == "" else 0) and nchk == 0 and last == 0 and errs.shape == (0,) and int(extra[0]) == niter + 1
    elif method == "sinkhorn_stabilized":
        assert flags == {"": 1, "noconv": 0, "numerr": 2}[warn], (tag, flags, warn)
        assert last == int(f["r64_absorptions"]) == int(extra[1]) and int(extra[0]) == niter + 1, (tag, last, int(f["r64_absorptions"]))
    else:
        assert flags == (1 if warn == "" else 0) + (2 if f["r64_inner_numerr"].any() else 0), (tag, flags, warn)
        assert last == int(f["r64_inner_noconv"].sum()) and int(extra[0]) == int((f["r64_inner_niter"] + 1).sum()), (tag, last, extra)
        assert int(extra[1]) == int(f["r64_inner_absorptions"].sum()) and int(extra[2]) == int(f["r64_inner_numerr"].sum()), (tag, extra)
    if method != "greenkhorn":
        r64_err = np.asarray(f["r64_err"], dtype=np.float64)
        n = len(r64_err)
        assert nchk == n, (tag, nchk, n)
        e = errs.astype(np.float64)
        print(f"{tag}: niter {niter} flags {flags} last {last} errs {e[:n][-2:]} r64 {r64_err[-2:]}")
        assert np.array_equal(np.isnan(e[:n]), np.isnan(r64_err)), (tag, e[:n], r64_err)
        with np.errstate(invalid="ignore"):
            assert np.all(np.isnan(r64_err) | (np.abs(e[:n] - r64_err) <= 2e-3 * np.abs(r64_err) + 1e-3 * thr)), (tag, e[:n], r64_err)
        assert np.isnan(e[n:]).all(), (tag, e)
    ref, r32 = f["r64_T"], f["r32_T"].astype(np.float64)
    mask = np.isnan(ref)
    assert np.array_equal(np.isnan(T), mask), (tag, int(np.isnan(T).sum()), int(mask.sum()))
    ma, mb = np.asarray(f["a"]) > 0, np.asarray(f["b"]) > 0
    if not mask.all():
        r64 = rel(T[~mask], ref[~mask])
        same_counts = int(f["r32_niter"]) == int(f["r64_niter"]) and np.array_equal(np.isnan(r32), mask)
        if same_counts:
            g32, base = rel(T[~mask], r32[~mask]), rel(r32[~mask], ref[~mask])
            print(f"{tag}: rel(T, r32) {g32:.2e} rel(T, r64) {r64:.2e} rel(r32, r64) {base:.2e}")
            assert g32 <= 1e-4 or r64 <= base, (tag, g32, r64, base)
        else:
            print(f"{tag}: rel(T, r64) {r64:.2e}")
            assert r64 <= 1e-4, (tag, r64)
    if not mask.any():
        el = abs(float(loss) - float(f["r64_loss"])) / abs(float(f["r64_loss"]))
        assert el <= 1e-4, (tag, el)
    with np.errstate(all="ignore"):
        if method == "greenkhorn":
            du = close_where_finite(lu, np.log(f["r64_u"]), 1e-4, ma, tag + " log u")
            dv = close_where_finite(lv, np.log(f["r64_v"]), 1e-4, mb, tag + " log v")
            assert not al.any() and not be.any()
        else:
            du = close_where_finite(al, f["r64_alpha"], 1e-4 * reg, ma, tag + " alpha")
            dv = close_where_finite(be, f["r64_beta"], 1e-4 * reg, mb, tag + " beta")
            if method == "sinkhorn_stabilized":
                close_where_finite(lu, f["r64_logu"], 1e-4, ma, tag + " logu")
                close_where_finite(lv, f["r64_logv"], 1e-4, mb, tag + " logv")
    print(f"{tag}: potentials off by {du:.2e} {dv:.2e}")


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_the_op(name):
    f = load(name)
    check(f, solve_fixture(f), name)


def expected_warnings(f):
    method, warn, niter = str(f["method"]), str(f["r64_warn"]), int(f["r64_niter"])
    if method == "sinkhorn_epsilon_scaling":
        numerr = np.flatnonzero(f["r64_inner_numerr"])
        return ((["Numerical errors at iteration %d" % int(f["r64_inner_niter"][numerr[-1]])] if len(numerr) else [])
                + ([_NOCONV] if f["r64_inner_noconv"].any() else []) + ([_NOCONV] if warn == "noconv" else []))
    return {"": [], "noconv": [_NOCONV], "numerr": ["Numerical errors at iteration %d" % niter]}[warn]


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_the_public_function(name):
    f = load(name)
    kw = params_of(f)
    method = kw.pop("method")
    pub = dict(numItermax=kw.pop("num_iter_max"), stopThr=kw.pop("stop_thr"))
    if "num_inner_iter_max" in kw:
        pub["numInnerItermax"] = kw.pop("num_inner_iter_max")
    reg = kw.pop("reg")
    pub.update(kw)
    warm = (gpu(f["warm_u"]), gpu(f["warm_v"])) if "warm_u" in f else None
    a, b, M = gpu(f["a"]), gpu(f["b"]), gpu(f["M"])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        T, log = sk.sinkhorn(a, b, M, reg, method=method, log=True, warmstart=warm, **pub)
    want = expected_warnings(f)
    assert [str(x.message) for x in w] == want
    ref = solve_fixture(f)                                                 # the same launch as the op: the same bits
    assert torch.equal(bits(T), bits(ref[0])) and not T.requires_grad
    if method == "greenkhorn":
        assert set(log) == {"n_iter", "u", "v"} and log["n_iter"] == int(ref[6][0]) and isinstance(log["n_iter"], int)
        assert torch.equal(bits(log["u"]), bits(torch.exp(ref[2]))) and torch.equal(bits(log["v"]), bits(torch.exp(ref[3])))
    else:
        nchk = int(ref[6][2])
        assert isinstance(log["err"], list) and len(log["err"]) == nchk == len(f["r64_err"])
        assert same_bits(log["err"], list(ref[7][:nchk]))
        assert torch.equal(bits(log["alpha"]), bits(ref[4])) and torch.equal(bits(log["beta"]), bits(ref[5]))
        assert log["warmstart"][0] is log["alpha"] and log["warmstart"][1] is log["beta"]
        if method == "sinkhorn_stabilized":
            assert set(log) == {"err", "n_iter", "logu", "logv", "alpha", "beta", "warmstart"} and log["n_iter"] == int(ref[6][0])
            assert torch.equal(bits(log["logu"]), bits(ref[2])) and torch.equal(bits(log["logv"]), bits(ref[3]))
        else:
            assert set(log) == {"err", "alpha", "beta", "warmstart", "niter"} and log["niter"] == int(ref[6][0])
    direct = {"greenkhorn": sk.greenkhorn, "sinkhorn_stabilized": sk.sinkhorn_stabilized, "sinkhorn_epsilon_scaling": sk.sinkhorn_epsilon_scaling}[method]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        T2 = direct(a, b, M, reg, warn=False, warmstart=warm, **pub)
    outer_noconv = str(f["r64_warn"]) == "noconv"                          # warn=False silences only the solver's own "did not converge"
    assert [str(x.message) for x in w] == (want[:-1] if outer_noconv else want) and torch.equal(bits(T2), bits(T))
    if method == "sinkhorn_stabilized":
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            cost, log2 = sk.sinkhorn2(a, b, M, reg, method="Sinkhorn_Stabilized", log=True, warn=True, warmstart=warm, **pub)
        assert [str(x.message) for x in w] == want and cost.dim() == 0 and torch.equal(bits(cost), bits(ref[1])) and log2["n_iter"] == log["n_iter"]


BATCH_KW = {"greenkhorn": dict(reg=0.1, num_iter_max=200, stop_thr=1e-5),
            "sinkhorn_stabilized": dict(reg=0.02, num_iter_max=100, stop_thr=1e-7, tau=100.0, print_period=10),
            "sinkhorn_epsilon_scaling": dict(reg=0.1, num_iter_max=10, stop_thr=1e-6, num_inner_iter_max=25, tau=100.0)}


@pytest.mark.parametrize("method", METHODS)
def test_batching_is_bit_identical(method):
    """A problem's outputs do not depend on the batch, its position, the container or on where the matrix lives: the ragged problems of the
    fixtures in one streamed container, in two orders, against each alone in its own container (all but 140x140 LDS-resident)."""
    fs = [load(f"stab_{s}") for s in ("1x5", "7x12", "33x33", "64x80", "65x257", "257x65", "140x140")]
    kw = dict(BATCH_KW[method], method=method)
    N1, N2 = 261, 259
    assert not _lib.lib().conan_sinkhorn_ext_lds_resident(N1, N2)
    alone = [solve_one(f["M"], f["a"], f["b"], **kw) for f in fs]
    for order in (list(range(len(fs))), [int(i) for i in np.random.default_rng(3).permutation(len(fs))]):
        sub = [fs[i] for i in order]
        Ms, as_, bs = [gpu(f["M"]) for f in sub], [gpu(f["a"]) for f in sub], [gpu(f["b"]) for f in sub]
        M, a, b, _w, n1, n2, sizes = ops._sinkhorn_list_stack(Ms, as_, bs, None, (N1, N2))
        full = ops.sinkhorn_ext_batched(M, a, b, n1=n1, n2=n2, **kw)
        assert same_bits(full, ops.sinkhorn_ext_batched(M, a, b, n1=n1, n2=n2, **kw))
        lists = ops.sinkhorn_ext_list(Ms, as_, bs, **kw)                   # ragged problems in one launch, the smallest container
        T, loss, lu, lv, al, be, info, errs, extra = full
        for k, (m1, m2) in enumerate(sizes):
            one = alone[order[k]]
            got = (T[k, :m1, :m2], loss[k], lu[k, :m1], lv[k, :m2], al[k, :m1], be[k, :m2], info[k], errs[k], extra[k])
            assert same_bits(got, one), (k, sizes[k], info[k], one[6])
            got = (lists[0][k], lists[1][k], lists[2][k], lists[3][k], lists[4][k], lists[5][k], lists[6][k], lists[7][k], lists[8][k])
            assert same_bits(got, one), (k, sizes[k])
            for pad in (T[k, m1:], T[k, :, m2:], lu[k, m1:], lv[k, m2:], al[k, m1:], be[k, m2:]):
                assert not bits(pad).any()
    assert len(set(int(o[8][0]) for o in alone)) > 1                       # the batch really mixes amounts of work


def yardstick(method, M, a, b, kw):
    if method == "greenkhorn":
        T, log = greenkhorn_ref(a, b, M, kw["reg"], kw["num_iter_max"], kw["stop_thr"])
        assert min(log["gaps"]) >= 1e-9
        return T, log["n_iter"]
    if method == "sinkhorn_stabilized":
        T, log = stabilized_ref(a, b, M, kw["reg"], kw["num_iter_max"], kw["tau"], kw["stop_thr"], None, kw["print_period"])
        return T, log["n_iter"]
    T, log = epsilon_scaling_ref(a, b, M, kw["reg"], kw["num_iter_max"], 1e4, kw["num_inner_iter_max"], kw["tau"], kw["stop_thr"])
    return T, log["niter"]


@pytest.mark.parametrize("method", METHODS)
def test_rectangular_and_streamed_against_the_restatement(method):
    """n1 != n2 both ways, and the largest LDS-resident shape beside the smallest streamed one.  stop_thr = 0 is never reached by an error that is
    a norm, so every run takes exactly its cap and counts compare without a margin (greenkhorn: the restatement's arg-max gaps are asserted)."""
    L = _lib.lib()
    n1, n2 = 64, 280
    assert L.conan_sinkhorn_ext_lds_resident(n1, n2) == 1
    while L.conan_sinkhorn_ext_lds_resident(n1, n2 + 1):
        n2 += 1
    assert 280 < n2 < 320 and not L.conan_sinkhorn_ext_lds_resident(n1, n2 + 1)
    kw = dict(BATCH_KW[method], stop_thr=0.0)
    for shape in ((7, 12), (12, 7), (n1, n2), (n1, n2 + 1)):
        M, a, b = problem(*shape, seed=1)
        want, niter = yardstick(method, M, a, b, kw)
        out = solve_one(M, a, b, method=method, **kw)
        assert int(out[6][0]) == niter and int(out[6][1]) == 0, (shape, out[6], niter)
        r = rel(out[0].cpu().numpy(), want)
        print(f"{method} {shape}: rel(T, restatement) {r:.2e}")
        assert r <= 1e-6, (shape, r)                                       # an fp64 iteration stored as fp32: 6e-8 per entry
    # the resident shape inside the streamed container: the same bits
    M, a, b = problem(n1, n2, seed=1)
    one = solve_one(M, a, b, method=method, **kw)
    lists = ops.sinkhorn_ext_list([gpu(M), gpu(problem(n1, n2 + 1, seed=1)[0])], [gpu(a), None], [gpu(b), None], method=method, **kw)
    assert same_bits((lists[0][0], lists[1][0], lists[6][0], lists[7][0]), (one[0], one[1], one[6], one[7]))


def test_shared_cost_matrix_stride_zero():
    M, a, _ = problem(33, 40, 11)
    bsets = np.stack([problem(33, 40, 20 + k)[2] for k in range(3)])
    for method in METHODS:
        kw = dict(BATCH_KW[method], method=method)
        shared = ops.sinkhorn_ext_batched(gpu(M), None, gpu(bsets), **kw)
        assert shared[0].shape == (3, 33, 40)
        for k in range(3):
            assert same_bits([x[k] for x in shared], solve_one(M, None, bsets[k], **kw))
        assert not torch.equal(shared[0][0], shared[0][1])


def test_no_host_synchronisation():
    M, a, b = problem(33, 40, 5)
    Mg, ag, bg = gpu(np.stack([M, M.copy()])), gpu(np.stack([a, a])), gpu(np.stack([b, b]))
    n1 = torch.tensor([33, 20], dtype=torch.int32, device=DEV)
    Mq = Mg.clone().requires_grad_(True)
    gout = torch.rand(2, device=DEV)
    for method in METHODS:                                                 # (first calls: library load, allocator warm-up)
        ops.sinkhorn_ext_batched(Mg, ag, bg, n1=n1, method=method, **BATCH_KW[method])
        ops.sinkhorn_ext_loss(Mq, ag, bg, method=method, **BATCH_KW[method]).backward(gout)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for method in METHODS:
            ops.sinkhorn_ext_batched(Mg, ag, bg, n1=n1, method=method, **BATCH_KW[method])
            ops.sinkhorn_ext_loss(Mq, ag, bg, method=method, **BATCH_KW[method]).backward(gout)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(Mq.grad).all()


def test_gradient_is_the_fixed_plan():
    M, a, b = problem(20, 25, 8)
    Mg, ag, bg = gpu(M).requires_grad_(True), gpu(a).requires_grad_(True), gpu(b).requires_grad_(True)
    cost = sk.sinkhorn2(ag, bg, Mg, 0.05, method="sinkhorn_stabilized", numItermax=100, stopThr=1e-5)
    assert cost.requires_grad and cost.dim() == 0
    cost.backward()
    T = sk.sinkhorn(ag, bg, Mg, 0.05, method="sinkhorn_stabilized", numItermax=100, stopThr=1e-5)
    assert not T.requires_grad and torch.equal(bits(Mg.grad), bits(T)) and ag.grad is None and bg.grad is None
    assert abs(float(cost.detach()) - float((Mg.detach() * T).sum())) <= 1e-5 * float(cost.detach())
    # the batched loss with a random upstream gradient, ragged sizes inside one container, every method
    Mb = gpu(np.stack([problem(20, 25, 8 + k)[0] for k in range(3)]))
    n1, n2 = torch.tensor([20, 7, 13], dtype=torch.int32, device=DEV), torch.tensor([25, 25, 9], dtype=torch.int32, device=DEV)
    gout = torch.rand(3, device=DEV) + 0.5
    for method in METHODS:
        Mq = Mb.clone().requires_grad_(True)
        loss, T, *_ = ops.sinkhorn_ext_loss(Mq, method=method, n1=n1, n2=n2, return_plan=True, **BATCH_KW[method])
        loss.backward(gout)
        assert torch.equal(bits(Mq.grad), bits(gout[:, None, None] * T)) and not Mq.grad[1, 7:].any() and Mq.grad[1, :7].any()
        assert same_bits((loss.detach(), T), ops.sinkhorn_ext_batched(Mb, method=method, n1=n1, n2=n2, **BATCH_KW[method])[1::-1])


def test_dispatcher_in_upper_and_lower_case():
    M, a, b = problem(12, 9, 2)
    Mg, ag, bg = gpu(M), gpu(a), gpu(b)
    for method, fn, extra in (("greenkhorn", sk.greenkhorn, {}), ("sinkhorn_stabilized", sk.sinkhorn_stabilized, dict(tau=50.0, print_period=5)),
                              ("sinkhorn_epsilon_scaling", sk.sinkhorn_epsilon_scaling, dict(numInnerItermax=20, epsilon0=100.0))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = fn(ag, bg, Mg, 0.05, numItermax=60, stopThr=1e-6, **extra)
            for spelling in (method, method.upper(), method.title()):
                got = sk.sinkhorn(ag, bg, Mg, 0.05, method=spelling, numItermax=60, stopThr=1e-6, **extra)
                assert torch.equal(bits(got), bits(want)), spelling
        assert torch.isfinite(want).all() and float(want.sum()) > 0.5     # (60 iterations: a plan, not a converged one)
    with pytest.raises(ValueError, match="Unknown method 'nope'"):
        sk.sinkhorn(ag, bg, Mg, 0.05, method="nope")
    with pytest.raises(ValueError, match="Unknown method"):
        sk.sinkhorn2(ag, bg, Mg, 0.05, method="greenkhorn")
    with pytest.raises(NotImplementedError, match="several histograms"):
        sk.sinkhorn_stabilized(ag, torch.ones(9, 2, device=DEV) / 9, Mg, 0.05)
    empty = torch.zeros(0, device=DEV)                                     # empty histograms mean uniform, as in the reference
    assert torch.equal(bits(sk.greenkhorn(empty, empty, Mg, 0.1, numItermax=50, warn=False)),
                       bits(solve_one(M, None, None, method="greenkhorn", reg=0.1, num_iter_max=50)[0]))


def test_bad_arguments_through_ctypes():
    L = _lib.lib()
    B, N1, N2 = 2, 6, 5
    M, T = torch.rand(B, N1, N2, device=DEV), torch.full((B, N1, N2), 7.0, device=DEV)
    ws = torch.empty(int(L.conan_sinkhorn_ext_workspace_bytes(B, N1, N2)), dtype=torch.uint8, device=DEV)
    good = dict(M=M.data_ptr(), B=B, N1=N1, N2=N2, stride=N1 * N2, reg=0.1, method=3, it=10, thr=1e-9, tau=1e3, pp=20, eps0=1e4, inner=10,
                T=T.data_ptr(), ws=ws.data_ptr(), stream=_lib.stream_ptr())
    for kw in BAD_ARGUMENTS:
        assert ext_rc(L, good, **kw) == -1, kw
    torch.cuda.synchronize()
    assert (T == 7.0).all()                                                # refused before any launch
    for method in (2, 3, 4):                                               # every output but T may be null
        assert ext_rc(L, good, method=method) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(T).all() and (T != 7.0).all() and abs(float(T.sum()) - B) < 0.2, method      # launched: every entry written (10 iterations: no converged plan)
        T.fill_(7.0)
