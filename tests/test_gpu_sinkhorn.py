"""Entropic OT on its own on the GPU (csrc/sinkhorn.hip through ops.sinkhorn_batched / sinkhorn_list / sinkhorn_loss and conan_fgw_amd.sinkhorn).

Yardsticks: the stored runs of the reference's sinkhorn.py (tests/golden/sinkhorn_*.npz: its fp32 run r32 and its fp64 run r64 on the same fp32
inputs) and, where no fixture exists, the fp64 restatement tests/sinkhorn_ref.py (held to every fixture by tests/test_sinkhorn_cpu.py).  The
kernel iterates in fp64, so its iteration count, flags and error list are r64's:
  niter and flags equal; errs within rtol 2e-3 of r64_err plus 1e-3 stopThr absolute (every fixture keeps its checks a factor 1.5 away from the
  threshold, so an error that small cannot move a stop decision), NaN beyond the executed checks;
  T: rel(T, r32_T) <= 1e-4 or rel(T, r64_T) <= rel(r32_T, r64_T); where r32 and r64 took different counts only rel(T, r64_T) <= 1e-4;
  loss within 1e-4 relative of r64's; log_u, log_v within 1e-4 absolute of r64's on entries with mass;
  exp(log_u + Mr + log_v) reproduces T to 1e-5 relative (rel = Frobenius norm of the difference over that of the yardstick)."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, ops
from conan_fgw_amd import sinkhorn as sk
from conan_fgw_amd.fgw import feature_cost

from sinkhorn_ref import fair, sinkhorn_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["1x5", "7x12", "33x33", "64x80", "257x65", "140x140", "9x11col", "zeroa", "warm", "65x257"]
NAMES = [f"{c}_{m}" for c in CASES for m in ("log", "knopp")]
DEV = "cuda"
_NOCONV = "Sinkhorn did not converge. You might want to increase the number of iterations `numItermax` or the regularization parameter `reg`."


def load(name):
    z = np.load(os.path.join(GOLDEN, f"sinkhorn_{name}.npz"))
    return {k: z[k] for k in z.files}


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


def gpu(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(DEV)


def problem(n1, n2, seed):
    """Squared distances of two Gaussian clouds over their maximum, random normalised marginals (the fixtures' construction)."""
    g = np.random.default_rng(seed)
    x, y = g.standard_normal((n1, 3)), g.standard_normal((n2, 3)) + 0.5
    M = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    M = (M / M.max()).astype(np.float32)
    a, b = g.random(n1) + 0.1, g.random(n2) + 0.1
    return M, (a / a.sum()).astype(np.float32), (b / b.sum()).astype(np.float32)


def yardstick_of_ref(a, b, M, reg, method, it, thr, warm=None):
    T, log = sinkhorn_ref(a, b, M, reg, method, it, thr, warm)
    assert fair(log["err"], log["niter"], it, thr, log["warn"]), (log["niter"], log["err"][-3:])
    return dict(M=M, a=a, b=b, reg=reg, stopThr=thr, r64_T=T.numpy(), r64_err=np.array(log["err"]), r64_niter=log["niter"], r64_loss=log["loss"],
                r64_log_u=log["log_u"].numpy(), r64_log_v=log["log_v"].numpy(), r64_warn=log["warn"])


def check(y, T, loss, log_u, log_v, niter, flags, errs, tag=""):
    """The yardsticks of the module docstring; y is a fixture or yardstick_of_ref's dict, the rest what the kernel returned (numpy / ints)."""
    warn, thr, r64_err = str(y["r64_warn"]), float(y["stopThr"]), np.asarray(y["r64_err"], dtype=np.float64)
    assert niter == int(y["r64_niter"]), (tag, niter, int(y["r64_niter"]))
    assert flags & 3 == (1 if warn == "" else (2 if warn == "numerr" else 0)), (tag, flags, warn)
    n = len(r64_err)
    errs = np.asarray(errs, dtype=np.float64)
    print(f"{tag}: niter {niter} flags {flags} errs {errs[:n][-2:]} r64 {r64_err[-2:]}")
    assert np.all(np.abs(errs[:n] - r64_err) <= 2e-3 * np.abs(r64_err) + 1e-3 * thr), (tag, errs[:n], r64_err)
    assert np.isnan(errs[n:]).all(), (tag, errs)
    r64 = rel(T, y["r64_T"])
    same_counts = "r32_T" in y and int(y["r32_niter"]) == int(y["r64_niter"]) and len(y["r32_err"]) == n
    if same_counts:
        r32, base = rel(T, y["r32_T"]), rel(y["r32_T"], y["r64_T"])
        print(f"{tag}: rel(T, r32) {r32:.2e} rel(T, r64) {r64:.2e} rel(r32, r64) {base:.2e}")
        assert r32 <= 1e-4 or r64 <= base, (tag, r32, r64, base)
    else:
        print(f"{tag}: rel(T, r64) {r64:.2e}")
        assert r64 <= 1e-4, (tag, r64)
    assert not np.isnan(T).any()
    el = abs(float(loss) - float(y["r64_loss"])) / abs(float(y["r64_loss"]))
    ma, mb = np.asarray(y["a"]) > 0, np.asarray(y["b"]) > 0
    with np.errstate(invalid="ignore"):                                   # (-inf - -inf on massless entries, masked out)
        du, dv = np.abs(log_u - y["r64_log_u"])[ma].max(), np.abs(log_v - y["r64_log_v"])[mb].max()
    Mr = -np.asarray(y["M"], dtype=np.float64) / float(y["reg"])
    with np.errstate(all="ignore"):
        rt = rel(np.exp(log_u.astype(np.float64)[:, None] + Mr + log_v.astype(np.float64)[None, :]), T)
    print(f"{tag}: loss rel {el:.2e} log_u {du:.2e} log_v {dv:.2e} exp(log_u + Mr + log_v) vs T {rt:.2e}")
    assert el <= 1e-4 and du <= 1e-4 and dv <= 1e-4, (tag, el, du, dv)
    assert rt <= 1e-5, (tag, rt)


def solve_one(M, a, b, reg, method, it, thr, warm=None):
    """B = 1 through ops.sinkhorn_batched in the problem's own container -> the six outputs as torch tensors without the batch axis."""
    w = None if warm is None else (gpu(warm[0])[None], gpu(warm[1])[None])
    out = ops.sinkhorn_batched(gpu(M)[None], None if a is None else gpu(a)[None], None if b is None else gpu(b)[None], reg=reg, method=method,
                               num_iter_max=it, stop_thr=thr, warmstart=w)
    return tuple(o[0] for o in out)


def as_numpy(out):
    T, loss, lu, lv, info, errs = (o.cpu().numpy() for o in out)
    return T, float(loss), lu, lv, int(info[0]), int(info[1]), errs


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_the_op(name):
    f = load(name)
    warm = (f["warm_u"], f["warm_v"]) if "warm_u" in f else None
    out = solve_one(f["M"], f["a"], f["b"], float(f["reg"]), str(f["method"]), int(f["numItermax"]), float(f["stopThr"]), warm)
    assert int(out[4][2]) == len(f["r64_err"]) and int(out[4][3]) == 0
    check(f, *as_numpy(out), tag=name)
    if name.startswith("zeroa"):
        assert not out[0][3].any() and out[2][3] == -np.inf                # a massless row: exactly zero, potential -inf


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_the_public_function(name):
    f = load(name)
    warm = (gpu(f["warm_u"]), gpu(f["warm_v"])) if "warm_u" in f else None
    method, it, thr = str(f["method"]), int(f["numItermax"]), float(f["stopThr"])
    a, b, M = gpu(f["a"]), gpu(f["b"]), gpu(f["M"])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        T, log = sk.sinkhorn(a, b, M, float(f["reg"]), method=method, numItermax=it, stopThr=thr, log=True, warmstart=warm)
    msgs = [str(x.message) for x in w]
    want = {"": [], "noconv": [_NOCONV], "numerr": ["Warning: numerical errors at iteration 0"]}[str(f["r64_warn"])]
    assert msgs == want
    assert set(log) == ({"err", "niter", "log_u", "log_v", "u", "v"} if method == "sinkhorn_log" else {"err", "niter", "u", "v"})
    assert isinstance(log["niter"], int) and isinstance(log["err"], list) and len(log["err"]) == len(f["r64_err"])
    lu, lv = torch.log(log["u"]), torch.log(log["v"])
    if method == "sinkhorn_log":
        lu, lv = log["log_u"], log["log_v"]
        assert torch.equal(log["u"], torch.exp(lu)) and torch.equal(log["v"], torch.exp(lv))
    # the same launch as the op: the same bits
    ref = solve_one(f["M"], f["a"], f["b"], float(f["reg"]), method, it, thr, None if warm is None else (f["warm_u"], f["warm_v"]))
    assert torch.equal(bits(T), bits(ref[0])) and log["niter"] == int(ref[4][0])
    assert torch.equal(bits(torch.stack(log["err"])) if log["err"] else torch.zeros(0, dtype=torch.int32), bits(ref[5][:len(log["err"])]))
    if method == "sinkhorn_log":
        assert torch.equal(bits(lu), bits(ref[2])) and torch.equal(bits(lv), bits(ref[3]))
    errs = np.full(ref[5].shape, np.nan)
    errs[:len(log["err"])] = [float(e) for e in log["err"]]
    flags = int(ref[4][1])
    if method == "sinkhorn_log":
        check(f, T.cpu().numpy(), float((M * T).sum()), lu.cpu().numpy(), lv.cpu().numpy(), log["niter"], flags, errs, tag=name)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cost, log2 = sk.sinkhorn2(a, b, M, float(f["reg"]), method=method, numItermax=it, stopThr=thr, log=True, warn=True, warmstart=warm)
        direct = (sk.sinkhorn_log if method == "sinkhorn_log" else sk.sinkhorn_knopp)(a, b, M, float(f["reg"]), numItermax=it, stopThr=thr, warn=False,
                                                                                       warmstart=warm)
    assert [str(x.message) for x in w] == want + [m for m in want if "numerical" in m]      # warn=False silences only "did not converge"
    assert cost.dim() == 0 and torch.equal(bits(cost), bits(ref[1])) and log2["niter"] == log["niter"] and torch.equal(bits(direct), bits(T))


@pytest.mark.parametrize("method", ["sinkhorn_log", "sinkhorn"])
def test_batching_is_bit_identical(method):
    tag = "log" if method == "sinkhorn_log" else "knopp"
    fs = [load(f"{c}_{tag}") for c in CASES]
    order = np.random.default_rng(3).permutation(len(fs))
    fs = [fs[i] for i in order]
    kw = dict(reg=0.05, method=method, num_iter_max=100, stop_thr=1e-5)
    Ms, as_, bs = [gpu(f["M"]) for f in fs], [gpu(f["a"]) for f in fs], [gpu(f["b"]) for f in fs]
    N1, N2 = 261, 259                                                      # larger than the largest problem in both directions (streamed)
    assert not _lib.lib().conan_sinkhorn_lds_resident(N1, N2)
    M, a, b, _w, n1, n2, sizes = ops._sinkhorn_list_stack(Ms, as_, bs, None, (N1, N2))
    full = ops.sinkhorn_batched(M, a, b, n1=n1, n2=n2, **kw)
    again = ops.sinkhorn_batched(M, a, b, n1=n1, n2=n2, **kw)
    for x, y in zip(full, again):
        assert torch.equal(bits(x), bits(y)) if x.dtype == torch.float32 else torch.equal(x, y)
    lists = ops.sinkhorn_list(Ms, as_, bs, container=(N1, N2), **kw)
    T, loss, lu, lv, info, errs = full
    for k, (m1, m2) in enumerate(sizes):
        one = solve_one(fs[k]["M"], fs[k]["a"], fs[k]["b"], 0.05, method, 100, 1e-5)
        assert torch.equal(bits(T[k, :m1, :m2]), bits(one[0])), (k, sizes[k])
        assert torch.equal(bits(lists[0][k]), bits(one[0])) and torch.equal(bits(lists[2][k]), bits(one[2])) and torch.equal(bits(lists[3][k]), bits(one[3]))
        assert torch.equal(bits(loss[k]), bits(one[1])) and torch.equal(bits(lu[k, :m1]), bits(one[2])) and torch.equal(bits(lv[k, :m2]), bits(one[3]))
        assert torch.equal(info[k].cpu(), one[4].cpu()) and torch.equal(bits(errs[k]), bits(one[5])), (k, info[k], one[4])
        assert not T[k, m1:].any() and not T[k, :, m2:].any() and not lu[k, m1:].any() and not lv[k, m2:].any()
        assert not bits(T[k, m1:]).any() and not bits(T[k, :, m2:]).any() and not bits(lu[k, m1:]).any() and not bits(lv[k, m2:]).any()
    assert len(set(int(i) for i in info[:, 0].cpu())) > 1                  # the batch really mixes iteration counts


def test_shared_cost_matrix_stride_zero():
    M, a, _ = problem(33, 40, 11)
    bsets = np.stack([problem(33, 40, 20 + k)[2] for k in range(3)])
    for method in ("sinkhorn_log", "sinkhorn"):
        kw = dict(reg=0.05, method=method, num_iter_max=100, stop_thr=1e-5)
        shared = ops.sinkhorn_batched(gpu(M), None, gpu(bsets), **kw)
        assert shared[0].shape == (3, 33, 40)
        for k in range(3):
            one = solve_one(M, None, bsets[k], 0.05, method, 100, 1e-5)
            for x, y in zip(shared, one):
                assert torch.equal(bits(x[k]), bits(y))
        assert not torch.equal(shared[0][0], shared[0][1])


@pytest.mark.parametrize("method", ["sinkhorn_log", "sinkhorn"])
def test_streamed_path_beside_the_residency_limit(method):
    L = _lib.lib()
    n1, n2 = 64, 290
    assert L.conan_sinkhorn_lds_resident(n1, n2) == 1
    while L.conan_sinkhorn_lds_resident(n1, n2 + 1):
        n2 += 1
    shapes = [(n1, n2), (n1, n2 + 1)]                                      # the largest resident shape and the smallest streamed one beside it
    assert 290 < n2 < 320 and not L.conan_sinkhorn_lds_resident(*shapes[1])
    reg, it, thr = float(np.float32(0.05)), 100, 1e-5
    probs = [problem(*s, seed=1) for s in shapes]
    Ts, loss, lus, lvs, info, errs = ops.sinkhorn_list([gpu(p[0]) for p in probs], [gpu(p[1]) for p in probs], [gpu(p[2]) for p in probs],
                                                       reg=reg, method=method, num_iter_max=it, stop_thr=thr)      # container 64 x (n2 + 1): streamed
    for k, (M, a, b) in enumerate(probs):
        y = yardstick_of_ref(a, b, M, reg, method, it, thr)
        check(y, Ts[k].cpu().numpy(), float(loss[k]), lus[k].cpu().numpy(), lvs[k].cpu().numpy(), int(info[k, 0]), int(info[k, 1]), errs[k].cpu().numpy(),
              tag=f"streamed {shapes[k]}")
    one = solve_one(*probs[0], reg, method, it, thr)                       # the resident launch of the resident shape: the same bits
    assert torch.equal(bits(one[0]), bits(Ts[0])) and torch.equal(bits(one[5]), bits(errs[0])) and torch.equal(bits(one[1]), bits(loss[0]))


def test_exact_log_domain_path():
    """A row of M at 900 reg: relative to its columns' largest entries the row underflows fp64, its row sum is zero, and the problem must take the
    exact log-domain iteration (flag bit 2) and still give the log-domain result."""
    reg, it, thr = float(np.float32(0.1)), 100, 1e-5
    M, a, b = problem(9, 11, 0)
    M[4, :] = np.float32(900.0 * reg)
    y = yardstick_of_ref(a, b, M, reg, "sinkhorn_log", it, thr)
    out = solve_one(M, a, b, reg, "sinkhorn_log", it, thr)
    assert int(out[4][1]) & 4
    check(y, *as_numpy(out), tag="exact path")
    regular = solve_one(*problem(9, 11, 0), reg, "sinkhorn_log", it, thr)
    assert not int(regular[4][1]) & 4


def test_rectangular_is_native():
    """7 x 12 solved directly equals the same problem embedded in 12 x 12 with five massless rows.  Run to the end of the loop (the fp32 marginals'
    sums differ by more than 1e-9, so neither reaches stopThr: the restatement is asserted to agree): both sit at the fixed point."""
    reg, it, thr = float(np.float32(0.1)), 1000, 1e-9
    M, a, b = problem(7, 12, 0)
    Me, ae = np.zeros((12, 12), np.float32), np.zeros(12, np.float32)
    Me[:7], ae[:7] = M, a
    r1, r2 = yardstick_of_ref(a, b, M, reg, "sinkhorn_log", it, thr), yardstick_of_ref(ae, b, Me, reg, "sinkhorn_log", it, thr)
    assert r1["r64_niter"] == r2["r64_niter"]
    direct, emb = solve_one(M, a, b, reg, "sinkhorn_log", it, thr), solve_one(Me, ae, b, reg, "sinkhorn_log", it, thr)
    assert int(direct[4][0]) == int(emb[4][0]) == r1["r64_niter"]
    assert rel(emb[0][:7].cpu().numpy(), direct[0].cpu().numpy()) <= 1e-6
    assert not emb[0][7:].any()
    assert rel(direct[0].cpu().numpy(), r1["r64_T"]) <= 1e-6


def test_no_host_synchronisation():
    M, a, b = problem(33, 40, 5)
    Mg, ag, bg = gpu(np.stack([M, M.copy()])), gpu(np.stack([a, a])), gpu(np.stack([b, b]))
    n1 = torch.tensor([33, 20], dtype=torch.int32, device=DEV)
    Mq = Mg.clone().requires_grad_(True)
    gout = torch.rand(2, device=DEV)
    kw = dict(reg=0.05, num_iter_max=100, stop_thr=1e-5)
    ops.sinkhorn_batched(Mg, ag, bg, n1=n1, **kw)                          # (first call: library load, allocator warm-up)
    ops.sinkhorn_loss(Mq, ag, bg, **kw).backward(gout)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for method in ("sinkhorn_log", "sinkhorn"):
            ops.sinkhorn_batched(Mg, ag, bg, n1=n1, method=method, **kw)
            ops.sinkhorn_loss(Mq, ag, bg, method=method, **kw).backward(gout)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(Mq.grad).all()


def test_gradient_is_the_fixed_plan():
    M, a, b = problem(20, 25, 8)
    Mg, ag, bg = gpu(M).requires_grad_(True), gpu(a).requires_grad_(True), gpu(b).requires_grad_(True)
    cost = sk.sinkhorn2(ag, bg, Mg, 0.05, method="sinkhorn_log", numItermax=100, stopThr=1e-5)
    assert cost.requires_grad and cost.dim() == 0
    cost.backward()
    T = sk.sinkhorn(ag, bg, Mg, 0.05, method="sinkhorn_log", numItermax=100, stopThr=1e-5)
    assert not T.requires_grad
    assert torch.equal(bits(Mg.grad), bits(T)) and ag.grad is None and bg.grad is None
    assert torch.equal(bits(cost.detach()), bits(solve_one(M, a, b, 0.05, "sinkhorn_log", 100, 1e-5)[1]))
    # the batched loss with a random upstream gradient, ragged sizes inside one container
    Mb = gpu(np.stack([problem(20, 25, 8 + k)[0] for k in range(3)])).requires_grad_(True)
    n1, n2 = torch.tensor([20, 7, 13], dtype=torch.int32, device=DEV), torch.tensor([25, 25, 9], dtype=torch.int32, device=DEV)
    loss, T, *_ = ops.sinkhorn_loss(Mb, reg=0.05, method="sinkhorn", num_iter_max=100, stop_thr=1e-5, n1=n1, n2=n2, return_plan=True)
    gout = torch.rand(3, device=DEV) + 0.5
    loss.backward(gout)
    assert torch.equal(bits(Mb.grad), bits(gout[:, None, None] * T)) and not Mb.grad[1, 7:].any() and Mb.grad[1, :7].any()
    with pytest.raises(RuntimeError):                                      # no double backward
        x = gpu(M).requires_grad_(True)
        (g,) = torch.autograd.grad(ops.sinkhorn_loss(x[None], reg=0.05).sum(), x, create_graph=True)
        g.sum().backward()


def clouds(sizes, d=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(0.4 * torch.randn(n, d, generator=g)).to(DEV) for n in sizes]


@pytest.mark.parametrize("sizes", [(5, 7, 7, 12, 33), (9, 9, 9, 9)])
def test_wasserstein_pairwise_distances(sizes):
    Ys = clouds(sizes)
    g = torch.Generator().manual_seed(1)
    ps = [torch.rand(n, generator=g) + 0.1 for n in sizes]
    ps = [(p / p.sum()).to(DEV) for p in ps]
    for weights, method in ((ps, "sinkhorn_log"), (None, "sinkhorn")):
        D = sk.wasserstein_pairwise_distances(Ys, weights, reg=0.1, method=method, numItermax=100, stopThr=1e-5)
        G = len(sizes)
        assert D.shape == (G, G) and torch.equal(D, D.T) and not D.diagonal().any() and not D.requires_grad
        for i in range(G):
            for j in range(i + 1, G):
                M = feature_cost(Ys[i], Ys[j])
                one = sk.sinkhorn2(None if weights is None else weights[i], None if weights is None else weights[j], M, 0.1, method=method,
                                   numItermax=100, stopThr=1e-5)
                assert torch.equal(bits(D[i, j]), bits(one)), (i, j, float(D[i, j]), float(one))
        assert (D[~torch.eye(G, dtype=torch.bool, device=DEV)] > 0).all()
    # gradients: sinkhorn2's fixed plan into every M, torch's through feature_cost
    Yq = [y.clone() for y in Ys]
    Yq[0].requires_grad_(True)
    D = sk.wasserstein_pairwise_distances(Yq, ps, reg=0.1, numItermax=100, stopThr=1e-5)
    w = torch.rand(len(sizes), len(sizes), generator=torch.Generator().manual_seed(2)).to(DEV)
    (D * w).sum().backward()
    got = Yq[0].grad
    assert torch.isfinite(got).all() and got.abs().max() > 0
    y0 = Ys[0].clone().requires_grad_(True)
    total = 0.0
    for j in range(1, len(sizes)):
        M = feature_cost(y0, Ys[j])
        T = sk.sinkhorn(ps[0], ps[j], M.detach(), 0.1, numItermax=100, stopThr=1e-5, warn=False)
        total = total + (w[0, j] + w[j, 0]) * (M * T).sum()
    total.backward()
    assert rel(got.cpu().numpy(), y0.grad.cpu().numpy()) <= 1e-5


def test_bad_arguments_through_ctypes():
    L = _lib.lib()
    B, N1, N2 = 2, 6, 5
    M, T = torch.rand(B, N1, N2, device=DEV), torch.full((B, N1, N2), 7.0, device=DEV)
    ws = torch.empty(int(L.conan_sinkhorn_workspace_bytes(B, N1, N2)), dtype=torch.uint8, device=DEV)
    good = dict(M=M.data_ptr(), B=B, N1=N1, N2=N2, stride=N1 * N2, reg=0.1, method=0, it=10, T=T.data_ptr(), ws=ws.data_ptr())

    def rc(**kw):
        a = dict(good, **kw)
        return L.conan_sinkhorn_fwd(a["M"], None, None, None, None, None, None, a["B"], a["N1"], a["N2"], a["stride"], a["reg"], a["method"], a["it"],
                                    1e-5, a["T"], None, None, None, None, None, a["ws"], _lib.stream_ptr())

    for kw in (dict(M=None), dict(T=None), dict(ws=None), dict(B=0), dict(B=-1), dict(N1=0), dict(N2=0), dict(it=0), dict(it=-5), dict(reg=0.0),
               dict(reg=-0.1), dict(reg=float("inf")), dict(reg=float("nan")), dict(method=2), dict(method=-1), dict(stride=-1)):
        assert rc(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (T == 7.0).all()                                                # refused before any launch
    assert rc() == 0                                                       # every output but T may be null
    torch.cuda.synchronize()
    assert abs(float(T.sum()) - B) < 1e-4
