"""The unrolled FGWMixup gradient on the GPU (csrc/fgw_acc_grad.hip: conan_fgw_acc_pair_bwd, conan_fgw_acc_pair_bwd_workspace_bytes,
conan_fgw_acc_pair_bwd_lds_resident, through ops.fgw_acc_pair_unrolled, fgw.fused_ACC_unrolled and fgw.fgw_mixup_distance_unrolled).

Yardsticks: torch autograd through the reference's own fused_ACC_torch in fp64 on the same fp32 inputs (tests/golden/grad_acc_*.npz: gX =
gradients of sum(W * X), gd = of the FGWMixup distance) and, where no fixture exists, the fp64 restatement tests/fgw_acc_grad_ref.py (held to
every fixture to 1e-9 by tests/test_fgw_acc_grad_cpu.py).

The bound on every gradient is 1e-6 (fgw_acc_grad_ref.grad_error: the Frobenius norm of the difference over that of the yardstick).  It is
derived, not measured: the inputs are the same fp32 values, the kernel iterates in fp64, so what remains is one fp32 rounding per output entry
(6e-8 relative), and the CPU test caps what reordering fp64 sums can add at 1e-9.  At a node without mass the gradient is exactly 0."""
import os

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, fgw, ops

from fgw_acc_grad_ref import acc_grad_ref, grad_error

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["1x5", "5x7", "5x7_stop", "12x9_directed", "7x7_start", "9x11_zeroa", "33x33", "62x62"]
DEV = "cuda"
TOL = 1e-6
KEYS = ("dM", "dA", "dB", "da", "db", "dX0")
_CACHE = {}


def load(name):
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"grad_acc_{name}.npz"))
        _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


def gpu(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def params(f):
    return dict(alpha=float(f["alpha"]), rho=float(f["rho"]), epoch=int(f["epoch"]), eps=float(f["eps"]))


def leaves(f, grad=True):
    """The fixture's inputs on the GPU, in KEYS' order; None where the fixture has none (uniform weights, no start)."""
    return [gpu(f[k]).requires_grad_(grad) if k in f else None for k in ("M", "A", "B", "a", "b", "X0")]


def one(t):
    return None if t is None else t[None]


def solve(f, ins):
    return ops.fgw_acc_pair_unrolled(*(one(t) for t in ins), **params(f))


def grads_of(obj, ins):
    """The gradients of one objective as fp64 numpy arrays by KEYS (None where there is no leaf)."""
    have = [t for t in ins if t is not None]
    gs = iter(torch.autograd.grad(obj, have, retain_graph=True, allow_unused=True))
    return {k: (None if t is None else next(gs).cpu().numpy().astype(np.float64)) for k, t in zip(KEYS, ins)}


def check(got, f, tags, cot, label):
    """got against the sum of the fixture's gradients of the objectives `tags` (added on the host in fp64): <= TOL each."""
    for k in KEYS:
        if got[k] is None:
            continue
        want = sum(f[f"{t}_{k}"].astype(np.float64) for t in tags)
        e = grad_error(got[k], want, cot)
        print(f"{label} {'+'.join(tags)} {k}: {e:.2e}")
        assert e <= TOL, (label, tags, k, e)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_the_op(name):
    f = load(name)
    ins = leaves(f)
    X, dist, objs, info = solve(f, ins)
    # the comparison means something only at the reference's epoch count
    assert int(info[0, 0]) == int(f["epochs"]) and int(info[0, 1]) == int(f["stored"]) and int(info[0, 2]) == 0, (name, info.tolist())
    assert X.requires_grad and dist.requires_grad and not objs.requires_grad and not info.requires_grad
    assert grad_error(X.detach().cpu().numpy(), f["X"]) <= TOL and abs(float(dist[0].detach()) - float(f["dist"])) <= TOL * abs(float(f["dist"]))
    plain = [None if t is None else t.detach() for t in ins]
    Xp, objs_p, info_p = ops.fgw_acc_pair_batched(*(one(t) for t in plain), **params(f))
    dist_p = ops.fgw_acc_pair_distance(*(one(t) for t in plain), **params(f))
    assert torch.equal(bits(X), bits(Xp)) and torch.equal(bits(objs), bits(objs_p)) and torch.equal(info, info_p) and torch.equal(bits(dist), bits(dist_p))
    W = gpu(f["W"])
    check(grads_of((W * X[0]).sum(), ins), f, ("gX",), f["W"], name)              # the plan's cotangent alone
    check(grads_of(dist[0], ins), f, ("gd",), 1.0, name)                          # the distance's alone
    check(grads_of((W * X[0]).sum() + dist[0], ins), f, ("gX", "gd"), f["W"], name)      # both in ONE backward launch (cotangents W and 1: fp32 inputs)
    if name == "9x11_zeroa":
        g = grads_of((W * X[0]).sum() + dist[0], ins)
        assert not g["dM"][3].any() and not g["dA"][3].any() and not g["dA"][:, 3].any() and g["da"][3] == 0.0 and not X[0, 3].any()
        assert all(np.isfinite(v).all() for v in g.values() if v is not None) and g["dM"].any() and g["da"].any()


@pytest.mark.parametrize("name", ["5x7", "7x7_start", "33x33", "62x62"])
def test_replay_retraces_the_forward_bit_for_bit(name):
    """conan_fgw_acc_pair_bwd through ctypes on the prepared operands: X_chk, the replay's final X, is conan_fgw_acc_pair_fwd's X."""
    f = load(name)
    L = _lib.lib()
    p = params(f)
    M, A, Bm, a, b, X0, (B, N, N1, N2) = ops._acc_prepare(*(one(t) for t in leaves(f, False)), None, None)
    X, objs, info = ops._acc_fwd(M, A, Bm, a, b, X0, B, N, p["alpha"], p["rho"], p["epoch"], p["eps"])
    assert bool(L.conan_fgw_acc_pair_bwd_lds_resident(N)) == (name != "62x62")                  # 62: the streamed path
    ws = torch.empty(int(L.conan_fgw_acc_pair_bwd_workspace_bytes(B, N, p["epoch"])), dtype=torch.uint8, device=DEV)
    dM, dA, dBm, chk = (torch.full((B, N, N), 7.0, device=DEV) for _ in range(4))
    dd = torch.ones(B, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = L.conan_fgw_acc_pair_bwd(ptr(M), ptr(A), ptr(Bm), ptr(a), ptr(b), ptr(X0), B, N, p["alpha"], p["rho"], p["epoch"], ptr(info), None, ptr(dd),
                                  ptr(dM), ptr(dA), ptr(dBm), None, None, None, ptr(chk), ptr(ws), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(bits(chk), bits(X))
    check(dict(dM=dM[0, :N1, :N2].cpu().numpy(), dA=dA[0, :N1, :N1].cpu().numpy(), dB=dBm[0, :N2, :N2].cpu().numpy(), da=None, db=None, dX0=None),
          f, ("gd",), 1.0, name + " ctypes")
    bad = L.conan_fgw_acc_pair_bwd(ptr(M), ptr(A), ptr(Bm), ptr(a), ptr(b), ptr(X0), B, N, p["alpha"], p["rho"], p["epoch"], ptr(info), None, None,
                                   ptr(dM), ptr(dA), ptr(dBm), None, None, None, ptr(chk), ptr(ws), _lib.stream_ptr())
    assert bad == -1                                                        # both cotangents null


def test_unrolled_differs_from_the_fixed_plan():
    f = load("5x7_stop")
    ins = leaves(f)
    X, dist, _objs, _info = solve(f, ins)
    unrolled = grads_of(dist[0], ins)["dM"]
    fixed_ins = leaves(f)
    fixed = grads_of(ops.fgw_acc_pair_distance(*(one(t) for t in fixed_ins), **params(f))[0], fixed_ins)["dM"]
    d = grad_error(unrolled, fixed)
    print(f"dM of the distance, unrolled against fixed-plan: {d:.3f}")
    assert d > 1e-3
    assert grad_error(fixed, (1 - float(f["alpha"])) * X[0].detach().cpu().numpy()) <= TOL


def problem(n1, n2, seed):
    """The fixtures' construction (make_fgw_mixup_golden.pair_inputs): squared feature distances, undirected 0 / 1 graphs, random weights."""
    rng = np.random.RandomState(seed)
    y, z = rng.uniform(0.1, 1.5, size=(n1, 4)), rng.uniform(0.1, 1.5, size=(n2, 4))
    M = ((y[:, None] - z[None]) ** 2).sum(-1).astype(np.float32)

    def graph(n):
        g = np.triu(rng.random_sample((n, n)) < 0.4, 1)
        return (g | g.T).astype(np.float32)
    a, b = rng.uniform(0.5, 1.5, n1), rng.uniform(0.5, 1.5, n2)
    return M, graph(n1), graph(n2), (a / a.sum()).astype(np.float32), (b / b.sum()).astype(np.float32)


def container(probs, N1, N2):
    """The problems zero-padded into [B,N1,N2] containers with their own sizes -> leaves M, A, Bm, a, b and n1, n2."""
    B = len(probs)
    shapes = ((B, N1, N2), (B, N1, N1), (B, N2, N2), (B, N1), (B, N2))
    out = [torch.zeros(s, device=DEV) for s in shapes]
    for k, p in enumerate(probs):
        for t, v in zip(out, p):
            t[(k,) + tuple(slice(0, n) for n in v.shape)] = gpu(v)
    n1 = torch.tensor([p[0].shape[0] for p in probs], dtype=torch.int32, device=DEV)
    n2 = torch.tensor([p[0].shape[1] for p in probs], dtype=torch.int32, device=DEV)
    return [t.requires_grad_(True) for t in out], n1, n2


def test_own_sizes_in_one_container_alone_and_batched():
    sizes = [(5, 7), (12, 9), (9, 11)]
    probs = [problem(n1, n2, 40 + k) for k, (n1, n2) in enumerate(sizes)]
    Ws = [np.random.default_rng(60 + k).standard_normal(s).astype(np.float32) for k, s in enumerate(sizes)]
    gd = np.array([0.7, 1.1, 1.6], dtype=np.float32)
    kw = dict(alpha=0.5, rho=0.3, epoch=60, eps=1e-5)
    N1, N2 = 12, 11

    def run(idx):
        ins, n1, n2 = container([probs[k] for k in idx], N1, N2)
        X, dist, objs, info = ops.fgw_acc_pair_unrolled(*ins, n1=n1, n2=n2, **kw)
        W = torch.zeros(len(idx), N1, N2, device=DEV)
        for q, k in enumerate(idx):
            W[q, :sizes[k][0], :sizes[k][1]] = gpu(Ws[k])
        gs = torch.autograd.grad([X, dist], ins, [W, gpu(gd[list(idx)])])
        return X, dist, info, gs

    X, dist, info, gs = run((0, 1, 2))
    for k, (n1, n2) in enumerate(sizes):
        Xk, distk, infok, gk = run((k,))                                   # the same pair alone in the same container
        assert torch.equal(bits(Xk[0]), bits(X[k])) and torch.equal(bits(distk[0]), bits(dist[k])) and torch.equal(infok[0], info[k])
        for x, y in zip(gk, gs):
            assert torch.equal(bits(x[0]), bits(y[k])), k
        dM, dA, dB, da, db = (g[k].cpu().numpy() for g in gs)
        assert not dM[n1:].any() and not dM[:, n2:].any() and not dA[n1:].any() and not dA[:, n1:].any() and not dB[n2:].any() and not dB[:, n2:].any()
        assert not da[n1:].any() and not db[n2:].any() and not bits(X[k, n1:]).any() and not bits(X[k, :, n2:]).any()
        M, A, Bm, a, b = probs[k]
        r = acc_grad_ref(M, A, Bm, a, b, None, alpha=kw["alpha"], rho=kw["rho"], epochs=int(info[k, 0]), dX=Ws[k], ddist=float(gd[k]))
        assert int(info[k, 2]) == 0 and grad_error(X[k, :n1, :n2].detach().cpu().numpy(), r["X"]) <= TOL
        for name, got, want in (("dM", dM[:n1, :n2], r["dM"]), ("dA", dA[:n1, :n1], r["dA"]), ("dBm", dB[:n2, :n2], r["dBm"]), ("da", da[:n1], r["da"]),
                                ("db", db[:n2], r["db"])):
            e = grad_error(got, want, Ws[k])
            print(f"pair {k} {sizes[k]} epochs {int(info[k, 0])} {name}: {e:.2e}")
            assert e <= TOL, (k, name, e)


def test_partial_leaves_and_launch_counts():
    f = load("12x9_directed")
    calls = []

    def trace(name, fn, args):
        calls.append(name)
        return fn(*args)

    prev = _lib.set_call_trace(trace)
    try:
        ins = leaves(f, False)
        X, dist, _objs, _info = solve(f, ins)                              # no leaf: nothing saved, nothing beyond the two forward launches
        assert not X.requires_grad and not dist.requires_grad and X.grad_fn is None
        assert calls == ["conan_fgw_acc_pair_fwd", "conan_fgw_pair_dist"], calls
        ins[0].requires_grad_(True)                                        # only M
        del calls[:]
        X, dist, _objs, _info = solve(f, ins)
        ((gpu(f["W"]) * X[0]).sum() + dist[0]).backward()                  # one backward(): exactly one launch, for both cotangents
        assert calls.count("conan_fgw_acc_pair_bwd") == 1 and calls.count("conan_fgw_acc_pair_fwd") == 1, calls
        assert "conan_fgw_pair_dist_bwd" not in calls
    finally:
        _lib.set_call_trace(prev)
    assert ins[0].grad is not None and all(t.grad is None for t in ins[1:] if t is not None)
    want = f["gX_dM"] + f["gd_dM"]
    assert grad_error(ins[0].grad.cpu().numpy(), want, f["W"]) <= TOL
    with torch.no_grad():                                                  # grad mode off: the plain path too
        ins = leaves(f)
        assert not solve(f, ins)[0].requires_grad
    with pytest.raises(RuntimeError):                                      # no double backward
        x = gpu(f["M"]).requires_grad_(True)
        (g,) = torch.autograd.grad(ops.fgw_acc_pair_unrolled(x[None], gpu(f["A"])[None], gpu(f["B"])[None], **params(f))[1].sum(), x, create_graph=True)
        g.sum().backward()


def test_a_flagged_pair_gets_nan_gradients():
    """exp underflow at a tiny rho: every row sum of the first half-step is zero, the forward raises flags bit 2 and returns the reference's NaN;
    the reference's autograd gives NaN gradients, and so does the kernel, beside a healthy pair of the same batch that keeps its numbers."""
    M, A, Bm, a, b = problem(5, 7, 3)
    Ms = gpu(np.stack([M, M * 1.0e5])).requires_grad_(True)
    rest = [gpu(np.stack([v, v])).requires_grad_(True) for v in (A, Bm, a, b)]
    X, dist, _objs, info = ops.fgw_acc_pair_unrolled(Ms, *rest, alpha=0.5, rho=0.5, epoch=12)
    assert int(info[0, 2]) == 0 and int(info[1, 2]) & 4 and torch.isnan(X[1]).all()
    gs = torch.autograd.grad([X, dist], [Ms] + rest, [torch.ones_like(X), torch.ones_like(dist)])
    for g in gs:
        assert torch.isfinite(g[0]).all() and g[0].any() and torch.isnan(g[1]).all()


def test_public_functions():
    f = load("12x9_directed")
    M, A, B, a, b, _ = leaves(f)
    p = params(f)
    X, obj_list = fgw.fused_ACC_unrolled(M, A, B, a, b, alpha=p["alpha"], epoch=p["epoch"], eps=p["eps"], rho=p["rho"])
    Xt, obj_t = fgw.fused_ACC_torch(M.detach(), A.detach(), B.detach(), a.detach(), b.detach(), alpha=p["alpha"], epoch=p["epoch"], eps=p["eps"], rho=p["rho"])
    assert X.requires_grad and not Xt.requires_grad and torch.equal(bits(X), bits(Xt)) and len(obj_list) == len(obj_t) == int(f["stored"])
    assert all(not o.requires_grad and torch.equal(bits(o), bits(q)) for o, q in zip(obj_list, obj_t))
    check(grads_of((gpu(f["W"]) * X).sum(), [M, A, B, a, b, None]), f, ("gX",), f["W"], "fused_ACC_unrolled")

    f = load("5x7_stop")
    M, A, B, a, b, _ = leaves(f)
    p = params(f)
    kw = dict(alpha=p["alpha"], epoch=p["epoch"], eps=p["eps"], rho=p["rho"])
    dist, log = fgw.fgw_mixup_distance_unrolled(M, A, B, a, b, log=True, **kw)
    plain = fgw.fgw_mixup_distance(M.detach(), A.detach(), B.detach(), a.detach(), b.detach(), **kw)
    assert dist.dim() == 0 and dist.requires_grad and torch.equal(bits(dist), bits(plain)) and len(log["obj_list"]) == int(f["stored"])
    assert log["T"].requires_grad and torch.equal(bits(log["T"]), bits(fgw.fused_ACC_torch(M.detach(), A.detach(), B.detach(), a.detach(), b.detach(), **kw)[0]))
    check(grads_of(dist, [M, A, B, a, b, None]), f, ("gd",), 1.0, "fgw_mixup_distance_unrolled")
    f = load("7x7_start")                                                  # the start is an argument of the public form too, and a leaf
    ins = leaves(f)
    p = params(f)
    d2 = fgw.fgw_mixup_distance_unrolled(*ins, alpha=p["alpha"], epoch=p["epoch"], eps=p["eps"], rho=p["rho"])
    assert d2.dim() == 0
    check(grads_of(d2, ins), f, ("gd",), 1.0, "fgw_mixup_distance_unrolled with a start")
