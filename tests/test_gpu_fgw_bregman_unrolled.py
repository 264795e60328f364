"""The unrolled BAPG pairwise FGW gradient on the GPU (csrc/fgw_bregman_grad.hip: conan_fgw_bregman_bwd, conan_fgw_bregman_bwd_workspace_bytes,
conan_fgw_bregman_bwd_lds_resident, through ops.fgw_bregman_unrolled / fgw_bregman_unrolled_list, fgw.fgw_bregman_unrolled and
fgw.fgw_bregman_distance_unrolled).

Yardsticks: torch autograd through the reference's own fgw_bregman in fp64 on the same fp32 inputs (tests/golden/fgw_bregman_unrollgrad_*.npz:
gT = gradients of sum(W * T), gd = of log["fgw_dist"], gl = of log["loss"]) and, where no fixture exists, the fp64 restatement
tests/fgw_bregman_unrolled_ref.py (held to every fixture to 1e-9 by tests/test_fgw_bregman_unrolled_cpu.py).

The bound on every gradient is 1e-6 (grad_error: the Frobenius norm of the difference over that of the yardstick), the one
tests/test_gpu_fgw_pair_unrolled.py uses for the same output path: the inputs are the same fp32 values, the kernel replays the solve in fp64
on the caller's parameters for the iteration count the forward reports, so what remains is one fp32 rounding per output entry (6e-8 relative),
and the CPU test caps what reordering fp64 sums can add at 1e-9.  At a node without mass the gradient is exactly 0."""
import os
import warnings

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, fgw, ops

from fgw_bregman_unrolled_ref import grad_error, unrolled

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FINITE = ["n12", "rect_7x12", "dir_n12_false", "1x5", "n33", "n80", "kl_n10", "kl_dir_n12_false", "dir_n12_none", "undir_n12_none", "n10_g0", "eps002_n12",
          "stop_n12", "zerop_9x11"]
LOSS = ("n12", "kl_n10")
NAN = "nan_n10"
DEV = "cuda"
TOL = 1e-6
KEYS = ("dM", "dC1", "dC2", "dp", "dq", "dG0")
SYM = {1: True, 0: False, -1: None}
_CACHE = {}


def load(name):
    """The fixture (it holds the parameters) and the file that holds its inputs (a reused case: tests/golden/fgw_pair_<src>.npz)."""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"fgw_bregman_unrollgrad_{name}.npz"))
        f = {k: z[k] for k in z.files}
        src = str(f["src"])
        if src:
            z = np.load(os.path.join(GOLDEN, f"fgw_pair_{src}.npz"))
        _CACHE[name] = (f, {k: z[k] for k in z.files})
    return _CACHE[name]


def gpu(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def params(f):
    return dict(alpha=float(f["alpha"]), epsilon=float(f["epsilon"]), max_iter=int(f["max_iter"]), tol=float(f["tol"]), loss_fun=str(f["loss_fun"]),
                symmetric=SYM[int(f["symmetric"])])


def leaves(g, grad=True):
    """The inputs on the GPU, in KEYS' order; None where there is no start."""
    return [gpu(g[k]).requires_grad_(grad) if g[k].size else None for k in ("M", "C1", "C2", "p", "q", "G0")]


def one(t):
    return None if t is None else t[None]


def solve(f, ins, **over):
    return ops.fgw_bregman_unrolled(*(one(t) for t in ins), **dict(params(f), **over))


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


def raw_bwd(g, prm, dT, dd):
    """conan_fgw_bregman_bwd through ctypes on the prepared operands of one pair -> (gradients by KEYS, T_chk, binfo, forward outputs, N)."""
    L = _lib.lib()
    M, C1, C2, p, q, G0, (B, N, n1, n2) = ops._pair_prepare(*(one(t) for t in leaves(g, False)))
    fprm, solver_code, sym_code = ops._pair_params(prm["alpha"], prm["epsilon"], prm["max_iter"], prm["tol"], 1, 1e-9, prm["loss_fun"], "BAPG", prm["symmetric"])
    T, dist, info, errs = ops._pair_fwd(M, C1, C2, p, q, G0, B, N, fprm, solver_code, sym_code, True)
    nbytes = int(L.conan_fgw_bregman_bwd_workspace_bytes(B, N, prm["max_iter"]))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dM, dC1, dC2, chk = (torch.full((B, N, N), 7.0, device=DEV) for _ in range(4))
    dp, dq = (torch.full((B, N), 7.0, device=DEV) for _ in range(2))
    dG0 = torch.full((B, N, N), 7.0, device=DEV) if G0 is not None else None
    binfo = torch.full((B, 2), -1, dtype=torch.int32, device=DEV)
    pad = None
    if dT is not None:
        pad = torch.zeros(B, N, N, device=DEV)
        pad[0, :n1, :n2] = gpu(dT)
    ddt = None if dd is None else torch.full((B,), float(dd), device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = L.conan_fgw_bregman_bwd(ptr(M), ptr(C1), ptr(C2), ptr(p), ptr(q), ptr(G0), B, N, prm["alpha"], prm["epsilon"], prm["max_iter"],
                                 ops._LOSS_CODE[prm["loss_fun"]], sym_code, ptr(info), ptr(pad), ptr(ddt), ptr(dM), ptr(dC1), ptr(dC2), ptr(dp), ptr(dq),
                                 ptr(dG0), ptr(chk), ptr(binfo), ptr(ws), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    host = lambda t: t[0].cpu().numpy().astype(np.float64)
    got = dict(dM=host(dM)[:n1, :n2], dC1=host(dC1)[:n1, :n1], dC2=host(dC2)[:n2, :n2], dp=host(dp)[:n1], dq=host(dq)[:n2],
               dG0=None if dG0 is None else host(dG0)[:n1, :n2])
    return got, chk[0, :n1, :n2].cpu().numpy(), binfo[0].tolist(), (T[0, :n1, :n2], dist, info, errs), N


@pytest.mark.parametrize("name", FINITE)
def test_fixture_through_the_op(name):
    f, g = load(name)
    ins = leaves(g)
    T, dist, info, errs = solve(f, ins)
    # the comparison means something only at the reference's iteration count
    assert int(info[0, 0]) == int(f["iters"]) and int(info[0, 2]) == 0, (name, info.tolist(), errs.tolist())
    assert T.requires_grad and dist.requires_grad and not info.requires_grad and not errs.requires_grad
    plain = ops.fgw_pair_batched(*(one(None if t is None else t.detach()) for t in ins), solver="BAPG", **params(f))
    for a, b in zip((T, dist, info, errs), plain):                        # the forward is fgw_pair_batched's, bit for bit (errs: NaN where not run)
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
    W = gpu(f["W"])
    check(grads_of((W * T[0]).sum(), ins), f, ("gT",), f["W"], name)              # the plan's cotangent alone
    check(grads_of(dist[0], ins), f, ("gd",), 1.0, name)                          # the distance's alone
    both = grads_of((W * T[0]).sum() + dist[0], ins)                              # both in ONE backward launch (cotangents W and 1: fp32 inputs)
    check(both, f, ("gT", "gd"), f["W"], name)
    assert all(np.isfinite(v).all() for v in both.values() if v is not None)
    if name == "zerop_9x11":
        assert not both["dM"][3].any() and not both["dC1"][3].any() and not both["dC1"][:, 3].any() and both["dp"][3] == 0.0 and not T[0, 3].any()
        assert both["dM"].any() and both["dp"].any()


@pytest.mark.parametrize("name", FINITE)
def test_replay_counts_and_final_plan(name):
    """conan_fgw_bregman_bwd through ctypes: binfo carries the fixture's iteration count with the flags clear; T_chk, the replay's final plan,
    within TOL of the fixture's."""
    f, g = load(name)
    got, chk, binfo, (_T, _dist, info, _errs), N = raw_bwd(g, params(f), f["W"], 1.0)
    assert binfo == [int(f["iters"]), 0], (name, binfo, info.tolist())
    assert bool(_lib.lib().conan_fgw_bregman_bwd_lds_resident(N)) == (N <= 61)
    check(got, f, ("gT", "gd"), f["W"], name + " ctypes")
    e = grad_error(chk, f["T"])
    print(f"{name}: T_chk against the fp64 reference {e:.2e}")
    assert e <= TOL, (name, e)


def random_pair(n, seed, directed=False, positive=False):
    rng = np.random.RandomState(seed)
    y, z = rng.uniform(0.1, 1.2, size=(n, 3)), rng.uniform(0.1, 1.2, size=(n, 3))
    M = ((y[:, None] - z[None]) ** 2).sum(-1).astype(np.float32)

    def graph():
        if positive:
            c = rng.uniform(0.05, 1.0, size=(n, n))
            return (c if directed else 0.5 * (c + c.T)).astype(np.float32)
        a = rng.random_sample((n, n)) < 0.3
        a = (a & ~np.eye(n, dtype=bool)) if directed else (np.triu(a, 1) | np.triu(a, 1).T)
        return a.astype(np.float32)
    p, q = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    return dict(M=M, C1=graph(), C2=graph(), p=(p / p.sum()).astype(np.float32), q=(q / q.sum()).astype(np.float32), G0=np.zeros((0, 0), np.float32))


@pytest.mark.parametrize("loss_fun", ["square_loss", "kl_loss"])
@pytest.mark.parametrize("symmetric", [True, False])
def test_residency_bound_and_one_above(loss_fun, symmetric):
    """Random pairs at the largest LDS-resident size and one above it (the streamed path), 3 iterations, against the restatement; and the pair of
    the bound once more inside a container one larger (a massless node: the streamed path on the same problem) against its LDS-resident run."""
    L = _lib.lib()
    bound = max(n for n in range(1, 200) if L.conan_fgw_bregman_bwd_lds_resident(n))
    assert bound == 61 and not L.conan_fgw_bregman_bwd_lds_resident(bound + 1)
    prm = dict(alpha=0.5, epsilon=0.5, max_iter=3, tol=1e-12, loss_fun=loss_fun, symmetric=symmetric)
    gs, Ws = {}, {}
    for n in (bound, bound + 1):
        g = gs[n] = random_pair(n, 100 + n, directed=not symmetric, positive=loss_fun == "kl_loss")
        W = Ws[n] = np.random.default_rng(n).standard_normal((n, n)).astype(np.float32)
        got, chk, binfo, (_T, _dist, info, _errs), N = raw_bwd(g, prm, W, 0.8)
        r = unrolled(g["M"], g["C1"], g["C2"], g["p"], g["q"], None, alpha=0.5, epsilon=0.5, iters=3, loss_fun=loss_fun, symmetric=symmetric, dT=W, ddist=0.8)
        assert N == n and int(info[0, 0]) == 3 and binfo == [3, 0] and not r["flagged"]
        assert grad_error(chk, r["T"]) <= TOL
        for k in KEYS[:5]:
            e = grad_error(got[k], r[k], W)
            print(f"N {n} {loss_fun} symmetric {symmetric} {k}: {e:.2e}")
            assert e <= TOL, (n, k, e)
    # the same 61-node problem on both paths
    def run(idx):
        ins = [[gpu(gs[n][key]).requires_grad_(True) for n in idx] for key in ("M", "C1", "C2", "p", "q")]
        Ts, dist, _info, _errs = ops.fgw_bregman_unrolled_list(*ins, **prm)
        obj = (gpu(Ws[bound]) * Ts[0]).sum() + 0.8 * dist[0]
        return [x.cpu().numpy() for x in torch.autograd.grad(obj, [ts[0] for ts in ins])]
    resident, streamed = run((bound,)), run((bound, bound + 1))
    for k, a, b in zip(KEYS, resident, streamed):
        e = grad_error(b, a, Ws[bound])
        print(f"{loss_fun} symmetric {symmetric} {k}: streamed against resident {e:.2e}")
        assert e <= 2.0 ** -23, (k, e)                                     # both round the same fp64 arithmetic once to fp32


def test_ragged_pairs_batched_and_alone():
    sizes = [(1, 5), (7, 12), (12, 12)]
    rng = np.random.RandomState(5)
    probs = []
    for n1, n2 in sizes:
        a, b = random_pair(n1, 40 + n1), random_pair(n2, 50 + n2)
        probs.append(dict(M=rng.uniform(0.0, 2.0, size=(n1, n2)).astype(np.float32), C1=a["C1"], C2=b["C2"], p=a["p"], q=b["q"]))
    Ws = [np.random.default_rng(60 + k).standard_normal(s).astype(np.float32) for k, s in enumerate(sizes)]
    gd = np.array([0.7, 1.1, 1.6], dtype=np.float32)
    kw = dict(alpha=0.5, epsilon=0.5, max_iter=12, tol=1e-12, loss_fun="square_loss", symmetric=True)

    def run(idx):
        ins = [[gpu(probs[k][key]).requires_grad_(True) for k in idx] for key in ("M", "C1", "C2", "p", "q")]
        Ts, dist, info, _errs = ops.fgw_bregman_unrolled_list(*ins, **kw)
        obj = sum((gpu(Ws[k]) * Ts[j]).sum() + float(gd[k]) * dist[j] for j, k in enumerate(idx))
        flat = [t for ts in ins for t in ts]
        gs = torch.autograd.grad(obj, flat)
        return Ts, dist, info, [gs[c * len(idx):(c + 1) * len(idx)] for c in range(5)]

    Ts, dist, info, gs = run((0, 1, 2))
    for k, (n1, n2) in enumerate(sizes):
        Tk, distk, infok, gk = run((k,))                                   # the same pair alone
        assert torch.equal(bits(Tk[0]), bits(Ts[k])) and torch.equal(bits(distk[0]), bits(dist[k])) and torch.equal(infok[0], info[k])
        for c in range(5):
            assert gs[c][k].shape == gk[c][0].shape and torch.equal(bits(gs[c][k]), bits(gk[c][0])), (k, c)
        pr = probs[k]
        r = unrolled(pr["M"], pr["C1"], pr["C2"], pr["p"], pr["q"], None, alpha=0.5, epsilon=0.5, iters=int(info[k, 0]), dT=Ws[k], ddist=float(gd[k]))
        assert int(info[k, 0]) in (1, 12) and int(info[k, 2]) == 0
        for c, name in enumerate(KEYS[:5]):
            e = grad_error(gs[c][k].cpu().numpy(), r[name], Ws[k])
            print(f"pair {k} {sizes[k]} iterations {int(info[k, 0])} {name}: {e:.2e}")
            assert e <= TOL, (k, name, e)
    # massless rows and columns of the common container: exactly zero (the batched form on the embedded operands)
    M, C1, C2, p, q, _G0, _sizes = ops._pair_list_stack(*[[gpu(pr[key]) for pr in probs] for key in ("M", "C1", "C2", "p", "q")], None)
    ins = [t.requires_grad_(True) for t in (M, C1, C2, p, q)]
    T, d, _info, _errs = ops.fgw_bregman_unrolled(*ins, **kw)
    dM, dC1, dC2, dp, dq = (x.cpu().numpy() for x in torch.autograd.grad([T, d], ins, [torch.ones_like(T), torch.ones_like(d)]))
    for k, (n1, n2) in enumerate(sizes):
        assert not dM[k, n1:].any() and not dM[k, :, n2:].any() and not dC1[k, n1:].any() and not dC1[k, :, n1:].any() and not dC2[k, n2:].any()
        assert not dC2[k, :, n2:].any() and not dp[k, n1:].any() and not dq[k, n2:].any() and dM[k].any() and dq[k].any()
        assert not bits(T[k, n1:]).any() and not bits(T[k, :, n2:]).any()


def test_a_nan_pair_beside_a_healthy_one():
    """epsilon = 5e-4 with M >= 1: every factor of the first half-step is an exact zero, every row sum is 0: the reference's plan and autograd are
    NaN, and so are the kernel's gradients (binfo bit 2), beside a healthy pair of the same batch that keeps its bits."""
    f, g = load(NAN)
    prm = params(f)
    healthy = dict(M=((g["M"] - 1.5) * 1e-4).astype(np.float32), C1=np.zeros_like(g["C1"], dtype=np.float32), C2=np.zeros_like(g["C2"], dtype=np.float32),
                   p=g["p"], q=g["q"])
    stack = lambda key: gpu(np.stack([healthy[key], g[key].astype(np.float32)])).requires_grad_(True)
    ins = [stack(k) for k in ("M", "C1", "C2", "p", "q")]
    T, dist, info, _errs = ops.fgw_bregman_unrolled(*ins, **prm)
    assert int(info[0, 2]) == 0 and torch.isfinite(T[0]).all() and int(info[1, 2]) & 4 and torch.isnan(T[1]).all() and int(info[1, 0]) == int(f["iters"])
    W = gpu(np.stack([f["W"], f["W"]]))
    gs = torch.autograd.grad([T, dist], ins, [W, torch.ones_like(dist)])
    alone = [gpu(healthy[k])[None].requires_grad_(True) for k in ("M", "C1", "C2", "p", "q")]
    Ta, da, _ia, _ea = ops.fgw_bregman_unrolled(*alone, **prm)
    ga = torch.autograd.grad([Ta, da], alone, [W[:1], torch.ones_like(da)])
    for x, y in zip(gs, ga):
        assert torch.isfinite(x[0]).all() and torch.equal(bits(x[0]), bits(y[0])) and torch.isnan(x[1]).all()
    assert gs[0][0].any() and gs[3][0].any()
    r = unrolled(healthy["M"], healthy["C1"], healthy["C2"], healthy["p"], healthy["q"], None, alpha=prm["alpha"], epsilon=prm["epsilon"], iters=int(info[0, 0]),
                 dT=f["W"], ddist=1.0)
    assert not r["flagged"] and grad_error(gs[0][0].cpu().numpy(), r["dM"], f["W"]) <= TOL and grad_error(gs[3][0].cpu().numpy(), r["dp"], f["W"]) <= TOL
    got, _chk, binfo, _fwd, _N = raw_bwd(g, prm, f["W"], 1.0)             # the NaN pair alone through ctypes: its flags
    assert binfo[1] & 4, binfo
    assert all(np.isnan(v).all() for v in got.values() if v is not None)
    M, C1, C2, p, q, _ = leaves(g)
    with pytest.warns(UserWarning, match="Solver failed to produce a transport plan"):
        Tn = fgw.fgw_bregman_unrolled(M, C1, C2, p, q, epsilon=prm["epsilon"], alpha=prm["alpha"], max_iter=prm["max_iter"], tol=prm["tol"], symmetric=True)
    assert torch.isnan(Tn).all()
    (gM,) = torch.autograd.grad(Tn.sum(), M)
    assert torch.isnan(gM).all()


def test_partial_leaves_launch_counts_and_a_shared_leaf():
    f, g = load("dir_n12_false")
    calls = []

    def trace(name, fn, args):
        calls.append(name)
        return fn(*args)

    prev = _lib.set_call_trace(trace)
    try:
        ins = leaves(g, False)
        T, dist, _info, _errs = solve(f, ins)                              # no leaf: nothing saved, the forward launch alone
        assert not T.requires_grad and not dist.requires_grad and T.grad_fn is None
        assert calls == ["conan_fgw_pair_fwd"], calls
        ins[1].requires_grad_(True)                                        # only C1
        del calls[:]
        T, dist, _info, _errs = solve(f, ins)
        obj = (gpu(f["W"]) * T[0]).sum() + dist[0]
        obj.backward(retain_graph=True)                                    # one backward(): exactly one launch, for both cotangents
        assert calls == ["conan_fgw_pair_fwd", "conan_fgw_bregman_bwd"], calls
        first = ins[1].grad.clone()
        ins[1].grad = None
        obj.backward()                                                     # a second backward of the retained graph: one more launch, the same bits
        assert calls == ["conan_fgw_pair_fwd", "conan_fgw_bregman_bwd", "conan_fgw_bregman_bwd"], calls
        assert torch.equal(bits(first), bits(ins[1].grad))
    finally:
        _lib.set_call_trace(prev)
    assert ins[1].grad is not None and all(t.grad is None for k, t in enumerate(ins) if t is not None and k != 1)
    assert grad_error(ins[1].grad.cpu().numpy(), f["gT_dC1"] + f["gd_dC1"], f["W"]) <= TOL
    with torch.no_grad():                                                  # grad mode off: the plain path too
        assert not solve(f, leaves(g))[0].requires_grad
    with pytest.raises(RuntimeError):                                      # no double backward
        x = gpu(g["M"]).requires_grad_(True)
        (gx,) = torch.autograd.grad(solve(f, [x] + leaves(g, False)[1:])[1].sum(), x, create_graph=True)
        gx.sum().backward()
    # a leaf shared by the batch gets the sum: M [n1,n2] expanded over two pairs with different structures
    M = gpu(g["M"]).requires_grad_(True)
    C1 = gpu(np.stack([g["C1"], g["C1"][::-1, ::-1]])); C2 = gpu(np.stack([g["C2"], g["C2"][::-1, ::-1]]))      # (the second pair: relabelled graphs)
    p = gpu(np.stack([g["p"], g["p"]])); q = gpu(np.stack([g["q"], g["q"]]))
    prm = params(f)
    _T, d, _i, _e = ops.fgw_bregman_unrolled(M[None].expand(2, -1, -1), C1, C2, p, q, **prm)
    d.sum().backward()
    each = []
    for b in range(2):
        Mb = gpu(g["M"]).requires_grad_(True)
        ops.fgw_bregman_unrolled(Mb[None], C1[b:b + 1], C2[b:b + 1], p[b:b + 1], q[b:b + 1], **prm)[1].sum().backward()
        each.append(Mb.grad.double())
    assert grad_error(M.grad.cpu().numpy(), (each[0] + each[1]).cpu().numpy()) <= 2e-7 and grad_error(each[0].cpu().numpy(), f["gd_dM"]) <= TOL
    assert grad_error(each[0].cpu().numpy(), each[1].cpu().numpy()) > 1e-3


@pytest.mark.parametrize("name", ["n10_g0", "n12", "kl_n10"])
def test_public_functions(name):
    f, g = load(name)
    M, C1, C2, p, q, G0 = leaves(g)
    prm = params(f)
    kw = dict(loss_fun=prm["loss_fun"], epsilon=prm["epsilon"], symmetric=prm["symmetric"], alpha=prm["alpha"], max_iter=prm["max_iter"], tol=prm["tol"])
    det = lambda *ts: [t.detach() for t in ts]
    G0d = None if G0 is None else G0.detach()
    T, log = fgw.fgw_bregman_unrolled(M, C1, C2, p, q, G0=G0, log=True, **kw)
    Tp, logp = fgw.fgw_bregman(*det(M, C1, C2, p, q), G0=G0d, log=True, **kw)
    assert sorted(log) == ["err", "fgw_dist", "loss", "n_iter", "n_sinkhorn"] and log["n_sinkhorn"] == 0
    assert T.requires_grad and log["fgw_dist"].requires_grad and log["loss"].requires_grad and not Tp.requires_grad and torch.equal(bits(T), bits(Tp))
    assert torch.equal(bits(log["fgw_dist"]), bits(logp["fgw_dist"])) and log["n_iter"] == logp["n_iter"] == int(f["iters"])
    assert len(log["err"]) == len(logp["err"]) and all(not e.requires_grad and torch.equal(bits(e), bits(ep)) for e, ep in zip(log["err"], logp["err"]))
    ins = [M, C1, C2, p, q, G0]
    check(grads_of((gpu(f["W"]) * T).sum(), ins), f, ("gT",), f["W"], "fgw_bregman_unrolled T")
    check(grads_of(log["fgw_dist"], ins), f, ("gd",), 1.0, 'fgw_bregman_unrolled log["fgw_dist"]')
    if name in LOSS:
        check(grads_of(log["loss"], ins), f, ("gl",), 1.0, 'fgw_bregman_unrolled log["loss"]')
    T_only = fgw.fgw_bregman_unrolled(M, C1, C2, p, q, G0=G0, **kw)
    assert T_only.requires_grad and torch.equal(bits(T_only), bits(T))
    dist, dlog = fgw.fgw_bregman_distance_unrolled(M, C1, C2, p, q, G0=G0, log=True, **kw)
    fixed_ins = leaves(g)
    fixed = fgw.fgw_distance(*fixed_ins[:5], G0=fixed_ins[5], solver="BAPG", **kw)
    assert dist.dim() == 0 and dist.requires_grad and torch.equal(bits(dist), bits(fixed)) and dlog["T"].requires_grad and not dlog["fgw_dist"].requires_grad
    assert sorted(dlog) == ["T", "err", "fgw_dist", "loss", "n_iter", "n_sinkhorn"]
    got = grads_of(dist, ins)
    check(got, f, ("gd",), 1.0, "fgw_bregman_distance_unrolled")
    d_only = fgw.fgw_bregman_distance_unrolled(M, C1, C2, p, q, G0=G0, **kw)
    assert d_only.dim() == 0 and torch.equal(bits(d_only), bits(dist))
    # fgw_distance still returns its fixed-plan gradient: (1 - alpha) T for M, a different quantity
    gM = torch.autograd.grad(fixed, fixed_ins[0])[0].cpu().numpy()
    assert grad_error(gM, (1 - prm["alpha"]) * dlog["T"].detach().cpu().numpy()) <= TOL and grad_error(gM, got["dM"]) > 1e-3


def test_central_difference_of_the_distance():
    """fgw_bregman_distance_unrolled on the 7 x 12 pair, 20 iterations (tol = 1e-12: the count is fixed): for a random direction V of every
    input, the difference D_s = L(x + s V) - L(x - s V), the perturbed inputs prepared in fp64 and rounded to the fp32 the function takes,
    against <gradient, x_plus - x_minus> with the ACTUAL fp32 difference of the inputs.  Bound, from the formats and the function's own values,
    not from the gradient: each L is an fp32 value, rounded once from fp64 sums over a plan rounded once to fp32: 2^-23 |L| per evaluation pair
    and as much again for the inputs' rounding, 3 * 2^-22 |L| in all; the truncation of a central difference, s^3 L''' / 3, is measured by
    Richardson's D_2s / 2 - D_s = s^3 L''' (taken whole, not a third: room for the next order).  Every directional derivative is required to
    exceed 30 times its bound.  The fixed-plan gradient of fgw_distance misses the same bound."""
    f, g = load("rect_7x12")
    prm = dict(params(f), max_iter=20, tol=1e-12)
    kw = dict(loss_fun=prm["loss_fun"], epsilon=prm["epsilon"], symmetric=prm["symmetric"], alpha=prm["alpha"], max_iter=20, tol=1e-12)
    x0 = {k: np.asarray(g[k], dtype=np.float64) for k in ("M", "C1", "C2", "p", "q")}

    def L(x):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            d, log = fgw.fgw_bregman_distance_unrolled(*(gpu(x[k]) for k in ("M", "C1", "C2", "p", "q")), log=True, **kw)
        assert log["n_iter"] == 20
        return float(d)

    ins = [gpu(x0[k]).requires_grad_(True) for k in ("M", "C1", "C2", "p", "q")]
    dist = fgw.fgw_bregman_distance_unrolled(*ins, **kw)
    grads = [t.cpu().numpy().astype(np.float64) for t in torch.autograd.grad(dist, ins)]
    fixed_ins = [gpu(x0[k]).requires_grad_(True) for k in ("M", "C1", "C2", "p", "q")]
    fixed = [t.cpu().numpy().astype(np.float64) for t in torch.autograd.grad(fgw.fgw_distance(*fixed_ins, solver="BAPG", **kw), fixed_ins)]
    L0, rng, s = float(dist.detach()), np.random.default_rng(17), 2.0 ** -6
    rho = 3 * 2.0 ** -22 * abs(L0)
    misses = 0
    for (k, gk), fk in zip(zip(("M", "C1", "C2", "p", "q"), grads), fixed):
        V = rng.standard_normal(x0[k].shape) * np.abs(x0[k]).mean()
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        xp, xm, xp2, xm2 = f32(x0[k] + s * V), f32(x0[k] - s * V), f32(x0[k] + 2 * s * V), f32(x0[k] - 2 * s * V)
        D1 = L(dict(x0, **{k: xp})) - L(dict(x0, **{k: xm}))
        D2 = L(dict(x0, **{k: xp2})) - L(dict(x0, **{k: xm2}))
        bound = rho + abs(D2 / 2 - D1)
        an, an_fixed = float((gk * (xp - xm)).sum()), float((fk * (xp - xm)).sum())
        print(f"{k}: difference {D1:+.6e} unrolled {an:+.6e} (fixed-plan {an_fixed:+.6e}) bound {bound:.2e}")
        assert abs(D1) > 30 * bound, (k, D1, bound)
        assert abs(D1 - an) <= bound, (k, D1, an, bound)
        misses += abs(D1 - an_fixed) > bound
    assert misses >= 1                                                     # the check the fixed-plan gradient cannot pass
