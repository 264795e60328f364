"""The unrolled pairwise FGW gradient on the GPU (csrc/fgw_pair_grad.hip: conan_fgw_pair_bwd, conan_fgw_pair_bwd_workspace_bytes,
conan_fgw_pair_bwd_lds_resident, through ops.fgw_pair_unrolled / fgw_pair_unrolled_list, fgw.fgw_unrolled, fgw.fgw_distance_unrolled and
fgw.fgw_pairwise_distances_unrolled).

Yardsticks: torch autograd through the reference's own fgw in fp64 on the same fp32 inputs (tests/golden/fgw_unrollgrad_*.npz: gT = gradients
of sum(W * T), gd = of log["fgw_dist"]) and, where no fixture exists, the fp64 restatement tests/fgw_pair_unrolled_ref.py (held to every
fixture to 1e-9 by tests/test_fgw_pair_unrolled_cpu.py).

The bound on every gradient is 1e-6 (grad_error: the Frobenius norm of the difference over that of the yardstick).  It is derived, not
measured: the inputs are the same fp32 values, the kernel replays the solve in fp64 on the caller's parameters and decides the same sweep
counts, so what remains is one fp32 rounding per output entry (6e-8 relative), and the CPU test caps what reordering fp64 sums can add at
1e-9.  At a node without mass the gradient is exactly 0."""
import os

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, fgw, ops

from fgw_pair_unrolled_ref import grad_error, pair_grad_ref
from helpers import rel

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REUSED = ["pgd_1x5", "pgd_model_n20", "pgd_n10", "pgd_n10_cap25", "pgd_n10_g0", "pgd_rect_7x12", "pgd_dir_n12_false", "pgd_dir_n12_none",
          "pgd_undir_n12_none", "pgd_n33", "pgd_n80", "ppa_dir_n80_false"]
FINITE = REUSED + ["ppa_12x9", "zerop_9x11"]
NAN = "nan_ppa_n10"
DEV = "cuda"
TOL = 1e-6
KEYS = ("dM", "dC1", "dC2", "dp", "dq", "dG0")
SYM = {1: True, 0: False, -1: None}
_CACHE = {}


def load(name):
    """The fixture and the file that holds its inputs and parameters (a reused case: tests/golden/fgw_pair_<src>.npz)."""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"fgw_unrollgrad_{name}.npz"))
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


def params(g):
    return dict(alpha=float(g["alpha"]), epsilon=float(g["epsilon"]), max_iter=int(g["max_iter"]), tol=float(g["tol"]), num_iter_max=int(g["num_iter_max"]),
                stop_thr=float(g["stop_thr"]), solver=str(g["solver"]), symmetric=SYM[int(g["symmetric"])])


def leaves(g, grad=True):
    """The inputs on the GPU, in KEYS' order; None where there is no start."""
    return [gpu(g[k]).requires_grad_(grad) if g[k].size else None for k in ("M", "C1", "C2", "p", "q", "G0")]


def one(t):
    return None if t is None else t[None]


def solve(g, ins, **over):
    return ops.fgw_pair_unrolled(*(one(t) for t in ins), **dict(params(g), **over))


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


def raw_bwd(g, f_or_none, dT, dd, **over):
    """conan_fgw_pair_bwd through ctypes on the prepared operands of one pair -> (gradients by KEYS [N..], T_chk, binfo, forward outputs)."""
    L = _lib.lib()
    prm = dict(params(g), **over)
    M, C1, C2, p, q, G0, (B, N, n1, n2) = ops._pair_prepare(*(one(t) for t in leaves(g, False)))
    fprm, solver_code, sym_code = ops._pair_params(prm["alpha"], prm["epsilon"], prm["max_iter"], prm["tol"], prm["num_iter_max"], prm["stop_thr"], "square_loss",
                                                   prm["solver"], prm["symmetric"])
    T, dist, info, errs = ops._pair_fwd(M, C1, C2, p, q, G0, B, N, fprm, solver_code, sym_code, True)
    nbytes = int(L.conan_fgw_pair_bwd_workspace_bytes(B, N, prm["max_iter"], prm["num_iter_max"]))
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
    rc = L.conan_fgw_pair_bwd(ptr(M), ptr(C1), ptr(C2), ptr(p), ptr(q), ptr(G0), B, N, prm["alpha"], prm["epsilon"], prm["max_iter"], prm["num_iter_max"],
                              prm["stop_thr"], solver_code, sym_code, ptr(info), ptr(pad), ptr(ddt), ptr(dM), ptr(dC1), ptr(dC2), ptr(dp), ptr(dq), ptr(dG0),
                              ptr(chk), ptr(binfo), ptr(ws), _lib.stream_ptr())
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
    T, dist, info, errs = solve(g, ins)
    # the comparison means something only at the reference's iteration and sweep counts
    assert int(info[0, 0]) == int(f["iters"]) and int(info[0, 1]) == int(f["sweeps"].sum()) and int(info[0, 2]) == 0, (name, info.tolist())
    assert T.requires_grad and dist.requires_grad and not info.requires_grad and not errs.requires_grad
    plain = ops.fgw_pair_batched(*(one(None if t is None else t.detach()) for t in ins), **params(g))
    for a, b in zip((T, dist, info, errs), plain):                        # the forward is fgw_pair_batched's, bit for bit (errs: NaN where not run)
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
    W = gpu(f["W"])
    check(grads_of((W * T[0]).sum(), ins), f, ("gT",), f["W"], name)              # the plan's cotangent alone
    check(grads_of(dist[0], ins), f, ("gd",), 1.0, name)                          # the distance's alone
    both = grads_of((W * T[0]).sum() + dist[0], ins)                              # both in ONE backward launch (cotangents W and 1: fp32 inputs)
    check(both, f, ("gT", "gd"), f["W"], name)
    if name == "zerop_9x11":
        assert not both["dM"][3].any() and not both["dC1"][3].any() and not both["dC1"][:, 3].any() and both["dp"][3] == 0.0 and not T[0, 3].any()
        assert all(np.isfinite(v).all() for v in both.values() if v is not None) and both["dM"].any() and both["dp"].any()


@pytest.mark.parametrize("name", FINITE)
def test_replay_counts_and_final_plan(name):
    """conan_fgw_pair_bwd through ctypes: binfo carries the fixture's sweep total with bit 0 (total differs from the forward's) and bit 2 (NaN)
    clear; T_chk, the replay's final plan, against the forward's T and the reference's by the pair solve's yardstick for T (within 1e-4 of
    the fp32 run, or no further from the fp64 reference than that run is: _check_matrices)."""
    f, g = load(name)
    got, chk, binfo, (T, _dist, info, _errs), N = raw_bwd(g, f, f["W"], 1.0)
    assert binfo == [int(f["sweeps"].sum()), 0], (name, binfo, info.tolist())
    assert bool(_lib.lib().conan_fgw_pair_bwd_lds_resident(N)) == (N <= 61)
    check(got, f, ("gT", "gd"), f["W"], name + " ctypes")
    Tf = T.cpu().numpy()
    r64 = f["T"]
    e_fwd, e64, yard_fwd = rel(chk, Tf), rel(chk, r64), rel(Tf, r64)
    print(f"{name}: T_chk against the forward's T {e_fwd:.2e}, against the fp64 reference {e64:.2e} (the forward's T: {yard_fwd:.2e})")
    assert e_fwd <= 1e-4 or e64 <= yard_fwd, (e_fwd, e64, yard_fwd)
    if "r32_T" in g:
        yard, e32 = rel(g["r32_T"], g["r64_T"]), rel(chk, g["r32_T"])
        assert e32 <= 1e-4 or rel(chk, g["r64_T"]) <= yard, (e32, yard)


def random_pair(n, seed, directed=False):
    rng = np.random.RandomState(seed)
    y, z = rng.uniform(0.1, 1.2, size=(n, 3)), rng.uniform(0.1, 1.2, size=(n, 3))
    M = ((y[:, None] - z[None]) ** 2).sum(-1).astype(np.float32)

    def graph():
        a = rng.random_sample((n, n)) < 0.3
        a = (a & ~np.eye(n, dtype=bool)) if directed else (np.triu(a, 1) | np.triu(a, 1).T)
        return a.astype(np.float32)
    p, q = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    return dict(M=M, C1=graph(), C2=graph(), p=(p / p.sum()).astype(np.float32), q=(q / q.sum()).astype(np.float32), G0=np.zeros((0, 0), np.float32))


@pytest.mark.parametrize("solver,symmetric", [("PGD", True), ("PPA", False)])
def test_residency_bound_and_one_above(solver, symmetric):
    """Random pairs at the largest LDS-resident size and one above it (the streamed path), 3 x 5 iterations, against the restatement."""
    L = _lib.lib()
    bound = max(n for n in range(1, 200) if L.conan_fgw_pair_bwd_lds_resident(n))
    assert bound == 61 and not L.conan_fgw_pair_bwd_lds_resident(bound + 1)
    for n in (bound, bound + 1):
        g = dict(random_pair(n, 100 + n, directed=not symmetric), alpha=0.5, epsilon=0.1, max_iter=3, tol=1e-12, num_iter_max=5, stop_thr=1e-9,
                 solver=solver, symmetric={True: 1, False: 0}[symmetric])
        W = np.random.default_rng(n).standard_normal((n, n)).astype(np.float32)
        got, chk, binfo, (_T, _dist, info, _errs), N = raw_bwd(g, None, W, 0.8)
        r = pair_grad_ref(g["M"], g["C1"], g["C2"], g["p"], g["q"], None, alpha=0.5, epsilon=0.1, solver=solver, symmetric=symmetric, iters=int(info[0, 0]),
                          num_iter_max=5, stop_thr=1e-9, dT=W, ddist=0.8)
        assert N == n and int(info[0, 0]) == 3 and binfo == [15, 0] and list(r["sweeps"]) == [5, 5, 5]
        assert grad_error(chk, r["T"]) <= TOL
        for k in KEYS[:5]:
            e = grad_error(got[k], r[k], W)
            print(f"N {n} {solver} symmetric {symmetric} {k}: {e:.2e}")
            assert e <= TOL, (n, k, e)


def test_ragged_pairs_batched_and_alone():
    sizes = [(5, 7), (12, 9), (9, 11)]
    rng = np.random.RandomState(5)
    probs = []
    for n1, n2 in sizes:
        a, b = random_pair(n1, 40 + n1), random_pair(n2, 50 + n2)
        probs.append(dict(M=rng.uniform(0.0, 2.0, size=(n1, n2)).astype(np.float32), C1=a["C1"], C2=b["C2"], p=a["p"], q=b["q"]))
    Ws = [np.random.default_rng(60 + k).standard_normal(s).astype(np.float32) for k, s in enumerate(sizes)]
    gd = np.array([0.7, 1.1, 1.6], dtype=np.float32)
    kw = dict(alpha=0.5, epsilon=0.1, max_iter=12, tol=1e-12, num_iter_max=30, stop_thr=1e-5, solver="PGD", symmetric=True)

    def run(idx):
        ins = [[gpu(probs[k][key]).requires_grad_(True) for k in idx] for key in ("M", "C1", "C2", "p", "q")]
        Ts, dist, info, _errs = ops.fgw_pair_unrolled_list(*ins, **kw)
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
        r = pair_grad_ref(pr["M"], pr["C1"], pr["C2"], pr["p"], pr["q"], None, alpha=0.5, epsilon=0.1, solver="PGD", symmetric=True, iters=int(info[k, 0]),
                          num_iter_max=30, stop_thr=1e-5, dT=Ws[k], ddist=float(gd[k]))
        assert int(info[k, 1]) == int(r["sweeps"].sum()) and int(info[k, 2]) == 0
        for c, name in enumerate(KEYS[:5]):
            e = grad_error(gs[c][k].cpu().numpy(), r[name], Ws[k])
            print(f"pair {k} {sizes[k]} iterations {int(info[k, 0])} {name}: {e:.2e}")
            assert e <= TOL, (k, name, e)
    # massless rows and columns of the common container: exactly zero (the batched form on the embedded operands)
    M, C1, C2, p, q, _G0, _sizes = ops._pair_list_stack(*[[gpu(pr[key]) for pr in probs] for key in ("M", "C1", "C2", "p", "q")], None)
    ins = [t.requires_grad_(True) for t in (M, C1, C2, p, q)]
    T, d, _info, _errs = ops.fgw_pair_unrolled(*ins, **kw)
    dM, dC1, dC2, dp, dq = (x.cpu().numpy() for x in torch.autograd.grad([T, d], ins, [torch.ones_like(T), torch.ones_like(d)]))
    for k, (n1, n2) in enumerate(sizes):
        assert not dM[k, n1:].any() and not dM[k, :, n2:].any() and not dC1[k, n1:].any() and not dC1[k, :, n1:].any() and not dC2[k, n2:].any()
        assert not dC2[k, :, n2:].any() and not dp[k, n1:].any() and not dq[k, n2:].any() and dM[k].any() and dp[k].any()
        assert not bits(T[k, n1:]).any() and not bits(T[k, :, n2:]).any()


def test_a_nan_pair_beside_a_healthy_one():
    """PPA at epsilon = 0.01: entries of the plan underflow to exact zero in fp64 and the next iteration takes their logarithm: the reference's
    autograd gives NaN in every gradient, and so does the kernel (binfo bit 2), beside a healthy pair of the same batch that keeps its numbers."""
    f, g = load(NAN)
    prm = params(g)
    healthy = dict(M=(g["M"] * 0.01).astype(np.float32), C1=np.zeros_like(g["C1"], dtype=np.float32), C2=np.zeros_like(g["C2"], dtype=np.float32), p=g["p"], q=g["q"])
    stack = lambda key: gpu(np.stack([healthy[key], g[key].astype(np.float32)])).requires_grad_(True)
    ins = [stack(k) for k in ("M", "C1", "C2", "p", "q")]
    T, dist, info, _errs = ops.fgw_pair_unrolled(*ins, **prm)
    assert int(info[0, 2]) == 0 and torch.isfinite(T[0]).all()
    W = gpu(np.stack([f["W"], f["W"]]))
    gs = torch.autograd.grad([T, dist], ins, [W, torch.ones_like(dist)])
    alone = [gpu(healthy[k])[None].requires_grad_(True) for k in ("M", "C1", "C2", "p", "q")]
    Ta, da, _ia, _ea = ops.fgw_pair_unrolled(*alone, **prm)
    ga = torch.autograd.grad([Ta, da], alone, [W[:1], torch.ones_like(da)])
    for x, y in zip(gs, ga):
        assert torch.isfinite(x[0]).all() and torch.equal(bits(x[0]), bits(y[0])) and torch.isnan(x[1]).all()
    assert gs[0][0].any() and gs[3][0].any()
    r = pair_grad_ref(healthy["M"], healthy["C1"], healthy["C2"], healthy["p"], healthy["q"], None, alpha=prm["alpha"], epsilon=prm["epsilon"], solver="PPA",
                      symmetric=True, iters=int(info[0, 0]), num_iter_max=prm["num_iter_max"], stop_thr=prm["stop_thr"], dT=f["W"], ddist=1.0)
    assert not r["nan"] and grad_error(gs[0][0].cpu().numpy(), r["dM"], f["W"]) <= TOL and grad_error(gs[3][0].cpu().numpy(), r["dp"], f["W"]) <= TOL
    _got, _chk, binfo, _fwd, _N = raw_bwd(g, f, f["W"], 1.0)              # the NaN pair alone through ctypes: its flags
    assert binfo[1] & 4, binfo
    assert all(np.isnan(v).all() for v in _got.values() if v is not None)


def test_partial_leaves_launch_counts_and_a_shared_leaf():
    f, g = load("pgd_dir_n12_false")
    calls = []

    def trace(name, fn, args):
        calls.append(name)
        return fn(*args)

    prev = _lib.set_call_trace(trace)
    try:
        ins = leaves(g, False)
        T, dist, _info, _errs = solve(g, ins)                              # no leaf: nothing saved, the forward launch alone
        assert not T.requires_grad and not dist.requires_grad and T.grad_fn is None
        assert calls == ["conan_fgw_pair_fwd"], calls
        ins[1].requires_grad_(True)                                        # only C1
        del calls[:]
        T, dist, _info, _errs = solve(g, ins)
        ((gpu(f["W"]) * T[0]).sum() + dist[0]).backward()                  # one backward(): exactly one launch, for both cotangents
        assert calls == ["conan_fgw_pair_fwd", "conan_fgw_pair_bwd"], calls
    finally:
        _lib.set_call_trace(prev)
    assert ins[1].grad is not None and all(t.grad is None for k, t in enumerate(ins) if t is not None and k != 1)
    assert grad_error(ins[1].grad.cpu().numpy(), f["gT_dC1"] + f["gd_dC1"], f["W"]) <= TOL
    with torch.no_grad():                                                  # grad mode off: the plain path too
        assert not solve(g, leaves(g))[0].requires_grad
    with pytest.raises(RuntimeError):                                      # no double backward
        x = gpu(g["M"]).requires_grad_(True)
        (gx,) = torch.autograd.grad(solve(g, [x] + leaves(g, False)[1:])[1].sum(), x, create_graph=True)
        gx.sum().backward()
    # a leaf shared by the batch gets the sum: M [n1,n2] expanded over two pairs with different structures
    M = gpu(g["M"]).requires_grad_(True)
    C1 = gpu(np.stack([g["C1"], g["C1"][::-1, ::-1]])); C2 = gpu(np.stack([g["C2"], g["C2"][::-1, ::-1]]))      # (the second pair: relabelled graphs)
    p = gpu(np.stack([g["p"], g["p"]])); q = gpu(np.stack([g["q"], g["q"]]))
    prm = params(g)
    _T, d, _i, _e = ops.fgw_pair_unrolled(M[None].expand(2, -1, -1), C1, C2, p, q, **prm)
    d.sum().backward()
    each = []
    for b in range(2):
        Mb = gpu(g["M"]).requires_grad_(True)
        ops.fgw_pair_unrolled(Mb[None], C1[b:b + 1], C2[b:b + 1], p[b:b + 1], q[b:b + 1], **prm)[1].sum().backward()
        each.append(Mb.grad.double())
    assert grad_error(M.grad.cpu().numpy(), (each[0] + each[1]).cpu().numpy()) <= 2e-7 and grad_error(each[0].cpu().numpy(), f["gd_dM"]) <= TOL
    assert grad_error(each[0].cpu().numpy(), each[1].cpu().numpy()) > 1e-3


def test_public_functions():
    f, g = load("pgd_n10_g0")
    M, C1, C2, p, q, G0 = leaves(g)
    prm = params(g)
    kw = dict(epsilon=prm["epsilon"], symmetric=prm["symmetric"], alpha=prm["alpha"], max_iter=prm["max_iter"], tol=prm["tol"], solver=prm["solver"],
              numItermax=prm["num_iter_max"], stopThr=prm["stop_thr"])
    det = lambda *ts: [t.detach() for t in ts]
    T, log = fgw.fgw_unrolled(M, C1, C2, p, q, G0=G0, log=True, **kw)
    Tp, logp = fgw.fgw(*det(M, C1, C2, p, q), G0=G0.detach(), log=True, **kw)
    assert T.requires_grad and log["fgw_dist"].requires_grad and not Tp.requires_grad and torch.equal(bits(T), bits(Tp))
    assert torch.equal(bits(log["fgw_dist"]), bits(logp["fgw_dist"])) and log["n_iter"] == logp["n_iter"] == int(f["iters"]) and log["n_sinkhorn"] == logp["n_sinkhorn"]
    assert len(log["err"]) == len(logp["err"]) and all(not e.requires_grad and torch.equal(bits(e), bits(ep)) for e, ep in zip(log["err"], logp["err"]))
    ins = [M, C1, C2, p, q, G0]
    check(grads_of((gpu(f["W"]) * T).sum(), ins), f, ("gT",), f["W"], "fgw_unrolled T")
    check(grads_of(log["fgw_dist"], ins), f, ("gd",), 1.0, 'fgw_unrolled log["fgw_dist"]')
    T_only = fgw.fgw_unrolled(M, C1, C2, p, q, G0=G0, **kw)
    assert T_only.requires_grad and torch.equal(bits(T_only), bits(T))

    f, g = load("ppa_12x9")
    M, C1, C2, p, q, _ = leaves(g)
    prm = params(g)
    kw = dict(epsilon=prm["epsilon"], symmetric=prm["symmetric"], alpha=prm["alpha"], max_iter=prm["max_iter"], tol=prm["tol"], solver=prm["solver"],
              numItermax=prm["num_iter_max"], stopThr=prm["stop_thr"])
    dist, log = fgw.fgw_distance_unrolled(M, C1, C2, p, q, log=True, **kw)
    fixed_ins = leaves(g)[:5]
    fixed = fgw.fgw_distance(*fixed_ins, **kw)
    assert dist.dim() == 0 and dist.requires_grad and torch.equal(bits(dist), bits(fixed)) and log["T"].requires_grad and not log["fgw_dist"].requires_grad
    unrolled = grads_of(dist, [M, C1, C2, p, q, None])
    check(unrolled, f, ("gd",), 1.0, "fgw_distance_unrolled")
    # fgw_distance still returns its fixed-plan gradient: (1 - alpha) T for M, a different quantity
    gM = torch.autograd.grad(fixed, fixed_ins[0])[0].cpu().numpy()
    assert grad_error(gM, (1 - prm["alpha"]) * log["T"].detach().cpu().numpy()) <= TOL and grad_error(gM, unrolled["dM"]) > 1e-3


def test_pairwise_distances_unrolled_against_the_pair_op():
    graphs = [random_pair(6, 70 + k) for k in range(3)]
    rng = np.random.RandomState(9)
    Ys = [gpu(rng.uniform(0.1, 1.0, size=(6, 3))).requires_grad_(True) for _ in range(3)]
    Cs = [gpu(gr["C1"]).requires_grad_(True) for gr in graphs]
    ps = [gpu(gr["p"]).requires_grad_(True) for gr in graphs]
    kw = dict(alpha=0.5, epsilon=0.1, max_iter=10, tol=1e-12, numItermax=20, stopThr=1e-6)
    D = fgw.fgw_pairwise_distances_unrolled(Ys, Cs, ps, **kw)
    plain = fgw.fgw_pairwise_distances([y.detach() for y in Ys], [c.detach() for c in Cs], [p.detach() for p in ps], **kw)
    assert D.requires_grad and torch.equal(bits(D), bits(plain)) and torch.equal(bits(D), bits(D.T)) and not D.diagonal().any()
    Wd = gpu(np.triu(rng.standard_normal((3, 3)), 1))
    got = torch.autograd.grad((Wd * D).sum(), Ys + Cs + ps)
    Y2, C2, p2 = [y.detach().clone().requires_grad_(True) for y in Ys], [c.detach().clone().requires_grad_(True) for c in Cs], [p.detach().clone().requires_grad_(True) for p in ps]
    obj = 0.0
    for a in range(3):
        for b in range(a + 1, 3):
            M = fgw.feature_cost(Y2[a], Y2[b])
            d = ops.fgw_pair_unrolled(M[None], C2[a][None], C2[b][None], p2[a][None], p2[b][None], alpha=0.5, epsilon=0.1, max_iter=10, tol=1e-12, num_iter_max=20,
                                      stop_thr=1e-6)[1]
            assert torch.equal(bits(d[0]), bits(D[a, b]))
            obj = obj + Wd[a, b] * d[0]
    want = torch.autograd.grad(obj, Y2 + C2 + p2)
    for x, y in zip(got, want):
        assert grad_error(x.cpu().numpy(), y.cpu().numpy()) <= 1e-6
    fixed = torch.autograd.grad((Wd * fgw.fgw_pairwise_distances(Ys, Cs, ps, **kw)).sum(), Cs)      # the existing name: still the fixed-plan gradient
    assert grad_error(fixed[0].cpu().numpy(), got[3].cpu().numpy()) > 1e-3
