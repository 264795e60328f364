"""The unrolled Sinkhorn gradient on the GPU (csrc/sinkhorn_grad.hip through ops.sinkhorn_unrolled / sinkhorn_unrolled_list / sinkhorn_loss and
the grad="unrolled" keyword of conan_fgw_amd.sinkhorn).

Yardsticks: torch autograd through the reference's own sinkhorn.py in fp64 on the same fp32 inputs (tests/golden/grad_sinkhorn_*.npz: g1 =
gradients of sum(M * T), g2 = of sum(M * T) + sum(dT * T)) and, where no fixture exists, the fp64 restatement tests/sinkhorn_grad_ref.py (held
to every fixture to 1e-9 by tests/test_sinkhorn_grad_cpu.py).

The bound on every gradient is rel <= 1e-6 (rel = Frobenius norm of the difference over that of the yardstick).  It is derived, not measured:
the inputs are the same fp32 values, the kernel iterates in fp64, so what remains is one fp32 rounding per output entry (6e-8 relative), and
the CPU test caps what reordering fp64 sums can add at 1e-9.  At a zero-weight entry the gradient is exactly 0."""
import os
import warnings

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, ops
from conan_fgw_amd import sinkhorn as sk
from conan_fgw_amd.fgw import feature_cost

from sinkhorn_grad_ref import sinkhorn_grad_ref, sweeps_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["1x5_log", "1x5_knopp", "7x12_log", "7x12_knopp", "33x33_log", "33x33_knopp", "64x80_log", "64x80_knopp", "zeroa_log", "warm_log",
         "warm_knopp", "9x11col_log", "9x11col_knopp", "9x11row_log"]
DEV = "cuda"
TOL = 1e-6
_CACHE = {}


def load(name):
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"grad_sinkhorn_{name}.npz"))
        _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


def gpu(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def problem(n1, n2, seed):
    """Squared distances of two Gaussian clouds over their maximum, random normalised marginals (the fixtures' construction)."""
    g = np.random.default_rng(seed)
    x, y = g.standard_normal((n1, 3)), g.standard_normal((n2, 3)) + 0.5
    M = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    M = (M / M.max()).astype(np.float32)
    a, b = g.random(n1) + 0.1, g.random(n2) + 0.1
    return M, (a / a.sum()).astype(np.float32), (b / b.sum()).astype(np.float32)


def leaves(M, a, b, warm):
    Mg, ag, bg = gpu(M).requires_grad_(True), gpu(a).requires_grad_(True), gpu(b).requires_grad_(True)
    wg = None if warm is None else (gpu(warm[0]).requires_grad_(True), gpu(warm[1]).requires_grad_(True))
    return Mg, ag, bg, wg


def grads_of(objs, Mg, ag, bg, wg):
    """The gradients of sum(objs) as fp64 numpy arrays (None where autograd delivers none).  Each objective is differentiated on its own and
    the results are added in fp64 on the host: every cotangent the kernel sees is then an fp32 INPUT of the test (M, dT, 1), not an fp32 sum
    formed by torch, which would be one more rounding than the bound accounts for."""
    ins = [Mg, ag, bg] + ([] if wg is None else [wg[0], wg[1]])
    objs = list(objs) if isinstance(objs, (list, tuple)) else [objs]
    total = [None] * len(ins)
    for n, obj in enumerate(objs):
        gs = torch.autograd.grad(obj, ins, allow_unused=True, retain_graph=n + 1 < len(objs))
        for k, g in enumerate(gs):
            if g is not None:
                total[k] = g.cpu().numpy().astype(np.float64) + (0.0 if total[k] is None else total[k])
    keys = ("dM", "da", "db", "dwu", "dwv")
    return {k: (total[i] if i < len(total) else None) for i, k in enumerate(keys)}


def solve_one(M, a, b, reg, method, it, thr, warm=None, gl=1.0, dT=None):
    """B = 1 through ops.sinkhorn_unrolled in the problem's own container -> (outputs without the batch axis, gradients of gl loss + sum(dT T))."""
    Mg, ag, bg, wg = leaves(M, a, b, warm)
    out = ops.sinkhorn_unrolled(Mg[None], ag[None], bg[None], reg=reg, method=method, num_iter_max=it, stop_thr=thr,
                                warmstart=None if wg is None else (wg[0][None], wg[1][None]))
    obj = gl * out[1][0] + (0.0 if dT is None else (gpu(dT) * out[0][0]).sum())      # (both cotangents in ONE backward launch)
    return tuple(o[0] for o in out), grads_of(obj, Mg, ag, bg, wg)


def check_grads(f, tag, g, label):
    """g against the fixture's gradients of objective `tag`: rel <= TOL each; exact zeros where the fixture has none."""
    S = sweeps_of(int(f["r64_niter"]), str(f["r64_warn"]) == "numerr")
    for k in ("dM", "da", "db") + (("dwu",) if "warm_u" in f else ()):
        want = f[f"{tag}_{k}"]
        if not want.any():                                                 # S = 0: nothing reaches a, b
            assert S == 0 and k in ("da", "db") and not g[k].any(), (label, tag, k)
            continue
        e = rel(g[k], want)
        print(f"{label} {tag} {k}: rel {e:.2e}")
        assert e <= TOL, (label, tag, k, e)
    if "warm_u" in f:
        assert g["dwv"] is None                                            # warmstart[1]: none, as in the reference
    if bool(f["ref_nan_at_zero_weight"]):
        assert g["da"][3] == 0.0 and np.isfinite(g["dM"]).all() and np.isfinite(g["da"]).all()


def fixture_args(f):
    warm = (f["warm_u"], f["warm_v"]) if "warm_u" in f else None
    return f["M"], f["a"], f["b"], float(f["reg"]), str(f["method"]), int(f["numItermax"]), float(f["stopThr"]), warm


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_the_op(name):
    f = load(name)
    M, a, b, reg, method, it, thr, warm = fixture_args(f)
    w = None if warm is None else (gpu(warm[0])[None], gpu(warm[1])[None])
    plain = ops.sinkhorn_batched(gpu(M)[None], gpu(a)[None], gpu(b)[None], reg=reg, method=method, num_iter_max=it, stop_thr=thr, warmstart=w)
    for tag, dT in (("g1", None), ("g2", f["dT"])):
        out, g = solve_one(M, a, b, reg, method, it, thr, warm, 1.0, dT)
        for x, y in zip(out, plain):                                       # the forward is sinkhorn_batched's launch, bit for bit
            assert torch.equal(bits(x), bits(y[0])) if x.dtype == torch.float32 else torch.equal(x, y[0])
        niter, flags = int(out[4][0]), int(out[4][1])
        warn = str(f["r64_warn"])
        assert niter == int(f["r64_niter"]) and flags & 3 == (1 if warn == "" else (2 if warn == "numerr" else 0)), (name, niter, flags)
        assert bool(flags & 4) == (name == "9x11row_log")                  # the exact log-domain path, and only there
        assert out[0].requires_grad and out[1].requires_grad and not out[2].requires_grad and not out[3].requires_grad
        check_grads(f, tag, g, name)
        if name == "9x11col_knopp":                                        # S = 0: the plan is u0 K v0, dM = gl T - (Tb o T) / reg
            T = out[0].detach().cpu().numpy().astype(np.float64)
            Tb = M.astype(np.float64) + (0.0 if dT is None else dT)
            assert rel(g["dM"], T - Tb * T / reg) <= TOL and not g["da"].any() and not g["db"].any()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_the_public_functions(name):
    f = load(name)
    M, a, b, reg, method, it, thr, warm = fixture_args(f)
    direct = sk.sinkhorn_log if method == "sinkhorn_log" else sk.sinkhorn_knopp
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # the plan's cotangent: sum(M * T) (+ sum(dT * T)) formed by torch on the returned plan
        for tag, dT in (("g1", None), ("g2", f["dT"])):
            Mg, ag, bg, wg = leaves(M, a, b, warm)
            T, log = sk.sinkhorn(ag, bg, Mg, reg, method=method, numItermax=it, stopThr=thr, log=True, warmstart=wg, grad="unrolled")
            assert T.requires_grad and log["niter"] == int(f["r64_niter"]) and len(log["err"]) == len(f["r64_err"])
            objs = [(Mg * T).sum()] + ([] if dT is None else [(gpu(dT) * T).sum()])
            check_grads(f, tag, grads_of(objs, Mg, ag, bg, wg), name + " sinkhorn")
        # the loss's cotangent: sinkhorn2's value
        Mg, ag, bg, wg = leaves(M, a, b, warm)
        cost = sk.sinkhorn2(ag, bg, Mg, reg, method=method, numItermax=it, stopThr=thr, warmstart=wg, grad="unrolled")
        assert cost.dim() == 0 and cost.requires_grad
        check_grads(f, "g1", grads_of(cost, Mg, ag, bg, wg), name + " sinkhorn2")
        Mg, ag, bg, wg = leaves(M, a, b, warm)
        T2 = direct(ag, bg, Mg, reg, numItermax=it, stopThr=thr, warmstart=wg, grad="unrolled")
        assert T2.requires_grad and torch.equal(bits(T2.detach()), bits(T.detach()))
        check_grads(f, "g1", grads_of((Mg * T2).sum(), Mg, ag, bg, wg), name + " direct")


def test_default_path_is_unchanged():
    M, a, b = problem(20, 25, 8)
    res = []
    for kw in ({}, {"grad": "plan"}):
        Mg, ag, bg, _ = leaves(M, a, b, None)
        cost = sk.sinkhorn2(ag, bg, Mg, 0.05, method="sinkhorn_log", numItermax=100, stopThr=1e-5, **kw)
        cost.backward()
        T = sk.sinkhorn(ag, bg, Mg, 0.05, method="sinkhorn_log", numItermax=100, stopThr=1e-5, **kw)
        assert not T.requires_grad and ag.grad is None and bg.grad is None and torch.equal(bits(Mg.grad), bits(T))
        loss = ops.sinkhorn_loss(Mg[None], ag[None], bg[None], reg=0.05, num_iter_max=100, stop_thr=1e-5, **kw)
        res.append((cost.detach(), T, Mg.grad, loss.detach()))
    for x, y in zip(*res):
        assert torch.equal(bits(x), bits(y))
    Ys = [(0.4 * torch.randn(n, 4, generator=torch.Generator().manual_seed(n))).to(DEV) for n in (5, 7, 7)]
    assert torch.equal(bits(sk.wasserstein_pairwise_distances(Ys)), bits(sk.wasserstein_pairwise_distances(Ys, grad="plan")))


def test_unrolled_differs_from_the_fixed_plan():
    M, a, b = problem(20, 25, 8)
    reg, it, thr = 0.05, 100, 1e-5
    Mg, ag, bg, _ = leaves(M, a, b, None)
    cost = sk.sinkhorn2(ag, bg, Mg, reg, method="sinkhorn_log", numItermax=it, stopThr=thr, grad="unrolled")
    cost.backward()
    assert ag.grad is not None and bg.grad is not None and ag.grad.abs().max() > 0 and bg.grad.abs().max() > 0
    out = ops.sinkhorn_batched(gpu(M)[None], gpu(a)[None], gpu(b)[None], reg=reg, method="sinkhorn_log", num_iter_max=it, stop_thr=thr)
    T, info = out[0][0].cpu().numpy(), out[4][0].tolist()
    d = rel(Mg.grad.cpu().numpy(), T)
    print(f"rel(dM, T) {d:.3f}")
    assert d > 0.1                                                         # the CPU measured 0.22 - 0.47 on like problems
    r = sinkhorn_grad_ref(a, b, M, np.float32(reg), sweeps_of(info[0], info[1] & 2), "sinkhorn_log")
    for k, got in (("dM", Mg.grad), ("da", ag.grad), ("db", bg.grad)):
        e = rel(got.cpu().numpy(), r[k])
        print(f"{k}: rel {e:.2e}")
        assert e <= TOL, (k, e)


def batch_grads(Ms, as_, bs, gl, dTs, container, method, **kw):
    """The problems in one container through ops.sinkhorn_unrolled -> (outputs, dM [B,N1,N2], da, db, sizes)."""
    M, a, b, _w, n1, n2, sizes = ops._sinkhorn_list_stack([gpu(m) for m in Ms], [gpu(x) for x in as_], [gpu(x) for x in bs], None, container)
    M, a, b = M.requires_grad_(True), a.requires_grad_(True), b.requires_grad_(True)
    dT = torch.zeros_like(M)
    for k, (m1, m2) in enumerate(sizes):
        dT[k, :m1, :m2] = gpu(dTs[k])
    out = ops.sinkhorn_unrolled(M, a, b, n1=n1, n2=n2, method=method, **kw)
    obj = (gpu(gl) * out[1]).sum() + (dT * out[0]).sum()
    return (out,) + torch.autograd.grad(obj, [M, a, b]) + (sizes,)


@pytest.mark.parametrize("method", ["sinkhorn_log", "sinkhorn"])
def test_gradients_are_bit_identical_alone_batched_and_streamed(method):
    fs = [load(n) for n in NAMES]
    order = np.random.default_rng(3).permutation(len(fs))
    fs = [fs[i] for i in order]
    kw = dict(reg=0.05, num_iter_max=100, stop_thr=1e-5)
    Ms, as_, bs, dTs = [f["M"] for f in fs], [f["a"] for f in fs], [f["b"] for f in fs], [f["dT"] for f in fs]
    gl = (np.random.default_rng(5).random(len(fs)) + 0.5).astype(np.float32)
    L = _lib.lib()
    assert L.conan_sinkhorn_bwd_lds_resident(64, 80) and L.conan_sinkhorn_bwd_lds_resident(70, 90) and not L.conan_sinkhorn_bwd_lds_resident(141, 143)
    runs = [batch_grads(Ms, as_, bs, gl, dTs, c, method, **kw) for c in ((64, 80), (70, 90), (141, 143))]      # resident, larger resident, streamed
    again = batch_grads(Ms, as_, bs, gl, dTs, (64, 80), method, **kw)
    for x, y in zip(runs[0][1:4], again[1:4]):
        assert torch.equal(bits(x), bits(y))
    sweeps = set()
    for k, (m1, m2) in enumerate(runs[0][4]):
        one = batch_grads([Ms[k]], [as_[k]], [bs[k]], gl[k:k + 1], [dTs[k]], None, method, **kw)       # alone, in its own container
        sweeps.add(int(one[0][4][0, 0]))
        for out, dM, da, db, _sizes in runs:
            assert torch.equal(bits(dM[k, :m1, :m2]), bits(one[1][0])), (k, m1, m2)
            assert torch.equal(bits(da[k, :m1]), bits(one[2][0])) and torch.equal(bits(db[k, :m2]), bits(one[3][0])), (k, m1, m2)
            # ragged sizes: zeros outside each block, something inside
            assert not bits(dM[k, m1:]).any() and not bits(dM[k, :, m2:]).any() and not bits(da[k, m1:]).any() and not bits(db[k, m2:]).any()
            assert dM[k, :m1, :m2].any() and torch.isfinite(dM[k]).all() and torch.isfinite(da[k]).all() and torch.isfinite(db[k]).all()
            if int(out[4][k, 0]) + 1 - ((int(out[4][k, 1]) >> 1) & 1) > 0:
                assert da[k, :m1].any() and db[k, :m2].any()
    assert len(sweeps) > 1                                                 # the batch really mixes sweep counts


def test_list_form_carries_the_gradient_to_every_entry():
    probs = [problem(20, 25, 8), problem(7, 25, 9), problem(13, 9, 10)]
    Ms, as_, bs = ([gpu(p[i]).requires_grad_(True) for p in probs] for i in range(3))
    Ts, loss, lus, lvs, info, errs = ops.sinkhorn_unrolled_list(Ms, as_, bs, reg=0.05, method="sinkhorn", num_iter_max=100, stop_thr=1e-5)
    assert [tuple(t.shape) for t in Ts] == [(20, 25), (7, 25), (13, 9)] and all(t.requires_grad for t in Ts)
    (loss.sum() + sum((t * t).sum() for t in Ts)).backward()
    for k, (M, a, b) in enumerate(probs):
        T = Ts[k].detach().cpu().numpy().astype(np.float64)
        r = sinkhorn_grad_ref(a, b, M, np.float32(0.05), sweeps_of(int(info[k, 0]), int(info[k, 1]) & 2), "sinkhorn", None, 1.0, 2.0 * T)
        for name, got in (("dM", Ms[k].grad), ("da", as_[k].grad), ("db", bs[k].grad)):
            e = rel(got.cpu().numpy(), r[name])
            print(f"problem {k} {name}: rel {e:.2e}")
            assert e <= TOL, (k, name, e)


def test_shared_cost_matrix_gets_the_sum_over_the_batch():
    M, a, _ = problem(33, 40, 11)
    bsets = np.stack([problem(33, 40, 20 + k)[2] for k in range(3)])
    gl = np.array([0.7, 1.1, 1.6], dtype=np.float32)
    for method in ("sinkhorn_log", "sinkhorn"):
        kw = dict(reg=0.05, method=method, num_iter_max=100, stop_thr=1e-5)
        Mg, bg = gpu(M).requires_grad_(True), gpu(bsets).requires_grad_(True)
        out = ops.sinkhorn_unrolled(Mg, None, bg, **kw)
        assert out[0].shape == (3, 33, 40)
        (gpu(gl) * out[1]).sum().backward()
        assert Mg.grad.shape == (33, 40)
        total = np.zeros((33, 40))
        for k in range(3):
            Mk, bk = gpu(M).requires_grad_(True), gpu(bsets[k]).requires_grad_(True)
            one = ops.sinkhorn_unrolled(Mk[None], None, bk[None], **kw)
            (float(gl[k]) * one[1][0]).backward()
            total += Mk.grad.cpu().numpy().astype(np.float64)
            assert torch.equal(bits(bg.grad[k]), bits(bk.grad))
        e = rel(Mg.grad.cpu().numpy(), total)
        print(f"{method}: shared dM vs the sum of three: rel {e:.2e}")
        assert e <= TOL


@pytest.mark.parametrize("method", ["sinkhorn_log", "sinkhorn"])
def test_streamed_path_beside_the_residency_limit(method):
    L = _lib.lib()
    n1, n2 = 64, 250
    assert L.conan_sinkhorn_bwd_lds_resident(n1, n2) == 1
    while L.conan_sinkhorn_bwd_lds_resident(n1, n2 + 1):
        n2 += 1
    shapes = [(n1, n2), (n1, n2 + 1)]                                      # the largest resident shape and the smallest streamed one beside it
    assert 250 < n2 < 300 and not L.conan_sinkhorn_bwd_lds_resident(*shapes[1])
    reg, it, thr = float(np.float32(0.05)), 100, 1e-5
    probs = [problem(*s, seed=1) for s in shapes]
    dTs = [np.random.default_rng(7 + k).standard_normal(s).astype(np.float32) for k, s in enumerate(shapes)]
    gl = np.array([1.0, 0.8], dtype=np.float32)
    out, dM, da, db, sizes = batch_grads([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs], gl, dTs, None, method,
                                         reg=reg, num_iter_max=it, stop_thr=thr)                      # container 64 x (n2 + 1): streamed
    for k, (M, a, b) in enumerate(probs):
        S = sweeps_of(int(out[4][k, 0]), int(out[4][k, 1]) & 2)
        assert 1 <= S <= it
        r = sinkhorn_grad_ref(a, b, M, reg, S, method, None, float(gl[k]), dTs[k])
        m1, m2 = sizes[k]
        for name, got in (("dM", dM[k, :m1, :m2]), ("da", da[k, :m1]), ("db", db[k, :m2])):
            e = rel(got.cpu().numpy(), r[name])
            print(f"streamed {shapes[k]} {name}: rel {e:.2e}")
            assert e <= TOL, (shapes[k], name, e)
    one = batch_grads([probs[0][0]], [probs[0][1]], [probs[0][2]], gl[:1], dTs[:1], None, method, reg=reg, num_iter_max=it, stop_thr=thr)
    assert torch.equal(bits(one[1][0]), bits(dM[0, :, :n2])) and torch.equal(bits(one[2][0]), bits(da[0])) and torch.equal(bits(one[3][0]), bits(db[0, :n2]))


def test_no_sweep_executed_with_a_warm_start():
    """Knopp on the underflowing column leaves at iteration 0 (S = 0) whatever the start: the plan is u0 K v0, so with a warm start
    d warmstart[0]_i = sum_j Tb_ij T_ij, and still nothing reaches a, b or warmstart[1]."""
    f = load("9x11col_knopp")
    M, a, b, reg, method, it, thr, _ = fixture_args(f)
    g0 = np.random.default_rng(2)
    warm = ((0.3 * g0.standard_normal(9)).astype(np.float32), (0.3 * g0.standard_normal(11) - 2.0).astype(np.float32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, g = solve_one(M, a, b, reg, method, it, thr, warm, 1.0, f["dT"])
    assert int(out[4][0]) == 0 and int(out[4][1]) & 2
    r = sinkhorn_grad_ref(a, b, M, reg, 0, method, warm, 1.0, f["dT"])
    assert rel(out[0].detach().cpu().numpy(), r["T"]) <= TOL
    assert rel(g["dM"], r["dM"]) <= TOL and rel(g["dwu"], r["dwu"]) <= TOL
    assert not g["da"].any() and not g["db"].any() and g["dwv"] is None


def test_sweep_count_is_clamped_and_bad_arguments_are_refused():
    """conan_sinkhorn_bwd through ctypes: an info whose iteration index lies outside [0, num_iter_max) is clamped to the cap (no loop grows,
    nothing leaves the workspace: the gradients are those of the count at the cap, bit for bit), and bad arguments return -1 before any
    launch."""
    L = _lib.lib()
    M, a, b = problem(9, 11, 3)
    B, N1, N2, it = 1, 9, 11, 12
    Mg, ag, bg = gpu(M)[None].contiguous(), gpu(a)[None].contiguous(), gpu(b)[None].contiguous()
    gl = torch.ones(1, device=DEV)
    ws = torch.empty(int(L.conan_sinkhorn_bwd_workspace_bytes(B, N1, N2, it)), dtype=torch.uint8, device=DEV)

    def run(niter, flags, method, **kw):
        info = torch.tensor([[niter, flags, 0, 0]], dtype=torch.int32, device=DEV)
        dM, da, db = (torch.full(s, 7.0, device=DEV) for s in ((B, N1, N2), (B, N1), (B, N2)))
        arg = dict(M=Mg.data_ptr(), B=B, it=it, info=info.data_ptr(), gl=gl.data_ptr(), dM=dM.data_ptr(), ws=ws.data_ptr(), reg=0.1, method=method)
        arg.update(kw)
        rc = L.conan_sinkhorn_bwd(arg["M"], ag.data_ptr(), bg.data_ptr(), None, None, None, None, arg["B"], N1, N2, N1 * N2, arg["reg"], arg["method"],
                                  arg["it"], arg["info"], arg["gl"], None, arg["dM"], da.data_ptr(), db.data_ptr(), None, arg["ws"], _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, dM, da, db

    for method in (0, 1):
        cap = run(it - 1, 0, method)
        assert cap[0] == 0 and torch.isfinite(cap[1]).all()
        r = sinkhorn_grad_ref(a, b, M, np.float32(0.1), it, "sinkhorn" if method else "sinkhorn_log")
        assert rel(cap[1][0].cpu().numpy(), r["dM"]) <= TOL and rel(cap[2][0].cpu().numpy(), r["da"]) <= TOL
        for niter in (it, 10 ** 6, 2 ** 31 - 1):                          # beyond the cap: the cap
            got = run(niter, 0, method)
            assert got[0] == 0 and all(torch.equal(bits(x), bits(y)) for x, y in zip(got[1:], cap[1:])), niter
        exit_flag = 2 if method else 0                                     # the smallest count: one sweep (sinkhorn_log), none (Knopp's exit at 0)
        low = run(0, exit_flag, method)
        for niter in (-1, -5, -2 ** 31):
            got = run(niter, exit_flag, method)
            assert got[0] == 0 and all(torch.equal(bits(x), bits(y)) for x, y in zip(got[1:], low[1:])), niter
    for kw in (dict(M=None), dict(info=None), dict(dM=None), dict(ws=None), dict(gl=None), dict(B=0), dict(it=0), dict(reg=0.0), dict(reg=float("nan")),
               dict(method=2), dict(method=-1)):
        rc, dM, da, db = run(3, 0, kw.get("method", 0), **{k: v for k, v in kw.items() if k != "method"})
        assert rc == -1 and (dM == 7.0).all() and (da == 7.0).all(), kw    # refused before any launch


def test_no_host_synchronisation_and_no_double_backward():
    M, a, b = problem(33, 40, 5)
    Mg, ag, bg = gpu(np.stack([M, M.copy()])), gpu(np.stack([a, a])), gpu(np.stack([b, b]))
    n1 = torch.tensor([33, 20], dtype=torch.int32, device=DEV)
    Mq, aq, bq = Mg.clone().requires_grad_(True), ag.clone().requires_grad_(True), bg.clone().requires_grad_(True)
    gout, gT = torch.rand(2, device=DEV), torch.randn(2, 33, 40, device=DEV)
    kw = dict(reg=0.05, num_iter_max=100, stop_thr=1e-5)

    def step(method):
        T, loss, *_ = ops.sinkhorn_unrolled(Mq, aq, bq, n1=n1, method=method, **kw)
        torch.autograd.backward([loss, T], [gout, gT])

    step("sinkhorn_log")                                                   # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for method in ("sinkhorn_log", "sinkhorn"):
            step(method)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(Mq.grad).all() and torch.isfinite(aq.grad).all() and torch.isfinite(bq.grad).all()
    with pytest.raises(RuntimeError):                                      # no double backward
        x = gpu(M).requires_grad_(True)
        (g,) = torch.autograd.grad(ops.sinkhorn_unrolled(x[None], reg=0.05)[1].sum(), x, create_graph=True)
        g.sum().backward()


def test_wasserstein_pairwise_distances_unrolled():
    sizes = (5, 7, 7, 12)
    g = torch.Generator().manual_seed(0)
    Ys = [(0.4 * torch.randn(n, 4, generator=g)).to(DEV) for n in sizes]
    ps = [torch.rand(n, generator=g) + 0.1 for n in sizes]
    ps = [(p / p.sum()).to(DEV) for p in ps]
    kw = dict(reg=0.1, method="sinkhorn_log", numItermax=100, stopThr=1e-5)
    Yq, pq = [y.clone().requires_grad_(True) for y in Ys], [p.clone().requires_grad_(True) for p in ps]
    D = sk.wasserstein_pairwise_distances(Yq, pq, grad="unrolled", **kw)
    G = len(sizes)
    assert D.requires_grad and torch.equal(bits(D.detach()), bits(sk.wasserstein_pairwise_distances(Ys, ps, **kw)))
    for i in range(G):
        for j in range(i + 1, G):
            got = torch.autograd.grad(D[i, j], [Yq[i], Yq[j], pq[i], pq[j]], retain_graph=True)
            yi, yj, pi, pj = (t.clone().requires_grad_(True) for t in (Ys[i], Ys[j], ps[i], ps[j]))
            one = sk.sinkhorn2(pi, pj, feature_cost(yi, yj), kw["reg"], method=kw["method"], numItermax=100, stopThr=1e-5, grad="unrolled")
            assert torch.equal(bits(one.detach()), bits(D[i, j].detach()))
            want = torch.autograd.grad(one, [yi, yj, pi, pj])
            for name, x, y in zip(("Y_i", "Y_j", "p_i", "p_j"), got, want):
                e = rel(x.cpu().numpy(), y.cpu().numpy())
                print(f"pair ({i}, {j}) {name}: rel {e:.2e}")
                assert e <= TOL and y.abs().max() > 0, (i, j, name, e)
    w = torch.rand(G, G, generator=torch.Generator().manual_seed(2)).to(DEV)
    (D * w).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in pq)
    assert all(y.grad is not None and torch.isfinite(y.grad).all() and y.grad.abs().max() > 0 for y in Yq)
