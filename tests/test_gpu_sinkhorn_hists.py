"""Sinkhorn-Knopp for several histograms at once (a 2-D b) on the GPU: csrc/sinkhorn_hists.hip through its C ABI (conan_sinkhorn_hists_fwd,
conan_sinkhorn_hists_loss_bwd, with conan_sinkhorn_hists_workspace_bytes, conan_sinkhorn_hists_lds_resident and conan_sinkhorn_hists_max_hists),
ops.sinkhorn_hists_batched / sinkhorn_hists_loss and conan_fgw_amd.sinkhorn.

Yardstick: the stored fp64 runs of the reference's sinkhorn_knopp with b [n2,H] on fp32-rounded inputs (tests/golden/hists_sinkhorn_*.npz, held
to the restatement tests/sinkhorn_hists_ref.py by tests/test_sinkhorn_hists_cpu.py).  The kernel iterates in fp64, so, with the tolerances of
tests/test_gpu_sinkhorn.py for the 1-D kernel:
  niter, flags and the number of checks equal r64's; errs within rtol 2e-3 of r64_err plus 1e-3 stopThr absolute (every fixture keeps its checks
  a factor 1.5 away from the threshold), NaN beyond the executed checks;
  every cost within 1e-4 relative of r64_loss; exp(log_u), exp(log_v) within 1e-4 of r64_u, r64_v (Frobenius norm of the difference over that
  of the yardstick);
  the gradient of sum_k g_k loss_k to M within 1e-4 (same norm) of the restatement's K o sum_k g_k u_k v_k^T at r64's u, v."""
import os
import warnings

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, ops
from conan_fgw_amd import sinkhorn as sk

from sinkhorn_hists_ref import loss_grad_M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["1x5_h2", "7x12_h3", "20x25_h1", "33x33_h5", "33x33_h16", "33x33_h17", "64x80_h33", "257x65_h4", "65x257_h4", "zeroa", "warm", "numerr"]
STREAMED = ("257x65_h4", "65x257_h4")
DEV = "cuda"
_NOCONV = "Sinkhorn did not converge. You might want to increase the number of iterations `numItermax` or the regularization parameter `reg`."
_CACHE = {}


def load(name):
    if name not in _CACHE:
        z = np.load(os.path.join(GOLDEN, f"hists_sinkhorn_{name}.npz"))
        _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


def gpu(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dtype).to(DEV)


def bits(t):
    return t.contiguous().reshape(-1).view(torch.int32).cpu()


def params(f):
    return dict(reg=float(f["reg"]), num_iter_max=int(f["numItermax"]), stop_thr=float(f["stopThr"]))


def warm_of(f, batch=True):
    if "warm_u" not in f:
        return None
    return (gpu(f["warm_u"])[None], gpu(f["warm_v"])[None]) if batch else (gpu(f["warm_u"]), gpu(f["warm_v"]))


def solve_op(f):
    """The fixture as B = 1 through ops.sinkhorn_hists_batched in its own container."""
    return ops.sinkhorn_hists_batched(gpu(f["M"])[None], gpu(f["a"])[None], gpu(f["b"])[None], warmstart=warm_of(f), **params(f))


def check(f, loss, log_u, log_v, info, errs, tag):
    """The yardsticks of the module docstring on numpy outputs without the batch axis."""
    warn, thr, r64_err = str(f["r64_warn"]), float(f["stopThr"]), np.asarray(f["r64_err"], dtype=np.float64)
    niter, flags, nchk, last = (int(v) for v in info)
    n = len(r64_err)
    errs = np.asarray(errs, dtype=np.float64)
    el = float(np.max(np.abs(loss.astype(np.float64) - f["r64_loss"]) / np.abs(f["r64_loss"])))
    with np.errstate(all="ignore"):
        eu, ev = rel(np.exp(log_u.astype(np.float64)), f["r64_u"]), rel(np.exp(log_v.astype(np.float64)), f["r64_v"])
    print(f"{tag}: niter {niter} (r64 {int(f['r64_niter'])}) flags {flags} checks {nchk} errs {errs[:n][-2:]} r64 {r64_err[-2:]} loss {el:.2e} u {eu:.2e} v {ev:.2e}")
    assert niter == int(f["r64_niter"]) and nchk == n and last == 0, (tag, niter, nchk)
    assert flags == (1 if warn == "" else (2 if warn == "numerr" else 0)), (tag, flags, warn)
    assert np.all(np.abs(errs[:n] - r64_err) <= 2e-3 * np.abs(r64_err) + 1e-3 * thr), (tag, errs[:n], r64_err)
    assert np.isnan(errs[n:]).all() and len(errs) == (int(f["numItermax"]) + 9) // 10, (tag, errs)
    assert el <= 1e-4 and eu <= 1e-4 and ev <= 1e-4, (tag, el, eu, ev)


@pytest.mark.parametrize("name", CASES)
def test_fixture_through_the_c_abi(name):
    f = load(name)
    L = _lib.lib()
    (n1, n2), H = f["M"].shape, f["b"].shape[1]
    it = int(f["numItermax"])
    assert H <= L.conan_sinkhorn_hists_max_hists(n1, n2)
    assert L.conan_sinkhorn_hists_lds_resident(n1, n2, H) == int(name not in STREAMED)
    M, a, b = gpu(f["M"]), gpu(f["a"]), gpu(f["b"])
    wu, wv = (gpu(f["warm_u"]), gpu(f["warm_v"])) if "warm_u" in f else (None, None)
    new = lambda *shape, dtype=torch.float32: torch.full(shape, 7, dtype=dtype, device=DEV)
    loss, log_u, log_v, info, errs = new(1, H), new(1, n1, H), new(1, n2, H), new(1, 4, dtype=torch.int32), new(1, (it + 9) // 10)
    ws = torch.empty(L.conan_sinkhorn_hists_workspace_bytes(1, n1, n2, H), dtype=torch.uint8, device=DEV)
    p = _lib.ptr
    _lib.call("conan_sinkhorn_hists_fwd", p(M), p(a), p(b), p(wu), p(wv), None, None, None, 1, n1, n2, H, n1 * n2, float(f["reg"]), it,
              float(f["stopThr"]), p(loss), p(log_u), p(log_v), p(info), p(errs), p(ws), _lib.stream_ptr())
    out = [t[0].cpu().numpy() for t in (loss, log_u, log_v, info, errs)]
    check(f, *out, tag=name)
    if name == "zeroa":
        assert (out[1][3] == -np.inf).all() and np.isfinite(out[0]).all()  # a massless row: u = 0 in every histogram
    if name == "numerr":                                                   # the previous (start) values, restored for ALL histograms
        assert np.allclose(np.exp(out[1]), 1.0 / n1, rtol=1e-6) and np.allclose(np.exp(out[2]), 1.0 / n2, rtol=1e-6)
    # the op is this launch
    got = solve_op(f)
    for x, y in zip(got, (loss, log_u, log_v, info, errs)):
        assert torch.equal(bits(x), bits(y))


def test_joint_stop_is_not_the_columns_own_stops():
    f = load("64x80_h33")
    k, H = int(f["early_col"]), f["b"].shape[1]
    info = solve_op(f)[3]
    niter = int(info[0, 0])
    assert niter == int(f["r64_niter"])
    # the same columns as H problems of the existing 1-D kernel, M shared: each stops on its own
    cols = ops.sinkhorn_batched(gpu(f["M"]), gpu(f["a"])[None].expand(H, -1), gpu(f["b"]).t(), method="sinkhorn", **params(f))[4][:, 0].cpu().numpy()
    print("joint", niter, "alone", cols, "r64 alone", f["r64_niter_cols"])
    assert cols[k] == int(f["r64_niter_cols"][k]) < niter and cols.min() < niter and (cols != niter).any()


def test_bits_do_not_depend_on_batch_position_or_container():
    names = ["7x12_h3", "33x33_h17", "33x33_h5", "1x5_h2"]                 # both product forms, ragged in all three sizes
    fs = [load(n) for n in names]
    alone = [solve_op(f) for f in fs[:3]]                                  # (the three that share reg, numItermax and stopThr with the batch below)
    prm = [params(f) for f in fs]
    assert prm[1] == prm[2]

    def batch(idx, N1, N2, H):
        B = len(idx)
        M, a, b = torch.full((B, N1, N2), 3.0, device=DEV), torch.full((B, N1), 5.0, device=DEV), torch.full((B, N2, H), 9.0, device=DEV)
        for p, i in enumerate(idx):
            (m1, m2), nh = fs[i]["M"].shape, fs[i]["b"].shape[1]
            M[p, :m1, :m2], a[p, :m1], b[p, :m2, :nh] = gpu(fs[i]["M"]), gpu(fs[i]["a"]), gpu(fs[i]["b"])
        size = lambda ax: torch.tensor([(fs[i]["M"].shape + fs[i]["b"].shape[1:])[ax] for i in idx], dtype=torch.int32, device=DEV)
        return M, a, b, dict(n1=size(0), n2=size(1), nh=size(2))

    def same(out, p, i, ref):
        (m1, m2), nh = fs[i]["M"].shape, fs[i]["b"].shape[1]
        loss, lu, lv, info, errs = out
        assert torch.equal(bits(loss[p, :nh]), bits(ref[0][0])) and torch.equal(bits(lu[p, :m1, :nh]), bits(ref[1][0]))
        assert torch.equal(bits(lv[p, :m2, :nh]), bits(ref[2][0])) and torch.equal(info[p].cpu(), ref[3][0].cpu()) and torch.equal(bits(errs[p]), bits(ref[4][0]))
        assert not loss[p, nh:].any() and not lu[p, m1:].any() and not lu[p, :, nh:].any() and not lv[p, m2:].any() and not lv[p, :, nh:].any()

    # 33x33_h17 and 33x33_h5 at other positions of a ragged batch in a larger container (LDS-resident)
    M, a, b, sizes = batch([2, 1, 2], 40, 45, 20)
    assert _lib.lib().conan_sinkhorn_hists_lds_resident(40, 45, 20) == 1
    out = ops.sinkhorn_hists_batched(M, a, b, **sizes, **prm[1])
    same(out, 0, 2, alone[2]); same(out, 1, 1, alone[1]); same(out, 2, 2, alone[2])
    # ... and in a container whose K is streamed from the workspace
    M, a, b, sizes = batch([1, 2], 150, 150, 17)
    assert _lib.lib().conan_sinkhorn_hists_lds_resident(150, 150, 17) == 0
    out = ops.sinkhorn_hists_batched(M, a, b, **sizes, **prm[1])
    same(out, 0, 1, alone[1]); same(out, 1, 2, alone[2])
    # the dot form (H <= 4): 7x12_h3 behind a 1x5_h2, padded
    M, a, b, sizes = batch([3, 0], 9, 14, 4)
    out = ops.sinkhorn_hists_batched(M, a, b, **sizes, **prm[0])
    same(out, 1, 0, alone[0])
    # an M shared by the batch (stride 0) or spelt out per problem
    f = fs[2]
    Ms, aa, bb = gpu(f["M"]), torch.stack([gpu(f["a"])] * 2), torch.stack([gpu(f["b"])] * 2)
    o1, o2 = ops.sinkhorn_hists_batched(Ms, aa, bb, **prm[2]), ops.sinkhorn_hists_batched(Ms[None].expand(2, -1, -1), aa, bb, **prm[2])
    for x, y, z in zip(o1, o2, alone[2]):
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x[0]), bits(x[1])) and torch.equal(bits(x[0]), bits(z[0]))


@pytest.mark.parametrize("name", ["33x33_h5", "7x12_h3", "numerr", "warm", "20x25_h1"])
def test_knopp_entry_points_are_the_op(name):
    f = load(name)
    a, b, M = gpu(f["a"]), gpu(f["b"]), gpu(f["M"])
    (n1, n2), H = f["M"].shape, f["b"].shape[1]
    kw = dict(numItermax=int(f["numItermax"]), stopThr=float(f["stopThr"]), warmstart=warm_of(f, batch=False))
    loss, log_u, log_v, info, errs = solve_op(f)
    want = {"": [], "noconv": [_NOCONV], "numerr": ["Warning: numerical errors at iteration 0"]}[str(f["r64_warn"])]
    calls = [lambda **k: sk.sinkhorn_knopp(a, b, M, float(f["reg"]), **kw, **k), lambda **k: sk.sinkhorn(a, b, M, float(f["reg"]), method="sinkhorn", **kw, **k),
             lambda **k: sk.sinkhorn2(a, b, M, float(f["reg"]), method="sinkhorn", **kw, **k)]
    for fn in calls:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            res, log = fn(log=True, warn=True)
            plain = fn(warn=True)
        assert [str(x.message) for x in w] == want + want
        assert res.shape == (H,) and torch.equal(bits(res), bits(loss[0])) and torch.equal(bits(plain), bits(loss[0]))
        assert set(log) == {"err", "niter", "u", "v"} and isinstance(log["niter"], int) and log["niter"] == int(info[0, 0]) == int(f["r64_niter"])
        assert isinstance(log["err"], list) and len(log["err"]) == len(f["r64_err"])
        assert all(float(e) == float(errs[0, i]) for i, e in enumerate(log["err"]))
        assert log["u"].shape == (n1, H) and log["v"].shape == (n2, H)
        assert torch.equal(bits(log["u"]), bits(torch.exp(log_u[0]))) and torch.equal(bits(log["v"]), bits(torch.exp(log_v[0])))
    with warnings.catch_warnings(record=True) as w:                        # warn=False silences "did not converge" only
        warnings.simplefilter("always")
        sk.sinkhorn2(a, b, M, float(f["reg"]), method="sinkhorn", **kw)
    assert [str(x.message) for x in w] == (want if str(f["r64_warn"]) == "numerr" else [])
    if name == "33x33_h5":                                                 # an empty a means uniform, as in the reference
        u1 = sk.sinkhorn_knopp(torch.empty(0, device=DEV), b, M, float(f["reg"]), **kw)
        u2 = ops.sinkhorn_hists_batched(M[None], None, b[None], **params(f))[0][0]
        assert torch.equal(bits(u1), bits(u2))


@pytest.mark.parametrize("name", ["33x33_h5", "20x25_h1", "7x12_h3"])
def test_sinkhorn_log_entry_points_are_the_columns_solved_alone(name):
    f = load(name)
    a, b, M, reg = gpu(f["a"]), gpu(f["b"]), gpu(f["M"]), float(f["reg"])
    (n1, n2), H = f["M"].shape, f["b"].shape[1]
    kw = dict(numItermax=int(f["numItermax"]), stopThr=float(f["stopThr"]))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cols = [sk.sinkhorn2(a, b[:, k].contiguous(), M, reg, method="sinkhorn_log", log=True, warn=False, **kw) for k in range(H)]
    assert not w
    ran_out = any(c[1]["niter"] == kw["numItermax"] - 1 and float(c[1]["err"][-1]) >= kw["stopThr"] for c in cols)
    assert ran_out == (name == "7x12_h3")
    want = [_NOCONV] if ran_out else []                                    # once, whatever `warn` says: the reference's inner calls warn by default
    calls = [lambda **k: sk.sinkhorn_log(a, b, M, reg, **kw, **k), lambda **k: sk.sinkhorn(a, b, M, reg, method="sinkhorn_log", **kw, **k),
             lambda **k: sk.sinkhorn2(a, b, M, reg, method="sinkhorn_log", **kw, **k)]
    for fn in calls:
        for warn in (True, False):
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                res, log = fn(log=True, warn=warn)
                plain = fn(warn=warn)
            assert [str(x.message) for x in w] == want + want
            assert res.shape == (H,) and torch.equal(bits(plain), bits(res))
            assert set(log) == {"log_u", "log_v", "u", "v"} and log["log_u"].shape == (n1, H) and log["log_v"].shape == (n2, H)
            for k in range(H):
                assert torch.equal(bits(res[k]), bits(cols[k][0]))
                assert torch.equal(bits(log["log_u"][:, k]), bits(cols[k][1]["log_u"])) and torch.equal(bits(log["log_v"][:, k]), bits(cols[k][1]["log_v"]))
            assert torch.equal(bits(log["u"]), bits(torch.exp(log["log_u"]))) and torch.equal(bits(log["v"]), bits(torch.exp(log["log_v"])))
    if name == "33x33_h5":                                                 # a warm-start list: one (log u, log v) pair per column
        warm = [(cols[k][1]["log_u"], cols[k][1]["log_v"]) for k in range(H)]
        res = sk.sinkhorn_log(a, b, M, reg, warmstart=warm, **kw)
        one = [sk.sinkhorn2(a, b[:, k].contiguous(), M, reg, method="sinkhorn_log", warmstart=warm[k], **kw) for k in range(H)]
        assert all(torch.equal(bits(res[k]), bits(one[k])) for k in range(H))
        with pytest.raises(ValueError, match="one .log u, log v. pair per column"):
            sk.sinkhorn_log(a, b, M, reg, warmstart=warm[:2], **kw)


def test_refusals_on_the_gpu():
    f = load("7x12_h3")
    a, b, M = gpu(f["a"]), gpu(f["b"]), gpu(f["M"])
    for fn in (sk.sinkhorn, sk.sinkhorn2, sk.sinkhorn_log, sk.sinkhorn_knopp):
        with pytest.raises(NotImplementedError, match="grad='unrolled' is not implemented for several histograms"):
            fn(a, b, M, 0.1, grad="unrolled")
    for m in ("sinkhorn", "sinkhorn_log"):
        with pytest.raises(NotImplementedError, match="grad='unrolled' is not implemented for several histograms"):
            sk.sinkhorn2(a, b, M, 0.1, method=m, grad="unrolled")
    for fn in (sk.greenkhorn, sk.sinkhorn_stabilized, sk.sinkhorn_epsilon_scaling):
        with pytest.raises(NotImplementedError, match="several histograms"):
            fn(a, b, M, 0.1)
    for m in ("greenkhorn", "sinkhorn_stabilized", "sinkhorn_epsilon_scaling"):
        with pytest.raises(NotImplementedError, match="several histograms"):
            sk.sinkhorn(a, b, M, 0.1, method=m)
    with pytest.raises(NotImplementedError, match="several histograms at once .a 2-D b. run on the GPU only"):
        sk.sinkhorn2(a, b.cpu(), M, 0.1)
    hmax = _lib.lib().conan_sinkhorn_hists_max_hists(7, 12)
    with pytest.raises(RuntimeError, match="conan_sinkhorn_hists_fwd failed: unsupported configuration"):      # past the vector bound: refused, never launched
        ops.sinkhorn_hists_batched(M[None], a[None], torch.ones(1, 12, hmax + 1, device=DEV) / 12, reg=0.1)
    with pytest.raises(ValueError, match="b must have shape"):
        ops.sinkhorn_hists_batched(M[None], a[None], torch.ones(1, 11, 3, device=DEV), reg=0.1)
    with pytest.raises(ValueError, match=r"b must be \[B,N2,H\]"):
        ops.sinkhorn_hists_batched(M[None], a[None], b, reg=0.1)


def test_fixed_plan_gradient_per_problem():
    """Two ragged problems with their own M: each block of M.grad is K o sum_k g_k u_k v_k^T at the fixture's r64 u, v; zero outside the block."""
    fa, fb = load("33x33_h5"), load("20x25_h1")
    M = torch.zeros(2, 33, 33, device=DEV)
    M[0], M[1, :20, :25] = gpu(fa["M"]), gpu(fb["M"])
    a, b = torch.zeros(2, 33, device=DEV), torch.zeros(2, 33, 5, device=DEV)
    a[0], a[1, :20], b[0], b[1, :25, :1] = gpu(fa["a"]), gpu(fb["a"]), gpu(fa["b"]), gpu(fb["b"])
    M.requires_grad_(True); a.requires_grad_(True); b.requires_grad_(True)
    size = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    n1, n2, nh = size(33, 20), size(33, 25), size(5, 1)
    loss = ops.sinkhorn_hists_loss(M, a, b, n1=n1, n2=n2, nh=nh, **params(fa))
    assert loss.shape == (2, 5) and loss.requires_grad
    g = np.array([[0.5, -1.25, 2.0, 1.0, 0.25], [3.0, 99.0, 99.0, 99.0, 99.0]])
    (loss * gpu(g)).sum().backward()
    assert a.grad is None and b.grad is None
    dM = M.grad.cpu().numpy()
    wa = loss_grad_M(fa["M"], fa["r64_u"], fa["r64_v"], g[0], float(fa["reg"]))
    wb = loss_grad_M(fb["M"], fb["r64_u"], fb["r64_v"], g[1, :1], float(fb["reg"]))
    ea, eb = rel(dM[0], wa), rel(dM[1, :20, :25], wb)
    print(f"dM per problem: {ea:.2e} {eb:.2e}")
    assert ea <= 1e-4 and eb <= 1e-4
    assert not dM[1, 20:].any() and not dM[1, :, 25:].any()
    # through the C entry point: the same launch
    out = ops.sinkhorn_hists_batched(M.detach(), a.detach(), b.detach(), n1=n1, n2=n2, nh=nh, **params(fa))
    dM2, gg, Md = torch.full((2, 33, 33), 7.0, device=DEV), gpu(g), M.detach()
    p = _lib.ptr
    _lib.call("conan_sinkhorn_hists_loss_bwd", p(Md), p(out[1]), p(out[2]), p(gg), p(n1), p(n2), p(nh), 2, 33, 33, 5, 33 * 33, float(fa["reg"]), p(dM2),
              _lib.stream_ptr())
    assert torch.equal(bits(dM2), bits(M.grad))


def test_fixed_plan_gradient_to_a_shared_M():
    """One M [N1,N2] for B = 2 problems (the fixture's columns, and the same columns in another order): M.grad is the sum over the problems."""
    f = load("33x33_h17")
    perm = np.roll(np.arange(17), 5)
    M = gpu(f["M"]).requires_grad_(True)
    a = torch.stack([gpu(f["a"])] * 2).requires_grad_(True)
    b = torch.stack([gpu(f["b"]), gpu(f["b"][:, perm])]).requires_grad_(True)
    loss, log_u, log_v, info, errs = ops.sinkhorn_hists_loss(M, a, b, return_log=True, **params(f))
    assert loss.requires_grad and not log_u.requires_grad and info[:, 0].tolist() == [int(f["r64_niter"])] * 2
    g = np.random.default_rng(5).standard_normal((2, 17))
    (loss * gpu(g)).sum().backward()
    assert M.grad.shape == (33, 33) and a.grad is None and b.grad is None
    want = loss_grad_M(f["M"], f["r64_u"], f["r64_v"], g[0], float(f["reg"])) + loss_grad_M(f["M"], f["r64_u"][:, perm], f["r64_v"][:, perm], g[1], float(f["reg"]))
    e = rel(M.grad.cpu().numpy(), want)
    print(f"dM shared: {e:.2e}")
    assert e <= 1e-4
    # sinkhorn2's costs carry it (grad="plan")
    M2 = gpu(f["M"]).requires_grad_(True)
    cost = sk.sinkhorn2(gpu(f["a"]), gpu(f["b"]), M2, float(f["reg"]), numItermax=int(f["numItermax"]), stopThr=float(f["stopThr"]))
    (cost * gpu(g[0])).sum().backward()
    e2 = rel(M2.grad.cpu().numpy(), loss_grad_M(f["M"], f["r64_u"], f["r64_v"], g[0], float(f["reg"])))
    print(f"dM through sinkhorn2: {e2:.2e}")
    assert e2 <= 1e-4
    with pytest.raises(RuntimeError):                                      # no double backward
        M3 = gpu(f["M"]).requires_grad_(True)
        l3 = ops.sinkhorn_hists_loss(M3, None, b.detach()[:1], **params(f))
        (g3,) = torch.autograd.grad(l3.sum(), M3, create_graph=True)
        g3.sum().backward()
