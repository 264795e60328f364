"""Every Linear and weight-gradient kernel on its own against the plain fp64 reference of the same operation (tests/dense_ref.py).

The 19 entry points named in OWNED (conan_linear_fwd / _act_fwd / _multi_fwd / _sum_fwd, the weight gradients in their immediate, scaled, RBF and
deferred forms, the two chained-Linear kernels of mlp2.hip) are called as C entry points (`raw`: the status code is visible) at the shapes at which
the host dispatch takes another path — dense_ref.linear_branch / wgrad_branch name the path, tests/test_dense_ref_cpu.py asserts that the case
lists reach every one — at the row counts around the tiles, at every device-side row count, on rows of very different magnitude and on
non-finite values.

Judging (visnet_ref.judge, unchanged): per row and per tensor, err(gpu, ref64) <= MARGIN * err(ref32, ref64) — the yardstick is the reference
formula in fp32 on the CPU, never the kernel; where that yardstick is 0 (the fp32 reference is exact) the kernel has to be exact too.  Every output
buffer and workspace is pre-filled with a NaN bit pattern and has a tail of 64 floats that must survive; every input sits in front of the same
pattern, and with a device-side row count the rows at and beyond it hold the pattern too, so that an over-read poisons a result; every case runs
twice and must give the same bits in every buffer.  The `RATIO` / `TABLE` lines printed by a run (-s) are the source of the table in DESIGN.md
section 3.9."""
import ctypes

import pytest
import torch

import dense_ref as D
import visnet_ref as R
from conan_fgw_amd import _lib
from conan_fgw_amd._lib import WgradJob, WgradSlabJob, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
f32, f64, i32 = torch.float32, torch.float64, torch.int32
OK, E_BADARG, E_UNSUPPORTED = 0, -1, -3
SENT, TAIL = 0x7FA5A5A5, 64              # a NaN bit pattern: reading it poisons a result, overwriting it is visible; floats beyond every documented size
CALLED, RATIOS, BRANCHES = set(), {}, set()
SHARED = (R.MARGIN_ROW, R.MARGIN_ALL)
# Outputs that need more than the shared margins: output -> (row, whole tensor) = 2 x the ratio measured on the MI355X against the fp32 reference's
# own error.  Measured values and reasons: DESIGN.md section 3.9.
DENSE_MARGIN = {
    # N <= 5 on the scalar reducers: the whole output is one to five numbers, each the sum of 4097 .. 5000 terms that the kernel adds serially in
    # 16-row stages per slice and then over 33 .. 40 slices in two levels, where torch's fp32 sum (the yardstick) is pairwise and so unusually
    # good: measured 7.7 (M = 5000, K = 128, N = 1), 5.04 and 4.12 at M = 4097, at most 3.8 up to M = 4096 and 1.1 from N = 52 on
    "wgrad.scalar.dbias/N<=5": (15.4, 15.4),
}

OWNED = ["conan_linear_fwd", "conan_linear_act_fwd", "conan_linear_multi_fwd", "conan_linear_sum_fwd",
         "conan_linear_wgrad_ws", "conan_linear_wgrad", "conan_linear_wgrad_scaled", "conan_rbf_wgrad",
         "conan_wgrad_batchable", "conan_linear_wgrad_slabs", "conan_rbf_wgrad_slabs", "conan_wgrad_reduce_batch", "conan_linear_wgrad_slabs_batch",
         "conan_mlp2_supported", "conan_mlp2_fwd", "conan_mlp2_bwd",
         "conan_mlp2_outact_supported", "conan_mlp2_outact_fwd", "conan_mlp2_outact_bwd"]


def raw(name, *args):
    """The C entry point itself: returns the status code instead of raising."""
    CALLED.add(name)
    return getattr(lib(), name)(*args)


def sent(numel):
    """A buffer of `numel` floats and the tail, all of the NaN pattern."""
    return torch.full((numel + TAIL,), SENT, dtype=i32, device=dev).view(f32)


def is_sent(t):
    return bool((t.contiguous().view(i32) == SENT).all())


def cut(t, numel, what=""):
    """The documented part of a buffer (CPU); the tail must still hold the pattern."""
    assert is_sent(t[numel:]), (what, "written beyond its documented size")
    return t[:numel].cpu()


def put(t, live=None):
    """A CPU tensor on the device in front of the pattern; rows at and beyond `live` hold the pattern too."""
    t = t.contiguous()
    buf = sent(t.numel())
    if t.numel():
        v = buf[:t.numel()].view(t.shape)
        if live is None:
            v.copy_(t)
        else:
            v[:live].copy_(t[:live])
    return buf


def mdev(m):
    return None if m is None else torch.tensor([m], dtype=i32, device=dev)


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def twice(fn):
    """Run a case twice on fresh buffers: the same bits in every buffer (tails and workspaces included)."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert same_bits(a, b), "two runs differ"
    return a


def both(fn, *floats):
    """(ref32, ref64) of a reference formula: the same function on the fp32 inputs and on their fp64 copies (CPU)."""
    return fn(*floats), fn(*[None if t is None else t.double() for t in floats])


def judge(fails, case, what, got, r32, r64):
    assert got.shape == r64.shape, (case, what, got.shape, r64.shape)
    mr, ma = DENSE_MARGIN.get(what, SHARED)
    ok, rr, ra = R.judge(got, r32, r64, mr, ma)
    old = RATIOS.get(what, (0.0, 0.0))
    RATIOS[what] = (max(old[0], rr), max(old[1], ra))
    print(f"RATIO {case} {what} row={rr:.3g} all={ra:.3g}")
    if not ok:
        fails.append((case, what, float("%.3g" % rr), float("%.3g" % ra)))


def own_norm(a, r64):
    """max over rows of ||a_row - ref_row|| / ||ref_row|| (rows whose reference is all zero are left out: they must be exactly zero)."""
    nz = r64.norm(dim=1) > 0
    return float(((a.double() - r64)[nz].norm(dim=1) / r64[nz].norm(dim=1)).max()) if bool(nz.any()) else 0.0


def judge_own(fails, case, what, got, r32, r64):
    """Every row against its own norm; all-zero reference rows exactly zero."""
    zero = r64.norm(dim=1) == 0
    if bool(zero.any()) and float(got[zero].abs().max()) != 0.0:
        fails.append((case, what, "a row whose reference is all zero is not"))
    e, y = own_norm(got, r64), own_norm(r32, r64)
    ratio = e / y if y > 0 else (0.0 if e == 0 else float("inf"))
    old = RATIOS.get(what + "/own", (0.0, 0.0))
    RATIOS[what + "/own"] = (max(old[0], ratio), 0.0)
    print(f"RATIO {case} {what}/own row={ratio:.3g} all=0")
    if e > DENSE_MARGIN.get(what + "/own", SHARED)[0] * y:
        fails.append((case, what + "/own", float("%.3g" % ratio)))


# ================================================================================================ Linear forward
def run_linear(c, x, w, b, r):
    """One LinCase through conan_linear_fwd (conan_linear_act_fwd when the pre-activation is wanted), twice."""
    live = c.M if c.m is None else min(c.m, c.M)
    lv = None if c.m is None else live
    xd, wd, bd, rd = put(x, lv), put(w), put(b) if c.bias else None, put(r, lv) if c.res else None
    md, s = mdev(c.m), stream_ptr()

    def run():
        o = {"y": sent(c.M * c.N)}
        if c.pre:
            o["pre"] = sent(c.M * c.N)
            rc = raw("conan_linear_act_fwd", ptr(xd), ptr(wd), ptr(bd), c.M, c.K, c.N, c.act, ptr(md), ptr(o["y"]), ptr(o["pre"]), s)
        else:
            rc = raw("conan_linear_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(rd), c.M, c.K, c.N, c.w_kn, c.act, ptr(md), ptr(o["y"]), s)
        assert rc == OK, (c.name, rc)
        return o
    return twice(run), live


def fam_of(branch):
    return branch.split("/")[0]


def check_linear(fails, c, o, live, x, w, b, r):
    fam = fam_of(c.branch)
    BRANCHES.add(c.branch)
    for k in o:
        assert is_sent(o[k][live * c.N:]), (c.name, k, "rows at or beyond the row count were written")
    if not live:
        return
    (y32, p32), (y64, p64) = both(lambda x_, w_, b_, r_: D.linear(x_, w_, b_, r_, c.w_kn, c.act), x[:live], w, b if c.bias else None,
                                  r[:live] if c.res else None)
    judge(fails, c.name, f"linear.{fam}.y", o["y"][:live * c.N].cpu().view(live, c.N), y32, y64)
    if c.pre:
        judge(fails, c.name, f"linear.{fam}.pre", o["pre"][:live * c.N].cpu().view(live, c.N), p32, p64)


def _by_shape(cases):
    d = {}
    for c in cases:
        d.setdefault(c.name.split(":")[0], []).append(c)
    return d


LIN = _by_shape(D.linear_cases())
EDGE = _by_shape(D.edge_cases())


@pytest.mark.parametrize("shape", list(LIN))
def test_linear_forward(shape):
    """Every (K, N) of dense_ref.linear_cases: act 0 / 1 / 3 with and without bias and residual, act 2 and W as [K,N] where listed, the
    pre-activation through conan_linear_act_fwd, a device row count; (128, 128) also on the second pass of the narrow persistent loop and on
    both sides of the narrow / wide switch, (96, 100) on the second pass of the 512-tile loop."""
    fails = []
    for c in LIN[shape]:
        x, w, b, r = D.linear_inputs(c.M, c.K, c.N, c.w_kn, c.act)
        o, live = run_linear(c, x, w, b, r)
        check_linear(fails, c, o, live, x, w, b, r)
    assert not fails, fails


@pytest.mark.parametrize("shape", list(EDGE))
def test_linear_row_counts_and_device_row_counts(shape):
    """M in {63, 64, 65, 127, 128, 129}; *m_dev in {0, 1, 33, M, M + 5} at M = 70: rows from min(M, *m_dev) on keep the pattern in y and pre,
    and the rows of x and residual there are never read (they hold the NaN pattern)."""
    fails = []
    for c in EDGE[shape]:
        x, w, b, r = D.linear_inputs(c.M, c.K, c.N, c.w_kn, c.act)
        o, live = run_linear(c, x, w, b, r)
        check_linear(fails, c, o, live, x, w, b, r)
    assert not fails, fails


def test_linear_status_codes_and_no_rows():
    x, w, b, y, s = put(torch.randn(8, 128)), put(torch.randn(128, 128)), put(torch.randn(128)), sent(8 * 128), stream_ptr()
    pre = sent(8 * 128)
    lin = lambda *a: raw("conan_linear_fwd", *a)
    assert lin(None, ptr(w), ptr(b), None, 8, 128, 128, 0, 0, None, ptr(y), s) == E_BADARG
    assert lin(ptr(x), None, ptr(b), None, 8, 128, 128, 0, 0, None, ptr(y), s) == E_BADARG
    assert lin(ptr(x), ptr(w), ptr(b), None, 8, 128, 128, 0, 0, None, None, s) == E_BADARG
    assert lin(ptr(x), ptr(w), ptr(b), None, -1, 128, 128, 0, 0, None, ptr(y), s) == E_BADARG
    assert lin(ptr(x), ptr(w), ptr(b), None, 8, 0, 128, 0, 0, None, ptr(y), s) == E_BADARG
    assert lin(ptr(x), ptr(w), ptr(b), None, 8, 128, 0, 0, 0, None, ptr(y), s) == E_BADARG
    assert lin(ptr(x), ptr(w), ptr(b), None, 8, 128, 128, 0, 4, None, ptr(y), s) == E_BADARG
    assert lin(ptr(x), ptr(w), ptr(b), None, 8, 128, 128, 0, -1, None, ptr(y), s) == E_BADARG
    assert lin(ptr(x), ptr(w), ptr(b), None, 8, 128, 128, 0, 2, None, ptr(y), s) == E_BADARG          # act 2 reads the saved output from `residual`
    act = lambda *a: raw("conan_linear_act_fwd", *a)
    assert act(ptr(x), ptr(w), ptr(b), 8, 128, 128, 0, None, ptr(y), ptr(pre), s) == E_BADARG          # act 0 / 2 have no pre-activation to keep
    assert act(ptr(x), ptr(w), ptr(b), 8, 128, 128, 2, None, ptr(y), ptr(pre), s) == E_BADARG
    assert act(ptr(x), ptr(w), ptr(b), 8, 128, 128, 1, None, ptr(y), None, s) == E_BADARG
    assert D.linear_branch(8, 50, 128, 0, 1, True) == "unsupported"
    assert act(ptr(x), ptr(w), ptr(b), 8, 50, 128, 1, None, ptr(y), ptr(pre), s) == E_UNSUPPORTED      # K = 50: compose it
    assert act(ptr(x), ptr(w), ptr(b), 8, 1088, 64, 3, None, ptr(y), ptr(pre), s) == E_UNSUPPORTED
    for K, N in ((128, 128), (256, 128), (128, 256), (256, 256), (96, 100), (50, 128)):                # M = 0 on every family: OK, nothing written
        assert lin(ptr(x), ptr(w), ptr(b), None, 0, K, N, 0, 1, None, ptr(y), s) == OK
    assert act(ptr(x), ptr(w), ptr(b), 0, 128, 128, 1, None, ptr(y), ptr(pre), s) == OK
    torch.cuda.synchronize()
    assert is_sent(y) and is_sent(pre)


@pytest.mark.parametrize("fam,K,N,branch", D.VALUE_SHAPES)
def test_linear_rows_of_very_different_magnitude(fam, K, N, branch):
    """40 rows of N(0, 1) scaled from 1e-5 to 1e5, a zero row, a row with one non-zero element; weights at 1, 1e-4 and 300 times N(0, 1 / K); an
    all-zero weight matrix.  Besides the usual judging every row is held to its own norm."""
    M, fails = 40, []
    assert D.linear_branch(M, K, N, 0, 0, False) == branch
    x = D.decade_rows(M, K)
    _, w0, b, r = D.linear_inputs(M, K, N, 0, 1)
    for tag, wscale, act, bias in (("w1", 1.0, 0, False), ("w1e-4", 1e-4, 0, False), ("w300", 300.0, 0, False), ("w1", 1.0, 1, True), ("w0", 0.0, 0, True),
                                   ("w0", 0.0, 1, True), ("w0", 0.0, 3, True)):
        w = w0 * wscale
        c = D.LinCase(f"{fam}-{K}x{N}:{tag}/act{act}/b{int(bias)}", M, K, N, 0, act, bias, False, False, None, branch)
        o, live = run_linear(c, x, w, b, r)
        check_linear(fails, c, o, live, x, w, b, r)
        got = o["y"][:M * N].cpu().view(M, N)
        (y32, _), (y64, _) = both(lambda x_, w_, b_: D.linear(x_, w_, b_, None, 0, act), x, w, b if bias else None)
        if wscale == 0.0 and act == 0:
            assert torch.equal(got, b.expand(M, N)), "an all-zero weight matrix: y is the bias, exactly"
        if not bias:
            judge_own(fails, c.name, f"linear.{fam_of(branch)}.y", got, y32, y64)
    assert not fails, fails


@pytest.mark.parametrize("fam,K,N,branch", D.VALUE_SHAPES)
def test_linear_a_row_below_the_scale_domain(fam, K, N, branch):
    """One row whose maximum (1e-37) is below 2^-118 among rows of N(0, 1), weights N(0, 1 / K) (and 300 times that).  Outside pow2_scale's domain
    the row scale is 1 (fp_planes.h): on the fp16 kernels the row's elements flush to zero and the row comes out as act(bias), which is its true
    value to 1e-34 — the fp32 kernels compute it as it is.  Held to the absolute bound 8 x 2^-24 x max |ref64|, the maximum taken over the whole
    tensor, whose rows are O(1) here (without bias the row's own reference is 1e-37 and gives no scale), or over the row itself where it has a bias
    and the weights are at 300."""
    M, tiny, fails = 40, 7, []
    x, w0, b, r = D.linear_inputs(M, K, N, 0, 1, seed=4)
    x[tiny] = torch.randn(K, generator=D.gen(3)) * 1e-37
    assert float(x[tiny].abs().max()) < 2.0 ** -118 and float(x[tiny].abs().min()) > 0.0
    for tag, wscale, act, bias in (("w1", 1.0, 0, False), ("w1", 1.0, 0, True), ("w1", 1.0, 1, True), ("w1", 1.0, 3, True), ("w300", 300.0, 1, True)):
        w = w0 * wscale
        c = D.LinCase(f"{fam}-{K}x{N}:tiny/{tag}/act{act}/b{int(bias)}", M, K, N, 0, act, bias, False, False, None, branch)
        o, live = run_linear(c, x, w, b, r)
        check_linear(fails, c, o, live, x, w, b, r)
        got = o["y"][:M * N].cpu().view(M, N)
        y64, _ = D.linear(x.double(), w.double(), b.double() if bias else None, None, 0, act)
        scale = float(y64[tiny].abs().max()) if wscale != 1.0 else float(y64.abs().max())
        assert scale < 16.0, (c.name, scale)                                # O(1): the bound below is a few 1e-6
        err = float((got[tiny].double() - y64[tiny]).abs().max())
        print(f"TINY {c.name} err={err:.3g} bound={8 * 2.0 ** -24 * scale:.3g}")
        assert err <= 8 * 2.0 ** -24 * scale, (c.name, "the tiny row", err)
    assert not fails, fails


NONFINITE_SHAPES = D.VALUE_SHAPES + [("ksum", 256, 128, "ksum2"), ("nc", 128, 256, "chunk_nc/narrow")]


@pytest.mark.parametrize("fam,K,N,branch", NONFINITE_SHAPES)
def test_linear_a_nan_stays_visible_and_stays_where_it_is(fam, K, N, branch):
    """A NaN and a +Inf in one row of x (the row maximum is Inf: pow2_scale's out-of-domain branch) and a lone NaN in another (fmaxf drops it from
    the maximum, the scale comes from the finite rest of the row): those rows of y are non-finite wherever the fp64 reference is, every other row
    has the bits it has with the finite input.  A NaN in one element of W: that column of y is non-finite in every row, the rest is finite and judged as usual."""
    M, bad, lone, fails = 40, 9, 21, []
    act = 0 if fam == "ksum" else 1
    assert D.linear_branch(M, K, N, 0, act, False) == branch
    x, w, b, r = D.linear_inputs(M, K, N, 0, act)
    c = D.LinCase(f"{fam}-{K}x{N}:nonfinite", M, K, N, 0, act, True, True, False, None, branch)
    base, _ = run_linear(c, x, w, b, r)
    xb = x.clone()
    xb[bad, 3], xb[bad, K - 2] = D.NAN, D.INF
    xb[lone, K // 2] = D.NAN
    o, _ = run_linear(c, xb, w, b, r)
    y0, y1 = base["y"][:M * N].cpu().view(M, N), o["y"][:M * N].cpu().view(M, N)
    y64, _ = D.linear(xb.double(), w.double(), b.double(), r.double(), 0, act)
    keep = (torch.arange(M) != bad) & (torch.arange(M) != lone)
    assert bool(torch.isnan(y64[lone]).all()) and bool((~torch.isfinite(y64[bad])).all())
    for row in (bad, lone):
        assert bool((~torch.isfinite(y1[row]))[~torch.isfinite(y64[row])].all()), (row, "a non-finite x row gave finite outputs where the reference has none")
    assert torch.equal(y0[keep].view(i32), y1[keep].view(i32)), "a non-finite x row changed other rows"
    assert bool(torch.isfinite(y0).all())
    wb = w.clone()
    n_bad, k_bad = N - 3, K // 2 + 1
    wb[n_bad, k_bad] = D.NAN
    o, _ = run_linear(c, x, wb, b, r)
    y2 = o["y"][:M * N].cpu().view(M, N)
    cols = torch.arange(N) != n_bad
    assert bool(torch.isnan(y2[:, n_bad]).all()), "a NaN weight did not reach its whole output column"
    assert bool(torch.isfinite(y2[:, cols]).all()), "a NaN weight reached other columns"
    (y32, _), (y64, _) = both(lambda x_, w_, b_, r_: D.linear(x_, w_, b_, r_, 0, act), x, w, b, r)
    judge(fails, c.name + "/nan-weight", f"linear.{fam_of(branch)}.y", y2[:, cols], y32[:, cols], y64[:, cols])
    assert not fails, fails


# ================================================================================================ several layers of one input
def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def run_multi(x, ws, bs, M, K, N, act, pre_mask, m=None, expect=OK):
    """conan_linear_multi_fwd; pre_mask: None (pre == NULL) or one bool per layer.  -> {"y0", "pre0", ...}"""
    L = len(ws)
    lv = None if m is None else min(m, M)
    xd, wd, bd, md, s = put(x, lv), [put(w) for w in ws], None if bs is None else [put(b) for b in bs], mdev(m), stream_ptr()

    def run():
        o = {f"y{q}": sent(M * N) for q in range(L)}
        if pre_mask is not None:
            o.update({f"pre{q}": sent(M * N) for q in range(L)})               # the unwanted ones must keep the pattern
        pre = None if pre_mask is None else _arr([o[f"pre{q}"] if pre_mask[q] else None for q in range(L)])
        rc = raw("conan_linear_multi_fwd", ptr(xd), _arr(wd), None if bd is None else _arr(bd), M, K, N, L, act, ptr(md), _arr([o[f"y{q}"] for q in range(L)]),
                 pre, s)
        assert rc == expect, rc
        return o
    return twice(run)


multi_inputs = D.multi_inputs


def single_layer(x, w, b, M, K, N, act, want_pre, m=None):
    """The single conan_linear_fwd / conan_linear_act_fwd call a layer of the multi form is compared with."""
    c = D.LinCase("single", M, K, N, 0, act, b is not None, False, want_pre, m, "")
    o, _ = run_linear(c, x, w, b if b is not None else torch.zeros(N), torch.zeros(M, N))
    return o


def check_multi(fails, tag, o, x, ws, bs, M, K, N, act, pre_mask, live, same_as_single):
    """Each layer judged against fp64; bit-identical to the single call where the header says so (the one-launch form of k_linear_t16 and the
    per-layer path are 'the same arithmetic'; k_linear_fan16 stages each layer's weights per 64-output half, each half with a scale of its own,
    so it is held to the margin instead)."""
    for q, w in enumerate(ws):
        b = None if bs is None else bs[q]
        assert is_sent(o[f"y{q}"][live * N:]), (tag, q)
        want_pre = pre_mask is not None and pre_mask[q]
        if pre_mask is not None:
            assert is_sent(o[f"pre{q}"][(live if want_pre else 0) * N:]), (tag, q, "pre")
        if not live:
            continue
        (y32, p32), (y64, p64) = both(lambda x_, w_, b_: D.linear(x_, w_, b_, None, 0, act), x[:live], w, b)
        judge(fails, f"{tag}/layer{q}", "multi.y", o[f"y{q}"][:live * N].cpu().view(live, N), y32, y64)
        if want_pre:
            judge(fails, f"{tag}/layer{q}", "multi.pre", o[f"pre{q}"][:live * N].cpu().view(live, N), p32, p64)
        if same_as_single:
            one = single_layer(x[:live], w, b, live, K, N, act, want_pre and act != 0)
            assert torch.equal(one["y"][:live * N].view(i32), o[f"y{q}"][:live * N].view(i32)), (tag, q, "differs from the single call")
            if want_pre and act != 0:
                assert torch.equal(one["pre"][:live * N].view(i32), o[f"pre{q}"][:live * N].view(i32)), (tag, q, "pre differs from the single call")


@pytest.mark.parametrize("L,act,M", D.MULTI_CASES)
def test_linear_multi_one_launch(L, act, M):
    """K = N = 128, 2..4 layers in one k_linear_t16 launch: pre all / none / some entries NULL, bias NULL or given, a device row count.  Every
    layer is bit-identical to its own conan_linear_fwd / _act_fwd call (same kernel, same tiles, same arithmetic)."""
    fails = []
    x, ws, bs = multi_inputs(M, 128, 128, L)
    some = [q % 2 == 0 for q in range(L)]
    for tag, bias, mask, m in (("b/none", bs, None, None), ("nob/all", None, [True] * L, None), ("b/some", bs, some, None), ("b/all/m", bs, [True] * L, M - 1),
                               ("b/none/m+5", bs, None, M + 5), ("b/all/m0", bs, [True] * L, 0), ("b/some/m1", bs, some, 1)):
        live = M if m is None else min(m, M)
        o = run_multi(x, ws, bias, M, 128, 128, act, mask, m)
        check_multi(fails, f"multi/L{L}/act{act}/M{M}/{tag}", o, x, ws, bias, M, 128, 128, act, mask, live, same_as_single=True)
    assert not fails, fails


@pytest.mark.parametrize("L", [2, 3, 4])
def test_linear_multi_edge_level(L):
    """M = 65536, act 0, no pre: 2 and 3 layers run on k_linear_fan16 (within margin of fp64; its weight scale is per 64-output half, not the single
    call's one per matrix), 4 layers stay on k_linear_t16 (bit-identical to the single call).  With pre wanted or an activation the fan form is not taken."""
    M, fails = D.MULTI_EDGE_M, []
    x, ws, bs = multi_inputs(M, 128, 128, L)
    o = run_multi(x, ws, bs, M, 128, 128, 0, None)
    check_multi(fails, f"multi/L{L}/act0/M{M}", o, x, ws, bs, M, 128, 128, 0, None, M, same_as_single=(L == 4))
    if L == 2:
        o = run_multi(x, ws, bs, M, 128, 128, 0, None, m=40000)
        check_multi(fails, f"multi/L{L}/act0/M{M}/m40000", o, x, ws, bs, M, 128, 128, 0, None, 40000, same_as_single=False)
        o = run_multi(x, ws, None, M, 128, 128, 3, [True, False])
        check_multi(fails, f"multi/L{L}/act3/M{M}/pre", o, x, ws, None, M, 128, 128, 3, [True, False], M, same_as_single=True)
    assert not fails, fails


def test_linear_multi_per_layer_path_and_status_codes():
    """1 and 5 layers and (K, N) = (64, 128) go layer by layer through conan_linear_t_try: the single call's bits.  (50, 128): UNSUPPORTED."""
    fails = []
    for L, K in ((1, 128), (5, 128), (3, 64)):
        x, ws, bs = multi_inputs(33, K, 128, L)
        o = run_multi(x, ws, bs, 33, K, 128, 3, [True] * L)
        check_multi(fails, f"multi/L{L}/K{K}", o, x, ws, bs, 33, K, 128, 3, [True] * L, 33, same_as_single=True)
    assert not fails, fails
    x, ws, bs = multi_inputs(33, 50, 128, 2)
    o = run_multi(x, ws, bs, 33, 50, 128, 0, None, expect=E_UNSUPPORTED)
    assert all(is_sent(t) for t in o.values())
    xd, wd, yd, s = put(x), [put(w) for w in ws], [sent(33 * 128) for _ in ws], stream_ptr()
    mf = lambda *a: raw("conan_linear_multi_fwd", *a)
    assert mf(ptr(xd), _arr(wd), None, 33, 50, 128, 2, 2, None, _arr(yd), None, s) == E_BADARG                 # act 2
    assert mf(ptr(xd), _arr(wd), None, 33, 50, 128, 0, 0, None, _arr(yd), None, s) == E_BADARG                 # no layers
    assert mf(ptr(xd), _arr([wd[0], None]), None, 33, 50, 128, 2, 0, None, _arr(yd), None, s) == E_BADARG      # a NULL weight
    assert mf(None, _arr(wd), None, 33, 50, 128, 2, 0, None, _arr(yd), None, s) == E_BADARG
    assert mf(ptr(xd), _arr(wd), None, 0, 128, 128, 2, 0, None, _arr(yd), None, s) == OK
    torch.cuda.synchronize()
    assert all(is_sent(t) for t in yd)


# ================================================================================================ sum of contractions
def run_sum(base, views_of, ws, b, r, nin, kn, ld, M, m=None, alias=False, expect=OK, N=128):
    """conan_linear_sum_fwd on device copies of `base` (the tensors behind the [M,128] views; views_of[c] = (base index, column offset))."""
    lv = None if m is None else min(m, M)
    bd = [put(t, lv) for t in base]
    wd, bb, md, s = [put(w) for w in ws], None if b is None else put(b), mdev(m), stream_ptr()
    xs = (ctypes.c_void_p * nin)(*[bd[i].data_ptr() + 4 * off for i, off in views_of])
    ldx = (ctypes.c_int * nin)(*([ld] * nin)) if isinstance(ld, int) else (ctypes.c_int * nin)(*ld)

    def run():
        o = {"y": sent(M * N)}
        rd = None
        if r is not None:
            if alias:                                                   # residual == y: the header allows it
                o["y"][:M * N].view(M, N)[:M if lv is None else lv].copy_(r[:M if lv is None else lv])
                rd = o["y"]
            else:
                rd = put(r, lv)
        rc = raw("conan_linear_sum_fwd", xs, ldx, _arr(wd), nin, kn, ptr(bb), ptr(rd), M, N, ptr(md), ptr(o["y"]), s)
        assert rc == expect, rc
        return o
    return twice(run)


def _views(nin, ld):
    return [(0, 128 * c) for c in range(nin)] if ld == 384 else [(c, 0) for c in range(nin)]


@pytest.mark.parametrize("nin,kn,ld,M", D.SUM_CASES)
def test_linear_sum(nin, kn, ld, M):
    """2 and 3 inputs, W as [N,128] and [128,N], row pitch 128 / 132 / 384 (three views of one tensor), with bias and residual, without both,
    residual aliasing y, chunk magnitudes 1e-6 / 3 / 1e-3, a device row count."""
    fails, tag = [], f"sum/n{nin}/kn{kn}/ld{ld}/M{M}"
    for sub, scales, bias, res, alias, m in (("plain", (1.0, 1.0, 1.0), False, False, False, None), ("b+r", (1.0, 1.0, 1.0), True, True, False, None),
                                             ("alias", (1.0, 1.0, 1.0), True, True, True, None), ("scales", D.SUM_SCALES, True, False, False, None),
                                             ("m", D.SUM_SCALES, True, True, True, M - 1), ("m+5", (1.0, 1.0, 1.0), False, True, False, M + 5),
                                             ("m0", (1.0, 1.0, 1.0), True, True, False, 0), ("m1", (1.0, 1.0, 1.0), True, True, True, 1)):
        base, xs, ws, b, r = D.sum_inputs(nin, kn, ld, M, scales)
        live = M if m is None else min(m, M)
        o = run_sum(base, _views(nin, ld), ws, b if bias else None, r if res else None, nin, kn, ld, M, m, alias)
        assert is_sent(o["y"][live * 128:]), (tag, sub)
        if live:
            y32 = D.linear_sum([t[:live] for t in xs], ws, b if bias else None, r[:live] if res else None, kn)
            y64 = D.linear_sum([t[:live].double() for t in xs], [w.double() for w in ws], b.double() if bias else None, r[:live].double() if res else None, kn)
            judge(fails, f"{tag}/{sub}", "sum.y", o["y"][:live * 128].cpu().view(live, 128), y32, y64)
    assert not fails, fails


def test_linear_sum_status_codes():
    base, xs, ws, b, r = D.sum_inputs(3, 0, 132, 8)
    for nin, N, ld, want in ((2, 64, 132, E_UNSUPPORTED), (1, 128, 132, E_UNSUPPORTED), (2, 128, 127, E_BADARG), (2, 128, 130, E_BADARG), (0, 128, 132, E_BADARG)):
        if nin == 0:
            assert raw("conan_linear_sum_fwd", _arr([]), (ctypes.c_int * 1)(132), _arr([]), 0, 0, None, None, 8, 128, None, ptr(sent(8 * 128)), stream_ptr()) == want
            continue
        o = run_sum(base[:nin], [(c, 0) for c in range(nin)], ws[:nin], b, None, nin, 0, ld, 8, expect=want, N=N)
        assert is_sent(o["y"]), (nin, N, ld)
    base4 = base + [base[0]]
    o = run_sum(base4, [(c, 0) for c in range(4)], ws + [ws[0]], b, None, 4, 0, 132, 8, expect=E_UNSUPPORTED)
    assert is_sent(o["y"])
    o = run_sum(base[:2], [(0, 0), (1, 0)], ws[:2], b, None, 2, 0, 132, 0)               # no rows: OK, nothing written
    assert is_sent(o["y"])


# ================================================================================================ weight gradients
def wgrad_out(M, K, N):
    wsn = int(raw("conan_linear_wgrad_ws", M, K, N))
    assert wsn == D.wgrad_ws(M, K, N), (M, K, N, wsn)
    return {"dW": sent(N * K), "dbias": sent(N), "ws": sent(wsn)}, wsn


def run_wgrad(g, x, M, K, N, m=None, bias=True, gmax=None, rbf=None, expect=OK):
    """The immediate forms: conan_linear_wgrad, conan_linear_wgrad_scaled (gmax: a float), conan_rbf_wgrad (rbf = (dist, offset, coeff); K = Gs)."""
    lv = None if m is None else min(m, M)
    gd, md, s = put(g, lv), mdev(m), stream_ptr()
    if rbf is None:
        xd = put(x, lv)
    else:
        dd, od = put(rbf[0], lv), put(rbf[1])
    gm = None if gmax is None else torch.tensor([gmax], dtype=f32, device=dev)

    def run():
        o, wsn = wgrad_out(M, K, N)
        db = ptr(o["dbias"]) if bias else None
        if rbf is not None:
            rc = raw("conan_rbf_wgrad", ptr(gd), ptr(dd), M, ptr(od), K, rbf[2], N, ptr(md), ptr(o["dW"]), db, ptr(o["ws"]), s)
        elif gmax is not None:
            rc = raw("conan_linear_wgrad_scaled", ptr(gd), ptr(xd), M, K, N, ptr(md), ptr(o["dW"]), db, ptr(o["ws"]), ptr(gm), s)
        else:
            rc = raw("conan_linear_wgrad", ptr(gd), ptr(xd), M, K, N, ptr(md), ptr(o["dW"]), db, ptr(o["ws"]), s)
        assert rc == expect, rc
        return o
    o = twice(run)
    cut(o["ws"], D.wgrad_ws(M, K, N), "ws")
    if not bias:
        assert is_sent(o["dbias"])
    return o


def check_wgrad(fails, tag, what, o, g, x, M, K, N, live, bias=True, bias_tag=""):
    dW, db = cut(o["dW"], N * K, "dW").view(N, K), cut(o["dbias"], N, "dbias")
    (w32, b32), (w64, b64) = both(lambda g_, x_: D.wgrad(g_, x_, live), g, x)
    if live == 0:
        assert float(dW.abs().max()) == 0.0 and (not bias or float(db.abs().max()) == 0.0), (tag, "no rows: exact zeros")
        return
    judge(fails, tag, what + ".dW", dW, w32, w64)
    if bias:
        judge(fails, tag, what + ".dbias" + bias_tag, db, b32, b64)      # M = 1: the fp32 reference is exact, so this demands equality


@pytest.mark.parametrize("M,K,N,names", D.WGRAD_IMMEDIATE)
def test_linear_wgrad_immediate(M, K, N, names):
    """dW = g^T x and dbias over the first min(M, *m_dev) rows; dbias NULL and not; the workspace is exactly conan_linear_wgrad_ws and nothing
    beyond it is written."""
    assert D.wgrad_branch(M, K, N, False, False, True) == names
    BRANCHES.update(names)
    fails, tag = [], f"wgrad/M{M}/K{K}/N{N}"
    g, x = D.wgrad_inputs(M, K, N)
    o = run_wgrad(g, x, M, K, N)
    check_wgrad(fails, tag, "wgrad", o, g, x, M, K, N, M)
    if M <= 2000:
        o2 = run_wgrad(g, x, M, K, N, bias=False)
        assert torch.equal(o2["dW"].view(i32), o["dW"].view(i32)), "dbias == NULL changes dW"
        for m in sorted({0, 1, max(M - 1, 0), M + 5}):
            o = run_wgrad(g, x, M, K, N, m=m)
            check_wgrad(fails, f"{tag}/m{m}", "wgrad", o, g, x, M, K, N, min(m, M))
    assert not fails, fails


@pytest.mark.parametrize("M,red", D.SCALAR_M)
def test_linear_wgrad_scalar_reducers(M, red):
    """N in {1, 3, 5, 130} x K in {50, 128, 63}: N or N K is no multiple of 4, so the slabs are summed by k_wgrad_reduce — in one level up to 32
    slices (M <= 4096), in two levels beyond.  These shapes are not batchable and conan_linear_wgrad_slabs refuses them."""
    fails = []
    for N in D.SCALAR_N:
        for K in D.SCALAR_K:
            names = D.wgrad_branch(M, K, N, False, False, True)
            assert names[-1] == red
            BRANCHES.update(names)
            assert raw("conan_wgrad_batchable", K, N) == 0
            g, x = D.wgrad_inputs(M, K, N)
            for bias in ((True, False) if M in (300, 4097) else (True,)):
                o = run_wgrad(g, x, M, K, N, bias=bias)
                check_wgrad(fails, f"wgrad/M{M}/K{K}/N{N}/b{int(bias)}", "wgrad.scalar", o, g, x, M, K, N, M, bias, "/N<=5" if N <= 5 else "")
            if M == 4097 and K == 63:
                o = run_wgrad(g, x, M, K, N, m=M - 1)                     # 33 slices by M, 4096 live rows
                check_wgrad(fails, f"wgrad/M{M}/K{K}/N{N}/m{M - 1}", "wgrad.scalar", o, g, x, M, K, N, M - 1, True, "/N<=5" if N <= 5 else "")
    ws, s = sent(D.wgrad_ws(300, 63, 130)), stream_ptr()
    g, x = D.wgrad_inputs(300, 63, 130)
    assert raw("conan_linear_wgrad_slabs", ptr(put(g)), ptr(put(x)), 300, 63, 130, None, ptr(ws), s) == E_BADARG
    torch.cuda.synchronize()
    assert is_sent(ws)
    assert not fails, fails


def test_wgrad_batchable_truth_table_and_status_codes():
    for K in (1, 2, 3, 4, 50, 63, 64, 128):
        for N in (1, 2, 3, 4, 5, 52, 128, 130):
            assert raw("conan_wgrad_batchable", K, N) == int(D.batchable(K, N)) == int(N % 4 == 0), (K, N)
    g, x = D.wgrad_inputs(8, 128, 128)
    gd, xd, s = put(g), put(x), stream_ptr()
    o, _ = wgrad_out(8, 128, 128)
    gm = torch.ones(1, device=dev)
    wg = lambda *a: raw("conan_linear_wgrad", *a)
    assert wg(None, ptr(xd), 8, 128, 128, None, ptr(o["dW"]), None, ptr(o["ws"]), s) == E_BADARG
    assert wg(ptr(gd), ptr(xd), 8, 128, 128, None, None, None, ptr(o["ws"]), s) == E_BADARG
    assert wg(ptr(gd), ptr(xd), 8, 128, 128, None, ptr(o["dW"]), None, None, s) == E_BADARG
    assert wg(ptr(gd), ptr(xd), -1, 128, 128, None, ptr(o["dW"]), None, ptr(o["ws"]), s) == E_BADARG
    assert wg(ptr(gd), ptr(xd), 8, 0, 128, None, ptr(o["dW"]), None, ptr(o["ws"]), s) == E_BADARG
    sc = lambda *a: raw("conan_linear_wgrad_scaled", *a)
    assert sc(ptr(gd), ptr(xd), 8, 64, 128, None, ptr(o["dW"]), None, ptr(o["ws"]), ptr(gm), s) == E_BADARG          # K <= 64
    assert sc(ptr(gd), ptr(xd), 8, 128, 128, None, ptr(o["dW"]), None, ptr(o["ws"]), None, s) == E_BADARG            # no gmax
    assert sc(ptr(gd), ptr(xd), 8, 128, 130, None, None, None, ptr(o["ws"]), ptr(gm), s) == E_BADARG                 # slabs only, not batchable
    assert raw("conan_rbf_wgrad", ptr(gd), ptr(xd), 8, ptr(xd), 0, -1.0, 128, None, ptr(o["dW"]), None, ptr(o["ws"]), s) == E_BADARG
    assert raw("conan_rbf_wgrad_slabs", ptr(gd), ptr(xd), 8, ptr(xd), 50, -1.0, 130, None, ptr(o["ws"]), s) == E_BADARG
    assert raw("conan_wgrad_reduce_batch", None, 1, s) == E_BADARG and raw("conan_wgrad_reduce_batch", None, 0, s) == OK
    assert raw("conan_linear_wgrad_slabs_batch", None, 1, s) == E_BADARG and raw("conan_linear_wgrad_slabs_batch", None, 0, s) == OK
    job = (WgradJob * 1)(WgradJob(o["ws"].data_ptr(), o["dW"].data_ptr(), None, 8, 63, 130, 0))
    assert raw("conan_wgrad_reduce_batch", job, 1, s) == E_BADARG                                                    # not batchable
    sjob = (WgradSlabJob * 1)(WgradSlabJob(gd.data_ptr(), xd.data_ptr(), None, o["ws"].data_ptr(), 8, 63, 130, 0))
    assert raw("conan_linear_wgrad_slabs_batch", sjob, 1, s) == E_BADARG
    torch.cuda.synchronize()
    assert all(is_sent(t) for t in o.values())


@pytest.mark.parametrize("M,K,N", D.SCALED_SHAPES)
def test_linear_wgrad_scaled(M, K, N):
    """g at the scales 2e-6, 1 and 3e3 with gmax = max |g| and 8 x that (an upper bound is allowed: three bits fewer in the second plane);
    g = 0 with gmax = 0: exact zeros.  x is N(0, 1): activations.  (The precision floor under an outlier is pinned in test_gpu_ops.py.)"""
    fails = []
    names = D.wgrad_branch(M, K, N, False, True, True)
    assert names[0] == "h16"
    BRANCHES.update(names)
    g0, x = D.wgrad_inputs(M, K, N)
    for scale in D.SCALED_G:
        g = g0 * scale
        for over in (1.0, 8.0):
            o = run_wgrad(g, x, M, K, N, gmax=float(g.abs().max()) * over)
            check_wgrad(fails, f"scaled/M{M}/K{K}/N{N}/g{scale:g}/gmax{over:g}", "wgrad.scaled" + ("" if over == 1.0 else "/gmax8"), o, g, x, M, K, N, M)
    o = run_wgrad(g0 * 0.0, x, M, K, N, gmax=0.0)
    assert float(o["dW"][:N * K].abs().max()) == 0.0 and float(o["dbias"][:N].abs().max()) == 0.0
    for m in (0, 1, M - 1, M + 5):
        o = run_wgrad(g0, x, M, K, N, gmax=float(g0[:max(min(m, M), 1)].abs().max()), m=m)
        check_wgrad(fails, f"scaled/M{M}/K{K}/N{N}/m{m}", "wgrad.scaled", o, g0, x, M, K, N, min(m, M))
    assert not fails, fails


def reduce_jobs(specs):
    """conan_wgrad_reduce_batch over [(ws, dW, dbias | None, M, K, N, slices)] in one call."""
    jobs = (WgradJob * len(specs))(*[WgradJob(ws.data_ptr(), dW.data_ptr(), None if db is None else db.data_ptr(), M, K, N, sl)
                                     for ws, dW, db, M, K, N, sl in specs])
    assert raw("conan_wgrad_reduce_batch", jobs, len(specs), stream_ptr()) == OK


@pytest.mark.parametrize("Gs", D.RBF_GS)
def test_rbf_wgrad(Gs):
    """dW = g^T rbf(dist) with the expansion generated on the fly, N in {32, 128, 130}, M in {1, 517, 4133}; distances at 0, at the last offset
    and beyond it.  For batchable shapes conan_rbf_wgrad_slabs + conan_wgrad_reduce_batch give the immediate form's bits."""
    fails = []
    for N in D.RBF_N:
        for M in D.RBF_M:
            g, dist, off, coeff = D.rbf_inputs(M, Gs, N)
            BRANCHES.update(D.wgrad_branch(M, Gs, N, True, False, True))
            tag = f"rbf/Gs{Gs}/N{N}/M{M}"
            o = run_wgrad(g, None, M, Gs, N, rbf=(dist, off, coeff))
            dW, db = cut(o["dW"], N * Gs).view(N, Gs), cut(o["dbias"], N)
            (w32, b32), (w64, b64) = both(lambda g_, d_, o_: D.wgrad(g_, D.rbf(d_, o_, coeff), M), g, dist, off)
            judge(fails, tag, "rbf_wgrad.dW", dW, w32, w64)
            judge(fails, tag, "rbf_wgrad.dbias", db, b32, b64)
            for m in ((0, 1, 300, M + 5) if M == 517 else ()):
                om = run_wgrad(g, None, M, Gs, N, rbf=(dist, off, coeff), m=m)
                live = min(m, M)
                if live == 0:
                    assert float(om["dW"][:N * Gs].abs().max()) == 0.0 and float(om["dbias"][:N].abs().max()) == 0.0
                    continue
                (w32, b32), (w64, b64) = both(lambda g_, d_, o_: D.wgrad(g_, D.rbf(d_, o_, coeff), live), g, dist, off)
                judge(fails, f"{tag}/m{m}", "rbf_wgrad.dW", cut(om["dW"], N * Gs).view(N, Gs), w32, w64)
                judge(fails, f"{tag}/m{m}", "rbf_wgrad.dbias", cut(om["dbias"], N), b32, b64)
            if D.batchable(Gs, N):
                assert raw("conan_wgrad_batchable", Gs, N) == 1
                gd, dd, od, s = put(g), put(dist), put(off), stream_ptr()
                d, wsn = wgrad_out(M, Gs, N)
                assert raw("conan_rbf_wgrad_slabs", ptr(gd), ptr(dd), M, ptr(od), Gs, coeff, N, None, ptr(d["ws"]), s) == OK
                reduce_jobs([(d["ws"], d["dW"], d["dbias"], M, Gs, N, 0)])
                torch.cuda.synchronize()
                assert same_bits({k: o[k] for k in ("dW", "dbias")}, d), (tag, "slabs + reduce_batch differ from the immediate form")
                cut(d["ws"], wsn, "ws")
    assert not fails, fails


BATCHABLE_SHAPES = [(M, K, N) for M, K, N, _ in D.WGRAD_IMMEDIATE if D.batchable(K, N)]


@pytest.mark.parametrize("M,K,N", BATCHABLE_SHAPES)
def test_wgrad_slabs_then_reduce_is_the_immediate_form(M, K, N):
    """conan_linear_wgrad_slabs + conan_wgrad_reduce_batch: the immediate call's bits in dW, dbias AND in the slabs; with a device row count too."""
    g, x = D.wgrad_inputs(M, K, N)
    gd, xd, s = put(g), put(x), stream_ptr()
    for m in ((None,) if M > 2000 or M == 0 else (None, M - 1)):
        o = run_wgrad(g, x, M, K, N, m=m)
        d, wsn = wgrad_out(M, K, N)
        md = mdev(m)
        assert raw("conan_linear_wgrad_slabs", ptr(gd), ptr(xd), M, K, N, ptr(md), ptr(d["ws"]), s) == OK
        torch.cuda.synchronize()
        used = D.wgrad_slices(M, K) * (N * K + N)
        assert torch.equal(d["ws"][:used].view(i32), o["ws"][:used].view(i32)) and is_sent(d["ws"][used:]) and is_sent(d["dW"])
        reduce_jobs([(d["ws"], d["dW"], d["dbias"], M, K, N, 0)])
        torch.cuda.synchronize()
        assert torch.equal(d["dW"].view(i32), o["dW"].view(i32)) and torch.equal(d["dbias"].view(i32), o["dbias"].view(i32)), (M, K, N, m)


def test_wgrad_reduce_batch_of_33_jobs():
    """33 jobs in one call: two launches (WG_BATCH = 32).  Jobs of different widths, with and without dbias, each the immediate form's bits."""
    shapes = [(300, 128, 128), (129, 64, 64), (300, 128, 52), (1000, 128, 256), (300, 52, 128)]
    imm, slabs = [], []
    for M, K, N in shapes:
        g, x = D.wgrad_inputs(M, K, N)
        imm.append(run_wgrad(g, x, M, K, N))
        slabs.append(imm[-1]["ws"])
    outs, specs = [], []
    for j in range(33):
        M, K, N = shapes[j % 5]
        dW, db = sent(N * K), sent(N)
        outs.append((dW, db))
        specs.append((slabs[j % 5], dW, db if j % 3 else None, M, K, N, 0))
    reduce_jobs(specs)
    torch.cuda.synchronize()
    for j, (dW, db) in enumerate(outs):
        assert torch.equal(dW.view(i32), imm[j % 5]["dW"].view(i32)), j
        assert torch.equal(db.view(i32), imm[j % 5]["dbias"].view(i32)) if j % 3 else is_sent(db), j


def slab_batch(jobs):
    """conan_linear_wgrad_slabs_batch over [(g_dev, x_dev, m_dev | None, M, K, N, slices)] -> the workspaces, one per job."""
    wss = [sent(D.wgrad_ws(M, K, N)) for _, _, _, M, K, N, _ in jobs]
    arr = (WgradSlabJob * len(jobs))(*[WgradSlabJob(g.data_ptr(), x.data_ptr(), None if md is None else md.data_ptr(), ws.data_ptr(), M, K, N, sl)
                                       for (g, x, md, M, K, N, sl), ws in zip(jobs, wss)])
    assert raw("conan_linear_wgrad_slabs_batch", arr, len(jobs), stream_ptr()) == OK
    torch.cuda.synchronize()
    return wss


def check_slab_jobs(fails, tag, jobs, host, wss, eff_slices):
    """Every job: its own conan_linear_wgrad_slabs call's bits (default slice count), then reduced and judged against fp64.
    (The deferred forms — slab_batch, reduce_jobs, the slab calls here and in the tests above — run once, not through twice(): they are compared bit
    for bit with an immediate or own-slab result, and the immediate results they are compared with did go through twice().)"""
    s = stream_ptr()
    for j, ((gd, xd, md, M, K, N, sl), ws) in enumerate(zip(jobs, wss)):
        g, x, live = host[j]
        eff = eff_slices[j]
        used = eff * (N * K + N)
        assert is_sent(ws[used:]), (tag, j, "written beyond its slabs")
        if eff == D.wgrad_slices(M, K):
            own = sent(D.wgrad_ws(M, K, N))
            assert raw("conan_linear_wgrad_slabs", ptr(gd), ptr(xd), M, K, N, ptr(md), ptr(own), s) == OK
            torch.cuda.synchronize()
            assert torch.equal(own.view(i32), ws.view(i32)), (tag, j, "differs from its own conan_linear_wgrad_slabs call")
        dW, db = sent(N * K), sent(N)
        reduce_jobs([(ws, dW, db, M, K, N, 0 if eff == D.wgrad_slices(M, K) else eff)])
        torch.cuda.synchronize()
        check_wgrad(fails, f"{tag}/job{j}", "wgrad.batch", {"dW": dW, "dbias": db}, g, x, M, K, N, live)


def test_wgrad_slabs_batch_of_25_jobs_and_mixed_widths():
    """25 jobs of one k-tile width in one call: a flush at WGS_BATCH = 24, for both widths; 20 jobs with k tiles of 64 and 128 mixed (two launch
    sequences in one call) and a job with M = 0 among them."""
    fails = []
    shapes = [(300, 64, 64), (300, 128, 128), (129, 52, 128), (300, 128, 52), (1000, 128, 256)]
    pool = [D.wgrad_inputs(M, K, N, seed=q) for q, (M, K, N) in enumerate(shapes)]
    dev_pool = [(put(g), put(x)) for g, x in pool]
    jobs, host = [], []
    for j in range(20):
        q = j % 5
        M, K, N = shapes[q]
        if j == 7:
            M = 0
        jobs.append((dev_pool[q][0], dev_pool[q][1], None, M, K, N, 0))
        host.append((pool[q][0], pool[q][1], M))
    check_slab_jobs(fails, "mixed20", jobs, host, slab_batch(jobs), [D.wgrad_slices(j[3], j[4]) for j in jobs])
    for q in (0, 1):
        M, K, N = shapes[q]
        same = [(dev_pool[q][0], dev_pool[q][1], None, M, K, N, 0)] * 25
        wss = slab_batch(same)
        assert all(torch.equal(w.view(i32), wss[0].view(i32)) for w in wss), "25 equal jobs, different slabs"
        check_slab_jobs(fails, f"same25/K{K}", [same[0], same[24]], [(pool[q][0], pool[q][1], M)] * 2, [wss[0], wss[24]], [3, 3])
    assert not fails, fails


@pytest.mark.parametrize("K,N", [(128, 128), (64, 64)])
def test_wgrad_slabs_batch_runs_over_one_x(K, N):
    """M = 1024 (8 slices, a multiple of 8): runs of 2, 3, 4 and 5 consecutive jobs over one x share their x tiles; a run broken by a different
    m_dev; explicit slice counts below the default (taken, and given to the reducer) and above it (ignored)."""
    fails, M = [], 1024
    _, x = D.wgrad_inputs(M, K, N)
    xd = put(x)
    gs = [D.wgrad_inputs(M, K, N, seed=10 + q)[0] for q in range(5)]
    gds = [put(g) for g in gs]
    md, md9 = mdev(1000), mdev(900)
    xm, gms = put(x, 1000), [put(g, 1000) for g in gs]                 # rows beyond the device count hold the pattern
    for run in (2, 3, 4, 5):
        jobs = [(gds[q], xd, None, M, K, N, 0) for q in range(run)]
        check_slab_jobs(fails, f"run{run}/K{K}", jobs, [(gs[q], x, M) for q in range(run)], slab_batch(jobs), [8] * run)
    jobs = [(gms[0], xm, md, M, K, N, 0), (gms[1], xm, md, M, K, N, 0), (gms[2], xm, md9, M, K, N, 0), (gms[3], xm, md, M, K, N, 0)]
    host = [(gs[0], x, 1000), (gs[1], x, 1000), (gs[2], x, 900), (gs[3], x, 1000)]
    check_slab_jobs(fails, f"broken-run/K{K}", jobs, host, slab_batch(jobs), [8] * 4)
    jobs = [(gds[0], xd, None, M, K, N, 4), (gds[1], xd, None, M, K, N, 4), (gds[2], xd, None, M, K, N, 16), (gds[3], xd, None, M, K, N, 8), (gds[4], xd, None, M, K, N, 1)]
    check_slab_jobs(fails, f"slices/K{K}", jobs, [(gs[q], x, M) for q in range(5)], slab_batch(jobs), [4, 4, 8, 8, 1])
    assert not fails, fails


@pytest.mark.parametrize("run", [2, 3])
def test_wgrad_slabs_batch_edge_level_run_over_one_x(run):
    """M = 65536, K = N = 128: a run of 2 or 3 jobs over one x leaves the shared grid for a launch of k_wgrad_lds_shared<2|3> — the same slabs bit
    for bit as each job's own conan_linear_wgrad_slabs call; a single job before and after the run stays on the grid."""
    fails, M, K, N = [], 65536, 128, 128
    assert D.slab_batch_form(run, M, K, N) == f"shared{run}" and D.slab_batch_form(4, M, K, N) == "grid" and D.slab_batch_form(run, 1024, K, N) == "grid"
    BRANCHES.add(f"batch/shared{run}")
    _, x = D.wgrad_inputs(M, K, N)
    xd = put(x)
    gs = [D.wgrad_inputs(M, K, N, seed=20 + q)[0] for q in range(run)]
    g1, x1 = D.wgrad_inputs(300, K, N)
    g1d, x1d = put(g1), put(x1)
    jobs = [(g1d, x1d, None, 300, K, N, 0)] + [(put(g), xd, None, M, K, N, 0) for g in gs] + [(g1d, x1d, None, 300, K, N, 0)]
    host = [(g1, x1, 300)] + [(g, x, M) for g in gs] + [(g1, x1, 300)]
    check_slab_jobs(fails, f"shared{run}", jobs, host, slab_batch(jobs), [3] + [512] * run + [3])
    assert not fails, fails


def test_wgrad_slabs_batch_run_across_the_flush():
    """22 single jobs, then a run of 3 over one x (M = 1024, 8 slices): 22 + 3 > WGS_BATCH = 24, so the table is flushed BEFORE the run (a run is
    kept inside one launch) and the run opens the next one."""
    fails, K, N = [], 128, 128
    g1, x1 = D.wgrad_inputs(300, K, N)
    g1d, x1d = put(g1), put(x1)
    _, x = D.wgrad_inputs(1024, K, N)
    xd = put(x)
    gs = [D.wgrad_inputs(1024, K, N, seed=30 + q)[0] for q in range(3)]
    jobs = [(g1d, x1d, None, 300, K, N, 0)] * 22 + [(put(g), xd, None, 1024, K, N, 0) for g in gs]
    assert D.slab_batch_form(3, 1024, K, N) == "grid"
    BRANCHES.add("batch/run-across-flush")
    wss = slab_batch(jobs)
    assert all(torch.equal(w.view(i32), wss[0].view(i32)) for w in wss[:22])
    pick = [0, 21, 22, 23, 24]
    check_slab_jobs(fails, "flush22+3", [jobs[j] for j in pick], [(g1, x1, 300)] * 2 + [(g, x, 1024) for g in gs], [wss[j] for j in pick], [3, 3, 8, 8, 8])
    assert not fails, fails


# ================================================================================================ mlp2
def test_mlp2_supported_truth_tables_and_status_codes():
    for fn, ok in (("conan_mlp2_supported", (128, 128, 128)), ("conan_mlp2_outact_supported", (128, 64, 64))):
        for M, want in ((0, 0), (1, 1), (65536, 1), (65537, 0)):
            assert raw(fn, M, *ok) == want, (fn, M)
        for q in range(3):
            for d in (-64, 64):
                dims = list(ok)
                dims[q] += d
                assert raw(fn, 33, *dims) == 0, (fn, dims)
    s = stream_ptr()
    for outact, (K, N1, N2) in ((False, (128, 128, 128)), (True, (128, 64, 64))):
        x, w1, b1, w2, b2, res, dy = D.mlp2_inputs(8, K, N1, N2)
        xd, w1d, b1d, w2d, b2d = put(x), put(w1), put(b1), put(w2), put(b2)
        M = 65537
        mid, y = sent(M * N1), sent(M * N2)
        for Mq, dims, want in ((M, (K, N1, N2), E_UNSUPPORTED), (8, (K, N1 + 64, N2), E_UNSUPPORTED), (0, (K, N1, N2), OK), (-1, (K, N1, N2), E_BADARG)):
            if outact:
                assert raw("conan_mlp2_outact_fwd", ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), Mq, *dims, ptr(mid), ptr(y), s) == want
                assert raw("conan_mlp2_outact_bwd", ptr(xd), ptr(xd), ptr(w2d), ptr(w1d), Mq, *dims, ptr(mid), ptr(mid), ptr(y), s) == want
            else:
                assert raw("conan_mlp2_fwd", ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), None, Mq, *dims, ptr(mid), ptr(y), s) == want
                assert raw("conan_mlp2_bwd", ptr(xd), ptr(w2d), ptr(w1d), ptr(xd), Mq, *dims, ptr(mid), ptr(y), s) == want
        if outact:
            assert raw("conan_mlp2_outact_fwd", ptr(xd), ptr(w1d), None, ptr(w2d), ptr(b2d), 8, K, N1, N2, ptr(mid), ptr(y), s) == E_BADARG
        else:
            assert raw("conan_mlp2_fwd", ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), None, 8, K, N1, N2, ptr(mid), None, s) == E_BADARG
        torch.cuda.synchronize()
        assert is_sent(mid) and is_sent(y)


def run_mlp2(x, w1, b1, w2, b2, res, dy, M, with_mid=True, with_dmid=True):
    """conan_mlp2_fwd, then conan_mlp2_bwd from the forward's own saved mid."""
    xd, w1d, b1d, w2d, b2d, rd, dyd, s = put(x), put(w1), put(b1), put(w2), put(b2), None if res is None else put(res), put(dy), stream_ptr()

    def run():
        o = {k: sent(M * 128) for k in ("mid", "y", "dmid", "dx")}
        assert raw("conan_mlp2_fwd", ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(rd), M, 128, 128, 128, ptr(o["mid"]), ptr(o["y"]), s) == OK
        assert raw("conan_mlp2_bwd", ptr(dyd), ptr(w2d), ptr(w1d), ptr(o["mid"]), M, 128, 128, 128, ptr(o["dmid"]) if with_dmid else None, ptr(o["dx"]), s) == OK
        if not with_mid:
            o["y2"] = sent(M * 128)
            assert raw("conan_mlp2_fwd", ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(rd), M, 128, 128, 128, None, ptr(o["y2"]), s) == OK
        return o
    o = twice(run)
    if not with_mid:
        assert torch.equal(o["y2"].view(i32), o["y"].view(i32)), "mid_out == NULL changes y"
    if not with_dmid:
        assert is_sent(o["dmid"])
    return o


def check_mlp2(fails, tag, o, x, w1, b1, w2, b2, res, dy, M, with_dmid=True):
    v = lambda k: cut(o[k], M * 128, k).view(M, 128)
    (m32, y32), (m64, y64) = both(D.mlp2_fwd, x, w1, b1, w2, b2, res)
    judge(fails, tag, "mlp2.mid", v("mid"), m32, m64)
    judge(fails, tag, "mlp2.y", v("y"), y32, y64)
    mid = v("mid")                                                       # the backward is judged as the operation (dy, mid) -> (dmid, dx) on the kernel's own mid
    (d32, x32), (d64, x64) = both(D.mlp2_bwd, dy, w2, w1, mid)
    if with_dmid:
        judge(fails, tag, "mlp2.dmid", v("dmid"), d32, d64)
    judge(fails, tag, "mlp2.dx", v("dx"), x32, x64)


@pytest.mark.parametrize("M", D.MLP2_M)
def test_mlp2_forward_and_backward(M):
    fails = []
    x, w1, b1, w2, b2, res, dy = D.mlp2_inputs(M, 128, 128, 128)
    variants = ((True, True, True),) if M > 1000 else ((True, True, True), (False, True, True), (True, False, False))
    for with_res, with_mid, with_dmid in variants:
        r = res if with_res else None
        o = run_mlp2(x, w1, b1, w2, b2, r, dy, M, with_mid, with_dmid)
        check_mlp2(fails, f"mlp2/M{M}/r{int(with_res)}/mid{int(with_mid)}/dmid{int(with_dmid)}", o, x, w1, b1, w2, b2, r, dy, M, with_dmid)
    assert not fails, fails


def test_mlp2_values():
    """Rows from 1 to 1e3 (the documented domain), a zero row (mid = ssp(b1)), b1 = -30 (mid -> -ln 2), w2 at 1e-4 and 300."""
    M, fails = 40, []
    for tag, x, w1, bb1, ww2, b2, res, dy in D.mlp2_value_cases(M):
        o = run_mlp2(x, w1, bb1, ww2, b2, res, dy, M)
        check_mlp2(fails, f"mlp2/values/{tag}", o, x, w1, bb1, ww2, b2, res, dy, M)
        mid = o["mid"][:M * 128].cpu().view(M, 128)                          # the zero row on its own: mid = ssp(b1)
        judge(fails, f"mlp2/values/{tag}", "mlp2.mid/zero-row", mid[3:4], D.ssp(bb1).view(1, -1), D.ssp(bb1.double()).view(1, -1))
    assert not fails, fails


def run_outact(x, w1, b1, w2, b2, dy, M, with_mid=True, with_g=True, with_dmid=True):
    xd, w1d, b1d, w2d, b2d, dyd, s = put(x), put(w1), put(b1), put(w2), put(b2), put(dy), stream_ptr()

    def run():
        o = {"mid": sent(M * 64), "y": sent(M * 64), "g": sent(M * 64), "dmid": sent(M * 64), "dx": sent(M * 128)}
        assert raw("conan_mlp2_outact_fwd", ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), M, 128, 64, 64, ptr(o["mid"]) if with_mid else None, ptr(o["y"]), s) == OK
        assert raw("conan_mlp2_outact_bwd", ptr(dyd), ptr(o["y"]), ptr(w2d), ptr(w1d), M, 128, 64, 64, ptr(o["g"]) if with_g else None,
                   ptr(o["dmid"]) if with_dmid else None, ptr(o["dx"]), s) == OK
        return o
    return twice(run)


@pytest.mark.parametrize("M", D.MLP2_M)
def test_mlp2_outact_forward_and_backward(M):
    fails = []
    x, w1, b1, w2, b2, _, dy = D.mlp2_inputs(M, 128, 64, 64)
    full = None
    for with_mid, with_g, with_dmid in ((True, True, True),) if M > 1000 else ((True, True, True), (False, False, True), (True, True, False)):
        o = run_outact(x, w1, b1, w2, b2, dy, M, with_mid, with_g, with_dmid)
        tag = f"outact/M{M}/mid{int(with_mid)}/g{int(with_g)}/dmid{int(with_dmid)}"
        if full is None:
            full = o
        for k, on in (("mid", with_mid), ("g", with_g), ("dmid", with_dmid), ("y", True), ("dx", True)):   # a NULL output changes no other output
            assert torch.equal(o[k].view(i32), full[k].view(i32)) if on else is_sent(o[k]), (tag, k)
    v = lambda k, W: cut(full[k], M * W, k).view(M, W)
    (m32, y32), (m64, y64) = both(D.mlp2_outact_fwd, x, w1, b1, w2, b2)
    judge(fails, f"outact/M{M}", "outact.mid", v("mid", 64), m32, m64)
    judge(fails, f"outact/M{M}", "outact.y", v("y", 64), y32, y64)
    (g32, d32, x32), (g64, d64, x64) = both(D.mlp2_outact_bwd, dy, v("y", 64), w2, w1)
    judge(fails, f"outact/M{M}", "outact.g", v("g", 64), g32, g64)
    judge(fails, f"outact/M{M}", "outact.dmid", v("dmid", 64), d32, d64)
    judge(fails, f"outact/M{M}", "outact.dx", v("dx", 128), x32, x64)
    assert not fails, fails


def test_mlp2_a_nan_stays_in_its_row():
    """A NaN in one row of x (forward) and of dy (backward): that row of mid, y, dmid, dx (g, dmid, dx) is NaN, every other row keeps its bits."""
    M, bad = 70, 37
    keep = torch.arange(M) != bad
    x, w1, b1, w2, b2, res, dy = D.mlp2_inputs(M, 128, 128, 128, seed=2)
    xb, dyb = x.clone(), dy.clone()
    xb[bad, 5], dyb[bad, 100] = D.NAN, D.NAN
    a, b = run_mlp2(x, w1, b1, w2, b2, res, dy, M), run_mlp2(xb, w1, b1, w2, b2, res, dyb, M)
    for k in ("mid", "y", "dmid", "dx"):
        va, vb = a[k][:M * 128].cpu().view(M, 128), b[k][:M * 128].cpu().view(M, 128)
        assert bool(torch.isnan(vb[bad]).all()), (k, "the NaN row")
        assert torch.equal(va[keep].view(i32), vb[keep].view(i32)) and bool(torch.isfinite(va).all()), (k, "other rows changed")
    x, w1, b1, w2, b2, _, dy = D.mlp2_inputs(M, 128, 64, 64, seed=2)
    xb, dyb = x.clone(), dy.clone()
    xb[bad, 5], dyb[bad, 60] = D.NAN, D.NAN
    a, b = run_outact(x, w1, b1, w2, b2, dy, M), run_outact(xb, w1, b1, w2, b2, dyb, M)
    for k, W in (("mid", 64), ("y", 64), ("g", 64), ("dmid", 64), ("dx", 128)):
        va, vb = a[k][:M * W].cpu().view(M, W), b[k][:M * W].cpu().view(M, W)
        assert bool(torch.isnan(vb[bad]).all()), (k, "the NaN row")
        assert torch.equal(va[keep].view(i32), vb[keep].view(i32)) and bool(torch.isfinite(va).all()), (k, "other rows changed")


def test_wgrad_a_nan_stays_in_its_column_or_row():
    """A NaN in one element of g: row n of dW and dbias[n] are NaN, the rest is finite and judged.  A NaN in one element of x: column k of dW."""
    fails = []
    for M, K, N in ((300, 128, 128), (300, 52, 36), (300, 63, 130)):
        g, x = D.wgrad_inputs(M, K, N)
        (w32, b32), (w64, b64) = both(lambda g_, x_: D.wgrad(g_, x_, M), g, x)
        n_bad, k_bad = N - 2, K // 3
        gb = g.clone()
        gb[211, n_bad] = D.NAN
        o = run_wgrad(gb, x, M, K, N)
        dW, db = o["dW"][:N * K].cpu().view(N, K), o["dbias"][:N].cpu()
        rows = torch.arange(N) != n_bad
        assert bool(torch.isnan(dW[n_bad]).all()) and bool(torch.isnan(db[n_bad])), "a NaN in g did not reach its row of dW / dbias"
        assert bool(torch.isfinite(dW[rows]).all()) and bool(torch.isfinite(db[rows]).all()), "a NaN in g reached other rows"
        judge(fails, f"wgrad-nan-g/K{K}/N{N}", "wgrad.dW", dW[rows], w32[rows], w64[rows])
        xb = x.clone()
        xb[17, k_bad] = D.NAN
        o = run_wgrad(g, xb, M, K, N)
        dW, db = o["dW"][:N * K].cpu().view(N, K), o["dbias"][:N].cpu()
        cols = torch.arange(K) != k_bad
        assert bool(torch.isnan(dW[:, k_bad]).all()), "a NaN in x did not reach its column of dW"
        assert bool(torch.isfinite(dW[:, cols]).all()) and bool(torch.isfinite(db).all()), "a NaN in x reached other columns"
        judge(fails, f"wgrad-nan-x/K{K}/N{N}", "wgrad.dW", dW[:, cols], w32[:, cols], w64[:, cols])
    assert not fails, fails


# ================================================================================================ closing: nothing was left out
def test_zz_every_dense_export_was_called():
    """The 19 entry points this module owns are declared in _lib.SIGNATURES and each was called by a test above; every branch name of the two
    branch functions was reached by a judged case.  (Run the whole module: this test looks at what the tests above did.)"""
    whole = "this test looks at what the other tests of the module did: run the whole module, in file order, in one process"
    assert len(OWNED) == 19 and len(set(OWNED)) == 19
    assert set(OWNED) <= set(_lib.SIGNATURES), sorted(set(OWNED) - set(_lib.SIGNATURES))
    assert set(OWNED) <= CALLED, (whole, sorted(set(OWNED) - CALLED))
    assert CALLED <= set(OWNED), sorted(CALLED - set(OWNED))
    assert {"batch/shared2", "batch/shared3", "batch/run-across-flush"} <= BRANCHES, whole
    assert D.LINEAR_BRANCHES | D.WGRAD_BRANCHES <= BRANCHES, (whole, sorted((D.LINEAR_BRANCHES | D.WGRAD_BRANCHES) - BRANCHES))
    print("\nworst err / yard per output (row, whole tensor):")
    for what, (rr, ra) in sorted(RATIOS.items()):
        print(f"TABLE {what:28s} row={rr:6.3g} all={ra:6.3g}")
