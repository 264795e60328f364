"""Every glue kernel on its own against the plain fp64 reference of the same operation (tests/glue_ref.py).

The 21 entry points named in OWNED (embedding lookup / gradient / one-hot rows, segment sum, graph_ptr, edge_index, the unary activations and
conan_ssp_bwd, RBF, cosine cutoff, zero tail, densify and its backward, the F_bary readout, MSE, global-norm clipping, the flat Adam step) are called
as C entry points (`raw`: the status code is visible) on crafted inputs: the sizes at which a kernel takes another path (partial tiles, 128-atom
chunks and their 32-deep batches, grids beyond their cap, n % 4 tails, graphs above 256 atoms), directed multigraphs, tied minima and maxima,
empty graphs, non-finite values.

Judging (visnet_ref.judge, unchanged, margins from visnet_ref): per row and per tensor, err(gpu, ref64) <= MARGIN * err(ref32, ref64) — the yardstick is
the reference formula in fp32 on the CPU, never the kernel.  Integer work and pure data movement (graph_ptr, edge_index, one-hot rows, the embedding
forward, the segment-sum broadcast, the zero tail, Cs, minmax) must be exact.  Every output buffer is pre-filled with a NaN bit pattern and has a
tail of 64 floats that must survive; every case runs twice and must give the same bits.  The conditions on the inputs are asserted by
tests/test_glue_ref_cpu.py.  The `RATIO` / `TABLE` lines printed by a run (-s) are the source of the table in DESIGN.md section 3.8."""
import math

import numpy as np
import pytest
import torch

import glue_ref as G
import visnet_ref as R
from conan_fgw_amd import _lib
from conan_fgw_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
OK, E_BADARG, E_UNSUPPORTED = 0, -1, -3
SENT, TAIL = 0x7FA5A5A5, 64              # a NaN bit pattern: reading it poisons a result, overwriting it is visible; floats beyond every documented size
CALLED, RATIOS = set(), {}
SHARED = (R.MARGIN_ROW, R.MARGIN_ALL)
# Outputs that need more than the shared margins: output -> (row, whole tensor) = 2 x the ratio measured on the MI355X against the fp32 reference's
# own error.  Measured values and reasons: DESIGN.md section 3.8.
GLUE_MARGIN = {
    # d = 1: the whole output is B numbers (1 or 3), each a serial fp32 sum of N = 33 terms where torch's sum is pairwise, judged as one short
    # row on which the yardstick is small by luck: measured 7.0 (N33/d1, mode 0) and 6.08 (mode 1), at most 2.9 at every other shape
    "readout0.out/d1": (14.0, 14.0),
    "readout1.out/d1": (12.2, 12.2),
    # n <= 5: one to five numbers; the kernel forms m + (1 - b1) (g - m) as torch's kernels do, the reference b1 m + (1 - b1) g, and on three
    # numbers the reference's own error happens to be small: measured 7.84 (n = 3, weight decay, step 2), 1.0 from n = 1023 on
    "adam.m/n<=5": (15.7, 15.7),
}

OWNED = ["conan_embedding_fwd", "conan_embedding_bwd", "conan_embedding_bwd_ws", "conan_onehot_rows", "conan_segment_sum_fwd", "conan_segment_sum_bwd",
         "conan_graph_ptr_from_batch", "conan_edge_index_i64", "conan_unary_fwd", "conan_unary_bwd", "conan_ssp_bwd", "conan_rbf_fwd",
         "conan_cutoff_scale", "conan_zero_tail", "conan_fgw_densify", "conan_fgw_densify_bwd", "conan_fgw_readout_fwd", "conan_fgw_readout_bwd",
         "conan_mse_loss_fwd", "conan_grad_clip_flat", "conan_adam_flat_step"]


def raw(name, *args):
    """The C entry point itself: returns the status code instead of raising."""
    CALLED.add(name)
    return getattr(lib(), name)(*args)


def sent_i(numel):
    return torch.full((numel,), SENT, dtype=i32, device=dev)


def sent(numel):
    """An output buffer of `numel` floats and the tail, all of the NaN pattern."""
    return sent_i(numel + TAIL).view(f32)


def is_sent(t):
    return bool((t.contiguous().view(i32) == SENT).all())


def cut(t, numel, what=""):
    """The documented part of a buffer (CPU); the tail must still hold the pattern."""
    assert is_sent(t[numel:]), (what, "written beyond its documented size")
    return t[:numel].cpu()


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def twice(fn):
    """Run a case twice on fresh buffers: the same bits in every buffer (tails and workspaces included)."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert same_bits(a, b), "two runs differ"
    return a


def d_(t):
    return None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(dev).contiguous()


def exact(a, b):
    """Bit-for-bit up to the NaN payload: NaN where b is NaN, equal elsewhere."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def both(fn, *floats):
    """(ref32, ref64) of a reference formula: the same function on the fp32 inputs and on their fp64 copies (CPU)."""
    return fn(*floats), fn(*[t.double() for t in floats])


def judge(fails, case, what, got, r32, r64):
    assert got.shape == r64.shape, (case, what, got.shape, r64.shape)
    mr, ma = GLUE_MARGIN.get(what, SHARED)
    ok, rr, ra = R.judge(got, r32, r64, mr, ma)
    old = RATIOS.get(what, (0.0, 0.0))
    RATIOS[what] = (max(old[0], rr), max(old[1], ra))
    print(f"RATIO {case} {what} row={rr:.3g} all={ra:.3g}")
    if not ok:
        fails.append((case, what, float("%.3g" % rr), float("%.3g" % ra)))


# ================================================================================================ embedding
EMB = {c[0]: c for c in G.embedding_cases()}


@pytest.mark.parametrize("name", list(EMB))
def test_embedding_forward_gradient_and_onehot_rows(name):
    """Forward and one-hot rows exact (an id outside [0, rows) — -1, rows, 2^40 — gives a NaN row / an all-zero row and adds nothing to the
    gradient); the gradient against index_add; the workspace beyond conan_embedding_bwd_ws keeps the pattern."""
    _, rows, H, n, pad, kind = EMB[name]
    z, w, dout = G.embedding_inputs(EMB[name])
    zd, wd, dd, s = d_(z), d_(w), d_(dout), stream_ptr()
    wsn = int(raw("conan_embedding_bwd_ws", n, H, rows))
    assert wsn == ((n + 127) // 128) * rows * H

    def run():
        o = {"out": sent(n * H), "onehot": sent(n * rows), "dw": sent(rows * H), "ws": sent(wsn)}
        assert raw("conan_embedding_fwd", ptr(zd), ptr(wd), n, H, rows, ptr(o["out"]), s) == OK
        assert raw("conan_onehot_rows", ptr(zd), n, rows, pad, ptr(o["onehot"]), s) == OK
        assert raw("conan_embedding_bwd", ptr(zd), ptr(dd), n, H, rows, pad, ptr(o["dw"]), ptr(o["ws"]), s) == OK
        return o
    o = twice(run)
    cut(o["ws"], wsn, "ws")
    want = G.embedding(w, z)
    assert exact(cut(o["out"], n * H, "out").view(n, H), want)
    if kind == "bad":
        assert bool(torch.isnan(want[[1, 5, n - 1]]).all()) and int(torch.isnan(want).any(dim=1).sum()) == 3
    oh = cut(o["onehot"], n * rows, "onehot").view(n, rows)
    assert torch.equal(oh, G.onehot_rows(z, rows, pad))
    if kind == "bad":
        assert float(oh[[1, 5, n - 1]].abs().max()) == 0.0
    dw = cut(o["dw"], rows * H, "dw").view(rows, H)
    assert bool(torch.isfinite(dw).all())
    if 0 <= pad < rows:
        assert float(dw[pad].abs().max()) == 0.0
    fails = []
    r32, r64 = both(lambda t: G.embedding_grad(z, t, rows, pad), dout)
    judge(fails, name, "embedding.dweight/one-type" if kind == "one" else "embedding.dweight", dw, r32, r64)
    assert not fails, fails


def test_embedding_status_codes():
    z, w, s = torch.zeros(8, dtype=i64, device=dev), torch.randn(101, 8, device=dev), stream_ptr()
    out, dw, ws = sent(8 * 8), sent(101 * 8), sent(101 * 8)
    assert raw("conan_embedding_fwd", ptr(z), ptr(w), 8, 6, 100, ptr(out), s) == E_BADARG                  # H not a multiple of 4
    assert raw("conan_embedding_bwd", ptr(z), ptr(w), 8, 8, 101, 0, ptr(dw), ptr(ws), s) == E_UNSUPPORTED  # more than 100 rows
    torch.cuda.synchronize()
    assert is_sent(out) and is_sent(dw) and is_sent(ws)
    assert raw("conan_embedding_fwd", ptr(z), ptr(w), 0, 8, 100, ptr(out), s) == OK
    assert raw("conan_onehot_rows", ptr(z), 0, 100, 0, ptr(out), s) == OK
    assert raw("conan_embedding_bwd_ws", 0, 8, 100) == 0
    assert raw("conan_embedding_bwd", ptr(z), ptr(w), 0, 8, 100, 0, ptr(dw), ptr(ws), s) == OK              # no atoms: dweight all zero
    torch.cuda.synchronize()
    assert is_sent(out) and is_sent(ws) and is_sent(dw[800:]) and float(dw[:800].abs().max()) == 0.0


# ================================================================================================ segment sum
@pytest.mark.parametrize("W", G.SEG_W)
def test_segment_sum_and_its_broadcast(W):
    """Graph sizes 0, 1, 7, 8, 9, 64, 65, 0: an empty graph gives a zero row (at the start, in the middle, at the end); the backward is data
    movement and must be bit-exact."""
    gptr = G.seg_gptr()
    Gn, n = len(gptr) - 1, int(gptr[-1])
    gen = G.gen(W)
    x, dout = torch.randn(n, W, generator=gen), torch.randn(Gn, W, generator=gen)
    xd, dd, gd, s = d_(x), d_(dout), d_(gptr), stream_ptr()

    def run():
        o = {"out": sent(Gn * W), "dx": sent(n * W)}
        assert raw("conan_segment_sum_fwd", ptr(xd), ptr(gd), Gn, W, ptr(o["out"]), s) == OK
        assert raw("conan_segment_sum_bwd", ptr(dd), ptr(gd), Gn, W, ptr(o["dx"]), s) == OK
        return o
    o = twice(run)
    out, dx = cut(o["out"], Gn * W, "out").view(Gn, W), cut(o["dx"], n * W, "dx").view(n, W)
    for g, size in enumerate(G.SEG_SIZES):
        if size == 0:
            assert float(out[g].abs().max()) == 0.0
    assert torch.equal(dx, G.segment_sum_grad(dout, gptr))
    fails = []
    judge(fails, f"W{W}", "segment_sum", out, *both(lambda t: G.segment_sum(t, gptr), x))
    assert not fails, fails
    assert raw("conan_segment_sum_fwd", ptr(xd), ptr(gd), 0, W, ptr(o["out"]), s) == OK


# ================================================================================================ graph_ptr / edge_index
def _batch(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


GRAPH_PTR_CASES = {"empties": [0, 0, 3, 0, 5, 1, 0, 0], "n0/G0": [], "n0/G1": [0], "n0/G300": [0] * 300, "n1": [1], "n256": [100, 0, 156],
                   "n257/one-graph": [257], "n257/owner-in-the-middle": [0, 257, 0], "n257/last-block-of-one": [256, 0, 1]}


@pytest.mark.parametrize("name", list(GRAPH_PTR_CASES))
def test_graph_ptr_is_searchsorted(name):
    sizes = GRAPH_PTR_CASES[name]
    batch, Gn = _batch(sizes), len(sizes)
    n, s = len(batch), stream_ptr()
    bd = d_(batch) if n else None

    def run():
        o = {"gptr": sent_i(Gn + 1 + TAIL)}
        assert raw("conan_graph_ptr_from_batch", ptr(bd), n, Gn, ptr(o["gptr"]), s) == OK
        return o
    o = twice(run)
    assert is_sent(o["gptr"][Gn + 1:])
    assert np.array_equal(o["gptr"][:Gn + 1].cpu().numpy(), G.graph_ptr(batch, Gn))
    assert np.array_equal(G.graph_ptr(batch, Gn), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))


@pytest.mark.parametrize("E", [0, 1, 255, 256, 257, 1000])
def test_edge_index_rows_are_source_and_target(E):
    rng = np.random.RandomState(E)
    col, tgt = rng.randint(0, 2 ** 31 - 1, max(E, 1)).astype(np.int32), rng.randint(0, 2 ** 31 - 1, max(E, 1)).astype(np.int32)
    cd, td, s = d_(col), d_(tgt), stream_ptr()

    def run():
        o = {"ei": sent_i(2 * (2 * E + TAIL))}
        assert raw("conan_edge_index_i64", ptr(cd), ptr(td), E, ptr(o["ei"]), s) == OK
        return o
    o = twice(run)
    assert is_sent(o["ei"][4 * E:])
    ei = o["ei"][:4 * E].view(i64).view(2, E).cpu().numpy()
    assert np.array_equal(ei[0], col[:E].astype(np.int64)) and np.array_equal(ei[1], tgt[:E].astype(np.int64))


# ================================================================================================ activations
@pytest.mark.parametrize("count", G.UNARY_COUNTS)
@pytest.mark.parametrize("op", [0, 1, 2])
def test_unary_forward_and_backward_from_the_output(op, count):
    """randn at the scales 1e-3, 1 and 30.  The backward is judged as the operation (y, dy) -> dx on outputs y of its own (op 2: down to
    -ln 2 + 1e-7, where 1 - 0.5 exp(-y) cancels); conan_ssp_bwd (rows = count, width 1) is the same operation through expf."""
    x = G.unary_x(count)
    y, dy = G.unary_y_dy(op, count)
    xd, yd, dyd, s = d_(x), d_(y), d_(dy), stream_ptr()

    def run():
        o = {"y": sent(count), "dx": sent(count)}
        assert raw("conan_unary_fwd", ptr(xd), count, op, ptr(o["y"]), s) == OK
        assert raw("conan_unary_bwd", ptr(yd), ptr(dyd), count, op, ptr(o["dx"]), s) == OK
        if op == 2:
            o["g"] = sent(count)
            assert raw("conan_ssp_bwd", ptr(dyd), ptr(yd), count, 1, None, ptr(o["g"]), s) == OK
        return o
    o = twice(run)
    fails, tag = [], f"op{op}/n{count}"
    name = ("relu", "sigmoid", "ssp")[op]
    judge(fails, tag, f"unary.{name}", cut(o["y"], count, "y"), *both(lambda t: G.unary(op, t), x))
    r32, r64 = both(lambda a, b: G.unary_grad_from_output(op, a, b), y, dy)
    judge(fails, tag, f"unary.{name}'", cut(o["dx"], count, "dx"), r32, r64)
    if op == 2:
        judge(fails, tag, "ssp_bwd", cut(o["g"], count, "g"), r32, r64)
    if op == 0:                                                         # a selection: exact
        assert torch.equal(o["y"][:count].cpu(), torch.relu(x)) and torch.equal(o["dx"][:count].cpu(), r32)
    assert not fails, fails
    assert raw("conan_unary_fwd", None, 0, op, None, s) == OK and raw("conan_unary_bwd", None, None, 0, op, None, s) == OK
    assert raw("conan_unary_fwd", ptr(xd), count, 3, ptr(o["y"]), s) == E_BADARG


def _same_class(got, want):
    """NaN where torch gives NaN, the same infinity, the exact value where torch gives exactly 0 or 1."""
    pinned = torch.isinf(want) | (want == 0) | (want == 1)
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[pinned], want[pinned])


@pytest.mark.parametrize("op", [0, 1, 2])
def test_unary_on_the_listed_values_is_torch_entry_by_entry(op):
    """+-0, +-1e-30, +-20, +-88, +-104, +-1e4, +-inf, NaN.  Forward: the class of torch's result (NaN, the same infinity, exact 0 or 1 where torch
    gives them) and, where it is finite, torch's value within the shared margin of the fp32 reference's own error, but no finer than four units in
    the last place of the result (the reference in fp32 is exact on most of these).  A NaN must stay visible: torch.relu(NaN) is NaN.  Backward from
    torch's outputs: torch's threshold_backward / sigmoid / softplus gradient, same non-finite class, finite entries within 4 ulp(1) |dy| (the
    from-output formulas 1 - 0.5 exp(-y) and y (1 - y) carry the rounding of y, at most one ulp of 1, into a derivative of at most 1)."""
    x = torch.tensor(G.SPECIAL, dtype=f32)
    n, s = x.numel(), stream_ptr()
    x32 = x.clone().requires_grad_(True)
    y32 = G.unary(op, x32)
    dy = torch.full((n,), 1.5)
    (gx32,) = torch.autograd.grad(y32, x32, dy)
    y32 = y32.detach()
    xd, yd, dyd = d_(x), d_(y32), d_(dy)

    def run():
        o = {"y": sent(n), "dx": sent(n), "g": sent(n)}
        assert raw("conan_unary_fwd", ptr(xd), n, op, ptr(o["y"]), s) == OK
        assert raw("conan_unary_bwd", ptr(yd), ptr(dyd), n, op, ptr(o["dx"]), s) == OK
        if op == 2:
            assert raw("conan_ssp_bwd", ptr(dyd), ptr(yd), n, 1, None, ptr(o["g"]), s) == OK
        return o
    o = twice(run)
    y, dx = cut(o["y"], n, "y"), cut(o["dx"], n, "dx")
    print("x   ", x.tolist(), "\ngpu ", y.tolist(), "\ntorch", y32.tolist(), "\ndx  ", dx.tolist(), "\ntorch", gx32.tolist())
    assert _same_class(y, y32), (y.tolist(), y32.tolist())
    fin = torch.isfinite(y32)
    y64 = G.unary(op, x.double())
    ulp = torch.from_numpy(np.spacing(np.abs(y32[fin].numpy()))).double()
    bound = torch.maximum(R.MARGIN_ROW * (y32[fin].double() - y64[fin]).abs(), 4 * ulp)
    assert bool(((y[fin].double() - y64[fin]).abs() <= bound).all()), ((y[fin].double() - y64[fin]).abs() / bound).tolist()
    for got in ([dx, cut(o["g"], n, "g")] if op == 2 else [dx]):
        nonfin = ~torch.isfinite(gx32)
        assert torch.equal(torch.isnan(got), torch.isnan(gx32)) and torch.equal(got[nonfin & ~torch.isnan(gx32)], gx32[nonfin & ~torch.isnan(gx32)])
        assert bool(((got[~nonfin] - gx32[~nonfin]).abs() <= 4 * 2.0 ** -23 * 1.5).all()), (got.tolist(), gx32.tolist())
    if op == 0:
        assert math.isnan(float(y[-1])) and float(dx[-1]) == 1.5          # NaN passes through, forward and backward (threshold_backward)


@pytest.mark.parametrize("m", [None, 0, 299, 300, 303])
def test_ssp_bwd_device_row_count(m):
    """rows = 300, width = 7: rows at or beyond *m_dev keep the pattern; a count beyond `rows` is clamped."""
    rows, W = 300, 7
    y, dy = G.unary_y_dy(2, rows * W, seed=5)
    yd, dyd, s = d_(y), d_(dy), stream_ptr()
    md = None if m is None else torch.tensor([m], dtype=i32, device=dev)

    def run():
        o = {"g": sent(rows * W)}
        assert raw("conan_ssp_bwd", ptr(dyd), ptr(yd), rows, W, ptr(md), ptr(o["g"]), s) == OK
        return o
    o = twice(run)
    live = (rows if m is None else min(m, rows)) * W
    assert is_sent(o["g"][live:])
    if live:
        fails = []
        r32, r64 = both(lambda a, b: G.unary_grad_from_output(2, a, b), y[:live], dy[:live])
        judge(fails, f"m{m}", "ssp_bwd", o["g"][:live].cpu(), r32, r64)
        assert not fails, fails
    assert raw("conan_ssp_bwd", None, None, 0, 7, None, None, s) == OK and raw("conan_ssp_bwd", ptr(dyd), ptr(yd), 3, 0, None, ptr(o["g"]), s) == E_BADARG


# ================================================================================================ rbf / cutoff / zero tail
def _edge_counts(max_edges):
    return [None, 0, max_edges - 1, max_edges, max_edges + 7]


RBF_SHAPES = [(Gs, me, None) for Gs in G.RBF_GS for me in (1, 1000)] + [(50, 1000, m) for m in _edge_counts(1000)[1:]] + [(50, 10500, None)]
CUT_SHAPES = [(F_, me, None) for F_ in G.CUT_F for me in (1, 1000)] + [(32, 1000, m) for m in _edge_counts(1000)[1:]] + [(128, 16400, None)]


@pytest.mark.parametrize("Gs,max_edges,m", RBF_SHAPES)
def test_rbf_expansion(Gs, max_edges, m):
    """dist holds 0, 1e-6, cutoff / 2, the float below the cutoff and the cutoff; 10500 x 50 is beyond the grid of 2048 x 256 threads; rows beyond
    the device-side count keep the pattern (a count beyond max_edges is clamped)."""
    dist = G.edge_dist(max_edges)
    off, coeff = G.rbf_offset(Gs)
    dd, od, s = d_(dist), d_(off), stream_ptr()
    md = None if m is None else torch.tensor([m], dtype=i32, device=dev)

    def run():
        o = {"rbf": sent(max_edges * Gs)}
        assert raw("conan_rbf_fwd", ptr(dd), ptr(md), max_edges, ptr(od), Gs, coeff, ptr(o["rbf"]), s) == OK
        return o
    o = twice(run)
    live = max_edges if m is None else min(m, max_edges)
    assert is_sent(o["rbf"][live * Gs:])
    if live:
        fails = []
        judge(fails, f"Gs{Gs}/E{max_edges}/m{m}", "rbf", o["rbf"][:live * Gs].cpu().view(live, Gs), *both(lambda a, b: G.rbf(a, b, coeff), dist[:live], off))
        assert not fails, fails


@pytest.mark.parametrize("F_,max_edges,m", CUT_SHAPES)
def test_cosine_cutoff_scaling(F_, max_edges, m):
    dist = G.edge_dist(max_edges, seed=1)
    x = torch.randn(max_edges, F_, generator=G.gen(F_ + max_edges))
    dd, xd, s = d_(dist), d_(x), stream_ptr()
    md = None if m is None else torch.tensor([m], dtype=i32, device=dev)

    def run():
        o = {"out": sent(max_edges * F_)}
        assert raw("conan_cutoff_scale", ptr(dd), ptr(md), max_edges, F_, G.CUTOFF, ptr(xd), ptr(o["out"]), s) == OK
        return o
    o = twice(run)
    live = max_edges if m is None else min(m, max_edges)
    assert is_sent(o["out"][live * F_:])
    if live:
        fails = []
        got = o["out"][:live * F_].cpu().view(live, F_)
        judge(fails, f"F{F_}/E{max_edges}/m{m}", "cutoff_scale", got, *both(lambda a, b: G.cutoff_scale(a, G.CUTOFF, b), dist[:live], x[:live]))
        assert not fails, fails
        if live >= 5:
            assert float(got[4].abs().max()) == 0.0                       # d == cutoff: the factor is exactly 0
            assert torch.equal(got[0], x[0])                              # d == 0: exactly 1


def test_rbf_and_cutoff_status_codes():
    dist, x, out, s = torch.rand(8, device=dev), torch.randn(8, 8, device=dev), sent(64), stream_ptr()
    assert raw("conan_cutoff_scale", ptr(dist), None, 8, 6, 10.0, ptr(x), ptr(out), s) == E_BADARG       # width not a multiple of 4
    assert raw("conan_rbf_fwd", ptr(dist), None, 8, ptr(dist), 0, -0.5, ptr(out), s) == E_BADARG
    assert raw("conan_cutoff_scale", ptr(dist), None, 0, 8, 10.0, ptr(x), ptr(out), s) == OK             # no edges: nothing written
    assert raw("conan_rbf_fwd", ptr(dist), None, 0, ptr(dist), 8, -0.5, ptr(out), s) == OK
    torch.cuda.synchronize()
    assert is_sent(out)


@pytest.mark.parametrize("rows,width", [(r, w) for r in (1, 1000, 2000) for w in (1, 3, 128)])
def test_zero_tail(rows, width):
    """Rows [*m_dev, rows) become +0.0, the head keeps the pattern, the guard floats are intact; 2000 x 128 is beyond 512 x 256 threads."""
    s = stream_ptr()
    for m in sorted({0, 1, rows - 1, rows, rows + 5}):
        md = torch.tensor([m], dtype=i32, device=dev)

        def run():
            o = {"buf": sent(rows * width)}
            assert raw("conan_zero_tail", ptr(o["buf"]), ptr(md), rows, width, s) == OK
            return o
        o = twice(run)
        lo = min(m, rows) * width
        assert is_sent(o["buf"][:lo]) and is_sent(o["buf"][rows * width:]), (rows, width, m)
        assert bool((o["buf"][lo:rows * width].view(i32) == 0).all()), (rows, width, m)        # +0.0 bit for bit
    assert raw("conan_zero_tail", ptr(o["buf"]), None, rows, width, s) == E_BADARG


# ================================================================================================ densify
DENS = G.densify_cases()


def run_densify(c, with_cs=True):
    fd, gd, rd, cd, dyd, s = d_(c.feat), d_(c.gptr), d_(c.rowptr), d_(c.col), d_(c.dYs), stream_ptr()
    o = {"Ys": sent(c.G * c.N * c.d), "minmax": sent(c.G * 2), "dfeat": sent(c.n_atoms * c.d)}
    if with_cs:
        o["Cs"] = sent(c.G * c.N * c.N)
    assert raw("conan_fgw_densify", ptr(fd), ptr(gd), ptr(rd), ptr(cd), c.G, c.N, c.d, c.shift, c.a, c.b, ptr(o["Ys"]), ptr(o["Cs"]) if with_cs else None,
               ptr(o["minmax"]), s) == OK
    assert raw("conan_fgw_densify_bwd", ptr(fd), ptr(dyd), ptr(gd), ptr(o["minmax"]), c.G, c.N, c.d, c.shift, c.a, c.b, ptr(o["dfeat"]), s) == OK
    return o


def densify_reference(c):
    """{"Ys32", "Ys64", "dfeat32", "dfeat64"} by torch autograd through glue_ref.densify."""
    r = {}
    for tag, dt in (("32", f32), ("64", f64)):
        feat = c.feat.to(dt).clone().requires_grad_(True)
        Ys = G.densify(feat, c.gptr, c.N, c.shift, c.a, c.b)
        (r["dfeat" + tag],) = torch.autograd.grad(Ys, feat, c.dYs.to(dt))
        r["Ys" + tag] = Ys.detach()
    return r


@pytest.mark.parametrize("name", list(DENS))
def test_densify_and_its_backward(name):
    """Hand-made CSR: directed edges fix Cs[g, src, tgt]; multiplicities 2 and 3; graphs without edges; a source outside the graph is dropped;
    n = N, n < N, n = 0; graphs of 257 and 300 atoms (row pointers in chunks of 256); features quantised to multiples of 0.25 (min and max tie,
    the padding zeros among the minima); a constant slab.  minmax is a min / max of fp32 numbers: exact.  NaN where the reference gives NaN (a slab
    of range 0) and nowhere else; Cs == NULL gives the same Ys bits and touches nothing else."""
    c = DENS[name]
    o = twice(lambda: run_densify(c))
    o2 = run_densify(c, with_cs=False)
    torch.cuda.synchronize()
    assert same_bits({k: o[k] for k in o2}, o2), "Cs == NULL changes Ys / minmax / dfeat"
    Ys, mm = cut(o["Ys"], c.G * c.N * c.d, "Ys").view(c.G, c.N, c.d), cut(o["minmax"], c.G * 2, "minmax").view(c.G, 2)
    Cs, df = cut(o["Cs"], c.G * c.N * c.N, "Cs").view(c.G, c.N, c.N), cut(o["dfeat"], c.n_atoms * c.d, "dfeat").view(c.n_atoms, c.d)
    want_adj = G.dense_adj(c.rowptr, c.col, c.gptr, c.N)
    assert torch.equal(Cs, want_adj), name
    if c.E:
        assert not torch.equal(want_adj, want_adj.transpose(1, 2)) and float(want_adj.max()) >= 3.0 and bool((want_adj == 2).any())      # directed, multi-edges
    for g in range(c.G):
        lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
        t = torch.cat([c.feat[lo:hi], torch.zeros(c.N - (hi - lo), c.d)]) + torch.tensor(c.shift, dtype=f32)
        assert float(mm[g, 0]) == float(t.min()) and float(mm[g, 1]) == float(t.max()), (name, g)
    r = densify_reference(c)
    bad = sorted(set(int(g) for g in torch.isnan(r["Ys64"]).any(dim=2).any(dim=1).nonzero().flatten()))
    assert bad == G.DEGENERATE_DENSIFY.get(name, []), (name, bad)
    assert torch.equal(torch.isnan(Ys), torch.isnan(r["Ys64"])) and torch.equal(torch.isnan(df), torch.isnan(r["dfeat64"])), name
    assert bool(torch.isfinite(Ys[~torch.isnan(Ys)]).all()) and bool(torch.isfinite(df[~torch.isnan(df)]).all())
    keep = [g for g in range(c.G) if g not in bad]
    rows = torch.cat([torch.arange(int(c.gptr[g]), int(c.gptr[g + 1])) for g in keep])
    fails = []
    judge(fails, name, "densify.Ys", Ys[keep].reshape(-1, c.d), r["Ys32"][keep].reshape(-1, c.d), r["Ys64"][keep].reshape(-1, c.d))
    judge(fails, name, "densify.dfeat", df[rows], r["dfeat32"][rows], r["dfeat64"][rows])
    assert not fails, fails


def test_densify_overflowing_graph_is_poisoned_and_leaves_the_others_alone():
    """A graph of N + 2 atoms: its slab of Ys, its minmax and ALL its rows of dfeat are NaN; every other graph has the bits it has when the
    overflowing graph is empty instead."""
    N, d = 8, 3
    base = G.DensifyCase("base", [5, 0, 6, 8], N, d, 0.5, seed=9)
    over = G.DensifyCase("over", [5, N + 2, 6, 8], N, d, 0.5, seed=9)
    over.feat = torch.cat([base.feat[:5], torch.randn(N + 2, d, generator=G.gen(3)), base.feat[5:]])
    over.dYs = base.dYs.clone()
    a, b = twice(lambda: run_densify(base)), twice(lambda: run_densify(over))
    sl = N * d
    Ya, Yb = cut(a["Ys"], 4 * sl).view(4, N, d), cut(b["Ys"], 4 * sl).view(4, N, d)
    ma, mb = cut(a["minmax"], 8).view(4, 2), cut(b["minmax"], 8).view(4, 2)
    Ca, Cb = cut(a["Cs"], 4 * N * N).view(4, N, N), cut(b["Cs"], 4 * N * N).view(4, N, N)
    da, db = cut(a["dfeat"], 19 * d).view(19, d), cut(b["dfeat"], (19 + N + 2) * d).view(19 + N + 2, d)
    assert bool(torch.isnan(Yb[1]).all()) and bool(torch.isnan(mb[1]).all()) and bool(torch.isnan(db[5:5 + N + 2]).all())
    for g in (0, 2, 3):
        assert torch.equal(Ya[g], Yb[g]) and torch.equal(ma[g], mb[g]) and torch.equal(Ca[g], Cb[g]), g
    assert torch.equal(da, torch.cat([db[:5], db[5 + N + 2:]])) and bool(torch.isfinite(da).all())
    s = stream_ptr()
    assert raw("conan_fgw_densify", None, None, None, None, 0, N, d, 0.5, 0.1, 2.0, None, None, None, s) == E_BADARG


# ================================================================================================ F_bary readout
RO = {c[0]: c for c in G.readout_cases()}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(RO))
def test_fgw_readout_and_its_backward(name, mode):
    """Column sums (mode 0) and the guarded, column-normalised sums (mode 1), N around the 8-deep unroll, d around the 64 lanes.  One NaN in one
    molecule / one all-zero column (mode 1): the non-finite pattern of output and gradient is the reference's — a molecule holding a NaN was
    replaced by zeros, so its output is 0 / 0 and no gradient reaches it — and everything else is judged as usual.  N = 1 in mode 1: the exact
    gradient of y / |y| is 0 and both references give rounding noise around it, so the kernel's is held to that noise instead: the two terms
    1 / |y| and y^2 / |y|^3 of the difference carry at most 8 roundings between them, |dY| <= 8 x 2^-24 |g| / |y|."""
    _, B, K, N, d, kind = RO[name]
    Y, dout = G.readout_inputs(RO[name])
    Yd, dd, s = d_(Y), d_(dout), stream_ptr()

    def run():
        o = {"out": sent(B * K * d), "dY": sent(B * N * d)}
        assert raw("conan_fgw_readout_fwd", ptr(Yd), B, K, N, d, mode, ptr(o["out"]), s) == OK
        assert raw("conan_fgw_readout_bwd", ptr(Yd), ptr(dd), B, K, N, d, mode, ptr(o["dY"]), s) == OK
        return o
    o = twice(run)
    out, dY = cut(o["out"], B * K * d, "out").view(B * K, d), cut(o["dY"], B * N * d, "dY").view(B, N, d)
    r = {}
    for tag, dt in (("32", f32), ("64", f64)):
        Yr = Y.to(dt).clone().requires_grad_(True)
        ro = G.readout(Yr, K, mode)
        (r["dY" + tag],) = torch.autograd.grad(ro, Yr, dout.to(dt))
        r["out" + tag] = ro.detach()
    assert torch.equal(torch.isfinite(out), torch.isfinite(r["out64"])), (name, "non-finite pattern of the output")
    assert torch.equal(torch.isfinite(dY), torch.isfinite(r["dY64"])), (name, "non-finite pattern of the gradient")
    if kind == "randn" or mode == 0 and kind == "zerocol":
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dY).all())
    if kind == "nan" and mode == 1:
        assert bool(torch.isnan(out[K:2 * K]).all()) and float(dY[1].abs().max()) == 0.0
    fin_o, fin_d = torch.isfinite(r["out64"]), torch.isfinite(r["dY64"])
    z = lambda t, m: torch.where(m, t, torch.zeros_like(t))                  # non-finite entries (equal patterns, asserted above) out of the norms
    fails = []
    judge(fails, f"{name}/mode{mode}", f"readout{mode}.out" + ("/d1" if d == 1 else ""), z(out, fin_o), z(r["out32"], fin_o), z(r["out64"], fin_o))
    if mode == 1 and N == 1:
        g = dout.view(B, K, d).sum(1)
        assert bool((dY[:, 0].abs() <= 8 * 2.0 ** -24 * g.abs() / Y[:, 0].abs()).all())
    else:
        judge(fails, f"{name}/mode{mode}", f"readout{mode}.dY", z(dY, fin_d).view(B * N, d), z(r["dY32"], fin_d).view(B * N, d), z(r["dY64"], fin_d).view(B * N, d))
    assert not fails, fails
    assert raw("conan_fgw_readout_fwd", ptr(Yd), B, K, N, d, 2, ptr(o["out"]), s) == E_BADARG


# ================================================================================================ MSE
@pytest.mark.parametrize("n", G.MSE_N)
def test_mse_loss_and_gradient(n):
    gen = G.gen(n)
    pred, target = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    pd, td, s = d_(pred), d_(target), stream_ptr()

    def run():
        o = {"loss": sent(1), "dpred": sent(n)}
        assert raw("conan_mse_loss_fwd", ptr(pd), ptr(td), n, ptr(o["loss"]), ptr(o["dpred"]), s) == OK
        return o
    o = twice(run)
    (l32, d32), (l64, d64) = both(G.mse, pred, target)
    fails = []
    judge(fails, f"n{n}", "mse.loss", cut(o["loss"], 1, "loss"), l32.reshape(1), l64.reshape(1))
    judge(fails, f"n{n}", "mse.dpred", cut(o["dpred"], n, "dpred"), d32, d64)
    assert not fails, fails
    assert raw("conan_mse_loss_fwd", ptr(pd), ptr(td), 0, ptr(o["loss"]), ptr(o["dpred"]), s) == E_BADARG


# ================================================================================================ global-norm clipping
def _within_one_ulp(got, want64):
    w = np.float32(want64)
    return bool(abs(np.float64(got) - np.float64(w)) <= np.float64(np.spacing(np.abs(w))))


def run_clip(g, max_norm):
    """One launch of conan_grad_clip_flat on a copy of g -> (gradient, norm, coefficient); partials and ticket checked."""
    n, s = g.numel(), stream_ptr()
    buf = sent(n + 4)                                                   # 16-byte aligned copy with a guard tail
    buf[:n] = g.to(dev)
    nc, part, ticket = sent(2), sent_i(2 * 256 + TAIL), torch.zeros(1, dtype=i32, device=dev)
    assert raw("conan_grad_clip_flat", ptr(buf), n, float(max_norm), ptr(nc), part.data_ptr(), ptr(ticket), s) == OK
    torch.cuda.synchronize()
    blocks = min(max(((n >> 2) + 255) // 256, 1), 256)
    assert int(ticket) == 0, "the ticket word is not back at 0"
    assert is_sent(part[2 * blocks:]), "a partial slot beyond the number of workgroups was written"
    assert not bool((part[:2 * blocks] == SENT).any())
    assert is_sent(nc[2:])
    return {"g": buf, "nc": nc}


@pytest.mark.parametrize("n", G.CLIP_N)
def test_grad_clip_flat(n):
    """Above the threshold: norm and coefficient are the fp64 values rounded to fp32 within one unit in the last place, the gradient is judged;
    below it and all-zero: the gradient keeps its bits.  One NaN: coefficient and every element NaN.  One +inf: norm inf, coefficient 0, NaN at
    that element and 0 elsewhere, as torch gives.  One launch per scenario and repeat."""
    g = G.clip_grad(n)
    if n == 0:
        o = twice(lambda: run_clip(g, 1.0))
        assert float(o["nc"][0]) == 0.0 and float(o["nc"][1]) == 1.0
        return
    nrm64 = float(g.double().norm())
    fails = []
    # above
    mx = 0.5 * nrm64
    o = twice(lambda: run_clip(g, mx))
    n64, c64, _ = G.clip(g.double(), mx)
    assert _within_one_ulp(float(o["nc"][0]), float(n64)) and _within_one_ulp(float(o["nc"][1]), float(c64)), (o["nc"][:2].tolist(), float(n64), float(c64))
    (_, _, g32), (_, _, g64) = both(lambda t: G.clip(t, mx), g)
    judge(fails, f"n{n}/above", "clip.grads", cut(o["g"], n, "g"), g32, g64)
    # below: bit-identical
    o = twice(lambda: run_clip(g, 2.0 * nrm64 + 1.0))
    assert float(o["nc"][1]) == 1.0 and _within_one_ulp(float(o["nc"][0]), nrm64)
    assert torch.equal(cut(o["g"], n, "g").view(i32), g.view(i32))
    # all-zero
    zero = torch.zeros(n)
    o = twice(lambda: run_clip(zero, 1.0))
    assert float(o["nc"][0]) == 0.0 and float(o["nc"][1]) == 1.0 and bool((cut(o["g"], n).view(i32) == 0).all())
    # one NaN, one +inf (at the last element: the n % 4 tail when there is one)
    bad = g.clone(); bad[n - 1] = G.NAN
    o = twice(lambda: run_clip(bad, 1.0))
    assert bool(torch.isnan(o["nc"][:2]).all()) and bool(torch.isnan(cut(o["g"], n)).all())
    bad = g.clone(); bad[n - 1] = G.INF
    o = twice(lambda: run_clip(bad, 1.0))
    got = cut(o["g"], n)
    _, c_t, g_t = G.clip(bad, 1.0)
    assert float(o["nc"][0]) == G.INF and float(o["nc"][1]) == 0.0 == float(c_t)
    assert math.isnan(float(got[n - 1])) and bool((got[:n - 1] == 0).all()) and exact(got, g_t)
    assert not fails, fails


def test_grad_clip_flat_status_codes():
    g, nc, part, ticket, s = sent(16), sent(2), sent_i(2 * 256), torch.zeros(1, dtype=i32, device=dev), stream_ptr()
    assert raw("conan_grad_clip_flat", g.data_ptr() + 4, 8, 1.0, ptr(nc), part.data_ptr(), ptr(ticket), s) == E_BADARG      # not 16-byte aligned
    assert raw("conan_grad_clip_flat", ptr(g), 8, 0.0, ptr(nc), part.data_ptr(), ptr(ticket), s) == E_BADARG
    torch.cuda.synchronize()
    assert is_sent(g) and is_sent(nc) and is_sent(part) and int(ticket) == 0


# ================================================================================================ the flat Adam step
ADAM_CASES = [(n, wd, lrd) for n in G.ADAM_N[:5] for wd in (0.0, 1e-2) for lrd in (False, True)] + \
             [(G.ADAM_N[5], 0.0, False), (G.ADAM_N[5], 1e-2, True), (G.ADAM_N[6], 0.0, True), (G.ADAM_N[6], 1e-2, False)]


@pytest.mark.parametrize("n,wd,lr_dev", ADAM_CASES)
def test_adam_flat_step(n, wd, lr_dev):
    """Three launches on one device step counter, gradients over six decades; p, m and v judged after every step; with lr_dev the learning rate is
    read from the device (halved between steps 2 and 3; the by-value one is then a decoy).  The two largest n are beyond the 1024-workgroup grid;
    n % 4 in {1, 3, 0}: the scalar tail."""
    hp, s = G.ADAM_HP, stream_ptr()
    p0, grads = G.adam_inputs(n)
    lrs = [hp["lr"], hp["lr"], 0.5 * hp["lr"] if lr_dev else hp["lr"]]

    def run():
        o = {k: sent(n + 4) for k in ("p", "m", "v")}
        o["p"][:n] = p0.to(dev); o["m"][:n] = 0.0; o["v"][:n] = 0.0
        step, ticket = torch.zeros(1, device=dev), torch.zeros(1, dtype=i32, device=dev)
        lrd = torch.tensor([lrs[0]], dtype=f64, device=dev) if lr_dev else None
        snaps = []
        for t in range(3):
            gd = sent(n + 4); gd[:n] = grads[t].to(dev)
            if lr_dev:
                lrd.fill_(lrs[t])
            assert raw("conan_adam_flat_step", ptr(o["p"]), ptr(gd), ptr(o["m"]), ptr(o["v"]), ptr(step), ptr(ticket), n, 7.0 if lr_dev else lrs[t], hp["b1"],
                       hp["b2"], hp["eps"], wd, ptr(lrd), s) == OK
            torch.cuda.synchronize()
            assert is_sent(gd[n:])
            snaps.append({k: cut(o[k], n, k).clone() for k in ("p", "m", "v")})
        assert float(step) == 3.0 and int(ticket) == 0
        o["snaps"] = torch.stack([torch.cat([sn["p"], sn["m"], sn["v"]]) for sn in snaps])
        return o
    o = twice(run)
    snaps = o["snaps"].view(3, 3, n)
    fails = []
    st = {"32": (p0.clone(), torch.zeros(n), torch.zeros(n)), "64": (p0.double(), torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64))}
    for t in range(3):
        for tag, dt in (("32", f32), ("64", f64)):
            st[tag] = G.adam_step(*st[tag][:1], grads[t].to(dt), *st[tag][1:], t + 1, lrs[t], hp["b1"], hp["b2"], hp["eps"], wd)
        for q, k in enumerate(("p", "m", "v")):
            judge(fails, f"n{n}/wd{wd}/lrdev{int(lr_dev)}/step{t + 1}", f"adam.{k}" + ("/n<=5" if n <= 5 else ""), snaps[t, q], st["32"][q], st["64"][q])
    assert not fails, fails


def test_adam_flat_step_status_codes():
    p, g, m, v = sent(16), sent(16), sent(16), sent(16)
    step, ticket, s = torch.zeros(1, device=dev), torch.zeros(1, dtype=i32, device=dev), stream_ptr()
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    for k in range(4):                                                   # each of the four buffers 4 bytes off its 16-byte alignment
        ptrs = [t.data_ptr() + (4 if q == k else 0) for q, t in enumerate((p, g, m, v))]
        assert raw("conan_adam_flat_step", *ptrs, ptr(step), ptr(ticket), 8, *hp, None, s) == E_BADARG
    assert raw("conan_adam_flat_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(step), ptr(ticket), 0, *hp, None, s) == OK       # nothing to do, nothing touched
    torch.cuda.synchronize()
    assert all(is_sent(t) for t in (p, g, m, v)) and float(step) == 0.0 and int(ticket) == 0


# ================================================================================================ closing: nothing was left out
def test_zz_every_glue_export_was_called():
    """The 21 entry points this module owns are declared in _lib.SIGNATURES and each was called by a test above.  Whoever adds a glue export adds
    it to OWNED and a case here.  (Run the whole module: this test looks at what the tests above did.)"""
    whole = "this test looks at what the other tests of the module did: run the whole module, in file order, in one process"
    assert len(OWNED) == 21 and len(set(OWNED)) == 21
    assert set(OWNED) <= set(_lib.SIGNATURES), sorted(set(OWNED) - set(_lib.SIGNATURES))
    assert set(OWNED) <= CALLED, (whole, sorted(set(OWNED) - CALLED))
    assert CALLED <= set(OWNED), sorted(CALLED - set(OWNED))
    print("\nworst err / yard per output (row, whole tensor):")
    for what, (rr, ra) in sorted(RATIOS.items()):
        print(f"TABLE {what:28s} row={rr:6.3g} all={ra:6.3g}")
