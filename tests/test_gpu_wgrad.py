"""The two-stage weight gradient and its deferral, producer by producer: what a producer returns immediately against what the same call
returns inside a deferral, read after the deferral closed.  With the library's slice count the two are the same slabs summed in the same
order, so every comparison is torch.equal.  The producers are called directly, not through autograd: a bare deferral is sound only without
autograd's adoption question (FlatGradients.backward answers it; tests/test_gpu_stage2.py covers that way in)."""
import pytest
import torch

from helpers import rel
from conan_fgw_amd import wgrad as W
from conan_fgw_amd._lib import lib

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
plain, shared_x, filter_bwd, filter_bwd2, deferred = W.plain, W.shared_x, W.filter_bwd, W.filter_bwd2, W.deferred


@pytest.fixture(autouse=True)
def _library_slices():
    """Auto slice switch off unless a case turns it on: the deferred batch then cuts its jobs exactly as the immediate launches do."""
    keep, W.LATE_SLICES_AUTO = W.LATE_SLICES_AUTO, False
    yield
    W.LATE_SLICES_AUTO = keep


def _flat(out):
    """The tensors of a producer's result, in order: (dw, db), a list of such pairs, or a pair of pairs; db may be None."""
    if out is None or isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in _flat(o)]


def _same(a, b):
    a, b = _flat(a), _flat(b)
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert u.shape == v.shape and torch.isfinite(u).all() and torch.equal(u, v)


def _both(fn, jobs):
    """fn() immediately and inside a deferral, where it must leave `jobs` pending jobs (no silent immediate path) and its outputs unwritten until the
    flush: they are poisoned inside the deferral, so nothing but the flush can have made them equal.  The second result is read after the deferral closed."""
    now = fn()
    with deferred():
        later = fn()
        assert W.pending() == jobs
        for t in _flat(later):
            if t is not None:
                t.fill_(float("nan"))
    assert W.pending() is None
    torch.cuda.synchronize()
    _same(now, later)
    return now


def _operands(M, K, N, seed=0):
    gen = torch.Generator().manual_seed(1000 * M + 10 * K + N + seed)
    return torch.randn(M, N, generator=gen).to(dev), torch.randn(M, K, generator=gen).to(dev), torch.empty(N, K, device=dev)


def _filter_operands(M=300, Gs=50, F=128):
    gen = torch.Generator().manual_seed(M + Gs)
    g = torch.randn(M, F, generator=gen).to(dev)
    h1 = (torch.rand(M, F, generator=gen) * 3 - 0.6).to(dev)              # ssp output range (> -ln 2)
    dist = (torch.rand(M, generator=gen) * 10).to(dev)
    w1, w2 = torch.empty(F, Gs, device=dev), (torch.randn(F, F, generator=gen) / 11).to(dev)
    off = torch.linspace(0, 10, Gs).to(dev)
    coeff = -0.5 / float(off[1] - off[0]) ** 2
    md = torch.tensor([M], dtype=torch.int32, device=dev)
    return g, h1, dist, off, coeff, w1, w2, M, md, g.abs().max().reshape(1).contiguous()


@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("M,K,N,rows", [(1, 64, 64, None), (129, 128, 128, None), (129, 128, 128, 100), (300, 50, 128, None), (257, 128, 256, None)])
def test_node_level_layers_postpone_both_stages(M, K, N, rows, has_bias):
    """Up to the late-stage-1 bound both the slab kernel and the sum wait for the flush (one batched launch each): 64-wide and 128-wide k tile,
    ragged K, two n tiles, one row, a device-side row count below M."""
    assert lib().conan_wgrad_batchable(K, N) and M <= W._LATE_STAGE1_ROWS
    g, x, w = _operands(M, K, N)
    md = None if rows is None else torch.tensor([rows], dtype=torch.int32, device=dev)
    dw, db = _both(lambda: plain(g, x, M, K, N, md, w, has_bias), 1)
    assert dw.shape == (N, K) and (db is not None) == has_bias
    if rows is not None:                                                  # (the count is honoured at all: not the gradient of all M rows)
        assert not torch.equal(dw, plain(g, x, M, K, N, None, w, has_bias)[0])


@pytest.mark.parametrize("M,K,N", [(300, 64, 1), (130, 10, 6)])
def test_shapes_the_batch_does_not_take_stay_immediate(M, K, N):
    assert not lib().conan_wgrad_batchable(K, N)
    g, x, w = _operands(M, K, N)
    now = plain(g, x, M, K, N, None, w, True)
    with deferred():
        later = plain(g, x, M, K, N, None, w, True)
        assert W.pending() == 0
        torch.cuda.synchronize()
        _same(now, later)                                                 # final before the deferral closes


def test_edge_level_layer_runs_stage_one_at_once_and_defers_the_sum():
    """65537 rows: the first count above the late-stage-1 bound, and the first to hit the 512-slice cap."""
    M, K, N = 65537, 128, 128
    assert M == W._LATE_STAGE1_ROWS + 1
    g, x, w = _operands(M, K, N)
    _both(lambda: plain(g, x, M, K, N, None, w, True), 1)


def test_scaled_form():
    """max |g| given and K > 64: the fp16-plane kernel, which has no batched launch — stage 1 at once, the sum deferred."""
    M, K, N = 300, 128, 128
    g, x, w = _operands(M, K, N)
    gmax = g.abs().max().reshape(1).contiguous()
    scaled = _both(lambda: plain(g, x, M, K, N, None, w, True, gmax=gmax), 1)
    assert rel(scaled[0].cpu(), plain(g, x, M, K, N, None, w, True)[0].cpu()) < 1e-5      # (the same gradient, on other planes)


def test_rbf_form():
    """g^T rbf(dist) with the Gaussians regenerated inside the GEMM: 300 rows, SchNet's 50 offsets, distances in [0, cutoff)."""
    M, Gs, N, cutoff = 300, 50, 128, 10.0
    gen = torch.Generator().manual_seed(77)
    g = torch.randn(M, N, generator=gen).to(dev)
    dist = (torch.rand(M, generator=gen) * cutoff).to(dev)
    off = torch.linspace(0, cutoff, Gs).to(dev)
    coeff = -0.5 / float(off[1] - off[0]) ** 2
    w = torch.empty(N, Gs, device=dev)
    dw, db = _both(lambda: plain(g, None, M, Gs, N, None, w, True, rbf=(dist, off, coeff)), 1)
    ref = g.double().T @ torch.exp(coeff * (dist[:, None].double() - off[None].double()) ** 2)
    assert rel(dw.double().cpu(), ref.cpu()) < 1e-5 and rel(db.double().cpu(), g.double().sum(0).cpu()) < 2e-6


@pytest.mark.parametrize("n", [2, 3])
def test_shared_x_equals_the_layers_one_by_one(n):
    """Several layers of one input at edge level: the shared slab launch, immediate or deferred, gives the bits of the separate launches; two
    layers on ONE weight tensor inside a deferral take the fallback (defer the first, flush and run the second at once) and still do."""
    M, K, N = 65537, 128, 128
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(M, K, generator=gen).to(dev)
    gs = [torch.randn(M, N, generator=gen).to(dev) for _ in range(n)]
    ws = [torch.empty(N, K, device=dev) for _ in range(n)]
    hb = [True, False, True][:n]
    one_by_one = [plain(g, x, M, K, N, None, w, b) for g, w, b in zip(gs, ws, hb)]
    shared = _both(lambda: shared_x(gs, x, M, K, N, None, ws, hb), n)
    _same(shared, one_by_one)
    with deferred():
        twice = shared_x(gs, x, M, K, N, None, [ws[0]] * n, hb)
        assert W.pending() == n % 2                                       # every second layer found the weight pending: flush + immediate
    torch.cuda.synchronize()
    _same(twice, one_by_one)


def test_filter_network_producers():
    """conan_filter_bwd (two gradients) and conan_filter_bwd2 (all four; its one workspace is cut into two jobs)."""
    a = _filter_operands()
    dw1, db1 = _both(lambda: filter_bwd(*a[:-1], gmax=a[-1]), 1)
    (ew1, eb1), (ew2, eb2) = _both(lambda: filter_bwd2(*a), 2)
    assert dw1.shape == ew1.shape == (128, 50) and ew2.shape == (128, 128) and db1.shape == eb1.shape == eb2.shape == (128,)
    assert rel(ew1.cpu(), dw1.cpu()) < 1e-5 and rel(eb1.cpu(), db1.cpu()) < 1e-5          # (the same arithmetic, summed in another order)


def test_the_same_weight_twice_inside_one_deferral():
    """The second producer call on a pending weight flushes and runs immediately: both results are final right after it."""
    M, K, N = 300, 128, 128
    g1, x1, w = _operands(M, K, N)
    g2, x2, _ = _operands(M, K, N, seed=1)
    r1, r2 = plain(g1, x1, M, K, N, None, w, True), plain(g2, x2, M, K, N, None, w, True)
    a = _filter_operands()
    f, f1 = filter_bwd2(*a), filter_bwd(*a[:-1], gmax=a[-1])
    r3 = plain(a[0], a[1], a[7], 128, 128, a[8], a[6], True)
    with deferred():
        d1 = plain(g1, x1, M, K, N, None, w, True)
        assert W.pending() == 1
        d2 = plain(g2, x2, M, K, N, None, w, True)
        assert W.pending() == 0
        torch.cuda.synchronize()
        _same(d1, r1); _same(d2, r2)
        e1 = filter_bwd2(*a)
        assert W.pending() == 2
        e2 = filter_bwd(*a[:-1], gmax=a[-1])                                  # w1 is pending: flush + immediate
        assert W.pending() == 0
        e3 = plain(a[0], a[1], a[7], 128, 128, a[8], a[6], True)              # w2 is no longer pending: deferred again
        assert W.pending() == 1
        torch.cuda.synchronize()
        _same(e1, f); _same(e2, f1)
    torch.cuda.synchronize()
    _same(d1, r1); _same(d2, r2); _same(e1, f)
    _same(e3, r3)


def test_auto_slices_sum_in_another_order_within_the_bar():
    """22 node-level jobs of 8321 rows: the slice rule cuts each into 64 slices against the library's 66 — other slabs, the same sums."""
    M, K, N, jobs = 8321, 64, 64, 22
    W.LATE_SLICES_AUTO = True
    assert W._late_slices(jobs, M) == 64 and (M + 127) // 128 == 66
    ops_ = [_operands(M, K, N, seed=q) for q in range(jobs)]
    now = [plain(g, x, M, K, N, None, w, True) for g, x, w in ops_]
    with deferred():
        later = [plain(g, x, M, K, N, None, w, True) for g, x, w in ops_]
        assert W.pending() == jobs
    torch.cuda.synchronize()
    for (dw, db), (ew, eb) in zip(now, later):
        assert rel(ew.cpu(), dw.cpu()) < 2e-6 and rel(eb.cpu(), db.cpu()) < 2e-6
    assert not all(torch.equal(dw, ew) for (dw, _), (ew, _) in zip(now, later))           # (the rule did apply: another order, other bits)
