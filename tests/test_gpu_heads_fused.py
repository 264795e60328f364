"""Both per-atom heads of the shared SchNet trunk in one launch each way (ops.mlp2_outact_dual: conan_mlp2_outact_dual_fwd / _bwd) against
the two single-head launches it replaces.  Nothing of the arithmetic changes, so every comparison is torch.equal: the two outputs, the
tensors handed to the weight-gradient queue (g, dmid, mid per head), dx against dx_a + dx_b, and — through the model — every parameter
gradient with the switch on and off, immediate and deferred.

The stage-2 head that forms the per-graph sums of h_3d and the readout of Y itself (ops.stage2_head_sums) against the three launches it replaces,
in the same way: output, the three input gradients and the six parameter gradients."""
import pytest
import torch

from conan_fgw_amd.synthetic import make_batch

pytestmark = pytest.mark.gpu

K, N1, N2 = 128, 64, 64             # the model's head: hidden -> hidden / 2 -> hidden / 2
FORMS = (0, 1)                      # forward: the head as a second grid dimension / both heads in every workgroup


def _heads(dev, seed, hidden=K):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=gen) * 0.2).to(dev)
    return [(mk(hidden // 2, hidden), mk(hidden // 2), mk(hidden // 2, hidden // 2), mk(hidden // 2)) for _ in range(2)]


def _single(x, head, dy):
    """One head through the single-head entry points: (mid, y, g, dmid, dx)."""
    from conan_fgw_amd._lib import call, ptr, stream_ptr
    w1, b1, w2, b2 = head
    M = x.shape[0]
    mid, y, g, dmid = (torch.empty(M, 64, device=x.device) for _ in range(4))
    dx = torch.empty(M, K, device=x.device)
    call("conan_mlp2_outact_fwd", ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), M, K, N1, N2, ptr(mid), ptr(y), stream_ptr())
    call("conan_mlp2_outact_bwd", ptr(dy), ptr(y), ptr(w2), ptr(w1), M, K, N1, N2, ptr(g), ptr(dmid), ptr(dx), stream_ptr())
    return mid, y, g, dmid, dx


def _dual(x, heads, dys, form, rows, m_dev=None, fill=None):
    """Both heads through the dual entry points on `rows` allocated rows: (mid_a, y_a, g_a, dmid_a, mid_b, y_b, g_b, dmid_b, dx)."""
    from conan_fgw_amd._lib import call, ptr, stream_ptr
    (w1a, b1a, w2a, b2a), (w1b, b1b, w2b, b2b) = heads
    new = lambda w: torch.empty(rows, w, device=x.device) if fill is None else torch.full((rows, w), fill, device=x.device)
    mid_a, y_a, g_a, dmid_a, mid_b, y_b, g_b, dmid_b = (new(64) for _ in range(8))
    dx = new(K)
    call("conan_mlp2_outact_dual_fwd", ptr(x), ptr(w1a), ptr(b1a), ptr(w2a), ptr(b2a), ptr(w1b), ptr(b1b), ptr(w2b), ptr(b2b), rows, K, N1, N2,
         ptr(m_dev), form, ptr(mid_a), ptr(y_a), ptr(mid_b), ptr(y_b), stream_ptr())
    call("conan_mlp2_outact_dual_bwd", ptr(dys[0]), ptr(y_a), ptr(w2a), ptr(w1a), ptr(dys[1]), ptr(y_b), ptr(w2b), ptr(w1b), rows, K, N1, N2,
         ptr(m_dev), ptr(g_a), ptr(dmid_a), ptr(g_b), ptr(dmid_b), ptr(dx), stream_ptr())
    return mid_a, y_a, g_a, dmid_a, mid_b, y_b, g_b, dmid_b, dx


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M", [1, 31, 33, 129, 300])
def test_dual_head_equals_two_single_head_launches(M, form):
    """A lone row; a partial 32-row wavefront tile; one row past a tile; one row past a 4-wavefront workgroup; several workgroups."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(100 + M)
    x = torch.randn(M, K, generator=gen).to(dev)
    dys = [torch.randn(M, N2, generator=gen).to(dev) for _ in range(2)]
    heads = _heads(dev, M)
    a, b = _single(x, heads[0], dys[0]), _single(x, heads[1], dys[1])
    d = _dual(x, heads, dys, form, M)
    torch.cuda.synchronize()
    for name, got, want in zip(("mid", "y", "g", "dmid"), d[0:4], a):
        assert torch.equal(got, want), ("head a", name)
    for name, got, want in zip(("mid", "y", "g", "dmid"), d[4:8], b):
        assert torch.equal(got, want), ("head b", name)
    assert torch.equal(d[8], a[4] + b[4])                              # dx: each addend finalised as on its own, then added


@pytest.mark.parametrize("form", FORMS)
def test_dual_head_respects_the_device_side_row_count(form):
    """70 of 200 allocated rows count (a partial tile in the third wavefront, a second workgroup with nothing to do): rows beyond are NaN in x
    and in both incoming gradients; they stay untouched in every output and nothing below the count turns NaN."""
    dev = torch.device("cuda:0")
    rows, m = 200, 70
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(rows, K, generator=gen).to(dev)
    dys = [torch.randn(rows, N2, generator=gen).to(dev) for _ in range(2)]
    for t in [x] + dys:
        t[m:] = float("nan")
    heads = _heads(dev, 8)
    m_dev = torch.tensor([m], dtype=torch.int32, device=dev)
    SENTINEL = -77.0
    d = _dual(x, heads, dys, form, rows, m_dev=m_dev, fill=SENTINEL)
    a, b = _single(x[:m].contiguous(), heads[0], dys[0][:m].contiguous()), _single(x[:m].contiguous(), heads[1], dys[1][:m].contiguous())
    torch.cuda.synchronize()
    want = list(a[:4]) + list(b[:4]) + [a[4] + b[4]]
    for i, (got, ref) in enumerate(zip(d, want)):
        assert torch.equal(got[:m], ref), i
        assert torch.isfinite(got[:m]).all(), i
        assert bool((got[m:] == SENTINEL).all()), i


def _model_and_batch(B, Kc, hidden=128, seed=3):
    from conan_fgw_amd.schnet import SchNetNoSum
    dev = torch.device("cuda:0")
    b = make_batch("esol", B, Kc, seed=seed)
    torch.manual_seed(11)
    model = SchNetNoSum(dev, hidden_channels=hidden, num_filters=128, num_interactions=2).to(dev)
    z, pos, batch = (torch.from_numpy(a).to(dev) for a in (b.z, b.pos, b.batch))
    return model, b, z, pos, batch


def _bary_grads(model, b, z, pos, batch, dual, deferred):
    from conan_fgw_amd import ops, wgrad
    from conan_fgw_amd.parallel import FlatGradients
    for p in model.parameters():
        p.grad = None
    ops.DUAL_HEAD = dual
    try:
        h, hb = model.forward_3d_bary(z, pos, batch, num_graphs=b.num_graphs)
        loss = (h * h).mean() + (hb * torch.linspace(-1, 1, hb.shape[1], device=hb.device)).mean()
        if deferred:
            FlatGradients(model.parameters()).backward(loss)
            assert wgrad.pending() is None
        else:
            loss.backward()
    finally:
        ops.DUAL_HEAD = True
    torch.cuda.synchronize()
    return h.detach().clone(), hb.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("deferred", [False, True])
def test_forward_3d_bary_gradients_do_not_depend_on_the_switch(deferred):
    """The deferred weight-gradient queue sees the same (g, x) operands in the same order: with the library's own slices every parameter
    gradient of a forward_3d_bary backward is bit-identical with the dual launch on and off."""
    from conan_fgw_amd import wgrad
    args = _model_and_batch(2, 2)
    wgrad.LATE_SLICES_AUTO = False
    try:
        on, off = _bary_grads(*args, dual=True, deferred=deferred), _bary_grads(*args, dual=False, deferred=deferred)
    finally:
        wgrad.LATE_SLICES_AUTO = True
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert set(on[2]) == set(off[2]) and any(k.startswith("lin1_bary") for k in on[2])
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k


def test_unsupported_width_takes_the_two_launch_path():
    """hidden 96 (heads 96 -> 48 -> 48): no dual kernel, ops.mlp2_outact_dual composes the single-head calls — same bits as with the switch off."""
    from conan_fgw_amd import ops
    assert not ops.mlp2_outact_dual_supported(300, 96, 48, 48)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(300, 96, generator=gen).to(dev).requires_grad_(True)
    heads = _heads(dev, 6, hidden=96)
    outs = []
    for dual in (True, False):
        ops.DUAL_HEAD = dual
        try:
            x.grad = None
            ya, yb = ops.mlp2_outact_dual(x, *heads)
            (ya.sum() + 2 * yb.sum()).backward()
        finally:
            ops.DUAL_HEAD = True
        outs.append((ya.detach(), yb.detach(), x.grad.clone()))
    torch.cuda.synchronize()
    for got, want in zip(*outs):
        assert torch.equal(got, want)


@pytest.mark.parametrize("B,Kc", [(1, 1), (7, 5), (3, 1)])
def test_head_with_its_own_sums_equals_the_three_launches(B, Kc):
    """Graphs of 1 .. 20 atoms in one batch (one of them a single atom; fewer and more than the 8 rows a sum keeps in flight), Y with more nodes than
    any graph has atoms, a number of molecules that does not fill the backward's workgroups."""
    from conan_fgw_amd import ops
    dev = torch.device("cuda:0")
    D, G = 64, B * Kc
    gen = torch.Generator().manual_seed(40 + G)
    sizes = torch.randint(2, 21, (G,), generator=gen)
    sizes[G // 2] = 1
    gptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
    N = int(sizes.max()) + 3
    mk = lambda *s: torch.randn(*s, generator=gen).to(dev).requires_grad_(True)
    h3, Y, xc = mk(int(sizes.sum()), D), mk(B, N, D), mk(G, D)
    torch.manual_seed(G)
    l3, lb, lr = torch.nn.Linear(D, D).to(dev), torch.nn.Linear(D, D).to(dev), torch.nn.Linear(D, 1).to(dev)
    gy = torch.randn(B, 1, generator=gen).to(dev)
    leaves = [h3, Y, xc, l3.weight, l3.bias, lb.weight, lb.bias, lr.weight, lr.bias]

    def run(fused):
        for t in leaves:
            t.grad = None
        if fused:
            out = ops.stage2_head_sums(Y, h3, gptr, xc, l3, lb, lr, 0.2, Kc)
        else:
            out = ops.stage2_head(ops.segment_sum(h3, gptr, G), xc, ops.fgw_readout(Y, Kc, 0), l3, lb, lr, 0.2, Kc)
        (out * gy).sum().backward()
        torch.cuda.synchronize()
        return [out.detach().clone()] + [t.grad.detach().clone() for t in leaves]

    assert ops.stage2_head_sums_supported(D, Kc, 0)
    for i, (got, want) in enumerate(zip(run(True), run(False))):
        assert torch.equal(got, want), i


def test_head_with_its_own_sums_refuses_what_it_does_not_cover():
    """The ViSNet readout (mode 1: NaN guard and column normalisation), more conformers than the kernel keeps sums for, a head wider than 64."""
    from conan_fgw_amd import ops
    assert not ops.stage2_head_sums_supported(64, 5, 1)
    assert not ops.stage2_head_sums_supported(64, 33, 0)
    assert not ops.stage2_head_sums_supported(256, 5, 0)


def test_whole_model_loss_and_gradients_do_not_depend_on_the_switch():
    """The stage-2 regression model on make_batch("esol", 3, 5): loss and every parameter gradient with both switches on and both off."""
    import types
    from conan_fgw_amd import ops
    from conan_fgw_amd.head import EmbeddingsWithGATAggregationBaryCenter
    from conan_fgw_amd.synthetic import make_bond_graph
    dev = torch.device("cuda:0")
    b = make_batch("esol", 3, 5, seed=17)
    g = make_bond_graph(b, seed=18)
    torch.manual_seed(5)
    m = EmbeddingsWithGATAggregationBaryCenter(5, dev).to(dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    data = types.SimpleNamespace(z=t(b.z), pos=t(b.pos), x=t(g.x), edge_index=t(g.edge_index), edge_attr=t(g.edge_attr), batch=t(b.batch))
    cidx = m.create_aggregation_index(b.num_graphs, dev)
    tgt = t(b.y)[:, None]
    res = []
    for on in (True, False):
        ops.DUAL_HEAD = ops.HEAD_SUMS_FUSED = on
        try:
            for p in m.parameters():
                p.grad = None
            loss = ops.mse_loss(m(data, cidx, data.batch), tgt)
            loss.backward()
        finally:
            ops.DUAL_HEAD = ops.HEAD_SUMS_FUSED = True
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
