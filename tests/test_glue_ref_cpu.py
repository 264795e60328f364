"""The references of tests/glue_ref.py held to what defines them (fp64), and the conditions on the inputs of tests/test_gpu_glue_ops.py (no GPU).

Every judged input must have an fp32 reference error within visnet_ref.COND_CAP (an input whose own reference is worse cannot tell a good kernel from
a bad one); the cases meant to be degenerate are listed by name in glue_ref (DEGENERATE_DENSIFY, DEGENERATE_READOUT) and are the only ones exempt,
apart from the N = 1 gradient of the normalised readout, which is exactly zero.  Ties must really occur in the tied cases."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as G
import visnet_ref as R
from oracle import pyg_semantics as ps
from oracle.schnet import normalize_tensor

f32, f64 = torch.float32, torch.float64
TIGHT = 1e-12


def close(a, b, tol=TIGHT):
    a, b = a.detach().double(), b.detach().double()
    return a.shape == b.shape and float((a - b).norm()) <= tol * max(float(b.norm()), 1e-300)


def cond(fn, *floats):
    """Whole-tensor error of the reference formula in fp32 against itself in fp64."""
    a, b = fn(*floats), fn(*[t.double() for t in floats])
    if isinstance(a, tuple):
        return max(R.all_err(x, y) for x, y in zip(a, b))
    return R.all_err(a, b)


# ================================================================================================ the references
@pytest.mark.parametrize("pad", [0, 9, None])
def test_embedding_and_its_gradient_are_torch(pad):
    gen = G.gen(1)
    w = torch.randn(10, 12, generator=gen, dtype=f64)
    z = torch.randint(0, 10, (300,), generator=gen)
    dout = torch.randn(300, 12, generator=gen, dtype=f64)
    wr = w.clone().requires_grad_(True)
    out = F.embedding(z, wr, padding_idx=pad)
    assert torch.equal(G.embedding(w, z), out.detach())
    (dw,) = torch.autograd.grad(out, wr, dout)
    assert close(G.embedding_grad(z, dout, 10, -1 if pad is None else pad), dw)
    # ids outside the table: NaN rows, nothing added, an all-zero one-hot row
    zb = z.clone(); zb[3], zb[7], zb[11] = -1, 10, 2 ** 40
    ok = torch.ones(300, dtype=torch.bool); ok[[3, 7, 11]] = False
    ob = G.embedding(w, zb)
    assert bool(torch.isnan(ob[~ok]).all()) and torch.equal(ob[ok], w[zb[ok]])
    assert close(G.embedding_grad(zb, dout, 10, -1), G.embedding_grad(zb[ok], dout[ok], 10, -1))
    oh = G.onehot_rows(zb, 10, -1 if pad is None else pad)
    assert float(oh[~ok].abs().max()) == 0.0
    assert close(oh.double().T @ dout, G.embedding_grad(zb, dout, 10, -1 if pad is None else pad))      # the gradient as onehot^T dout


def test_segment_sum_and_graph_ptr():
    gptr = G.seg_gptr()
    batch = G.batch_of(gptr)
    x = torch.randn(int(gptr[-1]), 5, dtype=f64)
    assert close(G.segment_sum(x, gptr), ps.scatter(x, batch, 0, len(gptr) - 1))
    assert np.array_equal(G.graph_ptr(batch.numpy(), len(gptr) - 1), gptr)
    dout = torch.randn(len(gptr) - 1, 5, dtype=f64)
    xr = x.clone().requires_grad_(True)
    (dx,) = torch.autograd.grad(G.segment_sum(xr, gptr), xr, dout)
    assert torch.equal(dx, G.segment_sum_grad(dout, gptr))


def test_unary_and_its_gradient_from_the_output():
    x = torch.cat([G.unary_x(3000).double(), torch.tensor([0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0], dtype=f64)])
    dy = torch.randn(x.numel(), dtype=f64, generator=G.gen(2))
    for op, fn in ((0, torch.relu), (1, torch.sigmoid), (2, lambda t: F.softplus(t) - math.log(2.0))):
        xr = x.clone().requires_grad_(True)
        y = G.unary(op, xr)
        assert torch.equal(y.detach(), fn(x))
        (gx,) = torch.autograd.grad(y, xr, dy)
        # the from-output formulas against autograd: exact for relu; for sigmoid and ssp up to the conditioning of y -> y' (1 - y and
        # 1 - 0.5 exp(-y) cancel for large |x|: absolute error of a few fp64 roundings of y, the derivative is at most 1).  torch's softplus
        # is the identity above its threshold x = 20, and its gradient exactly 1 there: that is e^-20 away from 1 - e^-x
        got = G.unary_grad_from_output(op, y.detach(), dy)
        assert float((got - gx).abs().max()) <= (1.01 * math.exp(-20.0) if op == 2 else 1e-14) * float(dy.abs().max()), op
    # torch on the non-finite values (what the GPU test holds the kernels to): a NaN stays a NaN through relu, and its gradient passes
    sp = torch.tensor(G.SPECIAL, dtype=f32, requires_grad=True)
    y = torch.relu(sp)
    (gx,) = torch.autograd.grad(y, sp, torch.full_like(sp, 1.5))
    y = y.detach()
    assert math.isnan(float(y[-1])) and float(gx[-1]) == 1.5 and float(y[12]) == G.INF and float(gx[12]) == 1.5


def test_rbf_and_cutoff():
    d = G.edge_dist(200).double()
    gs = ps.GaussianSmearing(0.0, G.CUTOFF, 50)
    off, coeff = G.rbf_offset(50)
    assert coeff == gs.coeff and torch.equal(off, gs.offset)
    assert close(G.rbf(d, off.double(), coeff), gs(d))
    x = torch.randn(200, 8, dtype=f64)
    assert close(G.cutoff_scale(d, G.CUTOFF, x), x * (0.5 * (torch.cos(d * math.pi / G.CUTOFF) + 1.0)).view(-1, 1))
    assert [float(v) for v in G.edge_dist(200)[:5]] == [0.0, float(np.float32(1e-6)), 5.0, float(np.nextafter(np.float32(10), np.float32(0))), 10.0]


@pytest.mark.parametrize("name", ["d64", "d16/shift1", "ties/N8/d3", "ties/N8/d16/shift.5", "n257+n300/N300/d4"])
def test_densify_is_the_oracle_with_its_autograd(name):
    c = G.densify_cases()[name]
    batch = G.batch_of(c.gptr)
    f1, f2 = c.feat.double().requires_grad_(True), c.feat.double().requires_grad_(True)
    dense, _ = ps.to_dense_batch(f1, batch, max_num_nodes=c.N)
    want = torch.stack([normalize_tensor(s + c.shift, c.a, c.b) for s in dense])
    got = G.densify(f2, c.gptr, c.N, c.shift, c.a, c.b)
    assert close(got, want)
    (g1,) = torch.autograd.grad(want, f1, c.dYs.double())
    (g2,) = torch.autograd.grad(got, f2, c.dYs.double())
    assert close(g2, g1)


@pytest.mark.parametrize("name", ["d64", "ties/N8/d3", "directed/N9/d3"])
def test_dense_adj_is_to_dense_adj_on_a_directed_multigraph(name):
    c = G.densify_cases()[name]
    batch = G.batch_of(c.gptr)
    tgt = np.repeat(np.arange(c.n_atoms), np.diff(c.rowptr))
    src = c.col[:c.E].astype(np.int64)
    inside = batch.numpy()[np.clip(src, 0, c.n_atoms - 1)] == batch.numpy()[tgt]
    assert int((~inside).sum()) >= 1                                          # the sources outside their graph: dropped by dense_adj
    ei = torch.from_numpy(np.stack([src[inside], tgt[inside]]))
    batch_full = torch.cat([batch, torch.tensor([c.G - 1])]) if c.sizes[-1] == 0 else batch
    want = ps.to_dense_adj(ei, batch_full, max_num_nodes=c.N)
    got = G.dense_adj(c.rowptr, c.col, c.gptr, c.N)
    assert torch.equal(got, want[:c.G])
    assert not torch.equal(got, got.transpose(1, 2)) and bool((got == 2).any()) and float(got.max()) >= 3.0


def test_readout_is_the_reference_formula():
    Y = torch.randn(3, 7, 5, dtype=f64)
    assert close(G.readout(Y, 4, 0), Y.sum(1).repeat_interleave(4, dim=0))
    assert close(G.readout(Y, 4, 1), (Y / Y.norm(dim=1, keepdim=True)).sum(1).repeat_interleave(4, dim=0))
    Yn = Y.clone(); Yn[1, 2, 3] = G.NAN
    Yr = Yn.clone().requires_grad_(True)
    out = G.readout(Yr, 2, 1)
    assert bool(torch.isnan(out[2:4]).all()) and bool(torch.isfinite(out[:2]).all()) and bool(torch.isfinite(out[4:]).all())
    (dY,) = torch.autograd.grad(out, Yr, torch.ones_like(out))
    assert float(dY[1].abs().max()) == 0.0 and bool(torch.isfinite(dY).all())    # the guarded molecule is a constant: no gradient reaches it


def test_mse_clip_and_adam_are_torch():
    gen = G.gen(3)
    pred, target = torch.randn(257, dtype=f64, generator=gen), torch.randn(257, dtype=f64, generator=gen)
    pr = pred.clone().requires_grad_(True)
    loss = F.mse_loss(pr, target)
    (dp,) = torch.autograd.grad(loss, pr)
    l, d = G.mse(pred, target)
    assert close(l, loss.detach()) and close(d, dp)
    # clip_grad_norm_: above and below the threshold, one NaN, one inf
    for kind in ("above", "below", "nan", "inf"):
        g = torch.randn(1000, dtype=f64, generator=gen)
        if kind == "nan":
            g[5] = G.NAN
        if kind == "inf":
            g[5] = G.INF
        mx = 1e3 if kind == "below" else 1.0
        prm = torch.nn.Parameter(torch.zeros(1000, dtype=f64)); prm.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([prm], mx)
        norm, coef, out = G.clip(g, mx)
        same = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and close(torch.nan_to_num(a), torch.nan_to_num(b))
        assert same(norm.reshape(1), total.reshape(1)) and same(out, prm.grad), kind
        assert (kind == "nan") == math.isnan(float(coef)) and (kind != "inf" or float(coef) == 0.0) and (kind != "below" or float(coef) == 1.0)
    # torch.optim.Adam, three steps, with and without weight decay
    hp = G.ADAM_HP
    for wd in (0.0, 1e-2):
        p0, grads = G.adam_inputs(1023)
        prm = torch.nn.Parameter(p0.double().clone())
        opt = torch.optim.Adam([prm], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd)
        st = (p0.double(), torch.zeros(1023, dtype=f64), torch.zeros(1023, dtype=f64))
        for t in range(3):
            prm.grad = grads[t].double()
            opt.step()
            st = G.adam_step(st[0], grads[t].double(), st[1], st[2], t + 1, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd)
            assert close(st[0], prm.detach()) and close(st[1], opt.state[prm]["exp_avg"]) and close(st[2], opt.state[prm]["exp_avg_sq"])
        assert float(torch.log10(grads[0].abs().max() / grads[0].abs().median())) > 2.5      # the gradients do span decades


# ================================================================================================ the conditions on the GPU test's inputs
def test_inputs_of_the_elementwise_and_reduction_cases_are_well_conditioned():
    cap, worst = R.COND_CAP, {}

    def note(what, v):
        worst[what] = max(worst.get(what, 0.0), v)
        assert v <= cap, (what, v)
    for count in G.UNARY_COUNTS:
        for op in (0, 1, 2):
            note(f"unary{op}", cond(lambda t: G.unary(op, t), G.unary_x(count)))
            y, dy = G.unary_y_dy(op, count)
            note(f"unary{op}'", cond(lambda a, b: G.unary_grad_from_output(op, a, b), y, dy))
            if op == 2 and count >= 3:
                assert float(y.min()) < -G.LN2 + 2e-7 and float(y.min()) >= np.float32(-G.LN2)      # sampled down to -ln 2 + 1e-7 (fp32 spacing there: 6e-8)
    y, dy = G.unary_y_dy(2, 2100, seed=5)
    note("ssp_bwd", cond(lambda a, b: G.unary_grad_from_output(2, a, b), y, dy))
    for case in G.embedding_cases():
        _, rows, H, n, pad, kind = case
        z, w, dout = G.embedding_inputs(case)
        note("embedding.dweight", cond(lambda t: G.embedding_grad(z, t, rows, pad), dout))
        if kind == "one":
            assert int((z == z[0]).sum()) == 1000
        if kind == "bad":
            assert int(((z < 0) | (z >= rows)).sum()) == 3
    gptr = G.seg_gptr()
    for W in G.SEG_W:
        note("segment_sum", cond(lambda t: G.segment_sum(t, gptr), torch.randn(int(gptr[-1]), W, generator=G.gen(W))))
    for Gs in G.RBF_GS:
        off, coeff = G.rbf_offset(Gs)
        for m in (1, 1000):
            note("rbf", cond(lambda a, b: G.rbf(a, b, coeff), G.edge_dist(m), off))
    for F_ in G.CUT_F:
        for m in (1, 1000):
            note("cutoff", cond(lambda a, b: G.cutoff_scale(a, G.CUTOFF, b), G.edge_dist(m, seed=1), torch.randn(m, F_, generator=G.gen(F_ + m))))
    for n in G.MSE_N:
        gen = G.gen(n)
        note("mse", cond(G.mse, torch.randn(n, generator=gen), torch.randn(n, generator=gen)))
    for n in G.CLIP_N[1:]:
        g = G.clip_grad(n)
        note("clip", cond(lambda t: G.clip(t, 0.5 * float(g.double().norm()))[2], g))
    print({k: float("%.2g" % v) for k, v in worst.items()})


@pytest.mark.parametrize("n", G.ADAM_N[:5] + G.ADAM_N[5:6])
def test_adam_inputs_are_well_conditioned(n):
    hp = G.ADAM_HP
    p0, grads = G.adam_inputs(n)
    s32, s64 = (p0, torch.zeros(n), torch.zeros(n)), (p0.double(), torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64))
    for t in range(3):
        s32 = G.adam_step(s32[0], grads[t], s32[1], s32[2], t + 1, hp["lr"], hp["b1"], hp["b2"], hp["eps"], 1e-2)
        s64 = G.adam_step(s64[0], grads[t].double(), s64[1], s64[2], t + 1, hp["lr"], hp["b1"], hp["b2"], hp["eps"], 1e-2)
        assert all(R.all_err(a, b) <= R.COND_CAP for a, b in zip(s32, s64)), (n, t)


def _densify_refs(c):
    r = {}
    for tag, dt in (("32", f32), ("64", f64)):
        feat = c.feat.to(dt).clone().requires_grad_(True)
        Ys = G.densify(feat, c.gptr, c.N, c.shift, c.a, c.b)
        (r["dfeat" + tag],) = torch.autograd.grad(Ys, feat, c.dYs.to(dt))
        r["Ys" + tag] = Ys.detach()
    return r


@pytest.mark.parametrize("name", list(G.densify_cases()))
def test_densify_inputs(name):
    """The slabs of range 0 are exactly the named ones; every other slab and its gradient are well conditioned; in the tied cases min and max are
    each attained at least twice in every slab, and in a slab with non-negative features and n < N the padding is among the minima."""
    c = G.densify_cases()[name]
    r = _densify_refs(c)
    bad = [int(g) for g in torch.isnan(r["Ys64"]).any(dim=2).any(dim=1).nonzero().flatten()]
    assert bad == G.DEGENERATE_DENSIFY.get(name, []) and set(G.DEGENERATE_DENSIFY) <= set(G.densify_cases())
    assert torch.equal(torch.isnan(r["Ys32"]), torch.isnan(r["Ys64"])) and torch.equal(torch.isnan(r["dfeat32"]), torch.isnan(r["dfeat64"]))
    keep = [g for g in range(c.G) if g not in bad]
    rows = torch.cat([torch.arange(int(c.gptr[g]), int(c.gptr[g + 1])) for g in keep])
    assert R.all_err(r["Ys32"][keep], r["Ys64"][keep]) <= R.COND_CAP
    assert R.all_err(r["dfeat32"][rows], r["dfeat64"][rows]) <= R.COND_CAP
    if c.kind == "quant":
        padded_min = 0
        for g in range(c.G):
            lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
            t = torch.cat([c.feat[lo:hi], torch.zeros(c.N - (hi - lo), c.d)]) + torch.tensor(c.shift, dtype=f32)
            assert int((t == t.min()).sum()) >= 2 and int((t == t.max()).sum()) >= 2, (name, g)
            if hi - lo < c.N and float(t.min()) == float(torch.tensor(c.shift, dtype=f32)):
                padded_min += 1
        assert padded_min >= 1, "no slab whose padding zeros are among the minima"
    if name == "n257+n300/N300/d4":
        assert sorted(c.sizes)[-2:] == [257, 300] and c.E > 600


@pytest.mark.parametrize("mode", [0, 1])
def test_readout_inputs(mode):
    names = set()
    for case in G.readout_cases():
        name, B, K, N, d, kind = case
        names.add(name)
        Y, dout = G.readout_inputs(case)
        r = {}
        for tag, dt in (("32", f32), ("64", f64)):
            Yr = Y.to(dt).clone().requires_grad_(True)
            ro = G.readout(Yr, K, mode)
            (r["dY" + tag],) = torch.autograd.grad(ro, Yr, dout.to(dt))
            r["out" + tag] = ro.detach()
        assert torch.equal(torch.isfinite(r["out32"]), torch.isfinite(r["out64"])) and torch.equal(torch.isfinite(r["dY32"]), torch.isfinite(r["dY64"]))
        degenerate = name in G.DEGENERATE_READOUT
        assert degenerate == (not bool(torch.isfinite(r["out64"]).all())) or mode == 0 and name == "zero-column"
        if degenerate:
            continue
        assert R.all_err(r["out32"], r["out64"]) <= R.COND_CAP, name
        if not (mode == 1 and N == 1):                                           # y / |y|: the exact gradient is 0
            assert R.all_err(r["dY32"], r["dY64"]) <= R.COND_CAP, name
    assert G.DEGENERATE_READOUT <= names
