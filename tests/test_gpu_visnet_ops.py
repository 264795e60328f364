"""Every ViSNet kernel on its own against the plain fp64 reference of the same operation (tests/visnet_ref.py).

Each export of the two ViSNet sections of include/conan_fgw_hip.h is called through the door the model uses (the visnet_ops autograd functions;
the C entry point directly where no wrapper exists or the wrapper cannot express the arguments) on graphs built by ops.RadiusGraph from crafted
positions: conformers of 1-3 atoms, edge counts that leave a partial 16-edge run, an isolated atom, a cluster beyond the 32-neighbour cap,
ragged batches, and one graph large enough for the grid-stride second pass of the node kernels (n > 16 384) and the edge kernels (E > 262 144).

Judging (visnet_ref.judge): per row and per tensor, err(gpu, ref64) <= MARGIN * err(ref32, ref64) — the yardstick is the reference formula itself
in fp32 on the CPU, never the kernel.  Pure data movement must be bitwise.  Inputs beyond the device-side edge count carry a NaN bit pattern and
outputs are pre-filled with it where the test owns the buffer: rows >= E must still hold it afterwards.  Every case (the large graph included) runs twice and must
give the same bits (fixed summation order, no atomics).  The `RATIO` lines printed by a run (-s) are the source of the table in DESIGN.md section 3.4."""
import os
import re

import numpy as np
import pytest
import torch

import visnet_ref as R
from conan_fgw_amd import _lib, ops, visnet_ops as vo
from conan_fgw_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
f32, i32 = torch.float32, torch.int32
OK, E_BADARG, E_UNSUPPORTED = 0, -1, -3
SENT = 0x7FA5A5A5                        # a NaN bit pattern: reading it poisons a result, overwriting it is visible
CALLED, TRACED, RATIOS, BRANCHES = set(), set(), {}, set()      # CALLED: every entry point touched; TRACED: those reached through the package's own call()
# kernels that need more than the shared margins: (row, whole tensor) = 2 x the measured ratio, reasons in DESIGN.md section 3.4
OP_MARGIN = {
    # (kernel, output) -> f(rows) -> (row, whole tensor).  The atomref gradient of `prior` is at most 19 numbers, each the sum of its atoms' rows through
    # k_rowsum (one thread adds a row's `width` entries one after another: error ~ sqrt(width) ulp, where torch's sum is pairwise) and
    # conan_embedding_bwd: measured 5.23 / 4.20 at n = 300, H = 256 (0.2 .. 5.2 over n = 53 / 300 / 16 440) -> 2 x that.  At n = 1 it is ONE number, and a
    # yardstick of one number is noise (the fp32 reference of a single scalar lands far below an ulp now and then: measured 66 at H = 64) -> 2 x that,
    # at n = 1 only.  At every n the textbook bound of fp32 summation is asserted beside the ratio (_prior_sum_bound).
    ("prior", "grad1"): lambda n: (133.0, 133.0) if n == 1 else (10.5, 8.4),
}


@pytest.fixture(scope="module", autouse=True)
def _record_entry_points():
    def trace(name, fn, args):
        CALLED.add(name)
        TRACED.add(name)
        return fn(*args)
    prev = _lib.set_call_trace(trace)
    yield
    _lib.set_call_trace(prev)


def raw(name, *args):
    """The C entry point itself: returns the status code instead of raising."""
    CALLED.add(name)
    return getattr(lib(), name)(*args)


def sent(*shape):
    return torch.full(shape, SENT, dtype=i32, device=dev).view(f32)


def is_sent(t):
    return bool((t.contiguous().view(i32) == SENT).all())


# ================================================================================================ graphs
class GG:
    pass


_GRAPHS = {}


def gpu_graph(name, cache=True):
    if cache and name in _GRAPHS:
        return _GRAPHS[name]
    pos, batch, E = R.graph_case(name)
    cpu = R.graph_on_cpu(pos, batch)
    counts = np.bincount(batch)
    gg = GG()
    gg.pos = torch.from_numpy(pos).to(dev)
    gp = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    g = gg.g = ops.RadiusGraph(gg.pos, gp, len(counts), R.CUTOFF, R.CAP, loop=True)
    En = g.num_edges
    assert torch.equal(g.edge_index().cpu(), torch.stack([cpu.src, cpu.tgt])), name          # the real graph equals the oracle's, once per graph
    assert E is None or En == E, name
    g.dist[En:] = float("nan")
    gg.dvec = sent(g.max_edges, 3)
    assert raw("conan_visnet_edge_unit", ptr(gg.pos), ptr(g.col), ptr(g.tgt), ptr(g.num_edges_dev), g.max_edges, ptr(gg.dvec), stream_ptr()) == OK
    assert is_sent(gg.dvec[En:]) and bool(torch.isfinite(gg.dvec[:En]).all())
    gg.ref = R.Graph(cpu.n, cpu.src, cpu.tgt, g.dist[:En].cpu(), gg.dvec[:En].cpu(), cpu.pos, cpu.batch)
    gg.tr, gg.te = g.transpose()
    if cache:
        _GRAPHS[name] = gg
    return gg


# ================================================================================================ the kernels through the model's doors
def _i_edge_unit(gg, G, H, fl, pos):
    g, out = gg.g, sent(gg.g.max_edges, 3)
    assert raw("conan_visnet_edge_unit", ptr(pos), ptr(g.col), ptr(g.tgt), ptr(g.num_edges_dev), g.max_edges, ptr(out), stream_ptr()) == OK
    assert is_sent(out[G.E:])
    return (out,)


def _i_expnormal(gg, G, H, fl, d, m, b):
    g, out = gg.g, sent(gg.g.max_edges, H)
    assert raw("conan_visnet_expnormal", ptr(d), ptr(g.num_edges_dev), g.max_edges, ptr(m), ptr(b), H, 5.0 / R.CUTOFF, R.CUTOFF, ptr(out), stream_ptr()) == OK
    assert is_sent(out[G.E:])
    return (out,)


def _i_node_update(gg, G, H, fl, x, vec, *rest):
    if fl["vdot"] == "free":
        vdot, o, vp, vagg = rest
        return vo.node_update(x, vec, vdot, o, vp, vagg, False)
    o, vp, vagg = rest
    if fl["vdot"] == "fold":                           # vec_dot outside autograd, its backward inside node_update's (dvdot == NULL)
        return vo.node_update(x, vec, vo.vecdot_detached(vp, G.n, H), o, vp, vagg, True)
    return vo.node_update(x, vec, vo.vecdot(vp, G.n, H), o, vp, vagg, False)       # conan_visnet_vecdot_bwd + dvdot written; autograd sums the two dvp


def _tup(r):
    return r if isinstance(r, tuple) else (r,)


IMPL = {
    "edge_unit": _i_edge_unit,
    "expnormal": _i_expnormal,
    "neighbor_scale": lambda gg, G, H, fl, W: (vo.neighbor_scale(W, gg.g, R.CUTOFF),),
    "edge_embed": lambda gg, G, H, fl, x, p: (vo.edge_embed(x, p, gg.g),),
    "attn_message": lambda gg, G, H, fl, q, k, v, dk, dv: vo.attn_message(q, k, v, dk, dv, gg.g, R.CUTOFF, fl["heads"], bool(fl["pre_act"])),
    "vec_aggregate": lambda gg, G, H, fl, vec, s: (vo.vec_aggregate(vec, s, gg.dvec, gg.g, bool(fl["pre_act"])),),
    "edge_update": lambda gg, G, H, fl, wt, ws, t, f: (vo.edge_update(wt.view(3 * G.n, H), ws.view(3 * G.n, H), t, gg.dvec, f, gg.g, bool(fl["pre_act"])),),
    "node_update": _i_node_update,
    "vecdot": lambda gg, G, H, fl, vp: (vo.vecdot(vp, G.n, H),),
    "layernorm": lambda gg, G, H, fl, x, gamma, beta: _tup(vo._LayerNorm.apply(x, gamma, beta, 1e-5, fl["tap"])),
    "scale_channels": lambda gg, G, H, fl, v, w: _tup(vo.scale_channels(v, w, fl["tap"])),
    "concat2": lambda gg, G, H, fl, a, b: (vo.concat2(a, b),),
    "spatial_norm": lambda gg, G, H, fl, v: (vo.spatial_norm(v, G.n, H),),
    "gate": lambda gg, G, H, fl, u, v2: vo.gate(u, v2, G.n, H, fl["act"]),
    "prior": lambda gg, G, H, fl, x, a, z, std: (vo.prior(x, z, a, std),),
    "silu": lambda gg, G, H, fl, x: (vo.silu(x, None),),
}


def pad(t, kind, gg):
    """To the device; edge-level tensors at their worst-case size with the NaN pattern beyond the edge count."""
    t = t.to(dev)
    if kind == "E":
        full = sent(gg.g.max_edges, *t.shape[1:])
        full[:t.shape[0]] = t
        t = full
    return t


def run_gpu(name, gg, G, H, fl, res):
    op = R.OPS[name]
    ins = [pad(t, k, gg) if t.is_floating_point() else t.to(dev) for t, k in zip(res["ins"], res["kinds"])]
    for t, d in zip(ins, res["diff"]):
        t.requires_grad_(d)
    outs = IMPL[name](gg, G, H, fl, *ins)
    gouts = [pad(g, k, gg) for g, k in zip(res["gouts"], op.out_kinds)]
    dx = [t for t, d in zip(ins, res["diff"]) if d]
    kdx = [k for k, d in zip(res["kinds"], res["diff"]) if d]
    live = [(o, g) for o, g in zip(outs, gouts) if o.requires_grad]
    grads = torch.autograd.grad([o for o, _ in live], dx, [g for _, g in live], allow_unused=True) if (dx and live) else [None] * len(dx)
    torch.cuda.synchronize()
    cut = lambda t, k: t[:G.E] if k == "E" else t
    return ([cut(o.detach(), k) for o, k in zip(outs, op.out_kinds)],
            [cut(torch.zeros_like(x) if g is None else g, k) for x, g, k in zip(dx, grads, kdx)], ins, gouts)


def check(name, case_id, res, outs, grads, fails, keep=None, n=None):
    """Judge every output and gradient.  keep(kind, rows) -> slice: judge only these rows (the `wide` case: the rows beyond the first grid pass)."""
    op = R.OPS[name]
    kdx = [k for k, d in zip(res["kinds"], res["diff"]) if d]
    items = [("out%d" % i, outs[i], res["out32"][i], res["out64"][i], op.out_kinds[i]) for i in range(len(outs))]
    items += [("grad%d" % i, grads[i], res["grad32"][i], res["grad64"][i], kdx[i]) for i in range(len(grads))]
    for what, got, r32, r64, kind in items:
        got = got.detach().cpu()
        assert got.shape == r64.shape, (name, case_id, what, got.shape, r64.shape)
        if keep is not None and kind != "C":
            sl = keep(kind, got.shape[0])
            got, r32, r64 = got[sl], r32[sl], r64[sl]
            assert got.shape[0] > 0, (name, case_id, what)
        if not bool(torch.isfinite(got).all()):
            fails.append((case_id, what, "not finite"))
            continue
        if R.all_err(r32, r64) > R.COND_CAP:
            fails.append((case_id, what, "fp32 reference beyond its cap: change the input", R.all_err(r32, r64)))
        mr, ma = OP_MARGIN[(name, what)](n) if (name, what) in OP_MARGIN else (R.MARGIN_ROW, R.MARGIN_ALL)
        if name in R.BITWISE:
            ok = torch.equal(got, r32)
            rr = ra = 0.0 if ok else float("inf")
        else:
            ok, rr, ra = R.judge(got, r32, r64, mr, ma)
        old = RATIOS.get((name, what[:-1]), (0.0, 0.0))
        RATIOS[(name, what[:-1])] = (max(old[0], rr), max(old[1], ra))
        print(f"RATIO {name} {case_id} {what} row={rr:.3g} all={ra:.3g}")
        if not ok:
            fails.append((case_id, what, rr, ra))


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _attn_buffers(gg, H):
    n, ME = gg.ref.n, gg.g.max_edges
    node = [torch.randn(n, H, device=dev) for _ in range(3)]
    edge = [torch.randn(ME, H, device=dev) for _ in range(2)]
    return n, ME, node, edge


def _attn_rejected(gg, H, heads, want):
    """A combination the entry points turn down: the same code from forward and backward, nothing written."""
    g = gg.g
    n, ME, (q, k, v), (dk, dv) = _attn_buffers(gg, H)
    vmsg, xagg = sent(ME, H), sent(n, H)
    rc = raw("conan_visnet_attn_message", ptr(q), ptr(k), ptr(v), ptr(dk), ptr(dv), ptr(g.rowptr), ptr(g.col), ptr(g.dist), R.CUTOFF, n, H, heads, 1,
             ptr(vmsg), ptr(xagg), stream_ptr())
    outs = [sent(n, H) for _ in range(3)] + [sent(ME, H) for _ in range(2)]
    rcb = raw("conan_visnet_attn_message_bwd", ptr(q), ptr(k), ptr(v), ptr(dk), ptr(dv), ptr(dk), ptr(q), ptr(g.rowptr),
              ptr(g.col), ptr(g.tgt), ptr(gg.tr), ptr(gg.te), ptr(g.dist), R.CUTOFF, n, H, heads, 1, *[ptr(o) for o in outs], stream_ptr())
    torch.cuda.synchronize()
    assert rc == want and rcb == want, (H, heads, rc, rcb, want)
    assert is_sent(vmsg) and is_sent(xagg) and all(is_sent(o) for o in outs), (H, heads)


def _prior_sum_bound(res, dw, width):
    """Atomref gradient, entry by entry: |error| <= (terms + 1) * 2^-24 * sum |terms| — the textbook bound of adding `terms` fp32 numbers in any order
    (from the number format, not from what the kernel gives)."""
    z, g = res["ins"][2], res["gouts"][0].double()
    cnt = torch.zeros(100, dtype=torch.float64).index_add_(0, z, torch.full((z.shape[0],), float(width), dtype=torch.float64))
    sabs = torch.zeros(100, dtype=torch.float64).index_add_(0, z, g.abs().sum(dim=1))
    err = (dw.double().view(-1) - res["grad64"][1].view(-1)).abs()
    assert bool((err <= (cnt + 1) * 2.0 ** -24 * sabs).all()), float((err / ((cnt + 1) * 2.0 ** -24 * sabs + 1e-300)).max())


# ================================================================================================ the cases of visnet_ref.op_cases
@pytest.mark.parametrize("name", sorted(R.OPS))
def test_kernel_against_fp64_reference(name):
    op, fails, ran = R.OPS[name], [], 0
    for g, H, fl in R.op_cases(name):
        case_id = f"{g}/H{H}/" + ",".join(f"{k}={v}" for k, v in fl.items())
        gg = gpu_graph(g) if op.graph else None
        G = gg.ref if op.graph else R.Rows(g)
        if name == "attn_message":
            # which instantiation this (H, num_heads) takes, re-derived from the dispatch arithmetic of conan_visnet_attn_message (visnet_ref.attn_branch)
            branch = R.attn_branch(H, fl["heads"])
            if branch in ("badarg", "unsupported"):
                # H not a whole number of heads fails the argument check (CONAN_E_BADARG) before the dispatch is reached; what the dispatch itself
                # cannot place is CONAN_E_UNSUPPORTED
                _attn_rejected(gg, H, fl["heads"], E_BADARG if branch == "badarg" else E_UNSUPPORTED)
                BRANCHES.add(branch)
                continue
            BRANCHES.add(branch)
        res = R.reference(op, G, H, fl, R.case_seed(name, g, H, fl))
        outs, grads, _, _ = run_gpu(name, gg, G, H, fl, res)
        outs2, grads2, _, _ = run_gpu(name, gg, G, H, fl, res)
        assert same_bits(outs, outs2) and same_bits(grads, grads2), (name, case_id, "two runs differ")
        check(name, case_id, res, outs, grads, fails, n=G.n)
        if name == "prior":
            _prior_sum_bound(res, grads[1].cpu(), H)
        ran += 1
    assert ran >= 6
    assert not fails, fails


# ================================================================================================ the grid-stride second pass
def _wide_n0(G):
    """First node of the molecule that holds edge EDGE_PASS (or node NODE_PASS, whichever comes first): the reference runs on the nodes from there on."""
    node = min(R.NODE_PASS, int(G.tgt[R.EDGE_PASS]))
    return int((G.batch == G.batch[node]).nonzero()[0])


@pytest.mark.parametrize("name", sorted(n for n, o in R.OPS.items() if o.graph))
def test_graph_kernels_beyond_the_first_grid_pass(name):
    """`wide`: 16 440 nodes, 329 348 edges.  A grid is capped at 4 096 blocks = 16 384 wavefronts: the node kernels (one wavefront per node) loop from node
    16 384, the edge kernels (16 edges per wavefront) from edge 262 144.  The GPU runs on the whole graph; the reference on the sub-graph of the
    last ~170 molecules (no edge crosses a molecule), and only rows beyond the first pass are judged."""
    op, fails = R.OPS[name], []
    gg = gpu_graph("wide")
    G = gg.ref
    assert G.n > R.NODE_PASS and G.E > R.EDGE_PASS and gg.g.max_edges > G.E
    n0 = _wide_n0(G)
    Gt, e0 = G.tail(n0)
    assert n0 < R.NODE_PASS and e0 < R.EDGE_PASS
    for H in ((32,) if name == "expnormal" else (3,) if name == "edge_unit" else (32, 128)):
        for fl in R.flag_cases(name, H, False)[:1]:
            gen = torch.Generator().manual_seed(R.case_seed(name, "wide", H, fl))
            spec = op.make(gen, G, H, fl)
            widths = {"edge_unit": [(3,)], "expnormal": [(H,)], "attn_message": [(H,), (H,)], "vec_aggregate": [(3, H)]}.get(name, [(H,)])
            gouts = [R.rows(gen, G.E if k == "E" else G.n, *w) for k, w in zip(op.out_kinds, widths)]
            full = {"ins": [t for t, _, _ in spec], "diff": [d for _, d, _ in spec], "kinds": [k for _, _, k in spec], "gouts": gouts}
            outs, grads, _, _ = run_gpu(name, gg, G, H, fl, full)
            outs2, grads2, _, _ = run_gpu(name, gg, G, H, fl, full)
            assert same_bits(outs, outs2) and same_bits(grads, grads2), (name, H, "two runs differ")
            del outs2, grads2
            lo = lambda k: e0 if k == "E" else n0
            tspec = [(t if k == "C" else t[lo(k):], d, k) for t, d, k in spec]
            res = R.reference(op, Gt, H, fl, 0, spec=tspec, gouts=[g[lo(k):] for g, k in zip(gouts, op.out_kinds)])
            kdx = [k for k, d in zip(full["kinds"], full["diff"]) if d]
            outs_t = [o[lo(k):] for o, k in zip(outs, op.out_kinds)]
            grads_t = [g if k == "C" else g[lo(k):] for g, k in zip(grads, kdx)]
            keep = lambda kind, r: slice((R.EDGE_PASS - e0) if kind == "E" else (R.NODE_PASS - n0), r)
            check(name, f"wide/H{H}/second-pass", res, outs_t, grads_t, fails, keep=keep)
            check(name, f"wide/H{H}/tail", res, outs_t, grads_t, fails)
            del outs, grads, outs_t, grads_t, res, spec, tspec, gouts, full
            torch.cuda.empty_cache()
    assert not fails, fails


@pytest.mark.parametrize("name", sorted(n for n, o in R.OPS.items() if not o.graph))
def test_row_kernels_beyond_the_first_grid_pass(name):
    """The kernels that take a row count, at n = 16 440: one wavefront per row (layernorm) loops from row 16 384; one thread per element
    (the rest; 4 096 blocks x 256 threads) from element 1 048 576, i.e. from row 8 192 at H = 128.  Judged on the rows from 16 384 on."""
    op, fails, n = R.OPS[name], [], 16440
    for H in (32, 128):
        fl = R.flag_cases(name, H, False)[-1]
        assert n > R.NODE_PASS and (H < 128 or n * H > (1 << 20))
        res = R.reference(op, R.Rows(n), H, fl, R.case_seed(name, n, H, fl))
        outs, grads, _, _ = run_gpu(name, None, R.Rows(n), H, fl, res)
        outs2, grads2, _, _ = run_gpu(name, None, R.Rows(n), H, fl, res)
        assert same_bits(outs, outs2) and same_bits(grads, grads2), (name, H, "two runs differ")
        check(name, f"{n}/H{H}/second-pass", res, outs, grads, fails, keep=lambda kind, r: slice(R.NODE_PASS, r), n=n)
        check(name, f"{n}/H{H}/all", res, outs, grads, fails, n=n)
        if name == "prior":
            _prior_sum_bound(res, grads[1].cpu(), H)
    assert not fails, fails


# ================================================================================================ tail contract on the C entry points
def _tail_cases():
    return [(g, H) for g in ("tiny", "capped") for H in (32, 128, 96)]


@pytest.mark.parametrize("gname,H", _tail_cases())
def test_rows_beyond_the_edge_count_are_neither_read_nor_written(gname, H):
    """Every export that takes num_edges_dev / max_edges, and the CSR walkers that write edge-level outputs: inputs beyond E hold the NaN pattern,
    outputs are pre-filled with it; afterwards rows < E equal what the autograd wrapper produced from the same inputs (bit for bit; that result is
    judged against the reference above) and rows >= E still hold the pattern."""
    gg = gpu_graph(gname)
    g, G = gg.g, gg.ref
    n, E, ME, s = G.n, G.E, g.max_edges, stream_ptr()
    ne = g.num_edges_dev
    assert ME > E

    def both(name, fl):
        res = R.reference(R.OPS[name], G, H, fl, R.case_seed(name, gname, H, fl))
        return run_gpu(name, gg, G, H, fl, res)

    def edge_ok(buf, want):
        torch.cuda.synchronize()
        assert is_sent(buf[E:]) and bool(torch.isfinite(buf[:E]).all()) and torch.equal(buf[:E], want)

    # neighbor_scale: out of place, and in place (bitwise the same)
    (o,), (dW,), (W,), (gW,) = both("neighbor_scale", {})
    out = sent(ME, H)
    assert raw("conan_visnet_neighbor_scale_to", ptr(W), ptr(g.dist), ptr(g.col), ptr(g.tgt), ptr(ne), ME, H, R.CUTOFF, ptr(out), s) == OK
    edge_ok(out, o)
    Wi = W.detach().clone()
    assert raw("conan_visnet_neighbor_scale", ptr(Wi), ptr(g.dist), ptr(g.col), ptr(g.tgt), ptr(ne), ME, H, R.CUTOFF, s) == OK
    edge_ok(Wi, o)
    # edge_embed and its backward
    (o,), (dx, dp), (x, p), (gf,) = both("edge_embed", {})
    out = sent(ME, H)
    assert raw("conan_visnet_edge_embed", ptr(x), ptr(p), ptr(g.col), ptr(g.tgt), ptr(ne), ME, H, ptr(out), s) == OK
    edge_ok(out, o)
    odp, odx = sent(ME, H), sent(n, H)
    assert raw("conan_visnet_edge_embed_bwd", ptr(x), ptr(p), ptr(gf), ptr(g.rowptr), ptr(g.col), ptr(g.tgt), ptr(gg.tr), ptr(gg.te), ptr(ne), ME, n, H,
               ptr(odp), ptr(odx), s) == OK
    edge_ok(odp, dp)
    assert torch.equal(odx, dx)
    for pre in (1, 0):
        # edge_update and its backward
        (o,), (dwt, dws, dt, df), (wt, ws, t, f), (gfo,) = both("edge_update", {"pre_act": pre})
        out = sent(ME, H)
        assert raw("conan_visnet_edge_update", ptr(wt), ptr(ws), ptr(t), ptr(gg.dvec), ptr(g.col), ptr(g.tgt), ptr(ne), ME, H, pre, ptr(f), ptr(out), s) == OK
        edge_ok(out, o)
        odwt, odws, odt = sent(n, 3, H), sent(n, 3, H), sent(ME, H)
        assert raw("conan_visnet_edge_update_bwd", ptr(wt), ptr(ws), ptr(t), ptr(gg.dvec), ptr(gfo), ptr(g.rowptr), ptr(g.col), ptr(g.tgt), ptr(gg.tr), ptr(gg.te),
                   n, H, pre, ptr(odwt), ptr(odws), ptr(odt), s) == OK
        edge_ok(odt, dt)
        assert torch.equal(odwt, dwt) and torch.equal(odws, dws) and torch.equal(df, gfo[:E])
        # vec_aggregate backward
        (o,), (dvec_, ds), (vec, sx), (gv,) = both("vec_aggregate", {"pre_act": pre})
        ods, odv = sent(ME, 2 * H), sent(n, 3, H)
        assert raw("conan_visnet_vec_aggregate_bwd", ptr(vec), ptr(sx), ptr(gg.dvec), ptr(gv), ptr(g.col), ptr(g.tgt), ptr(gg.tr), ptr(gg.te), ptr(ne), ME, n, H, pre,
                   ptr(ods), ptr(odv), s) == OK
        edge_ok(ods, ds)
        assert torch.equal(odv, dvec_)
        # attention message and its backward (H = 96 is turned down: covered by the rejection cases)
        if R.attn_branch(H, 8) in ("badarg", "unsupported"):
            continue
        (vm, xa), (dq, dk_, dv_, ddk, ddv), (q, k, v, dk, dv), (gvm, gxa) = both("attn_message", {"heads": 8, "pre_act": pre})
        ovm, oxa = sent(ME, H), sent(n, H)
        assert raw("conan_visnet_attn_message", ptr(q), ptr(k), ptr(v), ptr(dk), ptr(dv), ptr(g.rowptr), ptr(g.col), ptr(g.dist), R.CUTOFF, n, H, 8, pre,
                   ptr(ovm), ptr(oxa), s) == OK
        edge_ok(ovm, vm)
        assert torch.equal(oxa, xa)
        nd, ed = [sent(n, H) for _ in range(3)], [sent(ME, H) for _ in range(2)]
        assert raw("conan_visnet_attn_message_bwd", ptr(q), ptr(k), ptr(v), ptr(dk), ptr(dv), ptr(gvm), ptr(gxa), ptr(g.rowptr), ptr(g.col), ptr(g.tgt), ptr(gg.tr),
                   ptr(gg.te), ptr(g.dist), R.CUTOFF, n, H, 8, pre, *[ptr(t_) for t_ in nd + ed], s) == OK
        edge_ok(ed[0], ddk); edge_ok(ed[1], ddv)
        assert torch.equal(nd[0], dq) and torch.equal(nd[1], dk_) and torch.equal(nd[2], dv_)


@pytest.mark.parametrize("width", [32, 128, R.ODD_WIDTH])
def test_silu_with_a_device_row_count(width):
    """conan_silu_fwd / conan_silu_bwd with m_dev: rows < m computed, rows >= m untouched; judged like every other kernel."""
    m, rows_total, fails = 300, 347, []
    res = R.reference(R.OPS["silu"], R.Rows(m), width, {}, 11 + width)
    x, gy = sent(rows_total, width), sent(rows_total, width)
    x[:m], gy[:m] = res["ins"][0].to(dev), res["gouts"][0].to(dev)
    md = torch.tensor([m], dtype=i32, device=dev)
    y, dx = sent(rows_total, width), sent(rows_total, width)
    assert raw("conan_silu_fwd", ptr(x), rows_total, width, ptr(md), ptr(y), stream_ptr()) == OK
    assert raw("conan_silu_bwd", ptr(x), ptr(gy), rows_total, width, ptr(md), ptr(dx), stream_ptr()) == OK
    torch.cuda.synchronize()
    assert is_sent(y[m:]) and is_sent(dx[m:])
    check("silu", f"m_dev/W{width}", res, [y[:m]], [dx[:m]], fails)
    big = torch.tensor([rows_total + 5], dtype=i32, device=dev)                    # a count above the buffer is clamped to its rows
    x2 = torch.randn(rows_total, width, device=dev)
    y2 = sent(rows_total + 1, width)
    assert raw("conan_silu_fwd", ptr(x2), rows_total, width, ptr(big), ptr(y2), stream_ptr()) == OK
    torch.cuda.synchronize()
    assert is_sent(y2[rows_total:]) and bool(torch.isfinite(y2[:rows_total]).all())
    assert not fails, fails


def test_the_two_silu_forms_agree():
    """The forward file's SiLU (visnet.hip, reached through conan_visnet_gate with scalar_activation = 1) and the backward file's (visnet_bwd.hip, reached
    through conan_silu_fwd; the pre_act backward kernels regenerate the activation with it) over a sweep of |x| up to 80.  Both are
    v * rcp(1 + exp(-v)) with the fast exponential and the approximate reciprocal (about 1 ulp each, 2 ulp for exp at large arguments): two
    evaluations may differ by the sum of their errors, bounded here by 8 ulp of the value."""
    x = torch.cat([torch.linspace(-80, 80, 1 << 16), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 80.0, -80.0])]).to(dev)
    n = x.shape[0]
    u = torch.stack([x, torch.zeros_like(x)], dim=1).contiguous()                 # [n, 2 * O], O = 1: [x | gate]
    v2, xo, vout, y = torch.zeros(n, 3, 1, device=dev), sent(n, 1), sent(n, 3, 1), sent(n, 1)
    assert raw("conan_visnet_gate", ptr(u), ptr(v2), n, 1, 1, ptr(xo), ptr(vout), stream_ptr()) == OK
    assert raw("conan_silu_fwd", ptr(x), n, 1, None, ptr(y), stream_ptr()) == OK
    torch.cuda.synchronize()
    a, b = xo.view(-1).double().cpu(), y.view(-1).double().cpu()
    ref = R.silu(x.double().cpu())
    diff = float(((a - b).abs() / (ref.abs() + 1e-38)).max())
    print(f"SILU forward-file vs backward-file: max relative difference {diff:.3g}; vs fp64: {float(((a - ref).abs() / (ref.abs() + 1e-38)).max()):.3g} "
          f"/ {float(((b - ref).abs() / (ref.abs() + 1e-38)).max()):.3g}")
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert diff <= 8 * 2.0 ** -23


# ================================================================================================ element-wise kernels at awkward widths and alignments
def _carve(numel, offset):
    """`numel` floats `offset` floats into a buffer of the NaN pattern, with 64 guard floats on either side."""
    big = sent(64 + offset + numel + 64)
    return big, big[64 + offset: 64 + offset + numel]


def _guards_ok(big, offset, numel):
    return is_sent(big[:64 + offset]) and is_sent(big[64 + offset + numel:])


@pytest.mark.parametrize("H,offset", [(32, 0), (32, 1), (R.ODD_WIDTH, 0), (R.ODD_WIDTH, 3), (96, 2), (4, 0)])
def test_elementwise_kernels_stay_inside_exact_size_buffers(H, offset):
    """scale_channels / scale_channels_add (float4 form only for H % 4 == 0 and 16-byte aligned pointers, the scalar form otherwise), silu, concat2 /
    split2 with Ha != Hb, on buffers of exact size at aligned and unaligned offsets: correct values, and the floats on either side untouched."""
    rows_, fails = 7, []
    gen = torch.Generator().manual_seed(H * 10 + offset)
    v, w, add = R.rows(gen, rows_, H), 1.0 + 0.3 * torch.randn(H, generator=gen), R.rows(gen, rows_, H)
    bufs = {}
    for key, t in (("v", v), ("w", w), ("add", add)):
        bufs[key] = _carve(t.numel(), offset)
        bufs[key][1].copy_(t.reshape(-1).to(dev))
    for with_add in (False, True):
        big, out = _carve(rows_ * H, offset)
        if with_add:
            rc = raw("conan_scale_channels_add", ptr(bufs["v"][1]), ptr(bufs["w"][1]), ptr(bufs["add"][1]), rows_, H, ptr(out), stream_ptr())
        else:
            rc = raw("conan_scale_channels", ptr(bufs["v"][1]), ptr(bufs["w"][1]), rows_, H, ptr(out), stream_ptr())
        torch.cuda.synchronize()
        assert rc == OK and _guards_ok(big, offset, rows_ * H)
        f = lambda dt: (v.to(dt) * w.to(dt) + (add.to(dt) if with_add else 0)).reshape(rows_, H)
        ok, rr, ra = R.judge(out.view(rows_, H).cpu(), f(f32), f(torch.float64))
        print(f"RATIO scale_channels{'_add' if with_add else ''} raw/H{H}/off{offset} out row={rr:.3g} all={ra:.3g}")
        if not ok:
            fails.append(("scale_channels", with_add, rr, ra))
    # silu
    big, y = _carve(rows_ * H, offset)
    assert raw("conan_silu_fwd", ptr(bufs["v"][1]), rows_, H, None, ptr(y), stream_ptr()) == OK
    torch.cuda.synchronize()
    assert _guards_ok(big, offset, rows_ * H)
    ok, rr, ra = R.judge(y.view(rows_, H).cpu(), R.silu(v), R.silu(v.double()))
    if not ok:
        fails.append(("silu", rr, ra))
    # concat2 / split2 with Ha != Hb
    Hb = H // 2 + 1
    b = R.rows(gen, rows_, Hb)
    bb, bv = _carve(b.numel(), offset)
    bv.copy_(b.reshape(-1).to(dev))
    big, cat = _carve(rows_ * (H + Hb), offset)
    assert raw("conan_concat2", ptr(bufs["v"][1]), H, ptr(bv), Hb, rows_, ptr(cat), stream_ptr()) == OK
    torch.cuda.synchronize()
    assert _guards_ok(big, offset, rows_ * (H + Hb)) and torch.equal(cat.view(rows_, H + Hb).cpu(), torch.cat([v, b], dim=1))
    (ba, oa), (bb2, ob) = _carve(rows_ * H, offset), _carve(rows_ * Hb, offset)
    assert raw("conan_split2", ptr(cat), H, Hb, rows_, ptr(oa), ptr(ob), stream_ptr()) == OK
    torch.cuda.synchronize()
    assert _guards_ok(ba, offset, rows_ * H) and _guards_ok(bb2, offset, rows_ * Hb)
    assert torch.equal(oa.view(rows_, H).cpu(), v) and torch.equal(ob.view(rows_, Hb).cpu(), b)
    assert all(_guards_ok(bufs[k][0], offset, bufs[k][1].numel()) for k in bufs)
    assert not fails, fails


# ================================================================================================ distances at and beyond the cutoff
def test_distances_at_the_cutoff():
    """RadiusGraph keeps only d < cutoff, so a few entries of graph.dist are overwritten by hand: 1, 2 and 3 ulp below the cutoff (the cosine cutoff
    cancels to ~1e-14 there), exactly the cutoff and beyond it (factor exactly 0)."""
    gg = gpu_graph("capped", cache=False)
    g, G, fails = gg.g, gg.ref, []
    real = (G.src != G.tgt).nonzero().view(-1)[[3, 40, 77, 200, 333, 801]]
    c = np.float32(R.CUTOFF)
    vals = [c, np.float32(5.5), np.float32(7.0)]
    d = c
    for _ in range(3):
        d = np.nextafter(d, np.float32(0))
        vals.append(d)
    G.dist[real] = torch.tensor(vals, dtype=f32)
    g.dist[real.to(dev)] = torch.tensor(vals, dtype=f32, device=dev)
    zero_rows = real[:3]
    for name, H, fl in (("neighbor_scale", 32, {}), ("neighbor_scale", 128, {}), ("expnormal", 32, {}), ("attn_message", 32, {"heads": 8, "pre_act": 1}),
                        ("attn_message", 128, {"heads": 8, "pre_act": 1}), ("attn_message", 128, {"heads": 64, "pre_act": 0})):
        res = R.reference(R.OPS[name], G, H, fl, R.case_seed(name, "cutoff", H, fl))
        outs, grads, _, _ = run_gpu(name, gg, G, H, fl, res)
        check(name, f"cutoff/H{H}", res, outs, grads, fails)
        assert float(outs[0][zero_rows].abs().max()) == 0.0, (name, H)          # d >= cutoff: factor exactly 0
        if name == "attn_message":
            assert float(grads[3][zero_rows].abs().max()) == 0.0 and float(grads[4][zero_rows].abs().max()) == 0.0
    assert not fails, fails


# ================================================================================================ n = 0
def test_empty_inputs_return_ok_and_write_nothing():
    s, H = stream_ptr(), 32
    one = lambda: sent(4 * 3 * 3 * H)
    zi = torch.zeros(4, dtype=i32, device=dev)
    a, b, c, d, e = (torch.ones(4 * 3 * 3 * H, device=dev) for _ in range(5))
    outs = [one() for _ in range(6)]
    p = [ptr(o) for o in outs]
    codes = {
        "layernorm_fwd": raw("conan_layernorm_fwd", ptr(a), ptr(b), ptr(c), 0, H, 1e-5, p[0], s),
        "scale_channels": raw("conan_scale_channels", ptr(a), ptr(b), 0, H, p[0], s),
        "scale_channels_add": raw("conan_scale_channels_add", ptr(a), ptr(b), ptr(c), 0, H, p[0], s),
        "vecdot": raw("conan_visnet_vecdot", ptr(a), 0, H, p[0], s),
        "vecdot_bwd": raw("conan_visnet_vecdot_bwd", ptr(a), ptr(b), 0, H, p[0], s),
        "attn_message": raw("conan_visnet_attn_message", ptr(a), ptr(b), ptr(c), ptr(d), ptr(e), ptr(zi), ptr(zi), ptr(a), R.CUTOFF, 0, H, 8, 1, p[0], p[1], s),
        "attn_message_bwd": raw("conan_visnet_attn_message_bwd", ptr(a), ptr(b), ptr(c), ptr(d), ptr(e), ptr(a), ptr(b), ptr(zi), ptr(zi), ptr(zi), ptr(zi), ptr(zi),
                                ptr(a), R.CUTOFF, 0, H, 8, 1, p[0], p[1], p[2], p[3], p[4], s),
        "vec_aggregate": raw("conan_visnet_vec_aggregate", ptr(a), ptr(b), ptr(c), ptr(zi), ptr(zi), 0, H, 1, p[0], s),
        "node_update": raw("conan_visnet_node_update", ptr(a), ptr(b), ptr(c), ptr(d), ptr(e), ptr(a), 0, H, p[0], p[1], s),
        "node_update_bwd": raw("conan_visnet_node_update_bwd", ptr(a), ptr(b), ptr(c), ptr(d), ptr(e), 0, H, p[0], p[1], p[2], s),
        "edge_update_bwd": raw("conan_visnet_edge_update_bwd", ptr(a), ptr(b), ptr(c), ptr(d), ptr(e), ptr(zi), ptr(zi), ptr(zi), ptr(zi), ptr(zi), 0, H, 1,
                               p[0], p[1], p[2], s),
        "neighbor_scale_to": raw("conan_visnet_neighbor_scale_to", ptr(a), ptr(b), ptr(zi), ptr(zi), ptr(zi), 0, H, R.CUTOFF, p[0], s),
        "spatial_norm": raw("conan_visnet_spatial_norm", ptr(a), 0, H, p[0], s),
        "spatial_norm_bwd": raw("conan_visnet_spatial_norm_bwd", ptr(a), ptr(b), 0, H, p[0], s),
        "gate": raw("conan_visnet_gate", ptr(a), ptr(b), 0, H, 1, p[0], p[1], s),
        "gate_bwd": raw("conan_visnet_gate_bwd", ptr(a), ptr(b), ptr(c), ptr(d), 0, H, 1, p[0], p[1], s),
        "prior": raw("conan_visnet_prior", ptr(a), ptr(torch.zeros(4, dtype=torch.int64, device=dev)), ptr(b), ptr(c), 0, H, p[0], s),
        "concat2": raw("conan_concat2", ptr(a), H, ptr(b), 7, 0, p[0], s),
        "split2": raw("conan_split2", ptr(a), H, 7, 0, p[0], p[1], s),
        "silu_fwd": raw("conan_silu_fwd", ptr(a), 0, H, None, p[0], s),
        "silu_bwd": raw("conan_silu_bwd", ptr(a), ptr(b), 0, H, None, p[0], s),
        "rowsum": raw("conan_rowsum", ptr(a), 0, H, p[0], s),
        "scale_scalar": raw("conan_scale_scalar", ptr(a), ptr(b), 0, p[0], s),
    }
    torch.cuda.synchronize()
    assert all(rc == OK for rc in codes.values()), codes
    assert all(is_sent(o) for o in outs)
    # LayerNorm backward over no rows: dx untouched, the parameter gradients are the empty sum
    assert raw("conan_layernorm_bwd_ws", 0, H) == 0 and raw("conan_layernorm_bwd_ws", 300, H) == 2 * 300 + 2 * 2 * H
    dg, db = sent(H), sent(H)
    assert raw("conan_layernorm_bwd", ptr(a), ptr(b), ptr(c), 0, H, 1e-5, p[0], ptr(dg), ptr(db), p[1], s) == OK
    torch.cuda.synchronize()
    assert is_sent(outs[0]) and float(dg.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
    # a NULL pointer or a non-positive width is a bad argument
    assert raw("conan_visnet_vecdot", None, 1, H, p[0], s) == E_BADARG and raw("conan_visnet_vecdot", ptr(a), 1, 0, p[0], s) == E_BADARG


# ================================================================================================ closing: nothing was left out
def test_zz_every_visnet_export_was_exercised():
    """The names declared in the two ViSNet sections of the header that _lib.SIGNATURES binds == the names this module called: a kernel added later
    without a test fails here.  (Run the whole module: this test looks at what the tests above did.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "conan_fgw_hip.h")).read()
    sect = text[text.index("ViSNet (forward)"):text.index("FGW barycenter */")]
    declared = set(re.findall(r"^(?:int|long long)\s+(conan_\w+)\s*\(", sect, flags=re.M))
    assert len(declared) == 33, sorted(declared)      # 17 forward, 15 backward, the LayerNorm workspace query
    bound = declared & set(_lib.SIGNATURES)
    whole = "this test looks at what the other tests of the module did: run the whole module, in file order, in one process"
    assert bound == declared, sorted(declared - bound)
    assert bound == (CALLED & declared), (whole, sorted(bound - CALLED))
    # set equality alone would be satisfied by the raw n = 0 calls: the exports the model reaches only through switches that are off today must have
    # been reached through the autograd wrappers (run_gpu), with real data
    through_wrappers = {"conan_layernorm_bwd", "conan_layernorm_bwd_res", "conan_scale_channels", "conan_scale_channels_add", "conan_visnet_vecdot_bwd",
                        "conan_visnet_node_update_bwd", "conan_split2", "conan_rowsum", "conan_scale_scalar", "conan_silu_fwd", "conan_silu_bwd",
                        "conan_visnet_neighbor_scale_to", "conan_visnet_attn_message_bwd", "conan_visnet_vec_aggregate_bwd", "conan_visnet_edge_update_bwd",
                        "conan_visnet_edge_embed_bwd", "conan_visnet_spatial_norm_bwd", "conan_visnet_gate_bwd"}
    assert through_wrappers <= TRACED, (whole, sorted(through_wrappers - TRACED))
    assert BRANCHES == {"badarg", "unsupported", "blocks128", "cpl2", "cpl1"}, (whole, BRANCHES)      # all three k_attn_msg instantiations and both rejections
    assert "wide" in _GRAPHS, whole
    print("\nworst err / yard per kernel (row, whole tensor):")
    for (name, what), (rr, ra) in sorted(RATIOS.items()):
        print(f"TABLE {name:16s} {what:5s} row={rr:6.3g} all={ra:6.3g}")
