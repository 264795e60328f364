"""Every GAT kernel on its own against the plain fp64 reference of the same operation (tests/gat_ref.py).

The exports of the covalent section of include/conan_fgw_hip.h are called as C entry points (`raw`: the status code is visible) on crafted bond graphs:
a directed graph whose chosen nodes have in- or out-degree 0, 1, 5, 6, 7, 31, 32, 33, 63, 64, 65, 150 (GAT_MD = 6 separates the staged from the serial
rows of the 16-lane backward kernels, 64 edges those of the wavefront kernels), graphs of one and two nodes, without edges, without bias, with
multi-edges and interleaved self loops, with pre-activations of -70 .. +110, and two chains long enough for the second grid pass of either backward
family and for the long form of the row-pointer scan.  Widths 64 / 128 / 256 take the 16-lane kernels, 32 / 96 / 200 / 8 and edge_dim > 4 the
one-wavefront-per-node kernels with a partial last channel pass.  `BondGraph` / `_GATAggregateFn` are called where the Python door adds behaviour.

Judging (visnet_ref.judge, unchanged, margins from visnet_ref): per row and per tensor, err(gpu, ref64) <= MARGIN * err(ref32, ref64) — the yardstick is
the reference formula in fp32 on the CPU, never the kernel; per-node and per-edge scalars are judged entry by entry.  The CSR is integer work and must be
exact.  alpha + alpha_self of a row must sum to 1 within the same yardstick.  Every output buffer is pre-filled with a NaN bit pattern and has a tail
beyond its documented size: the tail, the alpha entries beyond the kept edges and the workspace beyond conan_gat_bwd_ws must still hold the pattern.
Every case runs twice and must give the same bits; on graphs without multi-edges a permuted edge_index must give the same bits too.  The conditions on
the inputs are asserted by tests/test_gat_ref_cpu.py.  The `RATIO` / `TABLE` lines printed by a run (-s) are the source of the table in DESIGN.md
section 3.6."""
import os
import re

import numpy as np
import pytest
import torch

import gat_ref as G
import visnet_ref as R
from conan_fgw_amd import _lib
from conan_fgw_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
f32, i32, i64 = torch.float32, torch.int32, torch.int64
OK, E_BADARG = 0, -1
SENT, TAIL = 0x7FA5A5A5, 64              # a NaN bit pattern: reading it poisons a result, overwriting it is visible; floats beyond every documented size
CALLED, TRACED, RATIOS, BRANCHES = set(), set(), {}, set()
CASES = G.cases()
def family(case):
    """Which backward kernels conan_gat_aggregate_bwd takes for this case: the 16-lane groups or one wavefront per node."""
    b = case.branches()
    return "g16" if "g16/target/staged" in b or "g16/target/serial" in b else "wave"


SHARED = (R.MARGIN_ROW, R.MARGIN_ALL)
# Outputs that need more than the shared margins: output -> f(case) -> (row, whole tensor) = 2 x the ratio measured on the MI355X.  All four are vectors
# of a few numbers judged as ONE row (so the whole-tensor margin of 4 is the one that binds), on which the yardstick — the fp32 reference's own error — is
# small by luck now and then.  Measured values and reasons: DESIGN.md section 3.6.
GAT_MARGIN = {
    # edge_dim numbers, each a serial fp32 sum of C products in one thread where torch's sum is pairwise: measured 6.75 (tiny/E0/C96), 4.94 (degree/C256/D3)
    "v": lambda case: (13.5, 13.5),
    # n = 1: ONE number from a 64-lane tree sum: measured 4.0 (tiny/n1/C96)
    "a_src": lambda case: (8.0, 8.0) if case.n == 1 else SHARED,
    # one-wavefront-per-node kernels: per-wavefront partials, then 2048 partial rows of which all but a few are zero: measured 5.56 / 4.32 on the
    # 9-node multi-edge graph (multi/C96), at most 2.05 / 2.35 on every other case
    "d_att_src": lambda case: (11.2, 11.2) if family(case) == "wave" else SHARED,
    "dv": lambda case: (8.7, 8.7) if family(case) == "wave" else SHARED,
}
ROWSUM_FLOOR = 2.0 ** -24                # the rounding unit of fp32 at 1: on a graph of a few rows the fp32 reference sums to exactly 1 in every row


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


def sent_i(numel):
    return torch.full((numel,), SENT, dtype=i32, device=dev)


def sent(numel):
    return sent_i(numel).view(f32)


def is_sent(t):
    return bool((t.contiguous().view(i32) == SENT).all())


def same_bits(a, b):
    return all(torch.equal(a[k].view(i32), b[k].view(i32)) for k in a)


_REF = {}


def case_ref(name):
    """(case, inputs, reference): computed once, shared by the tests, never modified."""
    if name not in _REF:
        c = CASES[name]
        inp = G.make_inputs(c)
        _REF[name] = (c, inp, G.reference(c, inp))
    return _REF[name]


# ================================================================================================ the bond graph
CSR_KEYS = ("rowptr", "col", "eid", "t_rowptr", "t_pos", "t_tgt")


def run_csr(ei, n):
    """conan_bond_graph_csr on buffers of the NaN pattern with tails -> the raw buffers; everything beyond the documented sizes (n + 1 row pointers, the
    kept edges) must be untouched.  E = 0: buffers of one element."""
    E = int(ei.shape[1])
    ei_d = torch.from_numpy(np.ascontiguousarray(ei)).to(dev) if E else torch.zeros(2, 1, dtype=i64, device=dev)
    ws = sent_i(2 * (n + 1) + TAIL)
    g = {k: sent_i((n + 1 if "rowptr" in k else max(E, 1)) + TAIL) for k in CSR_KEYS}
    rc = raw("conan_bond_graph_csr", ptr(ei_d), E, n, ptr(ws), *[ptr(g[k]) for k in CSR_KEYS], stream_ptr())
    torch.cuda.synchronize()
    assert rc == OK
    assert is_sent(ws[2 * (n + 1):])
    return g


def check_csr(g, want, n):
    K = want.K
    for k in CSR_KEYS:
        size = n + 1 if "rowptr" in k else K
        assert np.array_equal(g[k][:size].cpu().numpy(), getattr(want, k)), k          # integer work: exact
        assert is_sent(g[k][size:]), (k, "written beyond its documented size")


def csr_graphs():
    k = G.constants()
    return {"degree": G.degree_graph(), "multi+invalid": G.multi_graph(invalid=True), "multi": G.multi_graph(), "n1": (np.zeros((2, 0), np.int64), 1),
            "n2": (np.array([[1], [0]], np.int64), 2), "E0": (np.zeros((2, 0), np.int64), 40), "random": G.random_graph(300, 12, 3),
            "chain33000": G.chain_graph(33000, 1), "chain-global-scan": G.chain_graph(k.SCAN_LDS_MAX + 100, 3)}


@pytest.mark.parametrize("gname", list(csr_graphs()))
def test_bond_graph_csr_is_exact(gname):
    """Both CSRs, entry by entry, against gat_ref.bond_csr: per target (source, edge id) ascending, per source ascending by-target position; self loops and
    endpoints outside [0, n) dropped.  n = 33 000 takes the long form of the row-pointer scan, n > SCAN_LDS_MAX the scan that walks global memory."""
    ei, n = csr_graphs()[gname]
    want = G.bond_csr(ei, n)
    g1, g2 = run_csr(ei, n), run_csr(ei, n)
    check_csr(g1, want, n)
    assert same_bits(g1, g2), "two runs differ"
    BRANCHES.add("scan/" + G.scan_branch(n))
    if gname == "multi+invalid":
        assert want.K == ei.shape[1] - 4 - 3                                         # 4 self loops, 3 edges with an endpoint equal to n or -1
    if ei.shape[1] > 1:
        perm = np.random.RandomState(5).permutation(ei.shape[1])
        gp = run_csr(ei[:, perm].copy(), n)
        wp = G.bond_csr(ei[:, perm], n)
        check_csr(gp, wp, n)
        assert all(torch.equal(gp[k], g1[k]) for k in ("rowptr", "col", "t_rowptr", "t_pos", "t_tgt"))
        assert np.array_equal(np.sort(perm[wp.eid]), np.sort(want.eid))


def test_bond_graph_door_is_deterministic_and_equal_to_the_entry_point():
    from conan_fgw_amd.gat import BondGraph
    for ei, n in (G.degree_graph(), G.multi_graph(), (np.zeros((2, 0), np.int64), 40)):
        want = G.bond_csr(ei, n)
        ei_d = torch.from_numpy(ei).to(dev)
        a, b = BondGraph(ei_d, n), BondGraph(ei_d, n)
        torch.cuda.synchronize()
        assert a.num_nodes == n and a.num_edges == ei.shape[1]
        for k in CSR_KEYS:
            size = n + 1 if "rowptr" in k else want.K
            assert torch.equal(getattr(a, k)[:size], getattr(b, k)[:size]), k
            assert np.array_equal(getattr(a, k)[:size].cpu().numpy(), getattr(want, k)), k
    with pytest.raises(RuntimeError):
        BondGraph(torch.zeros(2, 3, dtype=i64), 4)                                     # no CPU path


# ================================================================================================ the kernels, one entry point after the other
def run_kernels(case, inp, g, dout=None):
    """edge_vec -> node_alpha -> aggregate_fwd (-> aggregate_bwd -> edge_vec_bwd), each into sentinel buffers with a tail.  Returns the raw buffers."""
    n, C, D, E, K, s = case.n, case.C, case.D, case.E, case.csr.K, stream_ptr()
    d = {k: (None if t is None else t.to(dev).contiguous()) for k, t in inp.items()}
    if dout is not None:
        d["dout"] = dout
    ea = d["ea"] if E else torch.zeros(1, D, device=dev)
    o = {"v": sent(D + TAIL), "a_src": sent(n + TAIL), "a_dst": sent(n + TAIL), "out": sent(n * C + TAIL), "alpha": sent(max(E, 1) + TAIL),
         "alpha_self": sent(n + TAIL)}
    assert raw("conan_gat_edge_vec", ptr(d["W_edge"]), ptr(d["att_edge"]), C, D, ptr(o["v"]), s) == OK
    assert raw("conan_gat_node_alpha", ptr(d["h"]), ptr(d["att_src"]), ptr(d["att_dst"]), n, C, ptr(o["a_src"]), ptr(o["a_dst"]), s) == OK
    assert raw("conan_gat_aggregate_fwd", ptr(d["h"]), ptr(o["a_src"]), ptr(o["a_dst"]), ptr(g["rowptr"]), ptr(g["col"]), ptr(g["eid"]), ptr(ea), D, ptr(o["v"]),
               ptr(d["bias"]), G.SLOPE, n, C, ptr(o["out"]), ptr(o["alpha"]), ptr(o["alpha_self"]), s) == OK
    torch.cuda.synchronize()
    sizes = {"v": D, "a_src": n, "a_dst": n, "out": n * C, "alpha": K, "alpha_self": n}
    if case.backward:
        wsn = int(raw("conan_gat_bwd_ws", n, E, C, D))
        assert wsn >= 2 * n + max(E, 1) + 3 * C + D
        o.update(ws=sent(wsn + TAIL), dh=sent(n * C + TAIL), dparams=sent(3 * C + D + TAIL), dW_edge=sent(C * D + TAIL), d_att_edge=sent(C + TAIL))
        assert raw("conan_gat_aggregate_bwd", ptr(d["h"]), ptr(d["dout"]), ptr(o["alpha"]), ptr(o["alpha_self"]), ptr(o["a_src"]), ptr(o["a_dst"]), ptr(d["att_src"]),
                   ptr(d["att_dst"]), ptr(g["rowptr"]), ptr(g["col"]), ptr(g["eid"]), ptr(g["t_rowptr"]), ptr(g["t_pos"]), ptr(g["t_tgt"]), ptr(ea), D, ptr(o["v"]),
                   G.SLOPE, n, E, C, ptr(o["ws"]), ptr(o["dh"]), ptr(o["dparams"]), s) == OK
        assert raw("conan_gat_edge_vec_bwd", ptr(d["W_edge"]), ptr(d["att_edge"]), ptr(d["dv_in"]), C, D, ptr(o["dW_edge"]), ptr(o["d_att_edge"]), s) == OK
        torch.cuda.synchronize()
        sizes.update(ws=wsn, dh=n * C, dparams=3 * C + D, dW_edge=C * D, d_att_edge=C)
    for k, size in sizes.items():
        assert is_sent(o[k][size:]), (case.name, k, "written beyond its documented size")
        if k != "ws":
            assert bool(torch.isfinite(o[k][:size]).all()), (case.name, k, "not finite")
    return o


def outputs(case, o):
    """The raw buffers cut to the reference's names and shapes (CPU)."""
    n, C, D, K = case.n, case.C, case.D, case.csr.K
    c = {k: t.cpu() for k, t in o.items() if k != "ws"}
    col = lambda t, m: t[:m].unsqueeze(1)
    tgt = torch.from_numpy(case.csr.tgt.astype(np.int64))
    r = {"v": c["v"][:D], "a_src": col(c["a_src"], n), "a_dst": col(c["a_dst"], n), "out": c["out"][:n * C].view(n, C), "alpha": col(c["alpha"], K),
         "alpha_self": col(c["alpha_self"], n),
         "rowsum": G.rowsum(c["alpha"][:K].double(), c["alpha_self"][:n].double(), tgt, n).unsqueeze(1)}
    if case.backward:
        p = c["dparams"]
        r.update(dh=c["dh"][:n * C].view(n, C), d_att_src=p[:C], d_att_dst=p[C:2 * C], d_bias=p[2 * C:3 * C], dv=p[3 * C:3 * C + D],
                 dW_edge=c["dW_edge"][:C * D].view(C, D), d_att_edge=c["d_att_edge"][:C])
    return r


def check(case, got, ref, fails, keep=None, tag=""):
    """Judge every output.  keep(name) -> slice of rows (the large cases: the rows beyond the first grid pass)."""
    for what, r64 in ref["64"].items():
        r32, a = ref["32"][what], got[what]
        assert a.shape == r64.shape, (case.name, what, a.shape, r64.shape)
        if keep is not None:
            sl = keep(what)
            if sl is None:
                continue
            a, r32, r64 = a[sl], r32[sl], r64[sl]
            assert a.shape[0] > 0, (case.name, what)
        if r64.numel() == 0:
            continue
        mr, ma = GAT_MARGIN[what](case) if what in GAT_MARGIN else SHARED
        if what == "rowsum":
            # alpha_self + the row's alphas against 1, row by row: |sum - 1| <= MARGIN_ROW * yardstick, the yardstick being the fp32 reference's worst
            # row but no less than one rounding of 1 in fp32 (a sum of fp32 numbers cannot be asked to hit 1 more finely than the format resolves it)
            yard = max(float((r32.double() - r64).abs().max()), ROWSUM_FLOOR)
            rr = ra = float((a.double() - r64).abs().max()) / yard
            ok = rr <= mr
        else:
            ok, rr, ra = R.judge(a, r32, r64, mr, ma)
        key = (what, family(case) if what in ("dh", "d_att_src", "d_att_dst", "d_bias", "dv") else "")
        old = RATIOS.get(key, (0.0, 0.0))
        RATIOS[key] = (max(old[0], rr), max(old[1], ra))
        print(f"RATIO {case.name}{tag} {what} row={rr:.3g} all={ra:.3g}")
        if not ok:
            fails.append((case.name + tag, what, float("%.3g" % rr), float("%.3g" % ra)))


def run_case(name, fails, keep=None):
    case, inp, ref = case_ref(name)
    g = run_csr(case.ei, case.n)
    check_csr(g, case.csr, case.n)
    o1, o2 = run_kernels(case, inp, g), run_kernels(case, inp, g)
    assert same_bits(o1, o2), (name, "two runs differ")
    got = outputs(case, o1)
    check(case, got, ref, fails)
    if keep is not None:
        check(case, got, ref, fails, keep=keep, tag="/second-pass")
    if case.simple and case.E > 1:
        cp, ip = G.permuted(case, inp)
        gp = run_csr(cp.ei, cp.n)
        op = run_kernels(cp, ip, gp)
        assert same_bits({k: v for k, v in o1.items() if k != "ws"}, op), (name, "a permuted edge_index changes the bits")
    BRANCHES.update(case.branches())
    return case, inp, g, o1


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.large])
def test_kernels_against_fp64_reference(name):
    fails = []
    run_case(name, fails)
    assert not fails, fails


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.large])
def test_kernels_beyond_the_first_grid_pass(name):
    """Chains of degree <= 4.  n = 33 000 at C = 64: the 16-lane kernels stride by 16 groups x GAT_BW_WGS workgroups = 32 768 nodes, and the row-pointer
    scan takes its long form; n = 8 300 at C = 96: the wavefront kernels stride by 4 x GAT_BW_WGS = 8 192 nodes.  Judged on all rows and, separately, on
    the rows (and the edges of the rows) beyond the first pass."""
    case, k, fails = CASES[name], G.constants(), []
    first = k.G16_PASS if "g16/second-pass" in case.branches() else k.WAVES
    assert case.n > first and ("g16/second-pass" in case.branches() or "wave/second-pass" in case.branches())
    e0 = int(case.csr.rowptr[first])
    per_node, per_edge = ("a_src", "a_dst", "out", "alpha_self", "rowsum", "dh"), ("alpha",)
    keep = lambda what: slice(first, None) if what in per_node else slice(e0, None) if what in per_edge else None
    run_case(name, fails, keep=keep)
    assert not fails, fails


# ================================================================================================ arguments the entry points turn down
def test_rejected_arguments_write_nothing():
    """Backward at C = 257 (channels <= 256) and edge_dim 0 / 9 (1 .. 8): the bad-argument status, every output still the NaN pattern."""
    case, inp, _ = case_ref("tiny/nobias/C64")
    g = run_csr(case.ei, case.n)
    n, E, s = case.n, case.E, stream_ptr()
    for C, D, fwd_ok in ((257, 3, True), (64, 0, False), (64, 9, False)):
        Dm = max(D, 1)
        h, dout, att, w = torch.randn(n, C, device=dev), torch.randn(n, C, device=dev), torch.randn(C, device=dev), torch.randn(C, Dm, device=dev)
        ea, v, a = torch.randn(max(E, 1), Dm, device=dev), torch.randn(16, device=dev), torch.randn(n, device=dev)
        alpha = torch.rand(max(E, 1), device=dev)
        outs = {k: sent(m + TAIL) for k, m in (("v", 16), ("out", n * C), ("alpha", max(E, 1)), ("alpha_self", n), ("ws", 2 * n + E + 2049 * (3 * C + 16)),
                                               ("dh", n * C), ("dparams", 3 * C + 16), ("dW", C * 16), ("dae", C))}
        rc_v = raw("conan_gat_edge_vec", ptr(w), ptr(att), C, D, ptr(outs["v"]), s)
        rc_f = raw("conan_gat_aggregate_fwd", ptr(h), ptr(a), ptr(a), ptr(g["rowptr"]), ptr(g["col"]), ptr(g["eid"]), ptr(ea), D, ptr(v), None, G.SLOPE, n, C,
                   ptr(outs["out"]), ptr(outs["alpha"]), ptr(outs["alpha_self"]), s)
        rc_b = raw("conan_gat_aggregate_bwd", ptr(h), ptr(dout), ptr(alpha), ptr(a), ptr(a), ptr(a), ptr(att), ptr(att), ptr(g["rowptr"]), ptr(g["col"]), ptr(g["eid"]),
                   ptr(g["t_rowptr"]), ptr(g["t_pos"]), ptr(g["t_tgt"]), ptr(ea), D, ptr(v), G.SLOPE, n, E, C, ptr(outs["ws"]), ptr(outs["dh"]), ptr(outs["dparams"]), s)
        rc_w = raw("conan_gat_edge_vec_bwd", ptr(w), ptr(att), ptr(v), C, D, ptr(outs["dW"]), ptr(outs["dae"]), s)
        torch.cuda.synchronize()
        assert rc_b == E_BADARG, (C, D, rc_b)
        assert (rc_v, rc_f, rc_w) == ((OK, OK, OK) if fwd_ok else (E_BADARG,) * 3), (C, D, rc_v, rc_f, rc_w)
        written = {"v", "out", "alpha", "alpha_self", "dW", "dae"} if fwd_ok else set()
        assert all(is_sent(t) for k, t in outs.items() if k not in written), (C, D)
    assert raw("conan_gat_node_alpha", None, None, None, 1, 64, None, None, s) == E_BADARG
    assert raw("conan_bond_graph_csr", None, 0, 0, None, None, None, None, None, None, None, s) == E_BADARG


# ================================================================================================ the Python door
def _door(case, inp, g_obj, frozen_bias=False, dout=None):
    from conan_fgw_amd.gat import _GATAggregateFn
    C = case.C
    leaf = lambda t, shape=None: (t.to(dev).view(shape) if shape else t.to(dev)).clone().requires_grad_(True)
    h, W = leaf(inp["h"]), leaf(inp["W_edge"])
    a_s, a_d, a_e = (leaf(inp[k], (1, 1, C)) for k in ("att_src", "att_dst", "att_edge"))
    bias = None if inp["bias"] is None else inp["bias"].to(dev).clone().requires_grad_(not frozen_bias)
    out = _GATAggregateFn.apply(h, a_s, a_d, W, a_e, bias, g_obj, inp["ea"].to(dev), G.SLOPE)
    if dout is None:
        out.sum().backward()                                                           # autograd hands over an expanded scalar: a stride-0 dout
    else:
        out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), {"dh": h.grad, "d_att_src": a_s.grad.view(-1), "d_att_dst": a_d.grad.view(-1), "dW_edge": W.grad, "d_att_edge": a_e.grad.view(-1),
                          "d_bias": None if bias is None else bias.grad}


@pytest.mark.parametrize("name", ["degree/C64/D3", "degree/C96/D3", "tiny/nobias/C96", "multi/C64"])
def test_python_door_adds_nothing_but_plumbing(name):
    """_GATAggregateFn on a BondGraph == the entry points called by hand, bit for bit (those are judged above): with `out.sum().backward()` (a stride-0
    dout), with a frozen bias (no gradient for it, the others unchanged), without a bias."""
    from conan_fgw_amd.gat import BondGraph
    case, inp, _ = case_ref(name)
    n, C, D = case.n, case.C, case.D
    g = run_csr(case.ei, case.n)
    ones = torch.ones(n, C, device=dev)
    o = run_kernels(case, inp, g, dout=ones)
    dW, dae, W_d, ae_d, dv_d = sent(C * D), sent(C), inp["W_edge"].to(dev), inp["att_edge"].to(dev), o["dparams"][3 * C:3 * C + D].clone()
    assert raw("conan_gat_edge_vec_bwd", ptr(W_d), ptr(ae_d), ptr(dv_d), C, D, ptr(dW), ptr(dae), stream_ptr()) == OK
    torch.cuda.synchronize()
    want = {"dh": o["dh"][:n * C].view(n, C), "d_att_src": o["dparams"][:C], "d_att_dst": o["dparams"][C:2 * C], "d_bias": o["dparams"][2 * C:3 * C],
            "dW_edge": dW.view(C, D), "d_att_edge": dae}
    graph = BondGraph(torch.from_numpy(case.ei).to(dev), n)
    for frozen in (False, True):
        out, grads = _door(case, inp, graph, frozen_bias=frozen)
        assert torch.equal(out.reshape(-1), o["out"][:n * C]), (name, "forward")
        for k, t in grads.items():
            if k == "d_bias" and (frozen or inp["bias"] is None):
                assert t is None, (name, "a frozen or absent bias gets no gradient")
            else:
                assert t is not None and torch.equal(t, want[k]), (name, k, frozen)
    # an ordinary dense dout too
    dout = inp["dout"].to(dev)
    o2 = run_kernels(case, inp, g)
    _, grads = _door(case, inp, graph, dout=dout)
    assert torch.equal(grads["dh"].reshape(-1), o2["dh"][:n * C]) and torch.equal(grads["d_att_dst"], o2["dparams"][C:2 * C])


# ================================================================================================ closing: nothing was left out
def test_zz_every_gat_export_and_branch_was_exercised():
    """The names declared in the covalent section of the header == the names this module called, the Python door reached each of its entry points, and
    every branch of gat_ref.REQUIRED_BRANCHES was taken by at least one case.  (Run the whole module: this test looks at what the tests above did.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "conan_fgw_hip.h")).read()
    sect = text[text.index("covalent (GAT) branch"):]
    declared = set(re.findall(r"^(?:int|long long)\s+(conan_\w+)\s*\(", sect, flags=re.M))
    assert len(declared) == 7 and "conan_bond_graph_csr" in declared, sorted(declared)
    assert all(n.startswith("conan_gat_") for n in declared - {"conan_bond_graph_csr"})
    whole = "this test looks at what the other tests of the module did: run the whole module, in file order, in one process"
    assert declared <= set(_lib.SIGNATURES) and declared <= CALLED, (whole, sorted(declared - CALLED))
    assert declared - {"conan_gat_bwd_ws"} <= TRACED, (whole, sorted(declared - TRACED))       # gat.py asks for the workspace size without call()
    assert G.REQUIRED_BRANCHES <= BRANCHES, (whole, sorted(G.REQUIRED_BRANCHES - BRANCHES))
    assert "scan/global" in BRANCHES, whole
    print("\nbranches taken:", ", ".join(sorted(BRANCHES)))
    print("worst err / yard per output (row, whole tensor):")
    for (what, fam), (rr, ra) in sorted(RATIOS.items()):
        print(f"TABLE {what:11s} {fam:5s} row={rr:6.3g} all={ra:6.3g}")
