"""Every CFConv, filter and stage-2 head kernel on its own against the plain fp64 reference of the same operation (tests/edge_ref.py).

The 24 entry points named in OWNED (cfconv.hip, filter_fused.hip, filter_bwd.hip, filter_bwd2.hip and the stage-2 heads of head.hip) are called as
C entry points (`raw`: the status code is visible) on hand-made graphs — targets of 0 .. 130 edges, atom counts that leave wavefronts idle or make
one walk a second target, pair tables with one-direction pairs at every kind of slot — at the row counts around the tiles and the capped grids, at
every device-side count, on rows of very different magnitude and on non-finite values.  edge_ref's form functions name the path a shape takes;
tests/test_edge_ref_cpu.py asserts that the case lists reach every one.

Judging (visnet_ref.judge, unchanged): per row and per tensor, err(gpu, ref64) <= MARGIN * err(ref32, ref64) — the yardstick is the reference
formula in fp32 on the CPU, never the kernel; where that yardstick is 0 the kernel has to be exact too.  Integer work, rows of targets without
edges and pure masking are exact.  Every output buffer and workspace is pre-filled with a NaN bit pattern and has a tail of 64 floats that must
survive; every float input sits in front of the same pattern, and with a device-side count the rows at and beyond it hold the pattern too, so that
an over-read poisons a result.  Index arrays sit in front of zeros instead (a valid index: no case gives a kernel an index outside its arrays).
Every case runs twice on fresh buffers and must give the same bits; the one exception is conan_filter_cfconv_fwd with a target of more than 33
edges: such a target spans three tiles, its row of `out` receives three float atomic adds whose order is not fixed, and the header promises
reproducible bits for targets of at most 33 edges only — those cases are judged by the margin alone.  (The non-finite cases run once: they are
compared bit for bit with the finite run of the same inputs.)  The `RATIO` / `TABLE` lines printed by a run
(-s) are the source of the table in DESIGN.md section 3.10."""
import pytest
import torch

import edge_ref as E
import visnet_ref as R
from conan_fgw_amd import _lib
from conan_fgw_amd._lib import WgradJob, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
f32, f64, i32 = torch.float32, torch.float64, torch.int32
OK, E_BADARG, E_UNSUPPORTED = 0, -1, -3
SENT, TAIL = 0x7FA5A5A5, 64
CALLED, RATIOS, FORMS = set(), {}, set()
SHARED = (R.MARGIN_ROW, R.MARGIN_ALL)
CUT = E.CUTOFF
# Outputs that need more than the shared margins: output -> (row, whole tensor) = 2 x the ratio measured on the MI355X against the fp32 reference's
# own error.  Measured values and reasons: DESIGN.md section 3.10.
EDGE_MARGIN = {
    # db1 of conan_filter_bwd at M = 32 768 + 33 only: 128 column sums of 32 801 rows each, |sum| ~ 0.7 % of the sum of |terms|, against torch's
    # cascaded column sum (yardstick 2.6e-7).  Measured 7.99 (three bf16 planes) and 5.96 (two fp16 planes), i.e. 2.1e-6 / 1.6e-6 of |sum| and
    # 1.4e-8 of the sum of |terms|; at most 1.1 up to M = 129, and dW1 of the same launch is at 1.8
    "filter_bwd.bf16.db1": (16.0, 16.0),
    "filter_bwd.fp16.db1": (11.9, 11.9),
    # ONE number, the sum of num_molecules values of dout added serially, against torch's vectorised sum: measured 4.33 (17 and 33 molecules);
    # as a one-row tensor it meets the whole-tensor margin of 4, not the row margin of 8
    "head.dbreg": (8.66, 8.66),
}

OWNED = ["conan_cfconv_fwd", "conan_cfconv_bwd_x", "conan_cfconv_bwd_w", "conan_cfconv_bwd_w_pairs", "conan_cfconv_bwd_xw_pairs_supported",
         "conan_cfconv_bwd_xw_pairs",
         "conan_filter_fused_supported", "conan_filter_fwd", "conan_filter_cfconv_fwd_supported", "conan_filter_cfconv_fwd",
         "conan_filter_bwd_supported", "conan_filter_bwd_slices", "conan_filter_bwd_ws", "conan_filter_bwd",
         "conan_filter_bwd2_supported", "conan_filter_bwd2_slices", "conan_filter_bwd2_ws", "conan_filter_bwd2",
         "conan_stage2_head_supported", "conan_stage2_head_fwd", "conan_stage2_head_bwd",
         "conan_stage2_head_sums_supported", "conan_stage2_head_sums_fwd", "conan_stage2_head_sums_bwd"]


def raw(name, *args):
    """The C entry point itself: returns the status code instead of raising."""
    CALLED.add(name)
    return getattr(lib(), name)(*args)


def other(name, *args):
    """An entry point another per-kernel file owns, used here to compose what a fused form is compared with."""
    rc = getattr(lib(), name)(*args)
    assert rc == OK, (name, rc)


def sent(numel):
    return torch.full((numel + TAIL,), SENT, dtype=i32, device=dev).view(f32)


def is_sent(t):
    return bool((t.contiguous().view(i32) == SENT).all())


def put(t, live=None):
    """A CPU float tensor on the device in front of the pattern; rows at and beyond `live` hold the pattern too."""
    t = t.contiguous()
    buf = sent(t.numel())
    if t.numel():
        v = buf[:t.numel()].view(t.shape)
        if live is None:
            v.copy_(t)
        else:
            v[:live].copy_(t[:live])
    return buf


def iput(t):
    """An index array on the device as int32, in front of TAIL zeros (a valid index)."""
    buf = torch.zeros(t.numel() + TAIL, dtype=i32, device=dev)
    buf[:t.numel()].copy_(t.to(i32))
    return buf


def mdev(m):
    return None if m is None else torch.tensor([m], dtype=i32, device=dev)


def slot7():
    """A one-float slot holding 7.0 in front of the pattern."""
    b = sent(1)
    b[0] = 7.0
    return b


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert same_bits(a, b), "two runs differ"
    return a


def take(t, *shape):
    """The documented part of a buffer on the CPU; the tail must still hold the pattern."""
    n = 1
    for s in shape:
        n *= s
    assert is_sent(t[n:]), "written beyond the documented size"
    return t[:n].cpu().view(*shape)


def both(fn, *args):
    """(ref32, ref64): the same formula on the fp32 inputs and on their fp64 copies (CPU); integer tensors and non-tensors pass through."""
    up = lambda a: a.double() if torch.is_tensor(a) and a.is_floating_point() else a
    return fn(*args), fn(*[up(a) for a in args])


def judge(fails, case, what, got, r32, r64):
    assert got.shape == r64.shape, (case, what, got.shape, r64.shape)
    mr, ma = EDGE_MARGIN.get(what, SHARED)
    ok, rr, ra = R.judge(got, r32, r64, mr, ma)
    old = RATIOS.get(what, (0.0, 0.0))
    RATIOS[what] = (max(old[0], rr), max(old[1], ra))
    print(f"RATIO {case} {what} row={rr:.3g} all={ra:.3g} yard={R.all_err(r32, r64):.3g}")
    if not ok:
        fails.append((case, what, float("%.3g" % rr), float("%.3g" % ra)))


def own_norm(a, r64):
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
    if e > EDGE_MARGIN.get(what + "/own", SHARED)[0] * y:
        fails.append((case, what + "/own", float("%.3g" % ratio)))


def nonfinite_rule(case, what, got, ref64, clean, finite_dependents=None):
    """Non-finite wherever the fp64 reference is; every other element keeps the bits it has on the finite input.  finite_dependents: a mask of
    elements that depend on the non-finite input and are finite all the same (they follow the reference instead).  Returns the number of
    non-finite elements of the reference."""
    bad = ~torch.isfinite(ref64)
    assert not bool(torch.isfinite(got[bad]).any()), (case, what, "a non-finite value did not reach an output that depends on it")
    keep = ~bad
    if finite_dependents is not None:
        keep &= ~finite_dependents
        assert torch.allclose(got[finite_dependents].double(), ref64[finite_dependents], rtol=1e-4, atol=1e-6), (case, what)
    same = got[keep].view(i32) == clean[keep].view(i32)
    assert bool(same.all()), (case, what, int((~same).sum()), "elements that do not depend on the non-finite value changed")
    return int(bad.sum())


# ================================================================================================ CFConv
class DevGraph:
    def __init__(self, G):
        self.G = G
        for k in ("rowptr", "col", "tgt", "t_rowptr", "t_eid", "pid", "pe0", "pe1"):
            setattr(self, k, iput(getattr(G, k)))
        self.pdist, self.dist = put(G.pdist), put(G.dist)
        self.P = mdev(G.P)


def cf_inputs(G, F, use_pid, seed, decades=True):
    """x, dout [n, F], W [P or E, F]."""
    x = E.decade_rows(G.n, F, seed) if decades else E.nrows(G.n, F, seed)
    return x, E.nrows(G.n, F, seed + 1), E.nrows(G.P if use_pid else G.E, F, seed + 2)


def cf_chain(gd, F, x, W, dout, use_pid, use_slot):
    """fwd, bwd_x (+ bwd_w_pairs and the one-launch bwd_xw_pairs where a pair table is used), on fresh buffers: a dict of device buffers."""
    G, s = gd.G, stream_ptr()
    n = G.n
    xd, Wd, dd = put(x), put(W), put(dout)
    pid = gd.pid if use_pid else None
    o = {"out": sent(n * F), "dx": sent(n * F), "slot_f": slot7(), "slot_b": slot7()}
    rc = raw("conan_cfconv_fwd", ptr(xd), ptr(Wd), ptr(gd.rowptr), ptr(gd.col), ptr(pid), n, F, ptr(o["out"]), ptr(o["slot_f"]) if use_slot else None, s)
    assert rc == OK, rc
    rc = raw("conan_cfconv_bwd_x", ptr(Wd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt), ptr(pid), n, F, ptr(o["dx"]),
             ptr(o["slot_b"]) if use_slot else None, s)
    assert rc == OK, rc
    if use_pid and G.P:
        gm = use_slot and F == 128
        o["dWp"] = sent(G.P * F)
        rc = raw("conan_cfconv_bwd_w_pairs", ptr(xd), ptr(dd), ptr(gd.P), G.P, ptr(gd.pe0), ptr(gd.pe1), ptr(gd.col), ptr(gd.tgt), F, ptr(gd.pdist), CUT,
                 ptr(o["dWp"]), ptr(o["slot_b"]) if gm else None, s)
        assert rc == OK, rc
        if F == 128:
            o["dx1"], o["dWp1"] = sent(n * F), sent(G.P * F)
            rc = raw("conan_cfconv_bwd_xw_pairs", ptr(Wd), ptr(xd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt), ptr(gd.pid), ptr(gd.pe0),
                     ptr(gd.pe1), ptr(gd.pdist), CUT, n, F, ptr(o["dx1"]), ptr(o["dWp1"]), ptr(o["slot_f"]) if gm else None, s)
            assert rc == OK, rc
    return o


def cf_check(fails, case, G, F, o, x, W, dout, use_pid, use_slot, own=True):
    n, pid = G.n, G.pid if use_pid else None
    FORMS.update({E.cfconv_form("fwd", n, F), E.cfconv_form("bwd_x", n, F)})
    out, dx = take(o["out"], n, F), take(o["dx"], n, F)
    deg, sdeg = G.degrees()
    assert not bool(out[torch.tensor(deg) == 0].any()) and not bool(dx[torch.tensor(sdeg) == 0].any()), (case, "a row without edges is not exactly zero")
    r32, r64 = both(E.cfconv_fwd, x, W, G.col, G.tgt, pid, n)
    judge(fails, case, f"cfconv.fwd.{F if F in (128, 256) else 'generic'}", out, r32, r64)
    r32, r64 = both(E.cfconv_bwd_x, W, dout, G.col, G.tgt, pid, n)
    judge(fails, case, f"cfconv.bwd_x.{F if F == 128 else 'generic'}", dx, r32, r64)
    if "dWp" in o:
        FORMS.add(E.bwd_wp_form(G.P, F, use_slot and F == 128))
        dWp = take(o["dWp"], G.P, F)
        r32, r64 = both(E.cfconv_bwd_w_pairs, x, dout, G.col, G.tgt, G.pe0, G.pe1, G.pdist)
        what = f"cfconv.bwd_wp.{F if F == 128 else 'generic'}"
        judge(fails, case, what, dWp, r32, r64)
        if own:
            judge_own(fails, case, what, dWp, r32, r64)
        if F == 128:
            FORMS.add(E.cfconv_form("bwd_xw", n, F))
            assert torch.equal(take(o["dx1"], n, F).view(i32), dx.view(i32)), (case, "dx of the one-launch backward is not conan_cfconv_bwd_x's")
            assert torch.equal(take(o["dWp1"], G.P, F).view(i32), dWp.view(i32)), (case, "dWp of the one-launch backward is not conan_cfconv_bwd_w_pairs'")
    sf, sb = take(o["slot_f"], 1), take(o["slot_b"], 1)
    if not use_slot:
        assert float(sf) == 7.0 and float(sb) == 7.0
    elif "dWp" in o and F == 128:
        want = dWp.abs().max().view(1)
        assert torch.equal(sb.view(i32), want.view(i32)), (case, "gmax after bwd_x + bwd_w_pairs is not max |dWp|", float(sb), float(want))
        assert torch.equal(sf.view(i32), want.view(i32)), (case, "gmax after fwd + bwd_xw_pairs is not max |dWp|", float(sf), float(want))
    else:
        assert float(sf) == 0.0 and float(sb) == 0.0, (case, "zero_slot was not cleared")


def cf_case(fails, case, G, gd, F, use_pid, use_slot, seed):
    x, dout, W = cf_inputs(G, F, use_pid, seed)
    o = twice(lambda: cf_chain(gd, F, x, W, dout, use_pid, use_slot))
    cf_check(fails, case, G, F, o, x, W, dout, use_pid, use_slot)


@pytest.mark.parametrize("F", [128, 256, 4, 32, 132])
def test_cfconv_every_degree(F):
    """Degrees {0, 1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130} by target (the graph) and by source (the reversed graph) in one graph of 140 atoms:
    the 8-edge step with its masked tail, the second and third 64-wide index hand-out.  pid NULL / given, zero_slot NULL / given.  At 128 the
    one-launch backward gives the bits of the two-kernel path in dx, dWp and gmax."""
    fails = []
    for tag, G in (("deg", E.degree_graph()), ("rev", E.degree_graph().reversed())):
        gd = DevGraph(G)
        for use_pid, use_slot in ((True, True), (False, False)) + (((True, False), (False, True)) if F in (128, 4) else ()):
            cf_case(fails, f"{tag}/F{F}/pid{int(use_pid)}/slot{int(use_slot)}", G, gd, F, use_pid, use_slot, 7 * F)
    assert not fails, fails


@pytest.mark.parametrize("n", E.SMALL_N)
def test_cfconv_atom_counts_with_idle_wavefronts(n):
    """num_atoms in {1, 2, 4, 5, 12, 33, 100}: grid = round_up8(ceil(n / 4)) leaves whole workgroups and single wavefronts without a target,
    per = 1 .. 4 targets per workgroup."""
    fails, G = [], E.small_graph(n)
    gd = DevGraph(G)
    for F in (128, 256, 32):
        cf_case(fails, f"n{n}/F{F}", G, gd, F, True, True, n + F)
    assert not fails, fails


@pytest.mark.parametrize("F", [128, 4])
def test_cfconv_beyond_the_block_cap(F):
    """num_atoms > 4 x 65 536: the block cap gives per = 5 and a wavefront walks a second target.  All but 300 atoms (spread over the range, its
    last three among them) have no edge either way: their rows are exactly zero, checked on the device; the others are judged on a compact copy
    of the graph."""
    G = E.big_graph()
    assert E.cfconv_per(G.n) == 5
    gd, fails = DevGraph(G), []
    used = torch.unique(torch.cat([G.col, G.tgt]))
    x, dout = torch.zeros(G.n, F), torch.zeros(G.n, F)
    x[used], dout[used] = E.nrows(len(used), F, 1), E.nrows(len(used), F, 2)
    W = E.nrows(G.P, F, 3)
    o = twice(lambda: cf_chain(gd, F, x, W, dout, True, True))
    torch.cuda.synchronize()
    live = torch.zeros(G.n, dtype=torch.bool)
    live[used] = True
    for k in ("out", "dx") + (("dx1",) if F == 128 else ()):
        assert is_sent(o[k][G.n * F:]), k
        v = o[k][:G.n * F].view(G.n, F)
        assert not bool(v[~live.to(dev)].any()), (k, "a row without edges is not exactly zero")
    relabel = lambda t: torch.searchsorted(used, t)
    col, tgt = relabel(G.col), relabel(G.tgt)
    nc, xc, dc = len(used), x[used], dout[used]
    r32, r64 = both(E.cfconv_fwd, xc, W, col, tgt, G.pid, nc)
    judge(fails, f"big/F{F}", f"cfconv.fwd.{F if F == 128 else 'generic'}", o["out"][:G.n * F].view(G.n, F)[used.to(dev)].cpu(), r32, r64)
    r32, r64 = both(E.cfconv_bwd_x, W, dc, col, tgt, G.pid, nc)
    dx = o["dx"][:G.n * F].view(G.n, F)[used.to(dev)].cpu()
    judge(fails, f"big/F{F}", f"cfconv.bwd_x.{F if F == 128 else 'generic'}", dx, r32, r64)
    dWp = take(o["dWp"], G.P, F)
    r32, r64 = both(E.cfconv_bwd_w_pairs, xc, dc, col, tgt, G.pe0, G.pe1, G.pdist)
    judge(fails, f"big/F{F}", f"cfconv.bwd_wp.{F if F == 128 else 'generic'}", dWp, r32, r64)
    if F == 128:
        assert torch.equal(o["dx1"][:G.n * F].view(i32), o["dx"][:G.n * F].view(i32)) and torch.equal(take(o["dWp1"], G.P, F).view(i32), dWp.view(i32))
        want = dWp.abs().max().view(1)
        assert torch.equal(take(o["slot_b"], 1).view(i32), want.view(i32)) and torch.equal(take(o["slot_f"], 1).view(i32), want.view(i32))
    assert not fails, fails


def test_cfconv_no_atoms_and_status_codes():
    """num_atoms = 0: OK, every buffer untouched, zero_slot cleared all the same.  The argument checks the host code answers before any launch."""
    G = E.small_graph(12)
    gd, s = DevGraph(G), stream_ptr()
    x, dout, W = cf_inputs(G, 128, True, 3)
    xd, Wd, dd, out, dx, dWp, z = put(x), put(W), put(dout), sent(12 * 128), sent(12 * 128), sent(G.P * 128), slot7()
    fwd = lambda *a: raw("conan_cfconv_fwd", *a)
    bx = lambda *a: raw("conan_cfconv_bwd_x", *a)
    for F in (128, 256, 4):
        assert E.cfconv_form("fwd", 0, F) == "none"
        z[0] = 7.0
        assert fwd(ptr(xd), ptr(Wd), ptr(gd.rowptr), ptr(gd.col), ptr(gd.pid), 0, F, ptr(out), ptr(z), s) == OK
        torch.cuda.synchronize()
        assert float(z[0]) == 0.0 and is_sent(z[1:])
        z[0] = 7.0
        assert bx(ptr(Wd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt), ptr(gd.pid), 0, F, ptr(dx), ptr(z), s) == OK
        torch.cuda.synchronize()
        assert float(z[0]) == 0.0 and is_sent(z[1:])
    FORMS.add("none")
    z[0] = 7.0
    xw = lambda n, F, W_=Wd, dx_=dx: raw("conan_cfconv_bwd_xw_pairs", ptr(W_), ptr(xd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt), ptr(gd.pid),
                                        ptr(gd.pe0), ptr(gd.pe1), ptr(gd.pdist), CUT, n, F, ptr(dx_), ptr(dWp), ptr(z), s)
    assert xw(0, 128) == OK and xw(-1, 128) == E_BADARG and xw(12, 256) == E_UNSUPPORTED and xw(12, 32) == E_UNSUPPORTED
    assert xw(12, 128, None) == E_BADARG and xw(12, 128, Wd, None) == E_BADARG
    for F in (128, 256, 32, 4, 132, 0, -4):
        assert raw("conan_cfconv_bwd_xw_pairs_supported", F) == int(F == 128) == int(E.cfconv_form("bwd_xw", 1, F) == "bwd_xw128")
    for bad in (dict(n=-1), dict(F=0), dict(F=-4), dict(F=130), dict(F=2)):
        n, F = bad.get("n", 12), bad.get("F", 128)
        assert E.cfconv_form("fwd", n, F) == "badarg"
        assert fwd(ptr(xd), ptr(Wd), ptr(gd.rowptr), ptr(gd.col), ptr(gd.pid), n, F, ptr(out), ptr(z), s) == E_BADARG
        assert bx(ptr(Wd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt), ptr(gd.pid), n, F, ptr(dx), ptr(z), s) == E_BADARG
    for k in range(4):                                                     # a NULL x / W / rowptr / col
        a = [ptr(xd), ptr(Wd), ptr(gd.rowptr), ptr(gd.col)]
        a[k] = None
        assert fwd(*a, ptr(gd.pid), 12, 128, ptr(out), ptr(z), s) == E_BADARG
    assert fwd(ptr(xd), ptr(Wd), ptr(gd.rowptr), ptr(gd.col), ptr(gd.pid), 12, 128, None, ptr(z), s) == E_BADARG
    for k in range(5):
        a = [ptr(Wd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt)]
        a[k] = None
        assert bx(*a, ptr(gd.pid), 12, 128, ptr(dx), ptr(z), s) == E_BADARG
    assert bx(ptr(Wd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt), ptr(gd.pid), 12, 128, None, ptr(z), s) == E_BADARG
    bw = lambda E_, F, x_=xd, dW_=dWp: raw("conan_cfconv_bwd_w", ptr(x_), ptr(dd), None, E_, ptr(gd.col), ptr(gd.tgt), F, None, CUT, ptr(dW_), s)
    assert bw(0, 128) == OK and bw(-1, 128) == E_BADARG and bw(4, 130) == E_BADARG and bw(4, 0) == E_BADARG and bw(4, 128, None) == E_BADARG
    assert bw(4, 128, xd, None) == E_BADARG
    wp = lambda P, F, np_=gd.P, gm=None: raw("conan_cfconv_bwd_w_pairs", ptr(xd), ptr(dd), ptr(np_), P, ptr(gd.pe0), ptr(gd.pe1), ptr(gd.col), ptr(gd.tgt), F,
                                             ptr(gd.pdist), CUT, ptr(dWp), ptr(gm), s)
    assert wp(0, 128) == OK and wp(-1, 128) == E_BADARG and wp(4, 130) == E_BADARG and wp(4, 128, None) == E_BADARG
    for F in (32, 256):
        assert E.bwd_wp_form(4, F, True) == "unsupported"
        assert wp(4, F, gd.P, z) == E_UNSUPPORTED                           # gmax at a width other than 128
    torch.cuda.synchronize()
    assert is_sent(out) and is_sent(dx) and is_sent(dWp) and float(z[0]) == 7.0 and is_sent(z[1:])


BWD_W_GRAPH = None


@pytest.mark.parametrize("F", [4, 128, 256])
def test_cfconv_bwd_w(F):
    """dW[e] = x[col[e]] dout[tgt[e]] (x C(d_e) with dist): *num_edges_dev in {NULL, 0, 1, 33, E, E + 5}, dist NULL and given; at F = 256 one graph of
    16 500 edges, E F / 4 > 4096 x 256: the grid-stride loop runs twice.  Rows at and beyond the count keep the pattern."""
    fails, s = [], stream_ptr()
    graphs = [("deg", E.degree_graph())] + ([("two-pass", E.graph_by_degrees(300, [55] * 300, 9))] if F == 256 else [])
    for tag, G in graphs:
        passes = E.bwd_w_passes(G.E, F)
        assert passes == (2 if tag == "two-pass" else 1)
        FORMS.add(f"bwd_w/{passes}")
        gd = DevGraph(G)
        x, dout, _ = cf_inputs(G, F, False, 5 + F)
        xd, dd = put(x), put(dout)
        for cnt in (E.counts(G.E) if tag == "deg" else [None]):
            live = G.E if cnt is None else min(cnt, G.E)
            for with_dist in (False, True):
                dist = put(G.dist, live) if with_dist else None
                o = twice(lambda: {"dW": _bwd_w(xd, dd, mdev(cnt), G.E, gd, F, dist, s)})
                assert is_sent(o["dW"][live * F:]), "rows at or beyond the count were written"
                if live:
                    r32, r64 = both(E.cfconv_bwd_w, x, dout, G.col[:live], G.tgt[:live], G.dist[:live] if with_dist else None)
                    got = o["dW"][:live * F].cpu().view(live, F)
                    judge(fails, f"{tag}/F{F}/cnt{cnt}/dist{int(with_dist)}", "cfconv.bwd_w", got, r32, r64)
                    judge_own(fails, f"{tag}/F{F}/cnt{cnt}/dist{int(with_dist)}", "cfconv.bwd_w", got, r32, r64)
    assert not fails, fails


def _bwd_w(xd, dd, cnt, Emax, gd, F, dist, s):
    dW = sent(Emax * F)
    assert raw("conan_cfconv_bwd_w", ptr(xd), ptr(dd), ptr(cnt), Emax, ptr(gd.col), ptr(gd.tgt), F, ptr(dist), CUT, ptr(dW), s) == OK
    return dW


@pytest.mark.parametrize("P", E.PAIR_P)
def test_cfconv_bwd_w_pairs(P):
    """P in {1, 2, 3, 63, 64, 65, 255, 257} pairs, one-direction pairs at slot 0, at the last slot of every 64-group and elsewhere; *num_pairs_dev in
    {0, 1, P, P + 5}; width 128 (k_cfconv_bwd_wp128, with gmax cleared by the preceding conan_cfconv_bwd_x) and 32 / 256 (k_cfconv_bwd_wp)."""
    fails, s, G = [], stream_ptr(), E.pair_graph(P, P)
    gd = DevGraph(G)
    assert bool((G.pe1 < 0).any()) and (P < 3 or bool((G.pe1 >= 0).any()))
    for F in (128, 32, 256):
        x, dout, W = cf_inputs(G, F, True, P + F)
        xd, dd, Wd = put(x), put(dout), put(W)
        for cnt in (0, 1, P, P + 5):
            live = min(cnt, P)
            pdist = put(G.pdist, live)

            def run():
                o = {"dWp": sent(P * F), "dx": sent(G.n * F), "gmax": slot7()}
                assert raw("conan_cfconv_bwd_x", ptr(Wd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt), ptr(gd.pid), G.n, F, ptr(o["dx"]), ptr(o["gmax"]), s) == OK
                assert raw("conan_cfconv_bwd_w_pairs", ptr(xd), ptr(dd), ptr(mdev(cnt)), P, ptr(gd.pe0), ptr(gd.pe1), ptr(gd.col), ptr(gd.tgt), F, ptr(pdist), CUT,
                           ptr(o["dWp"]), ptr(o["gmax"]) if F == 128 else None, s) == OK
                return o
            o = twice(run)
            FORMS.add(E.bwd_wp_form(P, F, F == 128))
            assert is_sent(o["dWp"][live * F:]), "pair rows at or beyond the count were written"
            gmax = take(o["gmax"], 1)
            if not live:
                assert float(gmax) == 0.0
                continue
            got = o["dWp"][:live * F].cpu().view(live, F)
            r32, r64 = both(E.cfconv_bwd_w_pairs, x, dout, G.col, G.tgt, G.pe0[:live], G.pe1[:live], G.pdist[:live])
            what = f"cfconv.bwd_wp.{F if F == 128 else 'generic'}"
            judge(fails, f"P{P}/F{F}/cnt{cnt}", what, got, r32, r64)
            judge_own(fails, f"P{P}/F{F}/cnt{cnt}", what, got, r32, r64)
            if F == 128:
                assert torch.equal(gmax.view(i32), got.abs().max().view(1).view(i32)), "gmax is not max |dWp| over the live pairs"
    assert not fails, fails


def test_cfconv_bwd_w_pairs_many_pairs():
    """P = 4096 x 65 + 7: a workgroup of k_cfconv_bwd_wp128 gets 66 contiguous pairs — wavefront 0 a full 64-wide hand-out, wavefront 1 a group of two
    with the masked tail step (up to 257 pairs every workgroup has ONE pair).  Every row is written (on the device: finite), gmax is max |dWp| of
    all rows bit for bit, 4000 sampled rows and the last 200 are judged."""
    fails, s, G = [], stream_ptr(), E.many_pairs_graph()
    gd, P, F = DevGraph(G), G.P, 128
    FORMS.add(f"wp128/per{E.wp_per(P)}")
    x, dout, W = E.nrows(G.n, F, 1), E.nrows(G.n, F, 2), E.nrows(8, F, 3)
    xd, dd, Wd, pid0 = put(x), put(dout), put(W), iput(G.pid % 8)                # bwd_x only clears the slot here: its W rows come from a table of 8

    def run():
        o = {"dWp": sent(P * F), "dx": sent(G.n * F), "gmax": slot7()}
        assert raw("conan_cfconv_bwd_x", ptr(Wd), ptr(dd), ptr(gd.t_rowptr), ptr(gd.t_eid), ptr(gd.tgt), ptr(pid0), G.n, F, ptr(o["dx"]), ptr(o["gmax"]), s) == OK
        assert raw("conan_cfconv_bwd_w_pairs", ptr(xd), ptr(dd), ptr(gd.P), P, ptr(gd.pe0), ptr(gd.pe1), ptr(gd.col), ptr(gd.tgt), F, ptr(gd.pdist), CUT,
                   ptr(o["dWp"]), ptr(o["gmax"]), s) == OK
        return o
    o = twice(run)
    rows = o["dWp"][:P * F].view(P, F)
    assert is_sent(o["dWp"][P * F:]) and bool(torch.isfinite(rows).all()), "a pair row was not written"
    assert torch.equal(take(o["gmax"], 1).view(i32), rows.abs().max().view(1).cpu().view(i32)), "gmax is not max |dWp|"
    sel = torch.cat([torch.randperm(P - 200, generator=E.gen(4))[:4000].sort().values, torch.arange(P - 200, P)])
    r32, r64 = both(E.cfconv_bwd_w_pairs, x, dout, G.col, G.tgt, G.pe0[sel], G.pe1[sel], G.pdist[sel])
    judge(fails, "many", "cfconv.bwd_wp.128", rows[sel.to(dev)].cpu(), r32, r64)
    assert not fails, fails


def _poison(t, r, c, v):
    t = t.clone()
    if c is None:
        t[r] = v
    else:
        t[r, c] = v
    return t


@pytest.mark.parametrize("F", [128, 32])
def test_cfconv_non_finite_values_reach_what_depends_on_them_and_nothing_else(F):
    """One NaN and one +Inf in one element of x, of dout, in one filter row, in x[0] / dout[0] with one-direction pairs present, and in x[target]
    / dout[source] of a one-direction pair (rows that pair's gradient does not depend on): every output is non-finite exactly where the fp64
    reference is and keeps the bits of the finite run everywhere else — in both forms of the backward."""
    G = E.degree_graph()
    gd = DevGraph(G)
    x, dout, W = cf_inputs(G, F, True, 77, decades=False)
    clean = {k: v.cpu() for k, v in cf_chain(gd, F, x, W, dout, True, False).items()}
    one = int((G.pe1 < 0).nonzero()[5])                         # a one-direction pair: its gradient is C x[j] dout[t]
    j, t = int(G.col[G.pe0[one]]), int(G.tgt[G.pe0[one]])
    assert j != 0 and t != 0
    places = [("x", 3, 5), ("dout", 9, 6), ("W", 40, None), ("x", 0, None), ("dout", 0, None), ("x", t, None), ("dout", j, None)]
    for which, r, c in places:
        for v in (E.NAN, E.INF):
            xs, ds, Ws = (_poison(a, r, c, v) if which == k else a for k, a in (("x", x), ("dout", dout), ("W", W)))
            o = cf_chain(gd, F, xs, Ws, ds, True, False)
            case = f"F{F}/{which}[{r},{c}]={v}"
            n, P = G.n, G.P
            refs = {"out": E.cfconv_fwd(xs.double(), Ws.double(), G.col, G.tgt, G.pid, n), "dx": E.cfconv_bwd_x(Ws.double(), ds.double(), G.col, G.tgt, G.pid, n),
                    "dWp": E.cfconv_bwd_w_pairs(xs.double(), ds.double(), G.col, G.tgt, G.pe0, G.pe1, G.pdist.double())}
            refs["dx1"], refs["dWp1"] = refs["dx"], refs["dWp"]
            hit = 0
            for k, ref in refs.items():
                if k in o:
                    rows = P if k.startswith("dWp") else n
                    hit += nonfinite_rule(case, k, take(o[k], rows, F), ref, clean[k][:rows * F].view(rows, F))
            assert hit or r in (0, t, j), (case, "the case poisons nothing")      # (row 0 has no edge as a target: nothing depends on dout[0])


# ================================================================================================ filter generator
def filt_run(dist, cnt, Emax, offset, coeff, F, w, want_h1):
    """conan_filter_fwd on fresh buffers; dist rows at and beyond the count hold the pattern."""
    Gs, s = offset.numel(), stream_ptr()
    live = Emax if cnt is None else min(cnt, Emax)
    dd, od, wd = put(dist, live), put(offset), [put(t) for t in w]

    def run():
        o = {"W": sent(Emax * F)}
        if want_h1:
            o["h1"] = sent(Emax * F)
        rc = raw("conan_filter_fwd", ptr(dd), ptr(mdev(cnt)), Emax, ptr(od), Gs, coeff, CUT, F, *[ptr(t) for t in wd], ptr(o["W"]), ptr(o.get("h1")), s)
        assert rc == OK, rc
        return o
    return twice(run), live


def filt_check(fails, case, o, live, dist, offset, coeff, F, w):
    for k in o:
        assert is_sent(o[k][live * F:]), (case, k, "rows at or beyond the count were written")
    if not live:
        return
    (W32, h32), (W64, h64) = both(lambda d, of, *ws: E.filter_fwd(d, of, coeff, CUT, *ws), dist[:live], offset, *w)
    judge(fails, case, f"filter.fwd.W/F{F}", o["W"][:live * F].cpu().view(live, F), W32, W64)
    if "h1" in o:
        judge(fails, case, f"filter.fwd.h1/F{F}", o["h1"][:live * F].cpu().view(live, F), h32, h64)


@pytest.mark.parametrize("F", E.FILTER_F)
def test_filter_fwd(F):
    """F in {32, 64, 128} x Gs in {2, 10, 50, 64} x E in {1, 31, 32, 33, 255, 257}, h1_out NULL and given, distances at 0, at the cutoff and beyond
    it; every device-side count at E = 70; at Gs = 50 the second pass of the 256 x 8-tile round-robin (E = 65 536 + 33)."""
    fails = []
    for Gs in E.FILTER_GS:
        assert raw("conan_filter_fused_supported", Gs, F) == 1 == int(E.filter_fused_supported(Gs, F))
        offset, coeff = E.gaussians(Gs)
        w = E.filter_weights(Gs, F, Gs + F)
        for k, Ecnt in enumerate(E.FILTER_E + ([E.FILTER_E_SECOND_PASS] if Gs == 50 else [])):
            dist = E.distances(Ecnt, Ecnt)
            o, live = filt_run(dist, None, Ecnt, offset, coeff, F, w, k % 2 == 0 or Ecnt > 1000)
            FORMS.add(f"filter_fwd/pass{E.filter_fwd_passes(Ecnt)}")
            filt_check(fails, f"F{F}/Gs{Gs}/E{Ecnt}", o, live, dist, offset, coeff, F, w)
        dist = E.distances(70, 70)
        for cnt in E.counts(70):
            o, live = filt_run(dist, cnt, 70, offset, coeff, F, w, True)
            filt_check(fails, f"F{F}/Gs{Gs}/cnt{cnt}", o, live, dist, offset, coeff, F, w)
    assert not fails, fails


def test_filter_fwd_supported_bounds_and_status_codes():
    s = stream_ptr()
    for Gs in (0, 1, 2, 63, 64, 65):
        for F in (0, 16, 32, 64, 96, 128, 256):
            assert raw("conan_filter_fused_supported", Gs, F) == int(E.filter_fused_supported(Gs, F)), (Gs, F)
            assert raw("conan_filter_cfconv_fwd_supported", Gs, F) == int(E.filter_cfconv_supported(Gs, F)), (Gs, F)
    offset, coeff = E.gaussians(10)
    w = [put(t) for t in E.filter_weights(10, 128, 1)]
    dd, od, W, h1 = put(E.distances(8, 1)), put(offset), sent(8 * 128), sent(8 * 128)
    ff = lambda dist, Emax, Gs, F, Wo=W: raw("conan_filter_fwd", ptr(dist), None, Emax, ptr(od), Gs, coeff, CUT, F, *[ptr(t) for t in w], ptr(Wo), ptr(h1), s)
    assert ff(dd, 0, 10, 128) == OK and ff(None, 8, 10, 128) == E_BADARG and ff(dd, -1, 10, 128) == E_BADARG and ff(dd, 8, 10, 128, None) == E_BADARG
    assert ff(dd, 8, 1, 128) == E_UNSUPPORTED and ff(dd, 8, 65, 128) == E_UNSUPPORTED and ff(dd, 8, 10, 96) == E_UNSUPPORTED
    xd, ci, out = put(E.nrows(4, 128, 2)), iput(torch.zeros(8, dtype=torch.int64)), sent(4 * 128)
    cf = lambda x_, Emax, Gs, F, n: raw("conan_filter_cfconv_fwd", ptr(x_), ptr(dd), ptr(ci), ptr(ci), None, Emax, ptr(od), Gs, coeff, CUT, F, *[ptr(t) for t in w], n,
                                       ptr(out), s)
    assert cf(None, 8, 10, 128, 4) == E_BADARG and cf(xd, -1, 10, 128, 4) == E_BADARG and cf(xd, 8, 10, 128, -1) == E_BADARG
    assert cf(xd, 8, 10, 64, 4) == E_UNSUPPORTED and cf(xd, 8, 65, 128, 4) == E_UNSUPPORTED and cf(xd, 8, 10, 128, 0) == OK
    torch.cuda.synchronize()
    assert is_sent(W) and is_sent(h1) and is_sent(out)
    assert cf(xd, 0, 10, 128, 4) == OK                                     # max_edges = 0: a zeroed out
    torch.cuda.synchronize()
    assert not bool(out[:4 * 128].any()) and is_sent(out[4 * 128:])


def test_filter_fwd_weight_scales_and_non_finite_distances():
    """Weights at 1e-4, 1 and 300 times their usual size and an all-zero w1 (h1 = ssp(b1) in every row); one NaN and one +Inf distance: the
    row of that edge is non-finite as in the fp64 reference, every other row keeps its bits."""
    fails, F, Gs, Ecnt = [], 128, 50, 257
    offset, coeff = E.gaussians(Gs)
    dist = E.distances(Ecnt, 5)
    for scale in E.FILTER_W_SCALES:
        w = E.filter_weights(Gs, F, 9, scale)
        o, live = filt_run(dist, None, Ecnt, offset, coeff, F, w, True)
        filt_check(fails, f"w{scale:g}", o, live, dist, offset, coeff, F, w)
    w = E.filter_weights(Gs, F, 9)
    w0 = (torch.zeros_like(w[0]),) + tuple(w[1:])
    o, live = filt_run(dist, None, Ecnt, offset, coeff, F, w0, True)
    filt_check(fails, "w1=0", o, live, dist, offset, coeff, F, w0)
    h1 = o["h1"][:Ecnt * F].cpu().view(Ecnt, F)
    assert bool((h1 == h1[0]).all()), "an all-zero w1: every row of h1 is the same ssp(b1)"
    clean, _ = filt_run(dist, None, Ecnt, offset, coeff, F, w, True)
    for v in (E.NAN, E.INF):
        db = dist.clone()
        db[100] = v
        o, _ = filt_run(db, None, Ecnt, offset, coeff, F, w, True)
        W64, h64 = E.filter_fwd(db.double(), offset.double(), coeff, CUT, *[t.double() for t in w])
        dep = torch.zeros(Ecnt, F, dtype=torch.bool)
        dep[100] = True                                                      # h1 of an edge at +Inf is ssp(b1): finite, and not what it was
        assert nonfinite_rule(f"dist={v}", "W", take(o["W"], Ecnt, F), W64, clean["W"][:Ecnt * F].cpu().view(Ecnt, F)) == F
        nonfinite_rule(f"dist={v}", "h1", take(o["h1"], Ecnt, F), h64, clean["h1"][:Ecnt * F].cpu().view(Ecnt, F), dep & torch.isfinite(h64))
    assert not fails, fails


# ================================================================================================ fused generator + gather
def cf_fused_run(x, dist, col, tgt, cnt, Emax, n, offset, coeff, w, again):
    Gs, s = offset.numel(), stream_ptr()
    live = Emax if cnt is None else min(cnt, Emax)
    xd, dd, cd, td, od, wd = put(x), put(dist, live), iput(col), iput(tgt), put(offset), [put(t) for t in w]

    def run():
        o = {"out": sent(n * 128)}
        rc = raw("conan_filter_cfconv_fwd", ptr(xd), ptr(dd), ptr(cd), ptr(td), ptr(mdev(cnt)), Emax, ptr(od), Gs, coeff, CUT, 128, *[ptr(t) for t in wd], n,
                 ptr(o["out"]), s)
        assert rc == OK, rc
        return o
    return (twice(run) if again else run()), live


@pytest.mark.parametrize("Ecnt", E.CF_E)
def test_filter_cfconv_fwd(Ecnt):
    """out = CFConv gather of the generated filter, E in {1, 32, 33, 8192 + 40, 65 536 + 33} (per_wg >= 2 tiles, a wavefront's second tile): targets
    without edges stay exactly zero, segments end and start at every position around rows 15|16 and 31|0 of a tile.  With every target at <= 33
    edges the run is repeated and must give the same bits; with one target of 70 edges (three tiles) it is judged by the margin only."""
    fails = []
    for Gs in (E.FILTER_GS if Ecnt < 1000 else [50]):
        offset, coeff = E.gaussians(Gs)
        w = E.filter_weights(Gs, 128, Gs)
        for big in (33, 70):
            tgt, n = E.segment_graph(Ecnt, Ecnt + big, big)
            assert tgt.numel() == Ecnt
            deg = torch.bincount(tgt, minlength=n)
            assert bool((deg == 0).any()) and (Ecnt < 1000 or int(deg.max()) == max(big, 33))
            col = torch.randint(0, n, (Ecnt,), generator=E.gen(Ecnt))
            x, dist = E.nrows(n, 128, Ecnt + 1), E.distances(Ecnt, Ecnt + 2)
            for cnt in (E.counts(Ecnt) if (Gs == 50 and Ecnt in (33, 8192 + 40) and big == 33) else [None]):
                o, live = cf_fused_run(x, dist, col, tgt, cnt, Ecnt, n, offset, coeff, w, again=int(deg.max()) <= 33)
                FORMS.add(f"filter_cf/per_wg{min(E.filter_cf_per_wg(live), 9)}")
                out = take(o["out"], n, 128)
                dl = torch.bincount(tgt[:live], minlength=n)
                assert not bool(out[dl == 0].any()), "a target without (live) edges is not exactly zero"
                if live:
                    r32, r64 = both(lambda x_, d_, of_, *ws: E.filter_cfconv_fwd(x_, d_, col[:live], tgt[:live], n, of_, coeff, CUT, *ws), x, dist[:live], offset, *w)
                    judge(fails, f"E{Ecnt}/Gs{Gs}/big{big}/cnt{cnt}", "filter_cfconv.out", out, r32, r64)
    assert not fails, fails


# ================================================================================================ filter-network backwards
def reduce_jobs(specs):
    jobs = (WgradJob * len(specs))(*[WgradJob(ws, dW.data_ptr(), db.data_ptr(), M, K, N, sl) for ws, dW, db, M, K, N, sl in specs])
    other("conan_wgrad_reduce_batch", jobs, len(specs), stream_ptr())


def fb_run(which, g, h1, dist, M, cnt, offset, coeff, w2, gmax, slabs=False):
    """conan_filter_bwd (which = 1) or conan_filter_bwd2 (2) on fresh buffers; rows at and beyond the count hold the pattern.  slabs: the
    deferred form, reduced by conan_wgrad_reduce_batch."""
    Gs, F, s = offset.numel(), 128, stream_ptr()
    live = M if cnt is None else min(cnt, M)
    gd, hd, dd, od, wd = put(g, live), put(h1, live), put(dist, live), put(offset), put(w2)
    gm = None if gmax is None else torch.tensor([gmax], dtype=f32, device=dev)
    name = "conan_filter_bwd" if which == 1 else "conan_filter_bwd2"
    sl, wsn = raw(name + "_slices", M), raw(name + "_ws", M, Gs, F)
    assert sl == (E.filter_bwd_slices(M) if which == 1 else E.filter_bwd2_slices(M)) and wsn == (E.filter_bwd_ws if which == 1 else E.filter_bwd2_ws)(M, Gs, F)

    def run():
        o = {"dW1": sent(F * Gs), "db1": sent(F), "ws": sent(wsn)}
        if which == 2:
            o["dW2"], o["db2"] = sent(F * F), sent(F)
        outs = [None if slabs else ptr(o[k]) for k in (("dW1", "db1") if which == 1 else ("dW1", "db1", "dW2", "db2"))]
        if which == 1:
            rc = raw(name, ptr(gd), ptr(hd), ptr(dd), M, ptr(od), Gs, coeff, ptr(wd), F, ptr(mdev(cnt)), *outs, ptr(o["ws"]), ptr(gm), s)
        else:
            rc = raw(name, ptr(gd), ptr(hd), ptr(dd), M, ptr(od), Gs, coeff, ptr(wd), F, ptr(mdev(cnt)), ptr(gm), *outs, ptr(o["ws"]), s)
        assert rc == OK, rc
        if slabs:
            jobs = [(o["ws"].data_ptr(), o["dW1"], o["db1"], M, Gs, F, sl)]
            if which == 2:
                jobs.append((o["ws"].data_ptr() + 4 * sl * (F * Gs + F), o["dW2"], o["db2"], M, F, F, sl))
            reduce_jobs(jobs)
        return o
    return twice(run), live


def fb_check(fails, case, which, form, o, live, g, h1, dist, offset, coeff, w2):
    Gs, F = offset.numel(), 128
    names = ("dW1", "db1") + (("dW2", "db2") if which == 2 else ())
    shapes = {"dW1": (F, Gs), "db1": (F,), "dW2": (F, F), "db2": (F,)}
    got = {k: take(o[k], *shapes[k]) for k in names}
    assert is_sent(o["ws"][(E.filter_bwd_ws if which == 1 else E.filter_bwd2_ws)(g.shape[0], Gs, F):]), "workspace overrun"
    if not live:
        assert all(not bool(v.any()) for v in got.values()), (case, "no live row: every gradient is exactly zero")
        return got
    fn = (lambda g_, h_, d_, of_, w_: (E.filter_bwd if which == 1 else E.filter_bwd2)(g_, h_, d_, of_, coeff, w_, live))
    r32, r64 = both(fn, g[:live], h1[:live], dist[:live], offset, w2)
    for k, a32, a64 in zip(names, r32, r64):
        judge(fails, case, f"filter_bwd{which if which == 2 else ''}.{form}.{k}", got[k], a32, a64)
    return got


@pytest.mark.parametrize("Gs", E.BWD_GS)
def test_filter_bwd(Gs):
    """conan_filter_bwd, M in {1, 31, 32, 33, 127, 129} and 32 768 + 33 (a wavefront's second tile of the capped grid, at Gs = 50), *m_dev in {NULL,
    0, 1, 33, M, M + 5}; gmax NULL (three bf16 planes) and given (two fp16 planes; exact and 8 x too large; g at 3e-7, 1 and 4e4).  The slab form
    reduced through conan_wgrad_reduce_batch gives the immediate form's bits; _slices / _ws agree with the form functions at every M."""
    fails = []
    assert raw("conan_filter_bwd_supported", Gs, 128) == 1
    for M in E.BWD_M + ([E.BWD_M_CAPPED] if Gs == 50 else []):
        assert E.filter_bwd_wave_tiles(M) == (2 if M == E.BWD_M_CAPPED else 1)
        FORMS.add(f"filter_bwd/tiles{E.filter_bwd_wave_tiles(M)}")
        g, h1, dist, offset, coeff, w2 = E.filter_bwd_inputs(M, Gs, M + Gs)
        gm = float(g.abs().max())
        for form, gmax in (("bf16", None), ("fp16", gm)):
            o, live = fb_run(1, g, h1, dist, M, None, offset, coeff, w2, gmax)
            fb_check(fails, f"M{M}/Gs{Gs}", 1, form, o, live, g, h1, dist, offset, coeff, w2)
            if M in (33, 129, E.BWD_M_CAPPED):
                sl, _ = fb_run(1, g, h1, dist, M, None, offset, coeff, w2, gmax, slabs=True)
                assert all(torch.equal(sl[k].view(i32), o[k].view(i32)) for k in ("dW1", "db1")), "slabs + reduce_batch differ from the immediate form"
    M = 70
    g, h1, dist, offset, coeff, w2 = E.filter_bwd_inputs(M, Gs, 3 * Gs)
    for cnt in E.counts(M):
        for form, gmax in (("bf16", None), ("fp16", float(g.abs().max()))):
            o, live = fb_run(1, g, h1, dist, M, cnt, offset, coeff, w2, gmax)
            fb_check(fails, f"M{M}/Gs{Gs}/cnt{cnt}", 1, form, o, live, g, h1, dist, offset, coeff, w2)
    for scale in E.BWD_G_SCALES:
        gs = g * scale
        gm = float(gs.abs().max())
        for tag, gmax in (("exact", gm), ("x8", 8 * gm), ("bf16", None)):
            o, live = fb_run(1, gs, h1, dist, M, None, offset, coeff, w2, gmax)
            fb_check(fails, f"g{scale:g}/{tag}", 1, "bf16" if gmax is None else "fp16" if tag == "exact" else "fp16.gmax8", o, live, gs, h1, dist, offset, coeff, w2)
    o, live = fb_run(1, torch.zeros_like(g), h1, dist, M, None, offset, coeff, w2, 0.0)
    assert not bool(take(o["dW1"], 128, Gs).any()) and not bool(take(o["db1"], 128).any()), "g = 0 with gmax = 0 is not exactly zero"
    assert not fails, fails


@pytest.mark.parametrize("Gs", E.BWD_GS)
def test_filter_bwd2(Gs):
    """conan_filter_bwd2 on the same M, *m_dev, Gs and g grid; M = 8192 + 33 and 16 384 + 65 (the second and third tile of a workgroup through the
    staging ring, at Gs = 20) and 32 768 + 33 (at Gs = 50); the slab form as two reduce jobs gives the immediate bits."""
    fails = []
    assert raw("conan_filter_bwd2_supported", Gs, 128) == 1
    for M in E.BWD_M + (E.BWD2_M_RING if Gs == 20 else []) + ([E.BWD_M_CAPPED] if Gs == 50 else []):
        FORMS.add(f"filter_bwd2/tiles{E.filter_bwd2_wg_tiles(M)}")
        g, h1, dist, offset, coeff, w2 = E.filter_bwd_inputs(M, Gs, M + Gs)
        gm = float(g.abs().max())
        o, live = fb_run(2, g, h1, dist, M, None, offset, coeff, w2, gm)
        fb_check(fails, f"M{M}/Gs{Gs}", 2, "fp16", o, live, g, h1, dist, offset, coeff, w2)
        if M in (33, 129) or M > 1000:
            sl, _ = fb_run(2, g, h1, dist, M, None, offset, coeff, w2, gm, slabs=True)
            assert all(torch.equal(sl[k].view(i32), o[k].view(i32)) for k in ("dW1", "db1", "dW2", "db2")), "slabs + two reduce jobs differ from the immediate form"
    M = 70
    g, h1, dist, offset, coeff, w2 = E.filter_bwd_inputs(M, Gs, 3 * Gs)
    for cnt in E.counts(M):
        o, live = fb_run(2, g, h1, dist, M, cnt, offset, coeff, w2, float(g.abs().max()))
        fb_check(fails, f"M{M}/Gs{Gs}/cnt{cnt}", 2, "fp16", o, live, g, h1, dist, offset, coeff, w2)
    for scale in E.BWD_G_SCALES:
        gs = g * scale
        gm = float(gs.abs().max())
        for tag, gmax in (("exact", gm), ("x8", 8 * gm)):
            o, live = fb_run(2, gs, h1, dist, M, None, offset, coeff, w2, gmax)
            fb_check(fails, f"g{scale:g}/{tag}", 2, "fp16" if tag == "exact" else "fp16.gmax8", o, live, gs, h1, dist, offset, coeff, w2)
    o, live = fb_run(2, torch.zeros_like(g), h1, dist, M, None, offset, coeff, w2, 0.0)
    assert all(not bool(take(o[k], *sh).any()) for k, sh in (("dW1", (128, Gs)), ("db1", (128,)), ("dW2", (128, 128)), ("db2", (128,)))), "g = 0, gmax = 0"
    assert not fails, fails


def test_filter_bwd_supported_sizes_and_status_codes():
    s = stream_ptr()
    for Gs in (0, 1, 2, 62, 63, 64):
        for F in (64, 128, 256):
            assert raw("conan_filter_bwd_supported", Gs, F) == raw("conan_filter_bwd2_supported", Gs, F) == int(E.filter_bwd_supported(Gs, F)), (Gs, F)
    for M in (0, 1, 32, 33, 127, 128, 129, 4096, 8192, 8193, 32768, 32769, 10 ** 6):
        assert raw("conan_filter_bwd_slices", M) == E.filter_bwd_slices(M) and raw("conan_filter_bwd2_slices", M) == E.filter_bwd2_slices(M), M
        for Gs in (1, 20, 63):
            assert raw("conan_filter_bwd_ws", M, Gs, 128) == E.filter_bwd_ws(M, Gs, 128) and raw("conan_filter_bwd2_ws", M, Gs, 128) == E.filter_bwd2_ws(M, Gs, 128)
    g, h1, dist, offset, coeff, w2 = E.filter_bwd_inputs(8, 20, 1)
    gd, hd, dd, od, wd, gm = put(g), put(h1), put(dist), put(offset), put(w2), torch.ones(1, device=dev)
    o = {k: sent(n) for k, n in (("dW1", 128 * 20), ("db1", 128), ("dW2", 128 * 128), ("db2", 128), ("ws", E.filter_bwd2_ws(8, 20, 128)))}
    b1 = lambda g_, M, Gs, F, ws_=o["ws"]: raw("conan_filter_bwd", ptr(g_), ptr(hd), ptr(dd), M, ptr(od), Gs, coeff, ptr(wd), F, None, ptr(o["dW1"]), ptr(o["db1"]),
                                               ptr(ws_), None, s)
    assert b1(None, 8, 20, 128) == E_BADARG and b1(gd, 0, 20, 128) == E_BADARG and b1(gd, 8, 20, 128, None) == E_BADARG
    assert b1(gd, 8, 64, 128) == E_UNSUPPORTED and b1(gd, 8, 0, 128) == E_UNSUPPORTED and b1(gd, 8, 20, 64) == E_UNSUPPORTED
    b2 = lambda M, Gs, F, gm_, dW1, dW2: raw("conan_filter_bwd2", ptr(gd), ptr(hd), ptr(dd), M, ptr(od), Gs, coeff, ptr(wd), F, None, ptr(gm_), ptr(dW1), ptr(o["db1"]),
                                             ptr(dW2), ptr(o["db2"]), ptr(o["ws"]), s)
    assert b2(8, 20, 128, None, o["dW1"], o["dW2"]) == E_BADARG and b2(0, 20, 128, gm, o["dW1"], o["dW2"]) == E_BADARG
    assert b2(8, 20, 128, gm, None, o["dW2"]) == E_BADARG and b2(8, 20, 128, gm, o["dW1"], None) == E_BADARG       # one of dW1 / dW2 NULL, the other given
    assert b2(8, 64, 128, gm, o["dW1"], o["dW2"]) == E_UNSUPPORTED and b2(8, 20, 64, gm, o["dW1"], o["dW2"]) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(is_sent(t) for t in o.values())


def test_filter_bwd_non_finite_rows():
    """A NaN / +Inf in one element of g or of h1: every output is non-finite wherever the fp64 reference is, and keeps its bits elsewhere."""
    M, Gs = 70, 20
    g, h1, dist, offset, coeff, w2 = E.filter_bwd_inputs(M, Gs, 4)
    gm = float(g.abs().max())
    shapes = {"dW1": (128, Gs), "db1": (128,), "dW2": (128, 128), "db2": (128,)}
    for which, gmax in ((1, None), (1, gm), (2, gm)):
        clean, _ = fb_run(which, g, h1, dist, M, None, offset, coeff, w2, gmax)
        for what, v in (("g", E.NAN), ("g", E.INF), ("h1", E.NAN), ("dist", E.NAN)):
            gs, hs, ds = g, h1, dist
            if what == "g":
                gs = _poison(g, 40, 7, v)
            elif what == "h1":
                hs = _poison(h1, 40, 7, v)
            else:
                ds = _poison(dist, 40, None, v)
            o, _ = fb_run(which, gs, hs, ds, M, None, offset, coeff, w2, gmax)
            ref = (E.filter_bwd if which == 1 else E.filter_bwd2)(gs.double(), hs.double(), ds.double(), offset.double(), coeff, w2.double(), M)
            hit = sum(nonfinite_rule(f"bwd{which}/gmax{gmax}/{what}={v}", k, take(o[k], *shapes[k]), r, take(clean[k], *shapes[k]))
                      for k, r in zip(("dW1", "db1", "dW2", "db2"), ref))
            assert hit, "the case poisons nothing"


# ================================================================================================ stage-2 heads
HEAD_OUT = ("out", "m3", "mb", "t")
HEAD_GRAD = ("dx3", "dxc", "dxb", "dW3", "db3", "dWb", "dbb", "dwreg", "dbreg")


def head_run(c, nmol, K, D, N, aw, sums_ok=True):
    """Both forms of the head, forward and backward, twice: the plain head on x3 = conan_segment_sum_fwd(h3) and xb = conan_fgw_readout_fwd(Y, mode 0),
    the *_sums form on h3, graph_ptr and Y themselves."""
    s, G = stream_ptr(), nmol * K
    atoms = c["h3"].shape[0]
    Yd, hd, gp, xcd, dd = put(c["Y"]), put(c["h3"]), iput(c["gptr"]), put(c["xc"]), put(c["dout"])
    par = [put(t) for t in c["par"]]
    W3, b3, Wb, bb, wreg, breg = par

    def run():
        o = {"x3": sent(G * D), "xb": sent(G * D)}
        other("conan_segment_sum_fwd", ptr(hd), ptr(gp), G, D, ptr(o["x3"]), s)
        other("conan_fgw_readout_fwd", ptr(Yd), nmol, K, N, D, 0, ptr(o["xb"]), s)
        for pre in ("", "s.") if sums_ok else ("",):
            o.update({pre + "out": sent(nmol), pre + "m3": sent(nmol * D), pre + "mb": sent(nmol * D), pre + "t": sent(nmol * D)})
            o.update({pre + k: sent(n) for k, n in (("dxc", G * D), ("dW3", D * D), ("db3", D), ("dWb", D * D), ("dbb", D), ("dwreg", D), ("dbreg", 1))})
        o.update({"dx3": sent(G * D), "dxb": sent(G * D)})
        fo = lambda pre: [ptr(o[pre + k]) for k in HEAD_OUT]
        assert raw("conan_stage2_head_fwd", ptr(o["x3"]), ptr(xcd), ptr(o["xb"]), *[ptr(t) for t in par], aw, nmol, K, D, *fo(""), s) == OK
        assert raw("conan_stage2_head_bwd", ptr(dd), ptr(W3), ptr(Wb), ptr(wreg), ptr(o["m3"]), ptr(o["mb"]), ptr(o["t"]), aw, nmol, K, D,
                   *[ptr(o[k]) for k in HEAD_GRAD], s) == OK
        if sums_ok:
            o.update({"s.dh3": sent(atoms * D), "s.dY": sent(nmol * N * D)})
            assert raw("conan_stage2_head_sums_fwd", ptr(Yd), ptr(hd), ptr(gp), ptr(xcd), *[ptr(t) for t in par], aw, nmol, K, N, D, 0, *fo("s."), s) == OK
            assert raw("conan_stage2_head_sums_bwd", ptr(dd), ptr(W3), ptr(Wb), ptr(wreg), ptr(o["s.m3"]), ptr(o["s.mb"]), ptr(o["s.t"]), ptr(gp), aw, nmol, K, N, D, 0,
                       ptr(o["s.dh3"]), ptr(o["s.dxc"]), ptr(o["s.dY"]), *[ptr(o["s." + k]) for k in HEAD_GRAD[3:]], s) == OK
        return o
    return twice(run)


def head_shapes(nmol, K, D, N, atoms):
    G = nmol * K
    sh = {"out": (nmol,), "m3": (nmol, D), "mb": (nmol, D), "t": (nmol, D), "dx3": (G, D), "dxc": (G, D), "dxb": (G, D), "dW3": (D, D), "db3": (D,),
          "dWb": (D, D), "dbb": (D,), "dwreg": (D,), "dbreg": (1,), "x3": (G, D), "xb": (G, D)}
    sh.update({"s." + k: v for k, v in sh.items()})
    sh.update({"s.dh3": (atoms, D), "s.dY": (nmol, N, D)})
    return sh


def head_bits_of_the_plain_head(case, got, c, nmol, K, D, N):
    """The *_sums form has the bits of the plain head on segment_sum(h3) and the repeated node sum of Y; dh3 and dY are the broadcast of its rows."""
    for k in HEAD_OUT + ("dxc",) + HEAD_GRAD[3:]:
        assert torch.equal(got["s." + k].view(i32), got[k].view(i32)), (case, k, "the *_sums form does not have the plain head's bits")
    sizes = (c["gptr"][1:] - c["gptr"][:-1])
    assert torch.equal(got["s.dh3"].view(i32), got["dx3"].repeat_interleave(sizes, dim=0).view(i32)), (case, "dh3 is not the broadcast of dx3")
    dY = torch.zeros(nmol, D)
    for k in range(K):                                                       # conan_fgw_readout_bwd mode 0: the K copies added one after the other
        dY = dY + got["dxb"].view(nmol, K, D)[:, k]
    assert torch.equal(got["s.dY"].view(i32), dY.unsqueeze(1).expand(nmol, N, D).contiguous().view(i32)), (case, "dY is not the broadcast of the summed dxb")


@pytest.mark.parametrize("nmol,K,D,N,aw", E.head_cases())
def test_stage2_heads(nmol, K, D, N, aw):
    """Both forms of the stage-2 head, D in {1, 3, 5, 32, 63, 64}, num_molecules in {1, 3, 4, 5, 15, 16, 17, 33} (the 4-molecule blocks, the
    16-molecule unrolled sums with their tail), K in {1, 2, 5, 32}, N in {1, 9}, agg_weight 0 and 0.37, conformer graphs of 0, 1 and 70 atoms."""
    fails, case = [], f"nmol{nmol}/K{K}/D{D}/N{N}/aw{aw}"
    FORMS.add("head/" + E.head_sum_form(nmol))
    c = E.head_inputs(nmol, K, D, N, E.head_seed(nmol, K, D))
    assert raw("conan_stage2_head_supported", D) == 1 and raw("conan_stage2_head_sums_supported", D, K, 0) == 1
    o = head_run(c, nmol, K, D, N, aw)
    sh = head_shapes(nmol, K, D, N, c["h3"].shape[0])
    got = {k: take(v, *sh[k]) for k, v in o.items()}
    head_bits_of_the_plain_head(case, got, c, nmol, K, D, N)
    x3, xb = got["x3"], got["xb"]
    f32_, f64_ = both(lambda x3_, xc_, xb_, *p: E.head_fwd(x3_, xc_, xb_, *p, aw, K), x3, c["xc"], xb, *c["par"])
    for k, a32, a64 in zip(HEAD_OUT, f32_, f64_):
        judge(fails, case, "head." + k, got[k].view(a64.shape), a32.view(a64.shape), a64)
    W3, _, Wb, _, wreg, _ = c["par"]
    b32, b64 = both(lambda d_, W3_, Wb_, wr_, m3_, mb_, t_: E.head_bwd(d_, W3_, Wb_, wr_, m3_, mb_, t_, aw, K), c["dout"], W3, Wb, wreg, got["m3"], got["mb"], got["t"])
    for k, a32, a64 in zip(HEAD_GRAD, b32, b64):
        judge(fails, case, "head." + k, got[k].view(a64.shape), a32.view(a64.shape), a64)
    # the *_sums form against the fp64 reference from h3 and Y themselves (the sums included)
    s32, s64 = both(lambda Y_, h3_, xc_, *p: E.head_sums_fwd(Y_, h3_, c["gptr"], xc_, *p, aw, K), c["Y"], c["h3"], c["xc"], *c["par"])
    for k, a32, a64 in zip(HEAD_OUT, s32, s64):
        judge(fails, case, "head_sums." + k, got["s." + k].view(a64.shape), a32.view(a64.shape), a64)
    assert not fails, fails


def test_stage2_head_supported_bounds_and_status_codes():
    """D = 0 and 65 unsupported; K = 33 accepted by the plain head, refused by the *_sums form; readout_mode 1 refused; num_molecules = 0 OK on the
    forwards and a bad argument on the backwards; no buffer touched."""
    for D in (-1, 0, 1, 64, 65):
        assert raw("conan_stage2_head_supported", D) == int(E.head_supported(D))
        for K in (0, 1, 32, 33):
            for mode in (0, 1):
                assert raw("conan_stage2_head_sums_supported", D, K, mode) == int(E.head_sums_supported(D, K, mode)), (D, K, mode)
    nmol, K, D, N, s = 3, 33, 8, 2, stream_ptr()
    c = E.head_inputs(nmol, K, D, N, E.head_seed(nmol, K, D))
    o = head_run(c, nmol, K, D, N, 0.37, sums_ok=False)                         # K = 33 on the plain head
    sh = head_shapes(nmol, K, D, N, c["h3"].shape[0])
    got = {k: take(v, *sh[k]) for k, v in o.items()}
    fails = []
    f32_, f64_ = both(lambda x3_, xc_, xb_, *p: E.head_fwd(x3_, xc_, xb_, *p, 0.37, K), got["x3"], c["xc"], got["xb"], *c["par"])
    for k, a32, a64 in zip(HEAD_OUT, f32_, f64_):
        judge(fails, "K33", "head." + k, got[k].view(a64.shape), a32.view(a64.shape), a64)
    assert not fails, fails
    bufs = {k: sent(4096) for k in ("a", "b", "c", "d", "e", "f", "g", "h", "i", "j", "k")}
    B = [ptr(bufs[k]) for k in bufs]
    inp, gp = put(torch.randn(4096)), iput(torch.arange(200))
    P = ptr(inp)
    hf = lambda nm, K_, D_, x3=P: raw("conan_stage2_head_fwd", x3, P, P, P, P, P, P, P, P, 0.3, nm, K_, D_, *B[:4], s)
    hb = lambda nm, K_, D_, d=P: raw("conan_stage2_head_bwd", d, P, P, P, P, P, P, 0.3, nm, K_, D_, *B[:9], s)
    sf = lambda nm, K_, N_, D_, mode, Y=P: raw("conan_stage2_head_sums_fwd", Y, P, ptr(gp), P, P, P, P, P, P, P, 0.3, nm, K_, N_, D_, mode, *B[:4], s)
    sb = lambda nm, K_, N_, D_, mode, d=P: raw("conan_stage2_head_sums_bwd", d, P, P, P, P, P, P, ptr(gp), 0.3, nm, K_, N_, D_, mode, *B[:9], s)
    assert hf(0, 2, 8) == OK and sf(0, 2, 3, 8, 0) == OK and hb(0, 2, 8) == E_BADARG and sb(0, 2, 3, 8, 0) == E_BADARG
    assert hf(-1, 2, 8) == E_BADARG and hf(2, 0, 8) == E_BADARG and hf(2, 2, 8, None) == E_BADARG and hb(2, 0, 8) == E_BADARG and hb(2, 2, 8, None) == E_BADARG
    assert sf(2, 0, 3, 8, 0) == E_BADARG and sf(2, 2, 0, 8, 0) == E_BADARG and sf(2, 2, 3, 8, 0, None) == E_BADARG
    assert sb(2, 0, 3, 8, 0) == E_BADARG and sb(2, 2, 0, 8, 0) == E_BADARG and sb(2, 2, 3, 8, 0, None) == E_BADARG
    assert hf(2, 2, 0) == E_UNSUPPORTED and hf(2, 2, 65) == E_UNSUPPORTED and hb(2, 2, 0) == E_UNSUPPORTED and hb(2, 2, 65) == E_UNSUPPORTED
    for call in (sf, sb):
        assert call(2, 33, 3, 8, 0) == E_UNSUPPORTED and call(2, 2, 3, 8, 1) == E_UNSUPPORTED and call(2, 2, 3, 65, 0) == E_UNSUPPORTED and call(2, 2, 3, 0, 0) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(is_sent(t) for t in bufs.values())


def test_stage2_head_a_nan_stays_in_its_molecule():
    """A NaN / +Inf in one conformer row of one molecule (h3, Y or xc) reaches that molecule's out, m3 / mb / t and, through t, dwreg; a NaN in one
    dout reaches that molecule's input gradients and every parameter gradient.  No other molecule's rows change a bit — in both forms."""
    nmol, K, D, N, aw = 5, 2, 32, 9, 0.37
    c = E.head_inputs(nmol, K, D, N, 21)
    sh = head_shapes(nmol, K, D, N, c["h3"].shape[0])
    clean = {k: take(v, *sh[k]) for k, v in head_run(c, nmol, K, D, N, aw).items()}
    b = 2
    assert int(c["gptr"][(b + 1) * K]) > int(c["gptr"][b * K]), "molecule b has atoms"
    atom = int(c["gptr"][(b + 1) * K]) - 1
    for what, v in (("h3", E.NAN), ("h3", E.INF), ("Y", E.NAN), ("xc", E.INF), ("dout", E.NAN)):
        cc = dict(c)
        if what == "h3":
            cc["h3"] = _poison(c["h3"], atom, 3, v)
        elif what == "Y":
            cc["Y"] = c["Y"].clone()
            cc["Y"][b, 4, 3] = v
        elif what == "xc":
            cc["xc"] = _poison(c["xc"], b * K + 1, 3, v)
        else:
            cc["dout"] = c["dout"].clone()
            cc["dout"][b] = v
        got = {k: take(t, *sh[k]) for k, t in head_run(cc, nmol, K, D, N, aw).items()}
        head_bits_of_the_plain_head(what, got, cc, nmol, K, D, N)
        dbl = lambda ts: [t.double() for t in ts]
        f64_ = E.head_sums_fwd(cc["Y"].double(), cc["h3"].double(), cc["gptr"], cc["xc"].double(), *dbl(cc["par"]), aw, K)
        W3, _, Wb, _, wreg, _ = dbl(cc["par"])
        g64 = E.head_bwd(cc["dout"].double(), W3, Wb, wreg, *f64_[1:], aw, K)
        hit = {k: nonfinite_rule(f"head/{what}={v}", k, got[k].view(r.shape), r, clean[k].view(r.shape))
               for k, r in list(zip(HEAD_OUT, f64_)) + list(zip(HEAD_GRAD, g64))}
        others = torch.arange(nmol) != b
        assert torch.equal(got["out"][others].view(i32), clean["out"][others].view(i32)) and torch.equal(got["dx3"].view(nmol, -1)[others].view(i32),
                                                                                                       clean["dx3"].view(nmol, -1)[others].view(i32))
        if what == "dout":
            assert hit["dx3"] == hit["dxc"] == hit["dxb"] == K * D and hit["dW3"] == hit["dWb"] == D * D and hit["db3"] == hit["dwreg"] == D and hit["dbreg"] == 1
        else:
            assert hit["out"] == 1 and hit["dwreg"] >= 1 and hit["dx3"] == 0


# ================================================================================================ closing: nothing was left out
def test_zz_every_edge_export_was_called():
    """The 24 entry points this module owns are declared in _lib.SIGNATURES and each was called by a test above; every form the form functions
    name was reached by a judged case.  (Run the whole module: this test looks at what the tests above did.)"""
    whole = "this test looks at what the other tests of the module did: run the whole module, in file order, in one process"
    assert len(OWNED) == 24 and len(set(OWNED)) == 24
    assert set(OWNED) <= set(_lib.SIGNATURES), sorted(set(OWNED) - set(_lib.SIGNATURES))
    assert set(OWNED) <= CALLED, (whole, sorted(set(OWNED) - CALLED))
    assert CALLED <= set(OWNED), sorted(CALLED - set(OWNED))
    want = E.CFCONV_FORMS | {"wp128", "wp128/per66", "wp_generic", "bwd_w/1", "bwd_w/2", "filter_fwd/pass1", "filter_fwd/pass2", "filter_cf/per_wg1", "filter_cf/per_wg2",
                             "filter_cf/per_wg9", "filter_bwd/tiles1", "filter_bwd/tiles2", "filter_bwd2/tiles1", "filter_bwd2/tiles2", "filter_bwd2/tiles3",
                             "filter_bwd2/tiles5", "head/+tail", "head/unrolled", "head/unrolled+tail"}
    assert want <= FORMS, (whole, sorted(want - FORMS))
    print("\nworst err / yard per output (row, whole tensor):")
    for what, (rr, ra) in sorted(RATIOS.items()):
        print(f"TABLE {what:34s} row={rr:6.3g} all={ra:6.3g}")
