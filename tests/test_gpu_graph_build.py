"""The fused graph build (conan_radius_graph_build: neighbour lists, undirected pairs and by-source transpose in three launches) against the three
entry points it replaces (conan_radius_graph_csr + conan_edge_pairs + conan_csr_transpose) on the same inputs: every list entry for entry, integer
and fp32 alike (`np.array_equal`).  Rows beyond the edge count E / the pair count P are unspecified on both sides and not compared."""
import types

import numpy as np
import pytest
import torch

from conan_fgw_amd import ops
from conan_fgw_amd._lib import call, lib, ptr, stream_ptr
from conan_fgw_amd.synthetic import make_batch, make_bond_graph

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
i32, f32 = torch.int32, torch.float32


def _build(pos, gp, G, cutoff, cap, loop, fused, pairs=False, transpose=False):
    ops.FUSED_GRAPH_BUILD = fused
    try:
        return ops.RadiusGraph(pos, gp, G, cutoff, cap, loop, pairs=pairs, transpose=transpose)
    finally:
        ops.FUSED_GRAPH_BUILD = True


def _lists(g, pairs, transpose):
    """Everything that is compared, as numpy arrays cut to E / P (`pairs()` / `transpose()` return what the constructor built, or build it now)."""
    E = g.num_edges
    out = {"E": np.int64(E), "rowptr": g.rowptr.cpu().numpy()}
    for k in ("col", "tgt", "dist"):
        out[k] = getattr(g, k)[:E].cpu().numpy()
    if pairs:
        g.pairs()
        P = int(g.num_pairs_dev.item())
        out["P"] = np.int64(P)
        out["pid"] = g.pid[:E].cpu().numpy()
        for k in ("pair_e0", "pair_e1", "pair_dist"):
            out[k] = getattr(g, k)[:P].cpu().numpy()
    if transpose:
        tr, te = g.transpose()
        out["t_rowptr"], out["t_eid"] = tr.cpu().numpy(), te[:E].cpu().numpy()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def _check(pos, gp, G, cutoff, cap, loop, pairs=True, transpose=True):
    new = _build(pos, gp, G, cutoff, cap, loop, True, pairs=pairs, transpose=transpose)
    assert (new.pid is not None) == pairs and (new._t_rowptr is not None) == transpose      # built by the constructor, not on first use
    old = _build(pos, gp, G, cutoff, cap, loop, False)
    assert old.pid is None and old._t_rowptr is None
    a, b = _lists(new, pairs, transpose), _lists(old, pairs, transpose)
    _same(a, b)
    return a


def _inputs(b):
    pos = torch.from_numpy(b.pos).to(dev)
    gp = ops.graph_ptr_from_batch(torch.from_numpy(b.batch).to(dev), b.num_graphs)
    return pos, gp


def _from_counts(counts, box, seed):
    rng = np.random.RandomState(seed)
    n = int(np.sum(counts))
    pos = torch.from_numpy(rng.uniform(0, box, size=(n, 3)).astype(np.float32)).to(dev)
    gp = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    return pos, gp


def test_esol_batch_pairs_and_transpose():
    b = make_batch("esol", 4, 5, seed=3)
    r = _check(*_inputs(b), b.num_graphs, 10.0, 32, False)
    assert r["E"] > 0 and 0 < r["P"] < r["E"]


def test_esol_batch_self_loops_without_pairs():
    b = make_batch("esol", 4, 5, seed=3)
    r = _check(*_inputs(b), b.num_graphs, 5.0, 32, True, pairs=False)
    assert np.any(r["col"] == r["tgt"])


@pytest.mark.parametrize("cap", [4, 32])
def test_truncated_rows(cap):
    """One 40-atom cluster, every atom within the cutoff of every other.  cap 4: rows keep the lowest sources only, so most edges have no reverse
    (one-directional pairs).  cap 32: targets 33 .. 39 never reach themselves in the cap + 1 window and keep cap + 1 edges."""
    pos, gp = _from_counts([40], 4.0, 5)
    r = _check(pos, gp, 1, 10.0, cap, False)
    if cap == 4:
        assert np.any(r["pair_e1"] == -1)
    else:
        assert np.diff(r["rowptr"]).max() == cap + 1


def test_empty_and_single_atom_graphs():
    pos, gp = _from_counts([5, 0, 7, 1, 1, 0, 0, 3, 1], 3.0, 7)       # an empty graph between two non-empty ones, single atoms, empty graphs in a row
    r = _check(pos, gp, 9, 10.0, 32, False)
    assert r["E"] == 5 * 4 + 7 * 6 + 3 * 2
    _check(pos, gp, 9, 10.0, 32, True)                                # with self loops a single atom has one edge and one pair without reverse


def test_no_atoms():
    """num_atoms = 0 (every graph empty), both sides through the C entry points: the three old ones take no NULL position pointer, so both get a
    dummy one."""
    G = 3
    gp = torch.zeros(G + 1, dtype=i32, device=dev)
    pos = torch.zeros(1, 3, device=dev)
    s = stream_ptr()

    def bufs():
        return {k: torch.full((2,), -7, dtype=f32 if k in ("dist", "pair_dist") else i32, device=dev)
                for k in ("rowptr", "col", "tgt", "dist", "pid", "pair_e0", "pair_e1", "pair_dist", "np", "t_rowptr", "t_eid")}
    n_ = bufs()
    ws = torch.empty(max(1, lib().conan_radius_graph_build_ws(0, G, 32, 0)), dtype=i32, device=dev)
    call("conan_radius_graph_build", ptr(pos), ptr(gp), 0, G, 10.0, 32, 0, ptr(ws), ptr(n_["rowptr"]), ptr(n_["col"]), ptr(n_["tgt"]), ptr(n_["dist"]),
         ptr(n_["pid"]), ptr(n_["pair_e0"]), ptr(n_["pair_e1"]), ptr(n_["pair_dist"]), ptr(n_["np"]), ptr(n_["t_rowptr"]), ptr(n_["t_eid"]), s)
    o_ = bufs()
    deg = torch.empty(1, dtype=i32, device=dev)
    flag, pidx, sws = torch.empty(2, dtype=i32, device=dev), torch.empty(2, dtype=i32, device=dev), torch.empty(4, dtype=i32, device=dev)
    call("conan_radius_graph_csr", ptr(pos), ptr(gp), 0, G, 10.0, 32, 0, ptr(deg), ptr(o_["rowptr"]), ptr(o_["col"]), ptr(o_["tgt"]), ptr(o_["dist"]), s)
    call("conan_edge_pairs", ptr(o_["rowptr"]), ptr(o_["col"]), ptr(o_["tgt"]), ptr(o_["dist"]), ptr(o_["rowptr"]), 1, ptr(flag), ptr(pidx), ptr(sws),
         ptr(o_["pid"]), ptr(o_["pair_e0"]), ptr(o_["pair_e1"]), ptr(o_["pair_dist"]), s)
    call("conan_csr_transpose", ptr(gp), G, 0, ptr(o_["rowptr"]), ptr(o_["col"]), None, ptr(o_["t_rowptr"]), ptr(o_["t_eid"]), s)
    assert int(n_["rowptr"][0]) == int(o_["rowptr"][0]) == 0            # rowptr[num_atoms] = E = 0
    assert int(n_["t_rowptr"][0]) == int(o_["t_rowptr"][0]) == 0
    assert int(n_["np"][0]) == int(pidx[1]) == 0                        # pair count
    for k in ("col", "tgt", "dist", "pid", "pair_e0", "pair_dist", "t_eid"):
        assert torch.equal(n_[k], torch.full_like(n_[k], -7)), k        # no edge, no pair: nothing else is written (pair_e1's tail is the old scan's scratch)
    # and through the constructor
    g = ops.RadiusGraph(torch.zeros(0, 3, device=dev), gp, G, 10.0, 32, pairs=True, transpose=True)
    assert g.num_edges == 0 and int(g.num_pairs_dev.item()) == 0 and g.rowptr.cpu().tolist() == [0] and g.transpose()[0].cpu().tolist() == [0]


def test_graph_beyond_the_lds_bounds():
    """2 100 atoms in one graph: beyond the position staging (2 048 atoms) and the list staging of the fused build, so positions and lists are read
    from global memory; three small graphs beside it, one of them behind it."""
    pos, gp = _from_counts([12, 2100, 9, 20], 30.0, 9)
    r = _check(pos, gp, 4, 5.0, 32, False)
    assert np.any(r["pair_e1"] == -1) and np.diff(r["rowptr"]).max() >= 32      # the dense graph is truncated


def test_many_tiny_graphs():
    """1 500 graphs of one or two atoms: the per-graph count scan runs with more than one entry per thread."""
    counts = np.random.RandomState(2).randint(1, 3, size=1500)
    pos, gp = _from_counts(counts, 2.0, 4)
    r = _check(pos, gp, 1500, 10.0, 32, False)
    assert r["E"] == 2 * int((counts == 2).sum()) and r["P"] == int((counts == 2).sum())


@pytest.mark.parametrize("pairs,transpose", [(True, False), (False, True), (False, False)])
def test_partial_requests_and_lazy_use(pairs, transpose):
    """Only the pairs, only the transpose, or neither from the constructor; what was not built there comes from the old entry point on first use."""
    b = make_batch("lipo", 2, 2, seed=8)                               # > 33 atoms per conformer: truncated rows, one-directional pairs
    pos, gp = _inputs(b)
    new = _build(pos, gp, b.num_graphs, 10.0, 32, False, True, pairs=pairs, transpose=transpose)
    assert (new.pid is not None) == pairs and (new._t_rowptr is not None) == transpose
    built = (new.pid, new._t_rowptr)
    a = _lists(new, True, True)                                        # pairs() / transpose() on a graph built without them
    if pairs:
        assert new.pid is built[0]
    if transpose:
        assert new._t_rowptr is built[1]
    _same(a, _lists(_build(pos, gp, b.num_graphs, 10.0, 32, False, False), True, True))


def test_captured_build_replays_with_new_positions():
    b = make_batch("esol", 4, 5, seed=21)
    pos, gp = _inputs(b)
    rng = np.random.RandomState(1)
    moved = [torch.from_numpy((b.pos + rng.normal(0, 0.4, size=b.pos.shape)).astype(np.float32)).to(dev) for _ in range(2)]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.RadiusGraph(pos, gp, b.num_graphs, 4.0, 32, pairs=True, transpose=True)      # warm-up outside the capture
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side, capture_error_mode="thread_local"):
            g = ops.RadiusGraph(pos, gp, b.num_graphs, 4.0, 32, pairs=True, transpose=True)
        for p in moved:
            pos.copy_(p)
            cg.replay()
            torch.cuda.synchronize()
            g._num_edges = None                                        # (the host copy of E belongs to the previous replay)
            eager = _build(p, gp, b.num_graphs, 4.0, 32, False, False)
            _same(_lists(g, True, True), _lists(eager, True, True))
    torch.cuda.current_stream().wait_stream(side)


def test_stage2_model_is_bit_identical_with_and_without_the_fused_build():
    from conan_fgw_amd.head import EmbeddingsWithGATAggregationBaryCenter
    K = 5
    b = make_batch("esol", 4, K, seed=3)
    bg = make_bond_graph(b, seed=4)
    t = lambda a: torch.from_numpy(a).to(dev)
    data = types.SimpleNamespace(z=t(b.z), pos=t(b.pos), batch=t(b.batch), x=t(bg.x), edge_index=t(bg.edge_index), edge_attr=t(bg.edge_attr))
    y = t(b.y)[:, None]
    torch.manual_seed(12)
    model = EmbeddingsWithGATAggregationBaryCenter(K, dev).to(dev)
    cidx = model.create_aggregation_index(b.num_graphs, dev)

    def run(fused):
        ops.FUSED_GRAPH_BUILD = fused
        try:
            model.zero_grad(set_to_none=True)
            pred = model(data, cidx, data.batch, num_graphs=b.num_graphs, max_nodes=b.max_nodes)
            ops.mse_loss(pred, y).backward()
            torch.cuda.synchronize()
            return pred.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        finally:
            ops.FUSED_GRAPH_BUILD = True

    p1, g1 = run(True)
    p0, g0 = run(False)
    assert torch.isfinite(p1).all() and torch.equal(p1, p0)
    assert g1.keys() == g0.keys() and len(g1) > 20
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n
