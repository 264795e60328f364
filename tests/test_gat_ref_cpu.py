"""The per-kernel GAT references (tests/gat_ref.py) are not a second unverified copy: composed (edge_vec -> aggregate) in fp64 they must reproduce
oracle.gat.GATConvOracle — output and all parameter gradients — to 1e-12 relative on every small case (both are fp64 sums of at most a few hundred
terms in different orders).  bond_csr is checked against a literal restatement of its ordering rule.

Also asserted here, on every CPU run, are the conditions on the INPUTS of tests/test_gpu_gat_ops.py, so that the GPU file never has to skip or
loosen anything: (a) the fp32 reference stays within visnet_ref.COND_CAP of the fp64 one (whole tensor) for every output and gradient; (b) no
pre-activation lies closer to the LeakyReLU kink than 1e-4 of the RMS pre-activation; (c) at least half of the rows with edges hold
pre-activations of both signs (otherwise the att_dst gradient is identically zero and judges nothing).  And the case list reaches every branch of
gat_ref.REQUIRED_BRANCHES, predicted from the constants in the kernel sources."""
import numpy as np
import pytest
import torch

import gat_ref as G
import visnet_ref as R
from helpers import rel
from oracle.gat import GATConvOracle

f64 = torch.float64
TOL = 1e-12
CASES = G.cases()
_REF = {}


def _case(name):
    """(case, inputs, reference), computed once and shared."""
    if name not in _REF:
        c = CASES[name]
        inp = G.make_inputs(c)
        _REF[name] = (c, inp, G.reference(c, inp))
    return _REF[name]


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.large and c.backward])
def test_reference_composes_to_the_oracle_layer(name):
    c, inp, _ = _case(name)
    n, C, D = c.n, c.C, c.D
    m = GATConvOracle(C, C, D).double()
    bias = inp["bias"] if inp["bias"] is not None else torch.zeros(C)
    with torch.no_grad():
        m.lin_src.weight.copy_(torch.eye(C, dtype=f64))             # h = x: the reference starts after lin_src
        m.att_src.copy_(inp["att_src"].double().view(1, 1, C)); m.att_dst.copy_(inp["att_dst"].double().view(1, 1, C))
        m.att_edge.copy_(inp["att_edge"].double().view(1, 1, C)); m.lin_edge.weight.copy_(inp["W_edge"].double()); m.bias.copy_(bias.double())
    x = inp["h"].double().requires_grad_(True)
    dout = inp["dout"].double()
    o = m(x, torch.from_numpy(c.ei), inp["ea"].double())
    wrt_o = [x, m.att_src, m.att_dst, m.lin_edge.weight, m.att_edge, m.bias]
    go = torch.autograd.grad(o, wrt_o, dout)
    src, tgt, ea = G._kept(inp, c.csr)
    leaves = [t.double().clone().requires_grad_(True) for t in (inp["h"], inp["att_src"], inp["att_dst"], inp["W_edge"], inp["att_edge"], bias)]
    h, a_s, a_d, W, a_e, b = leaves
    r, _, _ = G.aggregate(h, a_s, a_d, G.edge_vec(W, a_e), b, ea.double(), src, tgt, n, G.SLOPE)
    gr = torch.autograd.grad(r, leaves, dout)
    assert rel(r.detach().numpy(), o.detach().numpy()) < TOL
    # a gradient that is exactly zero (dv of a graph whose rows all hold one edge on the self loop's side of the kink) is compared on the scale of the
    # largest gradient of the layer
    gmax = max(float(e.norm()) for e in go)
    for k, (a, e) in enumerate(zip(gr, go)):
        assert float((a.reshape(-1) - e.reshape(-1)).norm()) <= TOL * max(float(e.norm()), 1e-3 * gmax), (name, k)


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_of_the_gpu_cases_meet_their_conditions(name):
    c, inp, ref = _case(name)
    # (a) the yardstick is usable
    for what in ref["64"]:
        if ref["64"][what].numel() == 0:
            continue
        e = R.all_err(ref["32"][what], ref["64"][what])
        assert e <= R.COND_CAP, (name, what, e)
        assert bool(torch.isfinite(ref["32"][what]).all()), (name, what)
    # (b) nothing on the kink, in fp64 and in fp32 alike
    for dt in (f64, torch.float32):
        pre_e, pre_s = G.pre_of(inp, c.csr, dt)
        allp = torch.cat([pre_e, pre_s]).double()
        assert float(allp.abs().min()) >= G.KINK_FLOOR * float(allp.square().mean().sqrt()), name
    pe64, ps64 = G.pre_of(inp, c.csr, f64)
    pe32, ps32 = G.pre_of(inp, c.csr, torch.float32)
    assert torch.equal(pe64 > 0, pe32 > 0) and torch.equal(ps64 > 0, ps32 > 0)
    # (c) rows with edges: at least half hold both signs
    tgt = torch.from_numpy(c.csr.tgt.astype(np.int64))
    pos = torch.zeros(c.n).index_add_(0, tgt, (pe64 > 0).float()) + (ps64 > 0).float()
    has = torch.from_numpy(c.csr.indeg > 0)
    if int(has.sum()):
        mixed = (pos > 0) & (pos < torch.from_numpy(c.csr.indeg + 1).float())
        assert int((mixed & has).sum()) * 2 >= int(has.sum()), (name, int((mixed & has).sum()), int(has.sum()))


@pytest.mark.parametrize("C", [64, 96])
def test_extreme_case_is_extreme(C):
    c, inp, ref = _case(f"extreme/C{C}")
    pe, ps = G.pre_of(inp, c.csr)
    x, rp = G.extreme_rows(c.csr), c.csr.rowptr
    row = lambda i: pe[rp[i]:rp[i + 1]]
    assert 100 < float(torch.cat([pe, ps]).abs().max()) < 140 and float(ps.min()) < -60 and float(pe.min()) < -30            # about -60 .. +110
    assert float(row(x.negative).max()) < 0 and float(ps[x.negative]) < 0                       # a row of negative pre-activations only
    assert float(ps[x.self_max]) > float(row(x.self_max).max()) + 10                           # the self loop holds the maximum
    lk = torch.nn.functional.leaky_relu(row(x.underflow), G.SLOPE)
    assert float(lk.max() - lk.min()) > 104                                                    # exp(-104) is 0 in fp32: one alpha underflows
    a32 = ref["32"]["alpha"][rp[x.underflow]:rp[x.underflow + 1]]
    assert float(a32.min()) == 0.0 and float(a32.max()) > 0.99


def test_degree_graph_has_every_row_length_in_both_roles():
    ei, n = G.degree_graph()
    csr, k = G.bond_csr(ei, n), G.constants()
    assert n < 400 and len(set(map(tuple, ei.T.tolist()))) == ei.shape[1]                     # no multi-edges
    for j, d in enumerate(G.DEGREES):
        assert csr.indeg[j] == d and csr.outdeg[j] == 0 and csr.outdeg[12 + j] == d and csr.indeg[12 + j] == 0
    assert csr.indeg[24] == 150 and csr.outdeg[24] == 150
    # the limits the list was written around are the ones in the source today
    assert {k.MD, k.MD + 1, k.STAGE - 1, k.STAGE, k.STAGE + 1} <= set(G.DEGREES) and (k.MD, k.STAGE, k.WGS, k.MAXC, k.MAXD) == (6, 64, 2048, 256, 8)


def test_case_list_reaches_every_branch():
    taken = set()
    for c in CASES.values():
        taken |= c.branches()
    assert G.REQUIRED_BRANCHES <= taken, sorted(G.REQUIRED_BRANCHES - taken)
    k = G.constants()
    assert CASES["large/n33000/C64"].n > k.G16_PASS and CASES["large/n8300/C96"].n > k.WAVES
    assert G.scan_branch(33000) == "long" and G.scan_branch(k.SCAN_LDS_MAX + 1) == "global"


def test_bond_csr_follows_its_ordering_rule():
    for ei, n in (G.multi_graph(invalid=True), G.degree_graph(), G.random_graph(30, 8, 5)):
        c = G.bond_csr(ei, n)
        keep = [e for e in range(ei.shape[1]) if ei[0, e] != ei[1, e] and 0 <= ei[0, e] < n and 0 <= ei[1, e] < n]
        assert c.K == len(keep) and c.rowptr[n] == c.K and c.t_rowptr[n] == c.K
        for i in range(n):
            want = sorted((int(ei[0, e]), e) for e in keep if ei[1, e] == i)
            assert list(zip(c.col[c.rowptr[i]:c.rowptr[i + 1]].tolist(), c.eid[c.rowptr[i]:c.rowptr[i + 1]].tolist())) == want
        for j in range(n):
            ps = c.t_pos[c.t_rowptr[j]:c.t_rowptr[j + 1]]
            assert ps.tolist() == [p for p in range(c.K) if c.col[p] == j]
            assert np.array_equal(c.t_tgt[c.t_rowptr[j]:c.t_rowptr[j + 1]], c.tgt[ps])
