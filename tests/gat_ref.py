"""TEST INFRASTRUCTURE — plain reference formulas of the GAT kernels (csrc/gat.hip, the bond-graph part of csrc/graph.hip), one small function per
kernel contract of the covalent section of include/conan_fgw_hip.h.  Nothing is imported from the package.

Every function is written with plain torch indexing on whatever dtype it is given (index_select / index_add_ / sum; no fusion): called with float64
it is the reference ("ref64"), called with float32 on the CPU it is the yardstick ("ref32") a kernel's error is measured against (visnet_ref.judge).
Gradients are torch.autograd.grad of the same functions in the same dtype: conan_gat_aggregate_bwd is the backward of node_alpha + aggregate
together (dh and d att_src | d att_dst | d bias | dv), conan_gat_edge_vec_bwd the backward of edge_vec.  tests/test_gat_ref_cpu.py demands 1e-12
agreement of their composition with oracle.gat.GATConvOracle in fp64 and asserts the input conditions of every case.

Conventions: `src`, `tgt`, `ea` of `aggregate` are the KEPT edges in the by-target CSR order of `bond_csr` (alpha comes back in that order);
the self loop of a node carries the mean of its incoming attributes (0 without any); softmax is exp(a - max) / (sum + 1e-16).

The case list, the input generator, the constants read from the kernel sources and the host-side prediction of the branch a case takes live here
too and are shared by the CPU and the GPU test files.
"""
from __future__ import annotations

import os
import re
import types

import numpy as np
import torch

SLOPE = 0.2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ================================================================================================ reference formulas
def edge_vec(W_edge, att_edge):
    """v[d] = sum_c W_edge[c, d] att_edge[c]  (W_edge = lin_edge.weight [C, D])."""
    return (W_edge * att_edge.unsqueeze(1)).sum(dim=0)


def node_alpha(h, att_src, att_dst):
    return (h * att_src).sum(dim=1), (h * att_dst).sum(dim=1)


def loop_attr(ea, tgt, n):
    cnt = torch.zeros(n, dtype=ea.dtype).index_add_(0, tgt, torch.ones(tgt.shape[0], dtype=ea.dtype))
    return torch.zeros(n, ea.shape[1], dtype=ea.dtype).index_add_(0, tgt, ea) / cnt.clamp(min=1.0).unsqueeze(1)


def pre_activations(a_src, a_dst, v, ea, src, tgt, n):
    """Arguments of the LeakyReLU: per kept edge and per self loop."""
    pre_e = a_src.index_select(0, src) + a_dst.index_select(0, tgt) + (ea * v).sum(dim=1)
    pre_s = a_src + a_dst + (loop_attr(ea, tgt, n) * v).sum(dim=1)
    return pre_e, pre_s


def aggregate(h, att_src, att_dst, v, bias, ea, src, tgt, n, slope=SLOPE):
    """-> out [n, C], alpha [K] (per kept edge), alpha_self [n]."""
    a_src, a_dst = node_alpha(h, att_src, att_dst)
    pre_e, pre_s = pre_activations(a_src, a_dst, v, ea, src, tgt, n)
    le, ls = torch.nn.functional.leaky_relu(pre_e, slope), torch.nn.functional.leaky_relu(pre_s, slope)
    mx = ls.detach().clone().scatter_reduce(0, tgt, le.detach(), "amax", include_self=True)
    ex_e, ex_s = torch.exp(le - mx.index_select(0, tgt)), torch.exp(ls - mx)
    den = ex_s + torch.zeros(n, dtype=h.dtype).index_add_(0, tgt, ex_e) + 1e-16
    alpha, alpha_self = ex_e / den.index_select(0, tgt), ex_s / den
    out = alpha_self.unsqueeze(1) * h + torch.zeros_like(h).index_add_(0, tgt, alpha.unsqueeze(1) * h.index_select(0, src))
    if bias is not None:
        out = out + bias
    return out, alpha, alpha_self


def bond_csr(edge_index, n):
    """numpy.  Per target: (source, edge id) ascending; per source: ascending by-target position.  Self loops and endpoints outside [0, n) are dropped."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    s, t = ei[0], ei[1]
    ids = np.nonzero((s != t) & (s >= 0) & (t >= 0) & (s < n) & (t < n))[0]
    order = ids[np.lexsort((ids, s[ids], t[ids]))]
    col, eid, tgt = s[order], order, t[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n))])
    pos = np.arange(len(order))
    t_pos = pos[np.lexsort((pos, col))]
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))])
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    return types.SimpleNamespace(n=n, K=len(order), rowptr=i32(rowptr), col=i32(col), eid=i32(eid), tgt=i32(tgt), t_rowptr=i32(t_rowptr),
                                 t_pos=i32(t_pos), t_tgt=i32(tgt[t_pos]), indeg=np.diff(rowptr), outdeg=np.diff(t_rowptr))


# ================================================================================================ constants of the kernels, read from their sources
_K = None


def constants():
    global _K
    if _K is None:
        gat = open(os.path.join(ROOT, "conan-fgw_amd", "csrc", "gat.hip")).read()
        graph = open(os.path.join(ROOT, "conan-fgw_amd", "csrc", "graph.hip")).read()
        num = lambda pat, text: int(eval(re.search(pat, text).group(1), {}))            # "36 * 1024" -> 36864
        stage = set(re.findall(r"\(deg <= (\d+)\)", gat))                              # the one-edge-per-lane limit of the wavefront kernels
        assert len(stage) == 1, stage
        _K = types.SimpleNamespace(
            MD=num(r"#define CONAN_GAT_MD (\d+)", gat), WGS=num(r"constexpr int GAT_BW_WGS = (\d+);", gat),
            WAVES_PER_WG=num(r"GAT_BW_WAVES = (\d+) \* GAT_BW_WGS;", gat), GROUPS_PER_WG=num(r"ngroups = gridDim\.x \* (\d+);", gat),
            STAGE=int(stage.pop()), MAXD=num(r"constexpr int GAT_MAXD = (\d+);", gat), MAXC=num(r"channels > (\d+) \|\|", gat),
            G16_WIDTHS=sorted(int(x) for x in set(re.findall(r"channels == (\d+)", gat))), G16_MAXD=num(r"if \(edge_dim <= (\d+) &&", gat),
            SCAN_LDS_MAX=num(r"constexpr int SCAN_LDS_MAX = ([\d *]+);", graph), SCAN_THREADS=num(r"constexpr int SCAN_THREADS = (\d+);", graph),
            SCAN_REGS=num(r"constexpr int MAXC = (\d+);", graph))
        _K.WAVES = _K.WAVES_PER_WG * _K.WGS
        _K.G16_PASS = _K.GROUPS_PER_WG * _K.WGS
    return _K


# every branch that at least one case must take (the closing GPU test and the CPU test both demand it)
REQUIRED_BRANCHES = {
    "g16/target/staged", "g16/target/serial", "g16/source/staged", "g16/source/serial",
    "wave4/target/staged", "wave4/target/serial", "wave8/target/staged", "wave8/target/serial", "wave/source/staged", "wave/source/serial",
    "wave/partial-channel-pass", "fwd/staged", "fwd/serial", "fwd/partial-channel-pass", "g16/second-pass", "wave/second-pass", "scan/long",
}


def scan_branch(n):
    """launch_exclusive_scan: 'lds' (one workgroup through LDS), 'long' (the same beyond the 64 KB that need no attribute — every n > 32 768 is
    here or further), 'global' (n > SCAN_LDS_MAX: chunks walked in global memory, serially once they outgrow the register array)."""
    k = constants()
    if n > k.SCAN_LDS_MAX:
        return "global"
    return "long" if (n + 16) * 4 > 64 * 1024 and n > k.SCAN_REGS * k.SCAN_THREADS else "lds"


def branches(C, D, n, indeg, outdeg, backward=True):
    """The kernels and row paths a call takes, predicted on the host from the dispatch arithmetic of conan_gat_aggregate_fwd / _bwd."""
    k, b = constants(), set()
    indeg, outdeg = np.asarray(indeg), np.asarray(outdeg)
    pick = lambda deg, lim, name: ({name + "/staged"} if (deg <= lim).any() else set()) | ({name + "/serial"} if (deg > lim).any() else set())
    b |= pick(indeg, k.STAGE, "fwd")
    if C % 64 and ((indeg > C % 64) & (indeg <= k.STAGE)).any():
        b.add("fwd/partial-channel-pass")          # staged row whose edges sit in lanes that own no channel in the last channel pass
    if backward:
        if D <= k.G16_MAXD and C in k.G16_WIDTHS:
            b |= pick(indeg, k.MD, "g16/target") | pick(outdeg, k.MD, "g16/source")
            if n > k.G16_PASS:
                b.add("g16/second-pass")
        else:
            b |= pick(indeg, k.STAGE, "wave4/target" if D <= 4 else "wave8/target") | pick(outdeg, k.STAGE, "wave/source")
            if C % 64 and ((outdeg > C % 64) & (outdeg <= k.STAGE)).any():
                b.add("wave/partial-channel-pass")
            if n > k.WAVES:
                b.add("wave/second-pass")
    b.add("scan/" + scan_branch(n))
    return b


# ================================================================================================ graphs
DEGREES = [0, 1, 5, 6, 7, 31, 32, 33, 63, 64, 65, 150]


def degree_graph():
    """Directed, no multi-edges, n = 390.  Node k < 12 has in-degree DEGREES[k] and out-degree 0; node 12 + k has out-degree DEGREES[k] and in-degree 0;
    node 24 (the hub) has in-degree 150 AND out-degree 150; the other endpoints are drawn from the pool 25 .. 389, whose nodes are joined among
    themselves by p -> p + 1 and p -> p + 3 (around the pool) and so end up with a few edges either way."""
    rng = np.random.RandomState(7)
    n, pool = 390, np.arange(25, 390)
    src, tgt = [], []
    for k, d in enumerate(DEGREES + [150]):
        i = 24 if k == 12 else k
        src += rng.choice(pool, d, replace=False).tolist(); tgt += [i] * d
    for k, d in enumerate(DEGREES + [150]):
        j = 24 if k == 12 else 12 + k
        tgt += rng.choice(pool, d, replace=False).tolist(); src += [j] * d
    for o in (1, 3):
        src += pool.tolist(); tgt += (25 + (pool - 25 + o) % len(pool)).tolist()
    ei = np.array([src, tgt], np.int64)
    return ei[:, rng.permutation(ei.shape[1])], n


def chain_graph(n, seed):
    """i <- i +- 1, i +- 2 with a fifth of the edges removed: in- and out-degree 0 .. 4, different from each other."""
    rng = np.random.RandomState(seed)
    i = np.arange(n)
    src = np.concatenate([i + o for o in (-2, -1, 1, 2)]); tgt = np.concatenate([i] * 4)
    keep = (src >= 0) & (src < n) & (rng.rand(len(src)) > 0.2)
    ei = np.array([src[keep], tgt[keep]], np.int64)
    return ei[:, rng.permutation(ei.shape[1])], n


def random_graph(n, maxdeg, seed):
    rng = np.random.RandomState(seed)
    src, tgt = [], []
    for i in range(n):
        for j in rng.choice(n, rng.randint(0, maxdeg + 1), replace=False):
            if j != i:
                src.append(int(j)); tgt.append(i)
    return np.array([src, tgt], np.int64).reshape(2, -1), n


def multi_graph(invalid=False):
    """Triple edges 1->0 and 5->4 (different attributes), a double edge 2->3, self loops in between (they shift the edge ids), ordinary edges; with
    `invalid` also an endpoint equal to n and one equal to -1 (the CSR drops them; the float kernels never see such a graph)."""
    n = 9
    e = [(1, 0), (3, 3), (1, 0), (2, 3), (0, 0), (5, 4), (1, 0), (2, 3), (6, 6), (5, 4), (4, 5), (7, 0), (5, 4), (8, 8), (0, 7), (2, 0), (6, 4)]
    if invalid:
        e = e[:4] + [(n, 2)] + e[4:9] + [(3, -1)] + e[9:] + [(-1, n)]
    return np.array(e, np.int64).T.copy(), n


# ================================================================================================ cases
class Case:
    def __init__(self, name, graph, C, D, seed, bias=True, scale=1.0, extreme=False, backward=True, simple=True, large=False):
        self.name, (self.ei, self.n), self.C, self.D, self.seed = name, graph, C, D, seed
        self.bias, self.scale, self.extreme, self.backward, self.simple, self.large = bias, scale, extreme, backward, simple, large
        self.E = int(self.ei.shape[1])
        self.csr = bond_csr(self.ei, self.n)

    def branches(self):
        return branches(self.C, self.D, self.n, self.csr.indeg, self.csr.outdeg, self.backward)


WIDTHS_G16, WIDTHS_WAVE = [64, 128, 256], [32, 96, 200, 8]
# SEEDS: the cases of one or five rows with edges (tiny/n2, multi) use the first seed of 310 + C + 1000 k (340 + C + 1000 k) for which the reference
# alone meets the conditions that tests/test_gat_ref_cpu.py asserts (the one edge and its self loop on different sides of the kink; fp32
# reference within half its cap); every other case met them with the seed it was first given.
_CASES = None


def cases():
    """name -> Case.  `simple`: no multi-edges, so a permuted edge_index must give the same bits."""
    global _CASES
    if _CASES is None:
        deg, out = degree_graph(), []
        for C in WIDTHS_G16 + WIDTHS_WAVE:
            out.append(Case(f"degree/C{C}/D3", deg, C, 3, 100 + C))
        for C in (64, 96):
            for D in (1, 4, 5, 8):
                out.append(Case(f"degree/C{C}/D{D}", deg, C, D, 200 + C + D))
        out.append(Case("degree/C320/D3/forward", deg, 320, 3, 320, backward=False))
        for C in (64, 96):
            out.append(Case(f"tiny/n1/C{C}", (np.zeros((2, 0), np.int64), 1), C, 3, 300 + C))
            out.append(Case(f"tiny/n2/C{C}", (np.array([[1], [0]], np.int64), 2), C, 3, {64: 6374, 96: 2406}[C]))      # seeds: see SEEDS below
            out.append(Case(f"tiny/E0/C{C}", (np.zeros((2, 0), np.int64), 40), C, 3, 320 + C))
            out.append(Case(f"tiny/nobias/C{C}", random_graph(30, 8, 5), C, 3, 330 + C, bias=False))
            out.append(Case(f"multi/C{C}", multi_graph(), C, 3, {64: 1404, 96: 3436}[C], simple=False))
            out.append(Case(f"extreme/C{C}", random_graph(60, 8, 6), C, 3, 350 + C, scale=2.0, extreme=True))
        out.append(Case("large/n33000/C64", chain_graph(33000, 1), 64, 3, 401, large=True))
        out.append(Case("large/n8300/C96", chain_graph(8300, 2), 96, 3, 402, large=True))
        _CASES = {c.name: c for c in out}
    return _CASES


def extreme_rows(csr):
    """Rows of the `extreme` cases that are set by hand: all pre-activations negative / the self loop holds the maximum / one exp underflows.  The
    first three rows of three or more edges none of which is the first neighbour of a later one."""
    rows = [i for i in range(csr.n) if csr.indeg[i] >= 3]
    neg, smax = rows[0], rows[1]
    under = next(i for i in rows[2:] if int(csr.col[csr.rowptr[i]]) not in (neg, smax))
    return types.SimpleNamespace(negative=neg, self_max=smax, underflow=under)


def _kept(inp, csr):
    src, tgt = torch.from_numpy(csr.col.astype(np.int64)), torch.from_numpy(csr.tgt.astype(np.int64))
    return src, tgt, inp["ea"].index_select(0, torch.from_numpy(csr.eid.astype(np.int64)))


def pre_of(inp, csr, dt=torch.float64):
    src, tgt, ea = _kept(inp, csr)
    a_s, a_d = node_alpha(inp["h"].to(dt), inp["att_src"].to(dt), inp["att_dst"].to(dt))
    return pre_activations(a_s, a_d, edge_vec(inp["W_edge"].to(dt), inp["att_edge"].to(dt)), ea.to(dt), src, tgt, csr.n)


KINK_FLOOR = 1e-4            # no pre-activation closer to 0 than this fraction of the RMS pre-activation (condition (b) of the CPU test)


def make_inputs(case):
    """fp32 CPU tensors: h, att_src, att_dst, W_edge, att_edge, bias | None, ea [E, D] (per ORIGINAL edge), dout, dv_in (the dv handed to edge_vec_bwd).
    Deterministic.  Pre-activations that land within 2 * KINK_FLOOR of the LeakyReLU kink are moved off it by adding 1/16 to an attribute of the edge
    (or of the row's first edge, for a self loop; to h_i itself for a node without edges): fp32 and fp64 then take the same branch everywhere."""
    gen = torch.Generator().manual_seed(case.seed)
    n, C, D, E, csr = case.n, case.C, case.D, case.E, case.csr
    rn = lambda *s: torch.randn(*s, generator=gen)
    inp = {"h": rn(n, C), "att_src": rn(C) * (case.scale / C ** 0.5), "att_dst": rn(C) * (case.scale / C ** 0.5), "W_edge": rn(C, D) / C ** 0.5,
           "att_edge": rn(C), "bias": 0.3 * rn(C) if case.bias else None, "ea": 0.5 * rn(E, D), "dv_in": rn(D)}
    inp["dout"] = rn(n, C) * torch.exp(0.5 * rn(n, 1))
    if case.extreme:
        s, d = inp["att_src"], inp["att_dst"]
        both = (s + d) / float((s + d).square().sum())
        x = extreme_rows(csr)
        inp["h"][x.negative] = -70.0 * both                 # a_src + a_dst = -70: the self loop, and a_dst ~ -35 under every incoming edge
        inp["h"][x.self_max] = 90.0 * both
        j = int(csr.col[csr.rowptr[x.underflow]])           # first neighbour of the underflow row: a_src[j] = +110, the others stay ~ N(0, 2)
        inp["h"][j] = 110.0 * s / float(s.square().sum())
    for _ in range(40):
        pre_e, pre_s = pre_of(inp, csr)
        allp = torch.cat([pre_e, pre_s])
        floor = 2 * KINK_FLOOR * float(allp.square().mean().sqrt())
        bad_e, bad_s = (pre_e.abs() < floor).nonzero().view(-1).tolist(), (pre_s.abs() < floor).nonzero().view(-1).tolist()
        if not bad_e and not bad_s:
            break
        for p in bad_e:
            inp["ea"][int(csr.eid[p]), 0] += 0.0625
        for i in bad_s:
            if csr.indeg[i]:
                inp["ea"][int(csr.eid[csr.rowptr[i]]), 0] += 0.0625
            else:
                inp["h"][i] += 0.0625 * torch.sign(inp["att_src"] + inp["att_dst"])
    else:
        raise AssertionError(("pre-activations could not be moved off the kink", case.name))
    return inp


OUTPUTS_FWD = ["v", "a_src", "a_dst", "out", "alpha", "alpha_self", "rowsum"]
OUTPUTS_BWD = ["dh", "d_att_src", "d_att_dst", "d_bias", "dv", "dW_edge", "d_att_edge"]


def rowsum(alpha, alpha_self, tgt, n):
    """alpha_self + the alphas of the row's kept edges, summed in the dtype given: 1 up to rounding."""
    return alpha_self + torch.zeros(n, dtype=alpha.dtype).index_add_(0, tgt, alpha)


def reference(case, inp):
    """{"64": {...}, "32": {...}}: every output of OUTPUTS_FWD (+ OUTPUTS_BWD) in fp64 and in fp32 on the CPU.  Per-node and per-edge scalars come back
    as columns ([n, 1], [K, 1]), so that visnet_ref.judge looks at every entry on its own."""
    src, tgt, ea = _kept(inp, case.csr)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        leaf = lambda key: None if inp[key] is None else inp[key].to(dt).clone().requires_grad_(True)
        h, a_s, a_d, W, a_e, bias = (leaf(k) for k in ("h", "att_src", "att_dst", "W_edge", "att_edge", "bias"))
        v = edge_vec(W, a_e)
        vl = v.detach().clone().requires_grad_(True)
        al_s, al_d = node_alpha(h, a_s, a_d)
        out, alpha, alpha_self = aggregate(h, a_s, a_d, vl, bias, ea.to(dt), src, tgt, case.n, SLOPE)
        col = lambda t: t.detach().unsqueeze(1)
        r = {"v": v.detach(), "a_src": col(al_s), "a_dst": col(al_d), "out": out.detach(), "alpha": col(alpha), "alpha_self": col(alpha_self),
             "rowsum": col(rowsum(alpha.detach(), alpha_self.detach(), tgt, case.n))}
        if case.backward:
            wrt = [h, a_s, a_d, vl] + ([bias] if bias is not None else [])
            g = torch.autograd.grad(out, wrt, inp["dout"].to(dt))
            r.update(dh=g[0], d_att_src=g[1], d_att_dst=g[2], dv=g[3], d_bias=g[4] if bias is not None else inp["dout"].to(dt).sum(dim=0))
            r["dW_edge"], r["d_att_edge"] = torch.autograd.grad(v, [W, a_e], inp["dv_in"].to(dt))
        res[tag] = r
    return res


def permuted(case, inp, seed=1):
    """The same graph with edge_index (and the attributes with it) in another order."""
    perm = np.random.RandomState(seed).permutation(case.E)
    c = Case(case.name + "/permuted", (case.ei[:, perm].copy(), case.n), case.C, case.D, case.seed, case.bias, case.scale, case.extreme, case.backward,
             case.simple, case.large)
    q = dict(inp)
    q["ea"] = inp["ea"][torch.from_numpy(perm)].contiguous()
    return c, q
