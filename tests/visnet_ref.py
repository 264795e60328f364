"""TEST INFRASTRUCTURE — plain reference formulas of the ViSNet kernels (csrc/visnet.hip, csrc/visnet_bwd.hip), one small function per kernel.

Every function is written with plain torch indexing on whatever dtype it is given (index_select / index_add_ / sum; no fusion): called with
float64 it is the reference ("ref64"), called with float32 on the CPU it is the yardstick ("ref32") a kernel's error is measured against.
Backward references are torch.autograd.grad of the same function.  Formulas: include/conan_fgw_hip.h (the two ViSNet sections), restated in
oracle/visnet.py; tests/test_visnet_ref_cpu.py composes them into the oracle's modules and demands 1e-12 agreement in fp64.

Conventions: edges are a CSR by target WITH self loops; a self loop has d_ij = 0 and factor 0 in neighbor_scale but takes part in
attn_message / vec_aggregate / edge_embed / edge_update; pre_act = 1 means SiLU is applied to dk, dv / s / t on load (gradients are then
w.r.t. the pre-activations); spatial_norm has the zero sub-gradient at the origin; vector tensors are [n, 3, H].

The case list (graphs, widths, flags) and the input generators live here too and are shared by the CPU and the GPU test files.
"""
from __future__ import annotations

import math

import numpy as np
import torch

CUTOFF, CAP = 5.0, 32
S_ROW = 1.0              # rows are randn * exp(S_ROW * randn): scales spread over ~ e^-3 .. e^3, SiLU arguments up to |x| ~ 60
COND_CAP = 2e-6          # an input whose fp32 REFERENCE is worse than this (whole tensor) is too ill-conditioned to judge a kernel by
MARGIN_ROW, MARGIN_ALL = 8.0, 4.0      # err <= MARGIN * yard (see judge); DESIGN.md holds the measured ratios
NODE_PASS, EDGE_PASS = 16384, 262144   # first grid pass: nblk() caps a grid at 4096 blocks of 4 wavefronts; edge kernels walk 16 edges per wavefront


# ================================================================================================ reference formulas
def silu(x):
    return x * torch.sigmoid(x)


def cosine_cutoff(d, cutoff=CUTOFF):
    return 0.5 * (torch.cos(d * math.pi / cutoff) + 1.0) * (d < cutoff).to(d.dtype)


def edge_unit(pos, src, tgt):
    d = pos.index_select(0, src) - pos.index_select(0, tgt)
    loop = (src == tgt).unsqueeze(1)
    nrm = torch.sqrt((d * d).sum(dim=1, keepdim=True))
    return torch.where(loop, torch.zeros_like(d), d / torch.where(loop, torch.ones_like(nrm), nrm))


def expnormal_params(num_rbf, cutoff=CUTOFF):
    start = torch.exp(torch.tensor(-cutoff))
    return torch.linspace(start, 1, num_rbf), torch.tensor([(2 / num_rbf * (1 - start)) ** -2] * num_rbf), 5.0 / cutoff


def expnormal(dist, means, betas, alpha, cutoff=CUTOFF):
    d = dist.unsqueeze(1)
    return cosine_cutoff(d, cutoff) * torch.exp(-betas * (torch.exp(alpha * (-d)) - means) ** 2)


def neighbor_scale(W, dist, src, tgt, cutoff=CUTOFF):
    return W * (cosine_cutoff(dist, cutoff) * (src != tgt).to(W.dtype)).unsqueeze(1)


def concat2(a, b):
    return torch.cat([a, b], dim=1)


def edge_embed(x, p, src, tgt):
    return (x.index_select(0, tgt) + x.index_select(0, src)) * p


def layernorm(x, gamma, beta, eps):
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def scale_channels(v, w):
    return v * w


def vecdot(vp, H):
    return (vp[..., :H] * vp[..., H:2 * H]).sum(dim=1)


def attn_message(q, k, v, dk, dv, src, tgt, dist, n, heads, pre_act, cutoff=CUTOFF):
    E, H = dk.shape
    if pre_act:
        dk, dv = silu(dk), silu(dv)
    a = (q.index_select(0, tgt) * k.index_select(0, src) * dk).view(E, heads, H // heads).sum(dim=2)
    a = silu(a) * cosine_cutoff(dist, cutoff).unsqueeze(1)
    vmsg = ((v.index_select(0, src) * dv).view(E, heads, H // heads) * a.unsqueeze(2)).reshape(E, H)
    return vmsg, torch.zeros(n, H, dtype=vmsg.dtype).index_add_(0, tgt, vmsg)


def vec_aggregate(vec, s, dvec, src, tgt, pre_act):
    H = vec.shape[2]
    if pre_act:
        s = silu(s)
    s1, s2 = s[:, :H], s[:, H:]
    vec_j = vec.index_select(0, src) * s1.unsqueeze(1) + s2.unsqueeze(1) * dvec.unsqueeze(2)
    return torch.zeros_like(vec).index_add_(0, tgt, vec_j)


def node_update(x, vec, vdot, o, vp, vagg):
    H = x.shape[1]
    o1, o2, o3 = o[:, :H], o[:, H:2 * H], o[:, 2 * H:]
    return x + (vdot * o2 + o3), vec + (vp[..., 2 * H:] * o1.unsqueeze(1) + vagg)


def edge_update(wt, ws, t, dvec, src, tgt, pre_act, f):
    d = dvec.unsqueeze(2)
    a, b = wt.index_select(0, tgt), ws.index_select(0, src)
    w1 = a - (a * d).sum(dim=1, keepdim=True) * d
    w2 = b - (b * (-d)).sum(dim=1, keepdim=True) * (-d)
    return f + (silu(t) if pre_act else t) * (w1 * w2).sum(dim=1)


def spatial_norm(v):
    return torch.norm(v, dim=1)


def gate(u, v2, act):
    O = v2.shape[2]
    x, g = u[:, :O], u[:, O:]
    return (silu(x) if act else x), g.unsqueeze(1) * v2


def prior(x, z, atomref, std):
    return x * std + atomref.index_select(0, z)


# ================================================================================================ graphs
class Graph:
    """Edge list in CSR-by-target order with what the kernels get from ops.RadiusGraph + conan_visnet_edge_unit (all fp32)."""

    def __init__(self, n, src, tgt, dist, dvec, pos=None, batch=None):
        self.n, self.src, self.tgt, self.dist, self.dvec, self.pos, self.batch = n, src, tgt, dist, dvec, pos, batch

    @property
    def E(self):
        return int(self.src.shape[0])

    def tail(self, n0):
        """Sub-graph of the nodes >= n0 (n0 starts a molecule: no edge crosses it), re-based to 0; and its first edge."""
        e0 = int((self.tgt < n0).sum())
        assert int(self.src[e0:].min()) >= n0
        return Graph(self.n - n0, self.src[e0:] - n0, self.tgt[e0:] - n0, self.dist[e0:], self.dvec[e0:], None if self.pos is None else self.pos[n0:]), e0


def graph_on_cpu(pos, batch):
    """The oracle's radius graph with self loops (the cap counts the atom itself) + fp32 distances and unit vectors."""
    from oracle.pyg_semantics import radius_graph
    p = torch.from_numpy(np.ascontiguousarray(pos, np.float32))
    b = torch.from_numpy(np.asarray(batch, np.int64))
    ei = radius_graph(p, CUTOFF, b, loop=True, max_num_neighbors=CAP)
    src, tgt = ei[0].contiguous(), ei[1].contiguous()
    d = p.index_select(0, src) - p.index_select(0, tgt)
    return Graph(p.shape[0], src, tgt, torch.sqrt((d * d).sum(dim=1)), edge_unit(p, src, tgt), p, b)


def _cluster(rng, m, side=4, spacing=0.7, jitter=0.12):
    """m atoms on a jittered lattice, by default 4x4x4 of spacing 0.7: every pair is 0.4 .. 4.1 apart, i.e. inside the cutoff and not degenerate."""
    idx = rng.choice(side ** 3, size=m, replace=False)
    p = np.stack([idx // side ** 2, (idx // side) % side, idx % side], axis=1) * spacing + rng.uniform(-jitter, jitter, size=(m, 3))
    return p.astype(np.float32)


def _molecules(rng, sizes):
    pos = [_cluster(rng, m) for m in sizes]
    return np.concatenate(pos), np.concatenate([np.full(m, g) for g, m in enumerate(sizes)]).astype(np.int64)


def wide_sizes(clusters):
    return [19 + (c % 3) for c in range(clusters)]


def graph_case(name):
    """(pos [n,3] fp32, batch [n] int64, expected edge count or None)."""
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "tiny":                       # a row that is only its self loop; E = 1 + 4 + 9 < 16
        return _molecules(rng, [1, 2, 3]) + (14,)
    if name == "partial_run1":               # 49 = 3 * 16 + 1
        return _molecules(rng, [7]) + (49,)
    if name == "partial_run13":              # 25 + 36 = 3 * 16 + 13
        return _molecules(rng, [5, 6]) + (61,)
    if name == "isolated":                   # the last atom of molecule 0 is 20 away from the rest: only its self loop
        pos, batch = _molecules(rng, [7, 4])
        pos[6] += np.float32([20.0, 0, 0])
        return pos, batch, 36 + 1 + 16
    if name == "capped":                     # 40 atoms inside the cutoff: every row truncated to 32; max_edges = 53 * 32 = 1696
        return _molecules(rng, [40, 5, 3, 2, 2, 1]) + (40 * 32 + 25 + 9 + 4 + 4 + 1,)
    if name == "long_lists":                 # 80 atoms inside the cutoff (5x5x5 lattice of spacing 0.5: pairs 0.38 .. 3.7 apart): a row keeps its 32 lowest
        big = _cluster(rng, 80, side=5, spacing=0.5, jitter=0.06)      # sources, so atoms 0 .. 31 are sources of all 80 rows: by-source lists of 80 > one 64-edge chunk
        pos, batch = _molecules(rng, [5])
        return np.concatenate([big, pos]), np.concatenate([np.zeros(80, np.int64), batch + 1]), 80 * 32 + 25
    if name == "ragged":                     # as tests/test_gpu_edge_cases.py
        pos, batch, g = [], [], 0
        for m in [4, 30, 2, 17]:
            for _ in range(3):
                pos.append(rng.uniform(0, 3.0 + m ** (1 / 3), size=(m, 3)).astype(np.float32)); batch.append(np.full(m, g)); g += 1
        return np.concatenate(pos), np.concatenate(batch).astype(np.int64), None
    if name in ("wide", "wide_small"):       # 822 clusters of 19 .. 21 atoms: 16 440 nodes, 329 348 edges (every cluster is complete)
        sizes = wide_sizes(822 if name == "wide" else 30)
        return _molecules(rng, sizes) + (sum(m * m for m in sizes),)
    raise KeyError(name)


GRAPHS = ["tiny", "partial_run1", "partial_run13", "isolated", "capped", "ragged", "long_lists"]


# ================================================================================================ ops: inputs + reference
def rows(gen, r, *w, s=S_ROW):
    x = torch.randn(r, *w, generator=gen)
    return x * torch.exp(s * torch.randn(r, *([1] * len(w)), generator=gen))


class Op:
    """make(gen, G, H, fl) -> [(tensor, differentiable, kind)], kind 'E' edge rows / 'N' other rows / 'C' constant;  fn(G, H, fl, *inputs) -> tuple;
    out_kinds: one letter per output."""

    def __init__(self, name, make, fn, graph, out_kinds):
        self.name, self.make, self.fn, self.graph, self.out_kinds = name, make, fn, graph, out_kinds


def _g(G, t):      # the graph's fp32 geometry in the dtype of the call
    return G.dist.to(t.dtype), G.dvec.to(t.dtype)


def _mk_attn(gen, G, H, fl):
    return [(rows(gen, G.n, H), True, "N") for _ in range(3)] + [(rows(gen, G.E, H), True, "E") for _ in range(2)]


def _mk_node_update(gen, G, H, fl):
    n = G.n
    ins = [(rows(gen, n, H), True, "N"), (rows(gen, n, 3, H), True, "N")]
    if fl["vdot"] == "free":
        ins.append((rows(gen, n, H), True, "N"))
    return ins + [(rows(gen, n, 3 * H), True, "N"), (rows(gen, n, 3, 3 * H), True, "N"), (rows(gen, n, 3, H), True, "N")]


def _fn_node_update(G, H, fl, x, vec, *rest):
    if fl["vdot"] == "free":
        vdot, o, vp, vagg = rest
    else:
        o, vp, vagg = rest
        vdot = vecdot(vp, H)
    return node_update(x, vec, vdot, o, vp, vagg)


def _mk_spatial(gen, G, H, fl):
    v = rows(gen, G.n, 3, H)
    v[::3, :, ::5] = 0.0                     # exactly-zero vectors: norm 0, zero sub-gradient
    return [(v, True, "N")]


def _mk_layernorm(gen, G, H, fl):
    return [(rows(gen, G.n, H) + 0.5 * rows(gen, G.n, 1), True, "N"), (1.0 + 0.3 * torch.randn(H, generator=gen), True, "C"), (0.3 * torch.randn(H, generator=gen), True, "C")]


def _fn_layernorm(G, H, fl, x, gamma, beta):
    y = layernorm(x, gamma, beta, 1e-5)
    return (y, x.clone()) if fl["tap"] else (y,)


def _fn_scale(G, H, fl, v, w):
    y = scale_channels(v, w)
    return (y, v.clone()) if fl["tap"] else (y,)


def _mk_prior(gen, G, H, fl):
    z = torch.randint(1, 20, (G.n,), generator=gen)
    return [(rows(gen, G.n, H), True, "N"), (torch.randn(100, 1, generator=gen), True, "C"), (z, False, "C"), (torch.tensor(1.7), False, "C")]


def _mk_expnormal(gen, G, H, fl):
    means, betas, _ = expnormal_params(H)
    return [(G.dist.clone(), False, "E"), (means, False, "C"), (betas, False, "C")]


OPS = {o.name: o for o in [
    Op("edge_unit", lambda gen, G, H, fl: [(G.pos.clone(), False, "N")], lambda G, H, fl, pos: (edge_unit(pos, G.src, G.tgt),), True, "E"),
    Op("expnormal", _mk_expnormal, lambda G, H, fl, d, m, b: (expnormal(d, m, b, 5.0 / CUTOFF),), True, "E"),
    Op("neighbor_scale", lambda gen, G, H, fl: [(rows(gen, G.E, H), True, "E")],
       lambda G, H, fl, W: (neighbor_scale(W, _g(G, W)[0], G.src, G.tgt),), True, "E"),
    Op("edge_embed", lambda gen, G, H, fl: [(rows(gen, G.n, H), True, "N"), (rows(gen, G.E, H), True, "E")],
       lambda G, H, fl, x, p: (edge_embed(x, p, G.src, G.tgt),), True, "E"),
    Op("attn_message", _mk_attn,
       lambda G, H, fl, q, k, v, dk, dv: attn_message(q, k, v, dk, dv, G.src, G.tgt, _g(G, q)[0], G.n, fl["heads"], fl["pre_act"]), True, "EN"),
    Op("vec_aggregate", lambda gen, G, H, fl: [(rows(gen, G.n, 3, H), True, "N"), (rows(gen, G.E, 2 * H), True, "E")],
       lambda G, H, fl, vec, s: (vec_aggregate(vec, s, _g(G, s)[1], G.src, G.tgt, fl["pre_act"]),), True, "N"),
    Op("edge_update", lambda gen, G, H, fl: [(rows(gen, G.n, 3, H), True, "N"), (rows(gen, G.n, 3, H), True, "N"), (rows(gen, G.E, H), True, "E"), (rows(gen, G.E, H), True, "E")],
       lambda G, H, fl, wt, ws, t, f: (edge_update(wt, ws, t, _g(G, t)[1], G.src, G.tgt, fl["pre_act"], f),), True, "E"),
    Op("node_update", _mk_node_update, _fn_node_update, False, "NN"),
    Op("vecdot", lambda gen, G, H, fl: [(rows(gen, G.n, 3, 3 * H), True, "N")], lambda G, H, fl, vp: (vecdot(vp, H),), False, "N"),
    Op("layernorm", _mk_layernorm, _fn_layernorm, False, "NN"),
    Op("scale_channels", lambda gen, G, H, fl: [(rows(gen, G.n, 3, H), True, "N"), (1.0 + 0.3 * torch.randn(H, generator=gen), False, "C")], _fn_scale, False, "NN"),
    Op("concat2", lambda gen, G, H, fl: [(rows(gen, G.n, H), True, "N"), (rows(gen, G.n, fl["Hb"]), True, "N")], lambda G, H, fl, a, b: (concat2(a, b),), False, "N"),
    Op("spatial_norm", _mk_spatial, lambda G, H, fl, v: (spatial_norm(v),), False, "N"),
    Op("gate", lambda gen, G, H, fl: [(rows(gen, G.n, 2 * H), True, "N"), (rows(gen, G.n, 3, H), True, "N")], lambda G, H, fl, u, v2: gate(u, v2, fl["act"]), False, "NN"),
    Op("prior", _mk_prior, lambda G, H, fl, x, a, z, std: (prior(x, z, a, std.to(x.dtype)),), False, "N"),
    Op("silu", lambda gen, G, H, fl: [(rows(gen, G.n, H), True, "N")], lambda G, H, fl, x: (silu(x),), False, "N"),
]}

BITWISE = {"concat2"}                        # pure data movement: outputs and gradients must equal torch fp32 bit for bit


class Rows:
    """Stand-in for a graph for the kernels that only take a row count."""

    def __init__(self, n):
        self.n, self.E = n, 0


def reference(op, G, H, fl, seed, spec=None, gouts=None):
    """Inputs, output gradients, and the op's outputs + input gradients in fp64 and in fp32 (CPU).  `spec` / `gouts`: given inputs and output
    gradients (the `wide` case hands in slices of what the GPU ran on) instead of generated ones."""
    gen = torch.Generator().manual_seed(seed)
    spec = op.make(gen, G, H, fl) if spec is None else spec
    res = {"ins": [t for t, _, _ in spec], "diff": [d for _, d, _ in spec], "kinds": [k for _, _, k in spec], "gouts": gouts}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        xs = [(t.to(dt) if t.is_floating_point() else t).clone().requires_grad_(d) for t, d, _ in spec]
        outs = op.fn(G, H, fl, *xs)
        if res["gouts"] is None:
            res["gouts"] = [rows(gen, *o.shape) for o in outs]
        dx = [x for x, d in zip(xs, res["diff"]) if d]
        grads = torch.autograd.grad(outs, dx, [g.to(dt) for g in res["gouts"]], allow_unused=True) if dx else ()
        res["out" + tag] = [o.detach() for o in outs]
        res["grad" + tag] = [torch.zeros_like(x) if g is None else g.detach() for x, g in zip(dx, grads)]
    return res


# ================================================================================================ judging
def _rows2d(t):
    t = t.detach().to(torch.float64).cpu()
    return t.reshape(t.shape[0], -1) if t.dim() >= 2 else t.reshape(1, -1)


def row_err(a, ref):
    """max over rows ||a_row - ref_row|| in units of ref's RMS row norm (an all-zero row then does not divide by zero)."""
    a, ref = _rows2d(a), _rows2d(ref)
    if ref.numel() == 0:
        return 0.0
    scale = float(torch.sqrt((ref * ref).sum(dim=1).mean()))
    return float(torch.sqrt(((a - ref) ** 2).sum(dim=1)).max()) / (scale if scale > 0 else 1.0)


def all_err(a, ref):
    a, ref = _rows2d(a), _rows2d(ref)
    nb = float(ref.norm())
    return float((a - ref).norm()) / (nb if nb > 0 else 1.0)


def judge(got, r32, r64, margin_row=MARGIN_ROW, margin_all=MARGIN_ALL):
    """(ok, row ratio, whole-tensor ratio): err <= margin * yard in both measures, the yardstick being the reference formula in fp32."""
    yr, ya, er, ea = row_err(r32, r64), all_err(r32, r64), row_err(got, r64), all_err(got, r64)
    ratio = lambda e, y: (e / y) if y > 0 else (0.0 if e == 0 else float("inf"))
    return (er <= margin_row * yr and ea <= margin_all * ya), ratio(er, yr), ratio(ea, ya)


# ================================================================================================ case list
ATTN_HEADS = [1, 2, 4, 8, 16, 64]
ATTN_WIDTHS = [32, 48, 64, 96, 128, 256, 512]
WIDTHS = [32, 64, 128, 256, 512, 96]         # 96: a multiple of 4, of neither 64 nor 128
ODD_WIDTH = 30                               # not a multiple of 4: element-wise kernels only


def attn_branch(H, heads):
    """Which way conan_visnet_attn_message(_bwd) goes, re-derived from the dispatch arithmetic: 'badarg' (H is not a whole number of heads),
    'unsupported', or the instantiation 'blocks128' (k_attn_msg<4,true>, 128-channel blocks on blockIdx.y), 'cpl2' (<2>), 'cpl1' (<1>)."""
    if H % heads:
        return "badarg"
    hd = H // heads
    lanes4 = hd // 4
    blocks128 = H % 128 == 0 and hd % 4 == 0 and (lanes4 & (lanes4 - 1)) == 0 and 128 % hd == 0
    cpl = (H + 63) // 64 if H > 64 else 1
    if not blocks128 and (H > 128 or (H > 64 and H != 128) or hd % cpl):
        return "unsupported"
    lph = lanes4 if blocks128 else hd // cpl
    if lph & (lph - 1):
        return "unsupported"
    return "blocks128" if blocks128 else ("cpl2" if cpl == 2 else "cpl1")


def flag_cases(name, H, sweep):
    """Flag combinations of one op at one width; `sweep` = the shape sweep (all head counts), otherwise the per-graph pass."""
    if name == "attn_message":
        heads = ATTN_HEADS if sweep else [8]
        return [{"heads": h, "pre_act": p} for h in heads for p in ((1, 0) if h == 8 else (1,))]
    if name in ("vec_aggregate", "edge_update"):
        return [{"pre_act": 1}, {"pre_act": 0}]
    if name == "node_update":
        return [{"vdot": "fold"}, {"vdot": "split"}, {"vdot": "free"}]
    if name in ("layernorm", "scale_channels"):
        return [{"tap": False}, {"tap": True}]
    if name == "gate":
        return [{"act": 0}, {"act": 1}]
    if name == "concat2":
        return [{"Hb": H}, {"Hb": H // 2 + 1}]
    return [{}]


def op_cases(name):
    """[(graph name | row count, H, flags)] of one op — every case except `wide` (the GPU file runs that one by itself).  For expnormal "H" is
    num_rbf, the number of radial basis functions, not the hidden width: 32 (ViSNet's), 20, and 50 / 7, which are not multiples of 4; edge_unit has
    no width at all (3 = the spatial axis)."""
    op, out = OPS[name], []
    if op.graph:
        for g in GRAPHS:
            for H in ((32, 20, 50, 7) if name == "expnormal" else (3,) if name == "edge_unit" else (32, 128)):
                out += [(g, H, fl) for fl in flag_cases(name, H, False)]
        if name == "attn_message":
            out += [("capped", H, fl) for H in ATTN_WIDTHS for fl in flag_cases(name, H, True)]
        elif name not in ("expnormal", "edge_unit"):
            out += [("capped", H, fl) for H in WIDTHS[1:] if H != 128 for fl in flag_cases(name, H, True)]
    else:
        elementwise = name in ("scale_channels", "silu", "concat2")
        for n in (1, 53, 300):
            for H in WIDTHS + ([ODD_WIDTH] if elementwise else []):
                out += [(n, H, fl) for fl in flag_cases(name, H, True)]
    return out


def case_seed(name, g, H, fl):
    return (sum(map(ord, name + str(g))) * 131 + H * 7 + sum((i + 3) * int(v if not isinstance(v, str) else len(v)) for i, v in enumerate(fl.values()))) % (2 ** 31)
