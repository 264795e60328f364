"""TEST INFRASTRUCTURE — plain reference formulas of the glue kernels (embedding, segment sum, activations, RBF / cutoff, graph_ptr, densify,
F_bary readout, MSE, global-norm clipping, the flat Adam step), one short function per operation, and the inputs the GPU tests run them on.

Every function is written with torch ops only and takes the dtype from its inputs: called with float64 it is the reference ("ref64"), called with
float32 on the CPU it is the yardstick ("ref32") a kernel's error is measured against (visnet_ref.judge).  Indices and CSR arrays stay integer.
Nothing is imported from the package under test.  tests/test_glue_ref_cpu.py holds every function to what defines it (torch.nn.functional, torch
autograd, torch.optim.Adam, the oracle's to_dense_batch / to_dense_adj / normalize_tensor) and asserts the conditions on the inputs below."""
from __future__ import annotations

import math

import numpy as np
import torch

LN2 = math.log(2.0)
NAN, INF = float("nan"), float("inf")


# ================================================================================================ reference formulas
def embedding(weight, z):
    """out[a] = weight[z[a]]; an index outside [0, rows) gives a NaN row (include/conan_fgw_hip.h: torch device-asserts there)."""
    rows = weight.shape[0]
    ok = (z >= 0) & (z < rows)
    out = weight[z.clamp(0, rows - 1)]
    return torch.where(ok[:, None], out, torch.full_like(out, NAN))


def embedding_grad(z, dout, rows, padding_idx):
    """index_add into zeros in atom order, out-of-range ids dropped, the padding row zeroed (padding_idx outside [0, rows): none)."""
    ok = (z >= 0) & (z < rows)
    dw = torch.zeros(rows, dout.shape[1], dtype=dout.dtype).index_add_(0, z[ok], dout[ok])
    if 0 <= padding_idx < rows:
        dw[padding_idx] = 0
    return dw


def onehot_rows(z, rows, padding_idx):
    r = torch.arange(rows)
    return ((z[:, None] == r[None, :]) & (r[None, :] != padding_idx)).to(torch.float32)


def batch_of(gptr):
    gptr = torch.as_tensor(gptr, dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(len(gptr) - 1), gptr[1:] - gptr[:-1])


def segment_sum(x, gptr):
    return torch.zeros(len(gptr) - 1, x.shape[1], dtype=x.dtype).index_add_(0, batch_of(gptr), x)


def segment_sum_grad(dout, gptr):
    return dout[batch_of(gptr)]


def unary(op, x):
    """0 = ReLU, 1 = sigmoid, 2 = shifted softplus."""
    return torch.relu(x) if op == 0 else torch.sigmoid(x) if op == 1 else torch.nn.functional.softplus(x) - LN2


def unary_grad_from_output(op, y, dy):
    """The header's formulas evaluated on the OUTPUT y: relu' = [y > 0], sigmoid' = y (1 - y), ssp' = 1 - 0.5 exp(-y)."""
    if op == 0:
        return dy * (y > 0).to(dy.dtype)
    return dy * y * (1 - y) if op == 1 else dy * (1 - 0.5 * torch.exp(-y))


def rbf(dist, offset, coeff):
    return torch.exp(coeff * (dist[:, None] - offset[None, :]) ** 2)


def cutoff_scale(dist, cutoff, x):
    return x * (0.5 * (torch.cos(dist * math.pi / cutoff) + 1.0))[:, None]


def graph_ptr(batch, G):
    """graph_ptr[g] = first atom whose graph id is >= g (np.searchsorted on the sorted id vector); empty graphs allowed."""
    return np.searchsorted(np.asarray(batch, dtype=np.int64), np.arange(G + 1), side="left").astype(np.int32)


def densify(feat, gptr, N, shift, a, b):
    """to_dense_batch (zero padding to N rows) + shift, min / max over the WHOLE padded slab, affine map onto [a, b] -> [G, N, d].  Written with
    Tensor.min() / .max(), so torch autograd gives the backward, ties included (split evenly; padding entries absorb their share).  A graph of
    more than N atoms cannot be represented: its slab is NaN (and so is the gradient of all its atoms)."""
    d, slabs = feat.shape[1], []
    for g in range(len(gptr) - 1):
        lo, hi = int(gptr[g]), int(gptr[g + 1])
        if hi - lo > N:
            slabs.append((feat[lo:hi].sum() * NAN).expand(N, d))
            continue
        t = torch.cat([feat[lo:hi], torch.zeros(N - (hi - lo), d, dtype=feat.dtype)]) + shift
        mn, mx = t.min(), t.max()
        slabs.append(a + (t - mn) * (b - a) / (mx - mn))
    return torch.stack(slabs)


def dense_adj(rowptr, col, gptr, N):
    """[G, N, N] fp32, entry [g, src, tgt] = multiplicity of the edge src -> tgt in the CSR by target (col = source); a source outside the
    graph is dropped; of a graph with more than N atoms only the first N targets and sources are kept."""
    G = len(gptr) - 1
    adj = np.zeros((G, N, N), np.float32)
    for g in range(G):
        lo, n = int(gptr[g]), min(int(gptr[g + 1] - gptr[g]), N)
        for i in range(n):
            for e in range(int(rowptr[lo + i]), int(rowptr[lo + i + 1])):
                j = int(col[e]) - lo
                if 0 <= j < n:
                    adj[g, j, i] += 1.0
    return torch.from_numpy(adj)


def readout(Y, K, mode):
    """F_bary readout -> [B * K, d]: the column sums over the N rows of post(Y[b]), repeated for the K conformers.  mode 0: post = identity;
    mode 1: the reference's NaN guard (a molecule holding a NaN is replaced by zeros: a constant) and then column L2 normalisation."""
    outs = []
    for Yb in Y:
        if mode == 1:
            Yb = torch.where(torch.isnan(Yb).any(), torch.zeros_like(Yb), Yb)
            Yb = Yb / torch.linalg.norm(Yb, dim=0)
        outs.append(Yb.sum(0, keepdim=True).expand(K, -1))
    return torch.cat(outs)


def mse(pred, target):
    diff = pred - target
    return (diff * diff).mean(), 2 * diff / pred.numel()


def clip(g, max_norm):
    """(norm, coefficient, clipped gradient) of torch.nn.utils.clip_grad_norm_: coefficient min(1, max_norm / (norm + 1e-6)); a NaN norm gives
    a NaN coefficient, an infinite norm gives 0."""
    norm = torch.sqrt((g * g).sum())
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return norm, coef, g * coef


def adam_step(p, g, m, v, t, lr, b1, b2, eps, wd):
    """Step number t (1 for the first) of torch.optim.Adam, the formula of the kernel comment: weight decay added to g, bias corrections from t."""
    g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** t) * m / (torch.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return p, m, v


# ================================================================================================ inputs of the GPU tests
def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- activations
SPECIAL = [0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4, INF, -INF, NAN]
UNARY_COUNTS = [1, 255, 256, 257, 2048 * 256 + 1]            # the last: one element beyond the 2048-workgroup grid of 256 threads


def unary_x(count, seed=0):
    """randn at the scales 1e-3, 1 and 30, a third of the vector each (one value: scale 1)."""
    x = torch.randn(count, generator=gen(100 + seed + count))
    if count >= 3:
        x[: count // 3] *= 1e-3
        x[count // 3: 2 * (count // 3)] *= 30.0
    return x


def unary_y_dy(op, count, seed=0):
    """A forward OUTPUT of the op and an incoming gradient.  op 0: relu of unary_x (zeros included); op 1: (0, 1) with exact 0 and 1 when
    there is room; op 2: y = -ln 2 + delta with delta log-uniform in [1e-7, 30] (the first one 1e-7 itself): ssp' = 1 - 0.5 exp(-y) cancels
    there."""
    g = gen(200 + 10 * op + seed + count)
    dy = torch.randn(count, generator=g)
    if op == 0:
        y = torch.relu(unary_x(count, seed + 1))
    elif op == 1:
        y = torch.sigmoid(unary_x(count, seed + 1))
        if count >= 3:
            y[0], y[1] = 0.0, 1.0
    else:
        delta = torch.exp(torch.rand(count, generator=g, dtype=torch.float64) * (math.log(30.0) - math.log(1e-7)) + math.log(1e-7))
        if count >= 3:
            delta[0] = 1e-7
        y = (delta - LN2).to(torch.float32)
    return y, dy


# ---- embedding
EMB_H = [4, 64, 128, 132, 256]
EMB_N = [1, 31, 32, 33, 127, 128, 129, 1000]
EMB_ROWS = [1, 10, 100]


def embedding_cases():
    """(name, rows, H, n, padding_idx, z kind): every (H, n) pair, rows and padding (0, last row, -1 = none) cycled through them; one case of
    1000 atoms of ONE type (the longest serial fp32 chain); one with the ids -1, rows and 2^40 mixed in."""
    cases, k = [], 0
    for H in EMB_H:
        for n in EMB_N:
            rows = EMB_ROWS[k % 3]
            pad = (0, rows - 1, -1)[(k // 3) % 3]
            cases.append((f"H{H}/n{n}/rows{rows}/pad{pad}", rows, H, n, pad, "random"))
            k += 1
    cases.append(("one-type/H132/n1000", 100, 132, 1000, 0, "one"))
    cases.append(("one-type/H256/n1000/nopad", 10, 256, 1000, -1, "one"))
    cases.append(("bad-ids/H64/n129", 100, 64, 129, 0, "bad"))
    cases.append(("bad-ids/H132/n33/nopad", 10, 132, 33, -1, "bad"))
    return cases


def embedding_inputs(case):
    name, rows, H, n, pad, kind = case
    g = gen(7 * rows + 13 * H + n + 3 * (pad + 1))
    z = torch.randint(0, rows, (n,), generator=g)
    if kind == "one":
        z[:] = rows - 3
    if kind == "bad":
        z[1], z[5], z[n - 1] = -1, rows, 2 ** 40
    return z, torch.randn(rows, H, generator=g), torch.randn(n, H, generator=g)


# ---- segment sum
SEG_SIZES = [0, 1, 7, 8, 9, 64, 65, 0]
SEG_W = [1, 4, 63, 64, 65, 128, 200]


def seg_gptr():
    return np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int32)


# ---- rbf / cutoff
CUTOFF = 10.0
RBF_GS = [1, 10, 50, 63]
CUT_F = [4, 32, 128, 132]


def edge_dist(m, seed=0):
    """m distances in [0, cutoff]; the first five are 0, 1e-6, cutoff / 2, the float just below the cutoff, the cutoff."""
    d = torch.rand(m, generator=gen(300 + seed + m)) * CUTOFF
    hand = torch.tensor([0.0, 1e-6, CUTOFF / 2, float(np.nextafter(np.float32(CUTOFF), np.float32(0))), CUTOFF])
    d[: min(m, 5)] = hand[: min(m, 5)]
    return d


def rbf_offset(Gs):
    """(offset, coeff) of GaussianSmearing(0, cutoff, Gs); one Gaussian: spacing taken as the cutoff."""
    off = torch.linspace(0.0, CUTOFF, Gs)
    step = float(off[1] - off[0]) if Gs > 1 else CUTOFF
    return off, -0.5 / step ** 2


# ---- densify
def csr_from_edges(n_atoms, edges):
    """CSR by target of a list of (src, tgt): rowptr[n_atoms + 1], col = sources, ascending inside a row."""
    rows = [[] for _ in range(n_atoms)]
    for s, t in edges:
        rows[t].append(s)
    rowptr = np.zeros(n_atoms + 1, np.int32)
    col = []
    for i, r in enumerate(rows):
        col += sorted(r)
        rowptr[i + 1] = len(col)
    return rowptr, np.asarray(col if col else [0], np.int32)[: max(len(col), 1)], len(col)


class DensifyCase:
    """Graph sizes, N, d, shift, a hand-made directed multigraph, and features by `kind`: "randn", "quant" (multiples of 0.25 in [-1, 1]:
    min and max tie; a slab with n < N and min 0 + shift ties with the padding), "const" (graph 0 constant: range 0)."""

    def __init__(self, name, sizes, N, d, shift, kind="randn", seed=0):
        self.name, self.sizes, self.N, self.d, self.shift, self.kind = name, list(sizes), N, d, float(shift), kind
        self.a, self.b = 0.1, 2.0
        self.gptr = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)
        self.G, self.n_atoms = len(self.sizes), int(self.gptr[-1])
        g = gen(400 + seed + 31 * N + d)
        if kind == "quant":
            feat = torch.randint(-4, 5, (self.n_atoms, d), generator=g).to(torch.float32) * 0.25
            for q in range(self.G):                            # every other graph: non-negative features, so that the padding zeros are minima
                sl = feat[self.gptr[q]: self.gptr[q + 1]].view(-1)
                if q % 2 == 1:
                    sl.abs_()
                else:
                    sl[0] = sl[-1] = -1.0                      # the minimum twice (the maximum twice in every graph)
                sl[1] = sl[-2] = 1.0
        else:
            feat = torch.randn(self.n_atoms, d, generator=g)
        if kind == "const":
            feat[self.gptr[0]: self.gptr[1]] = 0.75
        self.feat = feat
        self.dYs = torch.randn(self.G, N, d, generator=g)
        # directed edges: a one-way ring i -> i + 1, a one-way chord 0 -> n - 1, edge multiplicities 2 (1 -> 0) and 3 (2 -> 0), and a source
        # outside the graph on target 0 of every graph (the atom before the graph, or after it); the graphs of odd index have no edges at all
        edges = []
        rng = np.random.RandomState(N + d)
        for q, n in enumerate(self.sizes):
            lo = int(self.gptr[q])
            if n == 0 or q % 2 == 1:
                continue
            m = min(n, N)
            edges += [(lo + i, lo + (i + 1) % m) for i in range(m)] if m > 1 else []
            if m > 2:
                edges += [(lo, lo + m - 1), (lo + 1, lo), (lo + 1, lo), (lo + 2, lo), (lo + 2, lo), (lo + 2, lo)]
                edges += [(lo + int(s), lo + int(t)) for s, t in rng.randint(0, m, (2 * m, 2)) if s < t]      # upper-triangular extras: directed
            outside = lo - 1 if lo > 0 else lo + n
            if 0 <= outside < self.n_atoms:
                edges.append((outside, lo))
        self.rowptr, self.col, self.E = csr_from_edges(self.n_atoms, edges)


def densify_cases():
    c = [DensifyCase("directed/N9/d3", [9, 5, 0, 9, 4, 7], 9, 3, 0.5),
         DensifyCase("d1/shift0", [6, 3, 6, 0, 2], 6, 1, 0.0),
         DensifyCase("d16/shift1", [7, 7, 1, 3], 7, 16, 1.0),
         DensifyCase("d64", [12, 9, 10], 12, 64, 0.5),
         DensifyCase("d200", [5, 8, 3], 8, 200, 0.5),
         DensifyCase("n257+n300/N300/d4", [257, 10, 300], 300, 4, 0.5),
         DensifyCase("ties/N8/d3", [8, 5, 8, 6, 3], 8, 3, 0.0, kind="quant"),
         DensifyCase("ties/N8/d16/shift.5", [8, 5, 8, 6, 3], 8, 16, 0.5, kind="quant"),
         DensifyCase("const-slab", [6, 4, 6], 6, 3, 0.5, kind="const"),
         DensifyCase("empty-graph-only-nan", [0, 5], 5, 3, 0.5)]
    return {x.name: x for x in c}


# the slabs of range 0 (an empty or a constant graph: 0 / 0), by case: NaN in the reference, exempt from judging; every other slab is judged
DEGENERATE_DENSIFY = {"const-slab": [0], "empty-graph-only-nan": [0], "d1/shift0": [3], "directed/N9/d3": [2]}


# ---- readout
READOUT_N = [1, 7, 8, 9, 33]
READOUT_D = [1, 16, 64, 65, 200]
DEGENERATE_READOUT = {"nan-in-Y", "zero-column"}


def readout_cases():
    """(name, B, K, N, d, kind) -> every N x d pair, B and K cycled; two named degenerate cases for mode 1."""
    out, k = [], 0
    for N in READOUT_N:
        for d in READOUT_D:
            out.append((f"N{N}/d{d}", (1, 3)[k % 2], (1, 4)[(k // 2) % 2], N, d, "randn"))
            k += 1
    out.append(("nan-in-Y", 3, 4, 9, 65, "nan"))
    out.append(("zero-column", 3, 1, 8, 16, "zerocol"))
    return out


def readout_inputs(case):
    name, B, K, N, d, kind = case
    g = gen(500 + 7 * N + d + B)
    Y = torch.randn(B, N, d, generator=g) + 0.5
    if kind == "nan":
        Y[1, N // 2, 3] = NAN
    if kind == "zerocol":
        Y[2, :, 5] = 0.0
    return Y, torch.randn(B * K, d, generator=g)


# ---- loss / optimiser
MSE_N = [1, 63, 64, 255, 256, 257, 5000]
CLIP_N = [0, 1, 3, 4, 5, 1023, 262144, 262145, 524295]      # 262144 = 256 workgroups x 256 threads x 4: the last two need a second grid pass
ADAM_N = [1, 3, 4, 5, 1023, 1048576 + 5, 2 * 1048576 + 3]   # 1048576 = 1024 workgroups x 256 threads x 4
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def clip_grad(n, seed=0):
    return torch.randn(n, generator=gen(600 + seed + n % 9973))


def adam_inputs(n, seed=0):
    """p ~ randn, three gradients spread over six decades (randn x 10^U(-4, 2))."""
    g = gen(700 + seed + n % 9973)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 6.0 - 4.0) for _ in range(3)]
    return p, grads
