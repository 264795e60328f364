"""TEST INFRASTRUCTURE — plain reference formulas of the SchNet edge path and of the stage-2 heads (csrc/cfconv.hip, csrc/filter_fused.hip,
csrc/filter_bwd.hip, csrc/filter_bwd2.hip, the stage-2 part of csrc/head.hip): the CFConv gather and its three backwards, the filter generator, both
filter-network backwards, the aggregation head in its plain and its *_sums form.

Every function is plain torch on whatever dtype it is given: called with float64 it is the reference ("ref64"), called with float32 on the CPU it
is the yardstick ("ref32") a kernel's error is measured against (visnet_ref.judge).  Formulas: include/conan_fgw_hip.h; tests/test_edge_ref_cpu.py
holds them to torch autograd of the plain composition in fp64.  No formula multiplies a row it does not depend on by zero: a one-direction pair
is selected, not masked, so that a non-finite value reaches the outputs that depend on it and nothing else.

The *_form functions re-derive the host dispatch of each entry point and name the kernel form a shape runs on, as dense_ref.linear_branch does; the
case lists below are walked by both test files, and the CPU test asserts that they reach every named form.  Graphs are hand-made index arrays
(a by-target CSR, its by-source transpose, a pair table by conan_edge_pairs' rule), every index in range."""
from __future__ import annotations

import math

import numpy as np
import torch

from dense_ref import LN2, gen, rbf, ssp, ssp_prime_from_output

NAN, INF = float("nan"), float("inf")
CUTOFF = 5.0

# the numbers the form functions use; tests/test_edge_ref_cpu.py reads them from the sources
CF_BLOCK_CAP, CF_WAVES, CF_LAUNCH_BLOCKS, CF_THREADS = 65536, 4, 4096, 256
HD_WAVES, HD_MAXD, HD_U, HS_MAXK = 4, 64, 16, 32
FB_WAVES, FB_GRID_MAX, F2_GRID_MAX, F2_JP, GP, FF_THREADS = 4, 256, 256, 64, 64, 512
FF_GRID_MAX = 256


# ================================================================================================ reference formulas
def cos_cut(d, cutoff=CUTOFF):
    """CFConv's cosine cutoff, 0.5 (cos(d pi / cutoff) + 1): no mask beyond the cutoff (PyG's CFConv has none)."""
    return 0.5 * (torch.cos(d * math.pi / cutoff) + 1.0)


def _rows(W, pid):
    return W if pid is None else W.index_select(0, pid)


def cfconv_fwd(x, W, col, tgt, pid, n):
    """out[i] = sum over the edges e of target i of x[col[e]] * W[row(e)], row(e) = pid[e] or e."""
    return torch.zeros(n, x.shape[1], dtype=x.dtype).index_add_(0, tgt, x.index_select(0, col) * _rows(W, pid))


def cfconv_bwd_x(W, dout, col, tgt, pid, n):
    return torch.zeros(n, dout.shape[1], dtype=dout.dtype).index_add_(0, col, _rows(W, pid) * dout.index_select(0, tgt))


def cfconv_bwd_w(x, dout, col, tgt, dist, cutoff=CUTOFF):
    dW = x.index_select(0, col) * dout.index_select(0, tgt)
    return dW if dist is None else dW * cos_cut(dist, cutoff).unsqueeze(1)


def cfconv_bwd_w_pairs(x, dout, col, tgt, pe0, pe1, pdist, cutoff=CUTOFF):
    """dWp[p] = C(d_p) (x[src(e0)] dout[tgt(e0)] + x[src(e1)] dout[tgt(e1)]), the second term only where the pair has a second direction."""
    r = cfconv_bwd_w(x, dout, col.index_select(0, pe0), tgt.index_select(0, pe0), None)
    two = (pe1 >= 0).nonzero().flatten()
    e1 = pe1.index_select(0, two)
    r = r.index_add(0, two, cfconv_bwd_w(x, dout, col.index_select(0, e1), tgt.index_select(0, e1), None))
    return r * cos_cut(pdist, cutoff).unsqueeze(1)


def filter_fwd(dist, offset, coeff, cutoff, w1, b1, w2, b2):
    """(W, h1): h1 = ssp(rbf(d) w1^T + b1), W = (h1 w2^T + b2) C(d)."""
    h1 = ssp(rbf(dist, offset, coeff) @ w1.t() + b1)
    return (h1 @ w2.t() + b2) * cos_cut(dist, cutoff).unsqueeze(1), h1


def filter_cfconv_fwd(x, dist, col, tgt, n, offset, coeff, cutoff, w1, b1, w2, b2):
    return cfconv_fwd(x, filter_fwd(dist, offset, coeff, cutoff, w1, b1, w2, b2)[0], col, tgt, None, n)


def filter_bwd(g, h1, dist, offset, coeff, w2, live):
    """(dW1 [F,Gs], db1 [F]) over the first `live` rows: dh1 = (g w2) ssp'(h1), dW1 = dh1^T rbf(d), db1 = column sums of dh1."""
    dh1 = (g[:live] @ w2) * ssp_prime_from_output(h1[:live])
    return dh1.t() @ rbf(dist[:live], offset, coeff), dh1.sum(dim=0)


def filter_bwd2(g, h1, dist, offset, coeff, w2, live):
    """filter_bwd + (dW2 [F,F], db2 [F]) = (g^T h1, column sums of g)."""
    return filter_bwd(g, h1, dist, offset, coeff, w2, live) + (g[:live].t() @ h1[:live], g[:live].sum(dim=0))


def head_fwd(x3, xc, xb, W3, b3, Wb, bb, wreg, breg, aw, K):
    """(out [nmol], m3, mb, t [nmol, D]) — the conformer mean first, as the header states."""
    D = x3.shape[1]
    m3, mc, mb = (v.view(-1, K, D).mean(dim=1) for v in (x3, xc, xb))
    t = m3 @ W3.t() + b3 + mc + aw * (mb @ Wb.t() + bb)
    return t @ wreg + breg, m3, mb, t


def head_bwd(dout, W3, Wb, wreg, m3, mb, t, aw, K):
    """(dx3, dxc, dxb [nmol K, D], dW3, db3, dWb, dbb, dwreg, dbreg) from the forward's saved m3, mb, t."""
    u = dout.unsqueeze(1) * wreg.unsqueeze(0)                    # [nmol, D] gradient at t
    rep = lambda v: v.repeat_interleave(K, dim=0) / K
    db3 = u.sum(dim=0)
    return (rep(u @ W3), rep(u), rep(aw * (u @ Wb)), u.t() @ m3, db3, aw * (u.t() @ mb), aw * db3, (dout.unsqueeze(1) * t).sum(dim=0),
            dout.sum().reshape(1))


def segment_sum(h3, gptr):
    G = gptr.numel() - 1
    idx = torch.repeat_interleave(torch.arange(G), (gptr[1:] - gptr[:-1]).long())
    return torch.zeros(G, h3.shape[1], dtype=h3.dtype).index_add_(0, idx, h3)


def node_sum_repeated(Y, K):
    """conan_fgw_readout_fwd mode 0: the sum of Y over its N nodes, for each of the K conformers of the molecule."""
    return Y.sum(dim=1).repeat_interleave(K, dim=0)


def head_sums_fwd(Y, h3, gptr, xc, W3, b3, Wb, bb, wreg, breg, aw, K):
    return head_fwd(segment_sum(h3, gptr), xc, node_sum_repeated(Y, K), W3, b3, Wb, bb, wreg, breg, aw, K)


def head_sums_bwd(dout, W3, Wb, wreg, m3, mb, t, gptr, aw, K, N):
    """(dh3 [atoms, D], dxc, dY [nmol, N, D], parameter gradients...): dh3 = dx3 of the atom's graph, dY = the sum of dxb over the K copies."""
    dx3, dxc, dxb, *par = head_bwd(dout, W3, Wb, wreg, m3, mb, t, aw, K)
    G = gptr.numel() - 1
    idx = torch.repeat_interleave(torch.arange(G), (gptr[1:] - gptr[:-1]).long())
    dY = dxb.view(-1, K, dxb.shape[1]).sum(dim=1).unsqueeze(1).expand(-1, N, -1).contiguous()
    return (dx3.index_select(0, idx), dxc, dY, *par)


# ================================================================================================ forms (host dispatch, re-derived)
def round_up8(b):
    return (b + 7) // 8 * 8


def cfconv_grid(n):
    return round_up8(min((n + CF_WAVES - 1) // CF_WAVES, CF_BLOCK_CAP))


def cfconv_per(n):
    """Contiguous targets per workgroup (4 wavefronts): > 4 means a wavefront walks a second target."""
    g = cfconv_grid(n)
    return (n + g - 1) // g


CFCONV_FORMS = {"fwd128", "fwd256", "fwd_generic", "bwd_x128", "bwd_x_generic", "bwd_xw128", "none"}


def cfconv_form(entry, n, F):
    """entry in {'fwd', 'bwd_x', 'bwd_xw'} -> 'badarg' | 'unsupported' | 'none' (n = 0: no launch) | the kernel."""
    if n < 0 or F <= 0 or F % 4:
        return "badarg"
    if entry == "bwd_xw" and F != 128:
        return "unsupported"
    if n == 0:
        return "none"
    if entry == "fwd":
        return "fwd128" if F == 128 else "fwd256" if F == 256 else "fwd_generic"
    return ("bwd_x128" if F == 128 else "bwd_x_generic") if entry == "bwd_x" else "bwd_xw128"


def bwd_w_passes(E, F):
    """Trips of k_cfconv_bwd_w's grid-stride loop (4096 blocks of 256 threads, one float4 each)."""
    return max(1, -(-(E * F // 4) // (CF_LAUNCH_BLOCKS * CF_THREADS)))


def bwd_wp_form(P, F, gmax):
    if F <= 0 or F % 4 or P < 0:
        return "badarg"
    if P == 0:
        return "none"
    if gmax and F != 128:
        return "unsupported"
    return "wp128" if F == 128 else "wp_generic"


def filter_fused_supported(Gs, F):
    return 2 <= Gs <= GP and F in (32, 64, 128)


def filter_cfconv_supported(Gs, F):
    return 2 <= Gs <= GP and F == 128


def filter_fwd_passes(E):
    """Tiles a wavefront of conan_filter_fwd walks: <= 256 workgroups of FF_THREADS / 64 wavefronts deal the 32-edge tiles round-robin."""
    tiles, wv = (E + 31) // 32, FF_THREADS // 64
    grid = min((tiles + wv - 1) // wv, FF_GRID_MAX)
    return -(-tiles // (grid * wv)) if tiles else 0


def filter_cf_per_wg(E):
    """Contiguous tiles per workgroup of conan_filter_cfconv_fwd (always 256 workgroups of 8 wavefronts): > 8 is a wavefront's second tile."""
    return -(-((E + 31) // 32) // FF_GRID_MAX)


def filter_bwd_supported(Gs, F):
    return F == 128 and 1 <= Gs <= F2_JP - 1


def filter_bwd_slices(M):
    return min(max(1, ((M + 31) // 32 + FB_WAVES - 1) // FB_WAVES), FB_GRID_MAX)


def filter_bwd_ws(M, Gs, F):
    return filter_bwd_slices(M) * (F * Gs + F)


def filter_bwd_wave_tiles(M):
    """Most tiles one wavefront of k_filter_bwd walks."""
    return -(-((M + 31) // 32) // (filter_bwd_slices(M) * FB_WAVES))


def filter_bwd2_slices(M):
    return min(max(1, (M + 31) // 32), F2_GRID_MAX)


def filter_bwd2_ws(M, Gs, F):
    s = filter_bwd2_slices(M)
    return s * (F * Gs + F) + s * (F * F + F)


def filter_bwd2_wg_tiles(M):
    return -(-((M + 31) // 32) // filter_bwd2_slices(M))


def head_supported(D):
    return 1 <= D <= HD_MAXD


def head_sums_supported(D, K, mode):
    return head_supported(D) and 1 <= K <= HS_MAXK and mode == 0


def head_bwd_blocks(nmol, D):
    return (nmol + HD_WAVES - 1) // HD_WAVES + 2 * ((D + 3) // 4) + 1


def head_sum_form(nmol):
    """How k_stage2_head_bwd sums over the molecules: HD_U at a time, a tail, or both."""
    return ("unrolled" if nmol >= HD_U else "") + ("+tail" if nmol % HD_U else "")


# ================================================================================================ graphs
class EdgeGraph:
    """Hand-made directed graph without self loops and without repeated edges: the by-target CSR (rowptr, col, tgt), its by-source transpose
    (t_rowptr, t_eid) and the pair table (pid, pe0, pe1, pdist; conan_edge_pairs' rule: a pair belongs to the direction with source <= target, or
    to the only direction there is, then pe1 = -1; pairs are numbered in the order of their owning edge).  dist is symmetric in (i, j).  Index
    tensors are int64 here; the GPU file converts."""

    def __init__(self, n, src, tgt, seed=0):
        order = np.lexsort((src, tgt))
        src, tgt = np.asarray(src, np.int64)[order], np.asarray(tgt, np.int64)[order]
        assert not len(src) or (src != tgt).all()
        key = tgt * n + src
        assert len(np.unique(key)) == len(key), "repeated edge"
        self.n, self.E = n, len(src)
        self.col, self.tgt = torch.from_numpy(src.copy()), torch.from_numpy(tgt.copy())
        self.rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n))]).astype(np.int64))
        t_eid = np.lexsort((tgt, src))
        self.t_eid = torch.from_numpy(t_eid.astype(np.int64))
        self.t_rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64))
        lo, hi = np.minimum(src, tgt), np.maximum(src, tgt)
        h = (lo * 2654435761 + hi * 40503 + seed) % 9973
        self.dist = torch.from_numpy((0.3 + 4.6 * h / 9973.0).astype(np.float32))      # inside the cutoff, the same both ways
        at = np.minimum(np.searchsorted(key, src * n + tgt), max(self.E - 1, 0))      # key is ascending: the edges are sorted by (tgt, src)
        rev = np.where(key[at] == src * n + tgt, at, -1).astype(np.int64) if self.E else np.zeros(0, np.int64)
        owner = (rev < 0) | (src <= tgt)
        pe0 = np.nonzero(owner)[0]
        pid = np.empty(self.E, np.int64)
        pid[pe0] = np.arange(len(pe0))
        pid[~owner] = pid[rev[~owner]]
        self.P = len(pe0)
        self.pid, self.pe0, self.pe1 = torch.from_numpy(pid), torch.from_numpy(pe0), torch.from_numpy(rev[pe0])
        self.pdist = self.dist[self.pe0].clone()

    def reversed(self, seed=1):
        return EdgeGraph(self.n, self.tgt.numpy(), self.col.numpy(), seed)

    def degrees(self):
        return (self.rowptr[1:] - self.rowptr[:-1]).tolist(), (self.t_rowptr[1:] - self.t_rowptr[:-1]).tolist()


DEGREES = [0, 1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130]


def graph_by_degrees(n, degs, seed):
    """Target i gets degs[i] distinct sources != i, drawn from all atoms."""
    rng = np.random.RandomState(seed)
    src, tgt = [], []
    for i, d in enumerate(degs):
        assert d <= n - 1
        c = rng.choice(n - 1, size=d, replace=False)
        src.append(np.where(c >= i, c + 1, c)); tgt.append(np.full(d, i))
    return EdgeGraph(n, np.concatenate(src) if src else np.zeros(0, np.int64), np.concatenate(tgt) if tgt else np.zeros(0, np.int64), seed)


def degree_graph():
    """140 atoms; targets 0 .. 25 carry every degree of DEGREES twice (the second time in reverse order), the rest 3 edges each.  Used as it is
    (by-target degrees: the forward) and reversed (by-source degrees: the backwards)."""
    return graph_by_degrees(140, DEGREES + DEGREES[::-1] + [3] * (140 - 2 * len(DEGREES)), 11)


SMALL_N = [1, 2, 4, 5, 12, 33, 100]           # grid = round_up8(ceil(n / 4)): per = 1 .. 4, with idle wavefronts


def small_graph(n):
    rng = np.random.RandomState(n)
    return graph_by_degrees(n, [int(rng.randint(0, min(n, 6))) for _ in range(n)], 100 + n)


BIG_N = 262144 + 4 * 1000 + 3                  # beyond 4 x the 65 536-block cap: per = 5


def big_graph(live=300, pool=8, seed=5):
    """BIG_N atoms of which `live` (spread over the range, the last three atoms among them) have 1 .. 5 edges, from sources among the first
    `pool` atoms and among the live atoms; everyone else has degree 0 both ways."""
    rng = np.random.RandomState(seed)
    at = np.unique(np.concatenate([rng.choice(BIG_N - 3, size=live - 3, replace=False), [BIG_N - 3, BIG_N - 2, BIG_N - 1]]))
    cand = np.unique(np.concatenate([np.arange(pool), at]))
    src, tgt = [], []
    for i in at:
        c = rng.choice(cand[cand != i], size=int(rng.randint(1, 6)), replace=False)
        src.append(c); tgt.append(np.full(len(c), i))
    return EdgeGraph(BIG_N, np.concatenate(src), np.concatenate(tgt), seed)


def pair_graph(P, seed):
    """A graph with exactly P pairs, one-direction pairs mixed in — the last slot of every 64-group (slots 63, 127, ...) and slot 0 among them."""
    rng = np.random.RandomState(seed)
    n = max(8, int(math.ceil(math.sqrt(2 * P))) + 3)
    iu = np.stack(np.triu_indices(n, 1), axis=1)
    pairs = iu[np.sort(rng.choice(len(iu), size=P, replace=False))]          # sorted by (lo, hi)
    src, tgt = [], []
    kinds = rng.randint(0, 3, size=P)                                         # 0: both directions, 1: lo -> hi only, 2: hi -> lo only
    g = EdgeGraph(n, pairs[:, 0], pairs[:, 1], seed)                          # a first pass to learn the slot each pair gets when all are owned by lo -> hi
    assert g.P == P
    slot = {(int(g.col[e]), int(g.tgt[e])): p for p, e in enumerate(g.pe0.tolist())}
    for (lo, hi), k in zip(pairs, kinds):
        s = slot[(int(lo), int(hi))]
        if s % 64 == 63 or s == 0:
            k = 1
        elif s % 64 == 1:
            k = 0
        elif k == 2:
            k = 0 if s % 5 else 1      # hi -> lo alone would be owned by another edge index and move the slots; keep the layout simple
        if k in (0, 1):
            src.append(lo); tgt.append(hi)
        if k == 0:
            src.append(hi); tgt.append(lo)
    out = EdgeGraph(n, np.array(src), np.array(tgt), seed)
    assert out.P == P
    return out


PAIR_P = [1, 2, 3, 63, 64, 65, 255, 257]
MANY_P = 4096 * 65 + 7                  # k_cfconv_bwd_wp128 deals ceil(P / 4096) = 66 contiguous pairs to a workgroup: a full 64-group and a group of 2


def many_pairs_graph(seed=3):
    """MANY_P pairs among 1000 atoms, every third one with both directions."""
    rng = np.random.RandomState(seed)
    n = 1000
    iu = np.sort(rng.choice(n * (n - 1) // 2, size=MANY_P, replace=False))
    lo = (n - 2 - np.floor(np.sqrt(-8.0 * iu + 4.0 * n * (n - 1) - 7) / 2.0 - 0.5)).astype(np.int64)
    hi = (iu + lo + 1 - n * (n - 1) // 2 + (n - lo) * ((n - lo) - 1) // 2).astype(np.int64)
    both = np.arange(MANY_P) % 3 == 0
    return EdgeGraph(n, np.concatenate([lo, hi[both]]), np.concatenate([hi, lo[both]]), seed)


def wp_per(P):
    """Contiguous pairs per workgroup of the pair-gradient kernels (4096 workgroups; 4 wavefronts of 64 pairs in k_cfconv_bwd_wp128)."""
    return -(-P // CF_LAUNCH_BLOCKS)


# ================================================================================================ inputs
def nrows(r, w, seed, scale=1.0):
    return torch.randn(r, w, generator=gen(seed)) * scale


def decade_rows(r, w, seed):
    """O(1) rows among which every fourth is scaled by a power of ten from 1e-5 to 1e5."""
    x = nrows(r, w, seed)
    k = torch.arange(r)
    s = torch.where(k % 4 == 1, 10.0 ** (((k // 4) % 11) - 5).float(), torch.ones(r))
    return x * s.unsqueeze(1)


def gaussians(Gs, cutoff=CUTOFF):
    """GaussianSmearing(0, cutoff, Gs): (offset [Gs], coeff)."""
    offset = torch.linspace(0.0, cutoff, Gs)
    step = float(offset[1] - offset[0]) if Gs > 1 else cutoff
    return offset, -0.5 / step ** 2


def filter_weights(Gs, F, seed, scale=1.0):
    g = gen(seed)
    w1 = torch.randn(F, Gs, generator=g) / math.sqrt(Gs) * scale
    w2 = torch.randn(F, F, generator=g) / math.sqrt(F) * scale
    return w1, 0.1 * torch.randn(F, generator=g), w2, 0.1 * torch.randn(F, generator=g)


def distances(E, seed, cutoff=CUTOFF):
    """Uniform in (0, cutoff) with 0, the cutoff itself and a distance beyond it among the first rows."""
    d = torch.rand(E, generator=gen(seed)) * cutoff
    for i, v in enumerate((0.0, cutoff, 1.3 * cutoff)):
        if 2 * i + 1 < E:
            d[2 * i + 1] = v
    return d


FILTER_F, FILTER_GS = [32, 64, 128], [2, 10, 50, 64]
FILTER_E = [1, 31, 32, 33, 255, 257]
FILTER_E_SECOND_PASS = 65536 + 33
FILTER_W_SCALES = [1e-4, 1.0, 300.0]
CF_E = [1, 32, 33, 8192 + 40, 65536 + 33]
BWD_M = [1, 31, 32, 33, 127, 129]
BWD_M_CAPPED = 32768 + 33
BWD2_M_RING = [8192 + 33, 16384 + 65]
BWD_GS = [1, 2, 20, 50, 63]
BWD_G_SCALES = [3e-7, 1.0, 4e4]


def counts(E):
    """Device-side counts for a buffer of E rows: NULL, 0, 1, 33, E, E + 5."""
    return [None, 0, 1, 33, E, E + 5]


def filter_bwd_inputs(M, Gs, seed, gscale=1.0):
    """(g, h1, dist, offset, coeff, w2): h1 is a real shifted-softplus output (> -ln 2)."""
    F = 128
    offset, coeff = gaussians(max(Gs, 2))
    offset = offset[:Gs].contiguous()
    w1, b1, w2, _ = filter_weights(Gs, F, seed)
    dist = distances(M, seed + 1)
    h1 = ssp(rbf(dist, offset, coeff) @ w1.t() + b1)
    return nrows(M, F, seed + 2) * gscale, h1, dist, offset, coeff, w2


def segment_graph(E, seed, big=70):
    """tgt [E] ascending for conan_filter_cfconv_fwd: segment lengths 0 .. 5 mostly (so targets of degree 0 exist), segments that end / start at
    every position around rows 15|16 and 31|0 of the first tiles, and one target of `big` edges spanning three tiles.  Returns (tgt, n)."""
    rng = np.random.RandomState(seed)
    lens = []
    for cut_at in (14, 15, 16, 17, 30, 31, 32, 33):               # tile t = 0 .. 7: one segment boundary exactly at row cut_at of tile t, another at 32 t
        lens += [cut_at, 0, 32 - cut_at] if cut_at <= 32 else [32, 1, 31]
    lens += [20, big, 0, 0, 3]
    tot = sum(lens)
    if tot > E:
        lens, tot = [E], E
    while tot < E:
        d = int(min(rng.randint(0, 6), E - tot))
        lens.append(d); tot += d
    lens.append(0)
    tgt = np.repeat(np.arange(len(lens)), lens)
    return torch.from_numpy(tgt.astype(np.int64)), len(lens)


HEAD_D, HEAD_NMOL, HEAD_K, HEAD_N, HEAD_AW = [1, 3, 5, 32, 63, 64], [1, 3, 4, 5, 15, 16, 17, 33], [1, 2, 5, 32], [1, 9], [0.0, 0.37]


def head_cases():
    """(nmol, K, D, N, aw): every D, nmol, K, N and agg_weight at least once, without the full product."""
    out = []
    for i, nmol in enumerate(HEAD_NMOL):
        out.append((nmol, HEAD_K[i % 4], HEAD_D[i % 6], HEAD_N[i % 2], HEAD_AW[i % 2]))
    for i, D in enumerate(HEAD_D):
        out.append((HEAD_NMOL[(i + 3) % 8], HEAD_K[(i + 1) % 4], D, HEAD_N[(i + 1) % 2], HEAD_AW[(i + 1) % 2]))
    out += [(33, 32, 64, 9, 0.37), (17, 5, 63, 1, 0.37)]
    return sorted(set(out))


def head_seed(nmol, K, D):
    """Seed of a head case.  The offset 2 is the smallest at which no summed output (out, t, db3, dbb, dwreg, dbreg) of any case has an fp32
    reference that is EXACT: dbreg is the sum of nmol numbers, and with 3 .. 16 of them torch's fp32 sum often equals the fp64 one, which would
    demand bit equality of a sum taken in another order (tests/test_edge_ref_cpu.py asserts the yardsticks are not zero)."""
    return nmol * 1000 + K * 64 + D + 2


def head_inputs(nmol, K, D, N, seed):
    """Inputs of one case in the *_sums form (Y, h3, graph_ptr): conformer graphs of 0, 1 and 70 atoms among small ones.  The plain head's x3 / xb
    are segment_sum(h3) and the repeated node sum of Y."""
    g = gen(seed)
    G = nmol * K
    sizes = torch.randint(2, 6, (G,), generator=g)
    for i, s in enumerate((0, 1, 70)):
        sizes[(i * 7) % G if G > 2 else min(i, G - 1)] = s
    gptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    atoms = int(gptr[-1])
    h3 = torch.randn(max(atoms, 1), D, generator=g)[:atoms]
    Y = torch.randn(nmol, N, D, generator=g)
    xc = torch.randn(G, D, generator=g)
    par = [torch.randn(D, D, generator=g) / math.sqrt(D), 0.1 * torch.randn(D, generator=g), torch.randn(D, D, generator=g) / math.sqrt(D),
           0.1 * torch.randn(D, generator=g), torch.randn(D, generator=g), torch.randn(1, generator=g)]
    dout = torch.randn(nmol, generator=g)
    return {"Y": Y, "h3": h3, "gptr": gptr, "xc": xc, "par": par, "dout": dout}
