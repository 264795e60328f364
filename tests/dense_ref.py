"""TEST INFRASTRUCTURE — plain reference formulas of the dense path (csrc/gemm.hip, csrc/gemm_t.hip, csrc/mlp2.hip): Linear with its activations, the
sum of contractions, the weight gradients (plain and with the Gaussian expansion generated on the fly), the two chained-Linear kernels.

Every function is plain torch on whatever dtype it is given: called with float64 it is the reference ("ref64"), called with float32 on the CPU it
is the yardstick ("ref32") a kernel's error is measured against (visnet_ref.judge).  Formulas: include/conan_fgw_hip.h; tests/test_dense_ref_cpu.py
holds them to torch.nn.functional and torch autograd in fp64.

linear_branch / wgrad_branch re-derive the host dispatch (conan_linear_fwd -> conan_linear_t_try -> chunk_launch -> launch_t; wgrad_launch) and
name the kernel form a shape runs on, as visnet_ref.attn_branch does.  The case lists below carry the branch each case is meant to reach; the CPU
test asserts that the two agree and that every name is reached.  The lists and input generators are shared by the CPU and the GPU test files.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

LN2 = math.log(2.0)
NAN, INF = float("nan"), float("inf")


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================ reference formulas
def ssp(v):
    """softplus(v) - ln 2, in the overflow-free form."""
    return torch.clamp(v, min=0) + torch.log1p(torch.exp(-v.abs())) - LN2


def silu(v):
    return v / (1.0 + torch.exp(-v))


def ssp_prime_from_output(o):
    """ssp'(v) = sigmoid(v) from the OUTPUT o = ssp(v): 1 - 0.5 exp(-o)."""
    return 1.0 - 0.5 * torch.exp(-o)


def linear(x, w, bias, residual, w_kn, act):
    """(y, pre): pre = x W^T + b (W is [N,K], or [K,N] when w_kn); y = act(pre) + residual, or for act 2 pre * ssp'(.) from residual = o."""
    pre = x @ (w if w_kn else w.t())
    if bias is not None:
        pre = pre + bias
    if act == 2:
        return pre * ssp_prime_from_output(residual), pre
    y = pre if act == 0 else ssp(pre) if act == 1 else silu(pre)
    return (y if residual is None else y + residual), pre


def linear_sum(xs, ws, bias, residual, w_kn):
    """sum_c xs[c] W_c^T (+ bias) (+ residual); xs[c] is [M,128] (possibly a strided view)."""
    y = None
    for x, w in zip(xs, ws):
        t = x @ (w if w_kn else w.t())
        y = t if y is None else y + t
    if bias is not None:
        y = y + bias
    return y if residual is None else y + residual


def wgrad(g, x, live):
    """(dW [N,K], dbias [N]) = (g^T x, column sums of g) over the first `live` rows."""
    return g[:live].t() @ x[:live], g[:live].sum(dim=0)


def rbf(dist, offset, coeff):
    return torch.exp(coeff * (dist.unsqueeze(1) - offset.unsqueeze(0)) ** 2)


def mlp2_fwd(x, w1, b1, w2, b2, residual):
    mid = ssp(x @ w1.t() + b1)
    y = mid @ w2.t() + b2
    return mid, (y if residual is None else y + residual)


def mlp2_bwd(dy, w2, w1, mid):
    dmid = (dy @ w2) * ssp_prime_from_output(mid)
    return dmid, dmid @ w1


def mlp2_outact_fwd(x, w1, b1, w2, b2):
    mid = x @ w1.t() + b1
    return mid, ssp(mid @ w2.t() + b2)


def mlp2_outact_bwd(dy, y, w2, w1):
    g = dy * ssp_prime_from_output(y)
    dmid = g @ w2
    return g, dmid, dmid @ w1


# ================================================================================================ dispatch, re-derived
T16_TABLE = [(128, 128), (128, 64), (64, 64), (64, 128), (32, 128)]
MAX_WGS = 256                      # CONAN_LINEAR_MAX_WGS
WIDE_TILES = 8 * 256               # launch_t: 8-wave workgroups from this many 32-row tiles on


def t16_width(M):
    return "narrow" if (M + 31) // 32 < WIDE_TILES else "wide"


def t16_passes(M, nc=1):
    """How many tiles the busiest wavefront of launch_t walks (1: no second pass of the persistent loop)."""
    tiles = (M + 31) // 32
    per = 4 if tiles < WIDE_TILES else 8
    grid = min((tiles + per - 1) // per, MAX_WGS // nc)
    return -(-tiles // (grid * per))


def linear_branch(M, K, N, w_kn, act, pre):
    """The kernel form conan_linear_fwd (pre False) / conan_linear_act_fwd (pre True) runs this shape on:
    'ksum2' / 'ksum3' (k_linear_sum16), 't16/narrow|wide' (one k_linear_t16 launch of a table shape), 'chunk_nc/..' (one launch, N / NC chunks
    side by side), 'chunk_loop/..' (a launch per (n, k) chunk, accumulating through y), 'res1' / 'res2' (k_linear_res<1|2>), 'generic1' /
    'generic2' (k_linear<1|2>), 'unsupported' (pre wanted and no register-streamed form), 'none' (M == 0)."""
    if M < 1:
        return "none"
    if N == 128 and K in (256, 384) and act == 0 and not pre:
        return "ksum%d" % (K // 128)
    w = t16_width(M)
    if (K, N) in T16_TABLE and not ((K, N) == (32, 128) and w_kn):
        return "t16/" + w
    if K % 64 == 0 and N % 64 == 0 and K <= 1024 and N <= 1024:
        KC, NC = (128 if K % 128 == 0 else 64), (128 if N % 128 == 0 else 64)
        return ("chunk_nc/" if K == KC and 1 < N // NC <= 4 else "chunk_loop/") + w
    if pre:
        return "unsupported"
    if K <= 128 and N <= 128 and K % 32 == 0:
        return "res2" if N > 64 else "res1"
    return "generic2" if N > 64 else "generic1"


LINEAR_BRANCHES = {"ksum2", "ksum3", "t16/narrow", "t16/wide", "chunk_nc/narrow", "chunk_loop/narrow", "res1", "res2", "generic1", "generic2"}


def wgrad_slices(M, K):
    return min(max((M + 127) // 128, 1), 512 if K > 64 else 768)


def wgrad_ws(M, K, N):
    return (wgrad_slices(M, K) + 16) * (N * K + N)


def batchable(K, N):
    return (N * K) % 4 == 0 and N % 4 == 0


def wgrad_branch(M, K, N, rbf_, gmax, immediate):
    """Names of what wgrad_launch does for this shape: the stage-1 kernel ('kt64' / 'kt128': k_wgrad_lds<64|128>; 'h16': k_wgrad_lds_h16;
    'shared256': k_wgrad_lds_shared<2>), 'tn_remap' where the n tiles are folded into grid.x, and for the immediate form the reducer
    ('reduce4', 'reduce_1level', 'reduce_2level')."""
    slices = wgrad_slices(M, K)
    KT = 128 if K > 64 else 64
    ty, tz = (N + 127) // 128, (K + KT - 1) // KT
    names = []
    if not rbf_ and not gmax and K == 128 and N == 256 and M >= 65536:
        names.append("shared256")
    elif gmax:
        names.append("h16")
    else:
        names.append("kt%d" % KT)
        if ty > 1 and tz == 1 and slices % 8 == 0:
            names.append("tn_remap")
    if immediate:
        names.append("reduce4" if batchable(K, N) else "reduce_2level" if slices > 32 else "reduce_1level")
    return tuple(names)


def slab_batch_form(run, M, K, N):
    """How conan_linear_wgrad_slabs_batch launches a run of `run` consecutive jobs over one x (tn = tk = 1, slices % 8 == 0 already given):
    'shared2' / 'shared3' (k_wgrad_lds_shared<2|3>, a launch of its own) or 'grid' (slots of the shared k_wgrad_lds_batch grid)."""
    return "shared%d" % run if run in (2, 3) and K == 128 and N == 128 and M >= 65536 else "grid"


WGRAD_BRANCHES = {"kt64", "kt128", "tn_remap", "shared256", "h16", "reduce4", "reduce_1level", "reduce_2level"}


# ================================================================================================ case lists: Linear
# name, shape, layout, activation, bias / residual given, pre-activation wanted (conan_linear_act_fwd), device row count, expected branch
LinCase = namedtuple("LinCase", "name M K N w_kn act bias res pre m branch")
ACTS = (0, 1, 3)
T16_M = [1, 31, 32, 33, 129]
NC_SHAPES = [(128, 256), (128, 384), (128, 512), (64, 256), (128, 192), (64, 192)]
LOOP_SHAPES = [(256, 256), (192, 64), (128, 640), (1024, 128), (128, 1024), (1024, 1024)]
RES_SHAPES = [(32, 32, "res1"), (96, 64, "res1"), (96, 100, "res2"), (96, 1, "res1"), (128, 3, "res1"), (128, 127, "res2")]
GEN_SHAPES = [(50, 128, "generic2"), (10, 256, "generic2"), (1, 1, "generic1"), (3, 1, "generic1"), (50, 3, "generic1"), (33, 65, "generic2"),
              (160, 130, "generic2"), (1088, 64, "generic1"), (200, 300, "generic2")]
M_EDGES = [63, 64, 65, 127, 128, 129]
M_DEV_M = 70


def m_dev_values(M):
    return [0, 1, 33, M, M + 5]


def _c(group, M, K, N, w_kn, act, bias, res, pre, m, branch):
    tag = f"M{M}/kn{w_kn}/act{act}/b{int(bias)}/r{int(res)}" + ("/pre" if pre else "") + ("" if m is None else f"/m{m}")
    return LinCase(f"{group}-{K}x{N}:{tag}", M, K, N, w_kn, act, bias, res or act == 2, pre, m, branch)


def _sweep(group, K, N, Ms, branch, w_kns=(0,)):
    """act 0 / 1 / 3 x bias / no bias (the biased half with a residual) at every M."""
    return [_c(group, M, K, N, kn, act, b, b, False, None, branch) for M in Ms for kn in w_kns for act in ACTS for b in (True, False)]


def _extras(group, K, N, M, branch, w_kns=(0, 1)):
    """act 2 in both layouts (w_kns), the pre-activation through conan_linear_act_fwd, a device row count with and without it."""
    out = [_c(group, M, K, N, kn, 2, b, True, False, None, branch) for kn in w_kns for b in (True, False)]
    out += [_c(group, M, K, N, 0, act, b, False, True, None, branch) for act in (1, 3) for b in (True, False)]
    out += [_c(group, M, K, N, 0, 1, True, True, False, 20, branch), _c(group, M, K, N, w_kns[-1], 2, False, True, False, 20, branch),
            _c(group, M, K, N, 0, 3, True, False, True, 20, branch)]
    return out


def linear_cases():
    cs = []
    for K, N in T16_TABLE:
        cs += _sweep("t16", K, N, T16_M, "t16/narrow")
        if (K, N) != (32, 128):
            cs += [_c("t16", 33, K, N, 1, act, True, True, False, None, "t16/narrow") for act in ACTS] + _extras("t16", K, N, 33, "t16/narrow")
        else:                                                                   # W as [K,N] leaves the table for this shape (res2, below)
            cs += _extras("t16", K, N, 33, "t16/narrow", w_kns=(0,))
    # the second pass of the narrow persistent loop (256 workgroups x 4 waves x 32 rows = 32768 rows), the last narrow and the first wide size
    cs += [_c("t16", 32769 + 31, 128, 128, 0, 1, True, True, False, None, "t16/narrow"), _c("t16", 65504, 128, 128, 0, 3, True, False, False, None, "t16/narrow"),
           _c("t16", 65505, 128, 128, 0, 1, True, True, False, None, "t16/wide")]
    cs += _sweep("res", 32, 128, [33], "res2", w_kns=(1,))                       # the table's (32, 128) takes W as [N,K] only
    for K in (256, 384):
        ks = "ksum%d" % (K // 128)
        cs += [_c("ksum", M, K, 128, kn, 0, b, True, False, None, ks) for M in (1, 33, 129) for kn in (0, 1) for b in (True, False)]
        cs += [_c("ksum", 33, K, 128, 0, 0, True, False, False, None, ks), _c("ksum", 70, K, 128, 1, 0, True, True, False, 20, ks)]
        cs += [_c("ksum", 33, K, 128, 0, 1, b, b, False, None, "chunk_loop/narrow") for b in (True, False)]          # an activation: through y
        cs += [_c("ksum", 33, K, 128, 0, act, True, False, True, None, "chunk_loop/narrow") for act in (1, 3)]       # pre wanted: through y
    for K, N in NC_SHAPES:
        cs += _sweep("nc", K, N, [33], "chunk_nc/narrow") + _extras("nc", K, N, 33, "chunk_nc/narrow")
    cs += _sweep("nc", 128, 256, [129], "chunk_nc/narrow", w_kns=(1,))
    for K, N in LOOP_SHAPES:
        cs += _sweep("loop", K, N, [33], "chunk_loop/narrow") + _extras("loop", K, N, 33, "chunk_loop/narrow")
    for K, N, br in RES_SHAPES:
        cs += _sweep("res", K, N, [33, 129], br, w_kns=(0, 1))
        cs += [_c("res", 33, K, N, kn, 2, True, True, False, None, br) for kn in (0, 1)]
    cs += [_c("res", 65536 + 200, 96, 100, 0, 1, True, True, False, None, "res2")]    # second pass of the 512-tile x 128-row loop
    for K, N, br in GEN_SHAPES:
        cs += _sweep("gen", K, N, [33, 70], br, w_kns=(0, 1))
        cs += [_c("gen", 33, K, N, kn, 2, True, True, False, None, br) for kn in (0, 1)]
    return cs


FAMILY = [("t16", 128, 128, 0, "t16/narrow"), ("t16", 32, 128, 0, "t16/narrow"), ("ksum", 256, 128, 0, "ksum2"), ("nc", 128, 256, 0, "chunk_nc/narrow"),
          ("loop", 256, 256, 0, "chunk_loop/narrow"), ("res", 96, 100, 0, "res2"), ("gen", 50, 128, 0, "generic2")]


def edge_cases():
    """One shape per kernel family at the row counts around the tiles and at every device row count."""
    cs = []
    for grp, K, N, kn, br in FAMILY:
        act = 0 if grp == "ksum" else 1
        cs += [_c(grp, M, K, N, kn, act, True, True, False, None, br) for M in M_EDGES]
        cs += [_c(grp, M_DEV_M, K, N, kn, act, True, True, False, m, br) for m in m_dev_values(M_DEV_M)]
        if grp in ("t16", "nc", "loop"):
            cs += [_c(grp, M_DEV_M, K, N, 0, 3, True, False, True, m, br) for m in m_dev_values(M_DEV_M)]
    return cs


VALUE_SHAPES = [("t16", 128, 128, "t16/narrow"), ("loop", 256, 256, "chunk_loop/narrow"), ("res", 96, 100, "res2"), ("gen", 50, 128, "generic2")]


def linear_inputs(M, K, N, w_kn, act, seed=0):
    """x ~ N(0, 1), W ~ N(0, 1 / K), bias ~ N(0, 1), residual ~ N(0, 1) — for act 2 the saved output of an ssp layer, ssp(N(0, 2^2)) >= -ln 2."""
    g = gen(1000 * K + N + 7 * M + seed)
    x = torch.randn(max(M, 1), K, generator=g)[:M]
    w = torch.randn((K, N) if w_kn else (N, K), generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(max(M, 1), N, generator=g)[:M]
    if act == 2:
        r = ssp(2.0 * r)
    return x, w, b, r


def decade_rows(M, K, seed=0):
    """Rows of N(0, 1) scaled over ten decades (1e-5 .. 1e5), row 3 all zero, row 5 one non-zero element."""
    x = torch.randn(M, K, generator=gen(seed + K))
    x = x * (10.0 ** torch.linspace(-5, 5, M)).unsqueeze(1)
    x[3] = 0.0
    x[5] = 0.0
    x[5, K // 2] = 1.7
    return x


def judged_linear_inputs():
    """Every (x, w, b, r, w_kn, act) a GPU case is judged on, for the conditioning check (shapes repeat: one per distinct case key)."""
    seen = set()
    for c in linear_cases() + edge_cases():
        key = (c.M, c.K, c.N, c.w_kn, c.act)
        if key in seen or c.M == 0:
            continue
        seen.add(key)
        yield c, linear_inputs(c.M, c.K, c.N, c.w_kn, c.act)


# ================================================================================================ case lists: sum / multi
SUM_CASES = [(nin, kn, ld, M) for nin in (2, 3) for kn in (0, 1) for ld in (128, 132, 384) for M in (1, 33, 300)]
SUM_SCALES = (1e-6, 3.0, 1e-3)
MULTI_CASES = [(L, act, M) for L in (2, 3, 4) for act in ACTS for M in (1, 33, 1000)]


def sum_inputs(nin, kn, ld, M, scales=(1.0, 1.0, 1.0), seed=0):
    """xs: nin [M,128] views with row pitch ld (ld == 384: three views of ONE [M,384] tensor); base: the tensors behind them."""
    g = gen(31 * nin + 7 * ld + M + kn + seed)
    if ld == 384:
        base = [torch.randn(M, 384, generator=g)]
        for c in range(3):
            base[0][:, 128 * c:128 * c + 128] *= scales[c]
        xs = [base[0][:, 128 * c:128 * c + 128] for c in range(nin)]
    else:
        base = [torch.randn(M, ld, generator=g) * scales[c] for c in range(nin)]
        xs = [t[:, :128] for t in base]
    ws = [torch.randn(128, 128, generator=g) / math.sqrt(128 * nin) for _ in range(nin)]
    return base, xs, ws, torch.randn(128, generator=g), torch.randn(M, 128, generator=g)


# ================================================================================================ case lists: weight gradients
# (M, K, N, names wgrad_branch must give for the immediate form)
WGRAD_IMMEDIATE = [
    (0, 128, 128, ("kt128", "reduce4")), (1, 128, 128, ("kt128", "reduce4")),
    (127, 64, 64, ("kt64", "reduce4")), (128, 64, 64, ("kt64", "reduce4")), (129, 64, 64, ("kt64", "reduce4")),
    (300, 128, 52, ("kt128", "reduce4")), (300, 52, 128, ("kt64", "reduce4")),
    (1000, 128, 256, ("kt128", "tn_remap", "reduce4")), (1100, 128, 256, ("kt128", "reduce4")),
    (300, 200, 300, ("kt128", "reduce4")), (500, 65, 33, ("kt128", "reduce_1level")), (500, 63, 130, ("kt64", "reduce_1level")),
    (65536, 128, 256, ("shared256", "reduce4")), (98305, 64, 64, ("kt64", "reduce4")),
]
SCALAR_N, SCALAR_K = (1, 3, 5, 130), (50, 128, 63)
SCALAR_M = [(300, "reduce_1level"), (4096, "reduce_1level"), (4097, "reduce_2level"), (5000, "reduce_2level")]
RBF_GS, RBF_N, RBF_M = (3, 20, 50, 63, 64, 65, 128), (32, 128, 130), (1, 517, 4133)
RBF_CUTOFF = 10.0


def wgrad_inputs(M, K, N, seed=0):
    g = gen(13 * K + 5 * N + M + seed)
    return torch.randn(max(M, 1), N, generator=g)[:M], torch.randn(max(M, 1), K, generator=g)[:M]


def rbf_inputs(M, Gs, N, seed=0):
    """g ~ N(0, 1); distances uniform in [0, 1.2 cutoff) with 0, the last offset and a value beyond it planted; GaussianSmearing(0, cutoff, Gs)."""
    gn = gen(17 * Gs + 3 * N + M + seed)
    g = torch.randn(M, N, generator=gn)
    dist = torch.rand(M, generator=gn) * (1.2 * RBF_CUTOFF)
    dist[0] = 0.0
    if M > 2:
        dist[1], dist[2] = RBF_CUTOFF, 1.5 * RBF_CUTOFF
    offset = torch.linspace(0.0, RBF_CUTOFF, Gs) if Gs > 1 else torch.zeros(1)
    step = float(offset[1] - offset[0]) if Gs > 1 else 1.0
    return g, dist, offset, -0.5 / step ** 2


# ================================================================================================ case lists: mlp2
MLP2_M = [1, 31, 32, 33, 255, 256, 257, 65536]


def mlp2_inputs(M, K, N1, N2, seed=0, x_scale=1.0):
    g = gen(M + K + 3 * N1 + seed)
    x = torch.randn(M, K, generator=g) * x_scale
    w1, b1 = torch.randn(N1, K, generator=g) / math.sqrt(K), torch.randn(N1, generator=g)
    w2, b2 = torch.randn(N2, N1, generator=g) / math.sqrt(N1), torch.randn(N2, generator=g)
    return x, w1, b1, w2, b2, torch.randn(M, N2, generator=g), torch.randn(M, N2, generator=g)      # ..., residual, dy


def mlp2_value_cases(M=40):
    """[(tag, x, w1, b1, w2, b2, residual, dy)]: rows from 1 to 1e3 (the documented domain) with a zero row; b1 = -30 (mid -> -ln 2); w2 at 1e-4 and 300."""
    x, w1, b1, w2, b2, res, dy = mlp2_inputs(M, 128, 128, 128, seed=1)
    x = x * (10.0 ** torch.linspace(0, 3, M)).unsqueeze(1)
    x[3] = 0.0
    return [(tag, x, w1, bb1, ww2, b2, res, dy) for tag, bb1, ww2 in (("rows", b1, w2), ("b1-30", torch.full_like(b1, -30.0), w2), ("w2/1e-4", b1, w2 * 1e-4),
                                                                      ("w2/300", b1, w2 * 300.0))]


# ================================================================================================ case lists: several layers, scaled gradients
SCALED_SHAPES = [(300, 128, 128), (1000, 128, 256), (300, 200, 52), (300, 128, 130)]
SCALED_G = (2e-6, 1.0, 3e3)
MULTI_EDGE_M = 65536


def multi_inputs(M, K, N, L, seed=0):
    g = gen(M + K + N + L + seed)
    return torch.randn(M, K, generator=g), [torch.randn(N, K, generator=g) / K ** 0.5 for _ in range(L)], [torch.randn(N, generator=g) for _ in range(L)]
