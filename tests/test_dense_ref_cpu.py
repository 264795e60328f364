"""The dense reference (tests/dense_ref.py) checked on the CPU: every formula against torch.nn.functional / torch autograd in fp64, the fp32 run of
every judged input against the fp64 one (visnet_ref.COND_CAP), the branch functions against the case lists, and the ledger of which test file owns
which export of the library."""
import ast
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dense_ref as D
import visnet_ref as R
from conan_fgw_amd import _lib

f64 = torch.float64
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ================================================================================================ formulas
def test_activations_are_torchs():
    v = torch.cat([torch.randn(1000, generator=D.gen(0), dtype=f64) * 5, torch.tensor([0.0, -0.0, 40.0, -40.0, 700.0, -700.0], dtype=f64)])
    assert close(D.ssp(v), F.softplus(v) - math.log(2.0)) and close(D.silu(v), F.silu(v))
    assert close(D.ssp_prime_from_output(D.ssp(v)), torch.sigmoid(v))


@pytest.mark.parametrize("w_kn", [0, 1])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_linear_is_functional_linear(act, w_kn):
    x, w, b, r = (t.double() for t in D.linear_inputs(37, 96, 100, w_kn, act))
    y, pre = D.linear(x, w, b, r, w_kn, act)
    want_pre = F.linear(x, w.t() if w_kn else w, b)
    assert close(pre, want_pre)
    if act == 2:
        # residual holds o = ssp(v): pre * ssp'(v) is the gradient of ssp w.r.t. v, times pre
        v = torch.randn(37, 100, generator=D.gen(5), dtype=f64, requires_grad=True)
        o = F.softplus(v) - math.log(2.0)
        (gv,) = torch.autograd.grad(o, v, want_pre)
        assert close(D.linear(x, w, b, o.detach(), w_kn, 2)[0], gv)
    else:
        fn = (lambda t: t) if act == 0 else (lambda t: F.softplus(t) - math.log(2.0)) if act == 1 else F.silu
        assert close(y, fn(want_pre) + r)
        assert close(D.linear(x, w, None, None, w_kn, act)[0], fn(F.linear(x, w.t() if w_kn else w)))     # no bias, no residual


@pytest.mark.parametrize("nin,kn,ld", [(2, 0, 128), (3, 1, 132), (3, 0, 384), (2, 1, 384)])
def test_linear_sum_is_one_linear_of_the_concatenated_row(nin, kn, ld):
    _, xs, ws, b, r = D.sum_inputs(nin, kn, ld, 41, D.SUM_SCALES)
    xs, ws, b, r = [t.double() for t in xs], [t.double() for t in ws], b.double(), r.double()
    wcat = torch.cat([w.t() if kn else w for w in ws], dim=1)
    assert close(D.linear_sum(xs, ws, b, r, kn), F.linear(torch.cat(xs, dim=1), wcat, b) + r)


def test_weight_gradients_are_autograds():
    g, x = (t.double() for t in D.wgrad_inputs(300, 52, 36))
    w = torch.zeros(36, 52, dtype=f64, requires_grad=True)
    b = torch.zeros(36, dtype=f64, requires_grad=True)
    for live in (300, 299, 1, 0):
        gw, gb = torch.autograd.grad(F.linear(x[:live], w, b), (w, b), g[:live])
        dW, db = D.wgrad(g, x, live)
        assert close(dW, gw) and close(db, gb)
    gr, dist, off, coeff = D.rbf_inputs(100, 50, 32)
    e = D.rbf(dist.double(), off.double(), coeff)
    assert e.shape == (100, 50) and float(e[0, 0]) == 1.0 and abs(float(e[1, 49]) - 1.0) < 1e-6 and float(e[2].max()) < 1e-20
    assert close(e, torch.exp(coeff * (dist.double()[:, None] - off.double()[None, :]).pow(2)))


def test_mlp2_backwards_are_autograds():
    for outact, (K, N1, N2) in ((False, (128, 128, 128)), (True, (128, 64, 64))):
        x, w1, b1, w2, b2, res, dy = (t.double() for t in D.mlp2_inputs(33, K, N1, N2))
        x.requires_grad_(True)
        h = F.linear(x, w1, b1)
        if outact:
            mid = h
            mid.retain_grad()
            y = F.softplus(F.linear(mid, w2, b2)) - math.log(2.0)
            gm, gy = D.mlp2_outact_fwd(x.detach(), w1, b1, w2, b2)
        else:
            mid = F.softplus(h) - math.log(2.0)
            h.retain_grad()
            y = F.linear(mid, w2, b2) + res
            gm, gy = D.mlp2_fwd(x.detach(), w1, b1, w2, b2, res)
        assert close(gm, mid.detach()) and close(gy, y.detach())
        y.backward(dy)
        if outact:
            g, dmid, dx = D.mlp2_outact_bwd(dy, y.detach(), w2, w1)
            pre2 = F.linear(mid.detach(), w2, b2)
            assert close(g, dy * torch.sigmoid(pre2)) and close(dmid, mid.grad) and close(dx, x.grad)
        else:
            dmid, dx = D.mlp2_bwd(dy, w2, w1, mid.detach())
            assert close(dmid, h.grad) and close(dx, x.grad)             # header: dmid is the gradient at the pre-activation of the first layer


# ================================================================================================ conditioning of the judged inputs
def test_fp32_reference_of_every_judged_linear_input_is_within_the_cap():
    worst = 0.0
    for c, (x, w, b, r) in D.judged_linear_inputs():
        if c.M > 2000 and (c.K, c.N) != (128, 128):
            x, r = x[:2000], r[:2000]                                    # rows are independent: the large M changes nothing per row
        for bias in (b, None):
            y32, p32 = D.linear(x, w, bias, r, c.w_kn, c.act)
            y64, p64 = D.linear(x.double(), w.double(), None if bias is None else bias.double(), r.double(), c.w_kn, c.act)
            worst = max(worst, R.all_err(y32, y64), R.all_err(p32, p64))
            assert R.all_err(y32, y64) <= R.COND_CAP and R.all_err(p32, p64) <= R.COND_CAP, c.name
    print("worst fp32 reference error over the Linear cases:", worst)


def test_fp32_reference_of_the_value_and_gradient_inputs_is_within_the_cap():
    for _, K, N, _ in D.VALUE_SHAPES:
        x = D.decade_rows(40, K)
        _, w, b, r = D.linear_inputs(40, K, N, 0, 1)
        for ws in (1.0, 1e-4, 300.0):
            y32, _ = D.linear(x, w * ws, None, None, 0, 0)
            y64, _ = D.linear(x.double(), (w * ws).double(), None, None, 0, 0)
            assert R.all_err(y32, y64) <= R.COND_CAP
            own = lambda a: float(((a - y64).norm(dim=1) / y64.norm(dim=1).clamp_min(1e-300)).max())
            assert own(y32.double()) <= R.COND_CAP                       # every row to its own norm
    for M, K, N, _ in D.WGRAD_IMMEDIATE:
        if M == 0:
            continue
        g, x = D.wgrad_inputs(M, K, N)
        (w32, b32), (w64, b64) = D.wgrad(g, x, M), D.wgrad(g.double(), x.double(), M)
        assert R.all_err(w32, w64) <= R.COND_CAP and R.all_err(b32, b64) <= R.COND_CAP, (M, K, N)
    for Gs in D.RBF_GS:
        g, dist, off, coeff = D.rbf_inputs(4133, Gs, 32)
        w32, w64 = D.wgrad(g, D.rbf(dist, off, coeff), 4133)[0], D.wgrad(g.double(), D.rbf(dist.double(), off.double(), coeff), 4133)[0]
        assert R.all_err(w32, w64) <= R.COND_CAP, Gs
    for M, K, N1, N2 in ((257, 128, 128, 128), (257, 128, 64, 64)):
        x, w1, b1, w2, b2, res, dy = D.mlp2_inputs(M, K, N1, N2)
        a32 = D.mlp2_fwd(x, w1, b1, w2, b2, res) if N1 == 128 else D.mlp2_outact_fwd(x, w1, b1, w2, b2)
        a64 = D.mlp2_fwd(*[t.double() for t in (x, w1, b1, w2, b2, res)]) if N1 == 128 else D.mlp2_outact_fwd(*[t.double() for t in (x, w1, b1, w2, b2)])
        assert all(R.all_err(p, q) <= R.COND_CAP for p, q in zip(a32, a64))


def _cap(tag, a32, a64):
    for p, q in zip(a32, a64):
        assert R.all_err(p, q) <= R.COND_CAP, (tag, R.all_err(p, q))


def test_fp32_reference_of_the_scalar_reducer_inputs_is_within_the_cap():
    """All of SCALAR_M x SCALAR_N x SCALAR_K.  dbias with N <= 5 is one to five numbers and has a margin of its own: its yardstick —
    torch's pairwise fp32 sum of 300 .. 5000 terms against fp64 — is printed and must be neither zero nor beyond the cap."""
    for M, _ in D.SCALAR_M:
        for N in D.SCALAR_N:
            for K in D.SCALAR_K:
                g, x = D.wgrad_inputs(M, K, N)
                a32, a64 = D.wgrad(g, x, M), D.wgrad(g.double(), x.double(), M)
                _cap((M, K, N), a32, a64)
                yard = R.all_err(a32[1], a64[1])
                print(f"YARD dbias M{M} K{K} N{N} {yard:.3g}")
                assert yard > 0.0, (M, K, N, "an exact fp32 reference would demand bit equality of a 5000-term sum")
                if M == 4097 and K == 63:
                    _cap((M, K, N, "m"), D.wgrad(g, x, M - 1), D.wgrad(g.double(), x.double(), M - 1))


def test_fp32_reference_of_the_sum_multi_scaled_rbf_and_mlp2_inputs_is_within_the_cap():
    dbl = lambda ts: [None if t is None else t.double() for t in ts]
    for nin, kn, ld, M in D.SUM_CASES:
        for scales in ((1.0, 1.0, 1.0), D.SUM_SCALES):
            _, xs, ws, b, r = D.sum_inputs(nin, kn, ld, M, scales)
            for bias, res in ((None, None), (b, r), (b, None), (None, r)):
                y32 = D.linear_sum(xs, ws, bias, res, kn)
                y64 = D.linear_sum(dbl(xs), dbl(ws), *dbl([bias, res]), kn)
                _cap(("sum", nin, kn, ld, M), [y32], [y64])
    shapes = [(M, 128, 128, L) for L, _, M in D.MULTI_CASES] + [(D.MULTI_EDGE_M, 128, 128, 4), (33, 128, 128, 1), (33, 128, 128, 5), (33, 64, 128, 3)]
    for M, K, N, L in sorted(set(shapes)):
        x, ws, bs = D.multi_inputs(M, K, N, L)
        for act in D.ACTS:
            for w, b in zip(ws, bs):
                for bias in (b, None):
                    _cap(("multi", M, K, L, act), D.linear(x, w, bias, None, 0, act), D.linear(*dbl([x, w, bias]), None, 0, act))
    for M, K, N in D.SCALED_SHAPES:
        g0, x = D.wgrad_inputs(M, K, N)
        for scale in D.SCALED_G:
            for live in (M, M - 1, 1):
                _cap(("scaled", M, K, N, scale, live), D.wgrad(g0 * scale, x, live), D.wgrad((g0 * scale).double(), x.double(), live))
    for Gs in D.RBF_GS:
        for N in D.RBF_N:
            for M in D.RBF_M:
                g, dist, off, coeff = D.rbf_inputs(M, Gs, N)
                for live in sorted({M, min(M, 300), 1}):
                    _cap(("rbf", Gs, N, M, live), D.wgrad(g, D.rbf(dist, off, coeff), live), D.wgrad(g.double(), D.rbf(dist.double(), off.double(), coeff), live))
    for M in D.MLP2_M:
        for K, N1, N2 in ((128, 128, 128), (128, 64, 64)):
            x, w1, b1, w2, b2, res, dy = D.mlp2_inputs(M, K, N1, N2)
            if N1 == 128:
                for r in (res, None):
                    a32, a64 = D.mlp2_fwd(x, w1, b1, w2, b2, r), D.mlp2_fwd(*dbl([x, w1, b1, w2, b2, r]))
                    _cap(("mlp2", M), a32, a64)
                _cap(("mlp2 bwd", M), D.mlp2_bwd(dy, w2, w1, a32[0]), D.mlp2_bwd(*dbl([dy, w2, w1, a32[0]])))
            else:
                a32, a64 = D.mlp2_outact_fwd(x, w1, b1, w2, b2), D.mlp2_outact_fwd(*dbl([x, w1, b1, w2, b2]))
                _cap(("outact", M), a32, a64)
                _cap(("outact bwd", M), D.mlp2_outact_bwd(dy, a32[1], w2, w1), D.mlp2_outact_bwd(*dbl([dy, a32[1], w2, w1])))
    for tag, x, w1, b1, w2, b2, res, dy in D.mlp2_value_cases():
        a32, a64 = D.mlp2_fwd(x, w1, b1, w2, b2, res), D.mlp2_fwd(*dbl([x, w1, b1, w2, b2, res]))
        _cap(("mlp2 values", tag), a32, a64)
        _cap(("mlp2 values bwd", tag), D.mlp2_bwd(dy, w2, w1, a32[0]), D.mlp2_bwd(*dbl([dy, w2, w1, a32[0]])))
    for _, K, N, _ in D.VALUE_SHAPES:                                      # the remaining Linear value inputs: decade rows through act 1 with bias, O(1) rows
        _, w, b, r = D.linear_inputs(40, K, N, 0, 1)
        x = D.decade_rows(40, K)
        _cap(("decade act1", K, N), D.linear(x, w, b, None, 0, 1), D.linear(*dbl([x, w, b]), None, 0, 1))
        x4, w4, b4, _ = D.linear_inputs(40, K, N, 0, 1, seed=4)
        for act in D.ACTS:
            for ws_ in (1.0, 300.0):
                _cap(("tiny-row tensor", K, N, act), D.linear(x4, w4 * ws_, b4, None, 0, act), D.linear(*dbl([x4, w4 * ws_, b4]), None, 0, act))


# ================================================================================================ branches
def test_every_case_states_its_branch_and_every_branch_is_reached():
    cases = D.linear_cases() + D.edge_cases()
    for lst in (D.linear_cases(), D.edge_cases()):
        assert len({c.name for c in lst}) == len(lst), "duplicate case names"
    for c in cases:
        assert D.linear_branch(c.M, c.K, c.N, c.w_kn, c.act, c.pre) == c.branch, c
    assert {c.branch for c in cases} == D.LINEAR_BRANCHES
    for _, K, N, br in D.VALUE_SHAPES:
        assert D.linear_branch(40, K, N, 0, 0, False) == br
    # the persistent loops on their second pass
    assert D.t16_passes(32768) == 1 and D.t16_passes(32769 + 31) == 2 and D.t16_width(65504) == "narrow" and D.t16_width(65505) == "wide"
    assert (65536 + 200 + 127) // 128 > 512
    assert D.linear_branch(5, 50, 128, 0, 1, True) == "unsupported" and D.linear_branch(0, 128, 128, 0, 0, False) == "none"
    reached = set()
    for M, K, N, names in D.WGRAD_IMMEDIATE:
        assert D.wgrad_branch(M, K, N, False, False, True) == names, (M, K, N)
        reached |= set(names)
    for M, red in D.SCALAR_M:
        for N in D.SCALAR_N:
            for K in D.SCALAR_K:
                assert not D.batchable(K, N) and D.wgrad_branch(M, K, N, False, False, True)[-1] == red
                reached.add(red)
    assert D.wgrad_branch(300, 128, 128, False, True, True) == ("h16", "reduce4")
    reached |= {"h16"}
    assert D.wgrad_branch(517, 50, 128, True, False, False) == ("kt64",) and D.wgrad_branch(4133, 128, 32, True, False, True) == ("kt128", "reduce4")
    assert reached == D.WGRAD_BRANCHES, sorted(D.WGRAD_BRANCHES - reached)
    assert D.wgrad_slices(4096, 128) == 32 and D.wgrad_slices(4097, 128) == 33 and D.wgrad_slices(98305, 64) == 768 and D.wgrad_slices(10 ** 6, 128) == 512


def test_branch_constants_are_the_sources():
    """The numbers the branch functions re-derive, read from the kernels' sources (by name, whatever the spacing): a change there has to come
    here too."""
    csrc = os.path.join(ROOT, "conan-fgw_amd", "csrc")
    gt, gm = open(os.path.join(csrc, "gemm_t.hip")).read(), open(os.path.join(csrc, "gemm.hip")).read()

    def const(text, name):
        m = re.search(r"(?:#\s*define\s+%s\s+|\b%s\s*=\s*)(\d+)" % (name, name), text)
        assert m, name
        return int(m.group(1))
    assert const(gt, "CONAN_LINEAR_MAX_WGS") == D.MAX_WGS == 256
    m = re.search(r"narrow\s*=\s*tiles16\s*<\s*(\d+)\s*\*\s*(\d+)", gt)
    assert m and int(m.group(1)) * int(m.group(2)) == D.WIDE_TILES
    assert const(gt, "CONAN_LINEAR_FAN_MIN_ROWS") == D.MULTI_EDGE_M == 65536 and const(gm, "CONAN_WGRAD_SHARED_MIN_ROWS") == 65536
    assert const(gm, "WG_SLICES_MAX") == 768 and const(gm, "WG_GROUPS") == 16 and const(gm, "WG_BATCH") == 32 and const(gm, "WGS_BATCH") == 24
    assert re.search(r"slices\s*>\s*2\s*\*\s*WG_GROUPS", gm)
    assert D.slab_batch_form(2, 65536, 128, 128) == "shared2" and D.slab_batch_form(3, 65536, 128, 128) == "shared3"
    assert D.slab_batch_form(3, 65535, 128, 128) == D.slab_batch_form(4, 65536, 128, 128) == D.slab_batch_form(2, 65536, 64, 64) == "grid"


# ================================================================================================ the ledger
PER_KERNEL_FILES = ["test_gpu_visnet_ops.py", "test_gpu_gat_ops.py", "test_gpu_glue_ops.py", "test_gpu_dense_ops.py", "test_gpu_edge_ops.py"]
# exports owned by no per-kernel file -> a test file that names them (and calls them, or the op built on them)
ELSEWHERE = {
    "conan_abi_version": "test_abi.py",
    "conan_bce_loss_fwd": "test_bce_loss_cpu.py",
    "conan_collate_layout": "test_collate_cpu.py", "conan_collate_pack": "test_collate_cpu.py", "conan_collate_unpack": "test_gpu_collate.py",
    "conan_csr_transpose": "test_gpu_graph_build.py", "conan_edge_pairs": "test_gpu_graph_build.py",
    "conan_radius_graph_build": "test_gpu_graph_build.py", "conan_radius_graph_build_ws": "test_gpu_graph_build.py",
    "conan_radius_graph_csr": "test_gpu_graph_build.py",
    "conan_fgw_acc_lds_resident": "test_fgw_mixup_cpu.py", "conan_fgw_acc_pair_fwd": "test_fgw_mixup_cpu.py",
    "conan_fgw_acc_pair_workspace_bytes": "test_fgw_mixup_cpu.py", "conan_fgw_mixup_barycenter_fwd": "test_fgw_mixup_cpu.py",
    "conan_fgw_mixup_workspace_bytes": "test_fgw_mixup_cpu.py",
    "conan_fgw_barycenter_bwd": "test_gpu_fgw_grad.py", "conan_fgw_barycenter_bwd_full": "test_fgw_grad_cpu.py",
    "conan_fgw_barycenter_bwd_full_workspace_bytes": "test_fgw_grad_cpu.py",
    "conan_fgw_barycenter_fwd": "test_gpu_fgw_solvers.py", "conan_fgw_barycenter_fwd_ragged": "test_fgw_solvers_cpu.py",
    "conan_fgw_workspace_bytes": "test_fgw_workspace_cpu.py",
    "conan_fgw_pair_dist": "test_fgw_pair_cpu.py", "conan_fgw_pair_dist_bwd": "test_fgw_pair_grad_cpu.py", "conan_fgw_pair_fwd": "test_fgw_pair_cpu.py",
    "conan_fgw_pair_workspace_bytes": "test_fgw_pair_cpu.py",
    "conan_mlp2_outact_dual_bwd": "test_gpu_heads_fused.py", "conan_mlp2_outact_dual_fwd": "test_gpu_heads_fused.py",
    "conan_sinkhorn_bwd": "test_gpu_sinkhorn_grad.py", "conan_sinkhorn_bwd_lds_resident": "test_gpu_sinkhorn_grad.py",
    "conan_sinkhorn_bwd_workspace_bytes": "test_gpu_sinkhorn_grad.py",
    "conan_sinkhorn_ext_fwd": "test_sinkhorn_ext_cpu.py", "conan_sinkhorn_ext_lds_resident": "test_gpu_sinkhorn_ext.py",
    "conan_sinkhorn_ext_nerr": "test_sinkhorn_ext_cpu.py", "conan_sinkhorn_ext_workspace_bytes": "test_gpu_sinkhorn_ext.py",
    "conan_sinkhorn_fwd": "test_gpu_sinkhorn.py", "conan_sinkhorn_lds_resident": "test_gpu_sinkhorn.py",
    "conan_sinkhorn_workspace_bytes": "test_gpu_sinkhorn.py",
}
# exports that no test calls by name: none since test_gpu_edge_ops.py took the CFConv, filter and stage-2 head kernels.  An export added
# without a test has to be entered somewhere above, or here, for the ledger to pass.
UNNAMED = []


def owned_by(fname):
    """The exports a per-kernel GPU file owns, from its SOURCE (importing it would need a GPU): its OWNED list, or the header section its closing
    test cuts out with text.index(...)."""
    src = open(os.path.join(TESTS, fname)).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "OWNED" for t in node.targets):
            return list(ast.literal_eval(node.value))
    m = re.search(r"sect\s*=\s*text\[\s*text\.index\(\s*\"([^\"]+)\"\s*\)\s*:\s*(?:text\.index\(\s*\"([^\"]+)\"\s*\))?\s*\]", src)
    assert m, fname
    text = open(os.path.join(ROOT, "include", "conan_fgw_hip.h")).read()
    sect = text[text.index(m.group(1)):text.index(m.group(2)) if m.group(2) else None]
    return re.findall(r"^(?:int|long long)\s+(conan_\w+)\s*\(", sect, flags=re.M)


def test_ledger_every_export_has_an_owner():
    """Per-kernel files + ELSEWHERE + UNNAMED == _lib.SIGNATURES, without overlap: a new export without a test fails here."""
    owned = {f: owned_by(f) for f in PER_KERNEL_FILES}
    assert [len(owned[f]) for f in PER_KERNEL_FILES] == [33, 7, 21, 19, 24], {f: len(v) for f, v in owned.items()}
    names = [n for f in PER_KERNEL_FILES for n in owned[f]] + list(ELSEWHERE) + UNNAMED
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert set(names) == set(_lib.SIGNATURES), (sorted(set(_lib.SIGNATURES) - set(names)), sorted(set(names) - set(_lib.SIGNATURES)))
    for name, fname in ELSEWHERE.items():
        assert re.search(r"\b%s\b" % name, open(os.path.join(TESTS, fname)).read()), (name, fname)
    others = [f for f in sorted(os.listdir(TESTS)) if f.endswith(".py") and f not in ("test_abi.py", "test_dense_ref_cpu.py")]
    for name in UNNAMED:
        hits = [f for f in others if re.search(r"\b%s\b" % name, open(os.path.join(TESTS, f)).read())]
        assert not hits, (name, hits, "named by a test now: move it to ELSEWHERE or to a per-kernel file")
