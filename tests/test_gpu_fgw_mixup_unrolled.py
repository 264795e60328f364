"""The unrolled gradient of the FGWMixup barycenter on the GPU: ops.fgw_mixup_barycenter_unrolled / fgw.fgw_barycenters_BAPG_unrolled, i.e.
conan_fgw_mixup_barycenter_fwd_record + conan_fgw_mixup_barycenter_bwd (csrc/fgw_mixup_grad.hip; its size queries
conan_fgw_mixup_barycenter_bwd_workspace_bytes and conan_fgw_mixup_barycenter_bwd_lds_resident).

Yardstick: torch autograd through the reference's own fgw_barycenters_BAPG in fp64 (tests/golden/grad_mixup_unrolled_*.npz, written by
make_fgw_mixup_unrolled_golden.py), through the op and through the public function, for three cotangent choices served by one backward each.
The bound is 1e-6 in grad_error, derived as in test_gpu_fgw_acc_grad.py: the kernels read the fixture's own fp32 inputs, run in fp64 throughout
(the update steps' contributions fgw_part_t are fp64, the state record is fp64, every sum has a fixed order) and round each output entry to
fp32 once (2^-24 = 6e-8 relative per entry, so 6e-8 in the Frobenius ratio); what remains is fp64 rounding through at most 3 x 200 half-steps,
which the fp64 restatement measures against the same fixtures at 1.4e-12 at worst (test_fgw_mixup_unrolled_cpu.py).  1e-6 leaves a factor of ten over the
rounding (measured on the MI355X: 4.0e-8 at worst over the eleven fixtures).  The comparison means nothing at other iteration counts, so the counts are asserted first.

Where no fixture exists (a batch with unequal outer counts, a flagged molecule) the restatement tests/fgw_mixup_unrolled_ref.py and
fgw_mixup_ref.mixup_ref choose and check the inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fgw_mixup_unrolled_ref as R
from fgw_mixup_ref import fair, mixup_ref
from helpers import golden_files
from conan_fgw_amd import _lib
from conan_fgw_amd import fgw as pfgw
from conan_fgw_amd import ops
from conan_fgw_amd._lib import FgwParams, call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
FIX = golden_files("grad_mixup_unrolled_")
IDS = [os.path.basename(p)[len("grad_mixup_unrolled_"):-4] for p in FIX]
BOUND = 1e-6
bits = lambda x: x.detach().contiguous().view(torch.int32)
t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
fixture = lambda name: np.load([p for p in FIX if p.endswith(f"unrolled_{name}.npz")][0])


class Trace:
    """Records the name of every C-ABI call issued inside the block."""

    def __enter__(self):
        self.names = []

        def trace(name, fn, args):
            self.names.append(name)
            return fn(*args)
        self._prev = _lib.set_call_trace(trace)
        return self.names

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _lib.set_call_trace(self._prev)


def _kw(g):
    return dict(alpha=float(g["alpha"]), rho=float(g["rho"]), max_iter=int(g["max_iter"]), tol=float(g["tol"]), loss_fun=str(g["loss_fun"]),
                fixed_structure=bool(g["fixed_structure"]), fixed_features=bool(g["fixed_features"]))


def _op_leaves(g):
    """The fixture as the op's B = 1 leaves (the square embedded problem) -> (leaves dict, N, sizes, Np)."""
    (Ys, Cs, ps, p, lam, init_C, init_Y), _, N, sizes = R.fixture_problem(g)
    leaf = lambda a: None if a is None else t32(a)[None].requires_grad_(True)
    L = dict(Ys=leaf(Ys), Cs=leaf(Cs), ps=leaf(ps), p=leaf(p), lambdas=t32(lam).requires_grad_(True), init_C=leaf(init_C), init_Y=leaf(init_Y))
    return L, N, sizes, Ys.shape[1]


def _check_counts(g, info):
    assert int(info[0, 0]) == int(g["outer"]) and int(info[0, 1]) == int(g["epochs"].sum()), (info[0].tolist(), int(g["outer"]), g["epochs"].tolist())


def _compare(g, tag, got, label):
    worst = 0.0
    for k in R.GRADS:
        if f"{tag}_{k}" not in g.files:
            continue
        e = R.grad_error(got[k], g[f"{tag}_{k}"], R.cotangent_norm(g, tag))
        print(f"   {label} {tag} {k}: {e:.2e}")
        worst = max(worst, e)
    return worst


# ---------------------------------------------------------------------------------------------- 1. the reference's own gradient
@pytest.mark.parametrize("path", FIX, ids=IDS)
def test_op_matches_the_reference_gradient(path):
    g = np.load(path)
    L, N, sizes, Np = _op_leaves(g)
    Y, C, T, info, errs = ops.fgw_mixup_barycenter_unrolled(L["Ys"], L["Cs"], ps=L["ps"], p=L["p"], lambdas=L["lambdas"], init_C=L["init_C"],
                                                            init_Y=L["init_Y"], **_kw(g))
    _check_counts(g, info)
    assert Y.requires_grad and C.requires_grad and not any(x.requires_grad for x in (T, info, errs))
    names = [k for k in ("Ys", "Cs", "ps", "p", "lambdas", "init_C", "init_Y") if L[k] is not None]
    n_max, worst = g["Ys"].shape[1], 0.0
    for tag in R.TAGS:
        gY, gC = R.embed_cotangents(g, tag, Np)
        loss = sum((x[0] * t32(c)).sum() for x, c in ((Y, gY), (C, gC)) if c is not None)
        with Trace() as calls:
            gs = dict(zip(names, torch.autograd.grad(loss, [L[k] for k in names], retain_graph=True)))
        assert calls == ["conan_fgw_mixup_barycenter_bwd"]
        r = dict(dYs=gs["Ys"][0], dCs=gs["Cs"][0], dps=gs["ps"][0], dp=gs["p"][0], dlam=gs["lambdas"], dinit_C=gs["init_C"][0],
                 dinit_Y=gs["init_Y"][0] if "init_Y" in gs else None)
        got = R.cut({k: (None if v is None else v.cpu().numpy().astype(np.float64)) for k, v in r.items()}, N, sizes, n_max)
        worst = max(worst, _compare(g, tag, got, "op"))
    assert worst <= BOUND, worst


@pytest.mark.parametrize("path", FIX, ids=IDS)
def test_public_function_matches_the_reference_gradient(path):
    g = np.load(path)
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    K = len(sizes)
    leaf = lambda a: t32(a).requires_grad_(True)
    Ys = [leaf(g["Ys"][s, :n]) for s, n in enumerate(sizes)]
    Cs = [leaf(g["Cs"][s, :n, :n]) for s, n in enumerate(sizes)]
    ps = [leaf(g["ps"][s, :n]) for s, n in enumerate(sizes)]
    p = leaf(g["p"] if "p" in g.files else np.full(N, 1.0 / N))
    lam = leaf(g["lambdas"] if "lambdas" in g.files else np.full(K, 1.0 / K))
    init_C = leaf(g["init_C"])
    init_Y = leaf(g["init_Y"]) if "init_Y" in g.files else None
    kw = _kw(g)
    Y, C, log = pfgw.fgw_barycenters_BAPG_unrolled(N, Ys, Cs, ps=ps, p=p, lambdas=lam, init_C=init_C, init_Y=init_Y, log=True, **kw)
    assert log["n_outer"] == int(g["outer"]) and log["n_inner"] == int(g["epochs"].sum())
    assert not any(x.requires_grad for x in log["T"]) and tuple(Y.shape) == g["Y"].shape and tuple(C.shape) == g["C"].shape
    ins = Ys + Cs + ps + [p, lam, init_C] + ([] if init_Y is None else [init_Y])
    worst = 0.0
    for tag, (use_y, use_c) in R.TAGS.items():
        loss = ((Y * t32(g["gw"])).sum() if use_y else 0.0) + ((C * t32(g["gc"])).sum() if use_c else 0.0)
        gs = torch.autograd.grad(loss, ins, retain_graph=True)
        for x, gr in zip(ins, gs):
            assert gr.shape == x.shape                                  # ragged inputs: the caller's shapes
        dYs, dCs, dps = np.zeros(g["Ys"].shape), np.zeros(g["Cs"].shape), np.zeros(g["ps"].shape)
        for s, n in enumerate(sizes):
            dYs[s, :n], dCs[s, :n, :n], dps[s, :n] = gs[s].cpu().numpy(), gs[K + s].cpu().numpy(), gs[2 * K + s].cpu().numpy()
        got = dict(dYs=dYs, dCs=dCs, dps=dps, dp=gs[3 * K].cpu().numpy(), dlambdas=gs[3 * K + 1].cpu().numpy(), dinit_C=gs[3 * K + 2].cpu().numpy())
        if init_Y is not None:
            got["dinit_Y"] = gs[3 * K + 3].cpu().numpy()
        worst = max(worst, _compare(g, tag, got, "fgw"))
    assert worst <= BOUND, worst
    # lambdas as a list of 0-d tensors keeps its graph
    lam_l = [leaf(np.float32(v)) for v in (g["lambdas"] if "lambdas" in g.files else np.full(K, 1.0 / K))]
    Y2, C2 = pfgw.fgw_barycenters_BAPG_unrolled(N, Ys, Cs, ps=ps, p=p, lambdas=lam_l, init_C=init_C, init_Y=init_Y, **kw)
    g2 = torch.autograd.grad((Y2 * t32(g["gw"])).sum() + (C2 * t32(g["gc"])).sum(), lam_l)
    assert R.grad_error(np.array([float(v) for v in g2]), g["gB_dlambdas"], R.cotangent_norm(g, "gB")) <= BOUND


# ---------------------------------------------------------------------------------------------- 2. the same solve; the replay retraces it
@pytest.mark.parametrize("name", ["k3_n10_d4", "k5_n33_d8_weights", "k2_n66_d4", "kl", "tol_stop"])
def test_forward_is_the_batched_ops_bit_for_bit_and_the_replay_retraces_it(name):
    g = fixture(name)
    L, N, sizes, Np = _op_leaves(g)
    D = {k: (None if v is None else v.detach()) for k, v in L.items()}
    kw = dict(_kw(g), keep_iterates=True)
    want = ops.fgw_mixup_barycenter_batched(D["Ys"], D["Cs"], ps=D["ps"], p=D["p"], lambdas=D["lambdas"], init_C=D["init_C"], init_Y=D["init_Y"], **kw)
    with Trace() as calls:
        got = ops.fgw_mixup_barycenter_unrolled(L["Ys"], L["Cs"], ps=L["ps"], p=L["p"], lambdas=L["lambdas"], init_C=L["init_C"], init_Y=L["init_Y"], **kw)
    assert calls == ["conan_fgw_mixup_barycenter_fwd_record"] and len(got) == 6
    for a, b in zip(want, got):
        assert torch.equal(bits(a), bits(b))
    # the C entry points directly, with the check outputs
    B, K, d = 1, len(sizes), g["Ys"].shape[2]
    mi, k = int(g["max_iter"]), _kw(g)
    assert lib().conan_fgw_mixup_barycenter_bwd_lds_resident(Np) == (0 if name == "k2_n66_d4" else 1)
    prm = FgwParams(k["alpha"], 0.0, mi, k["tol"], 0.0, 1, 0.0, 0, 0, 0, int(k["loss_fun"] == "kl_loss"), 0)
    Y = torch.empty(B, Np, d, device=dev); C = torch.empty(B, Np, Np, device=dev); T = torch.empty(B, K, Np, Np, device=dev)
    info = torch.empty(B, 4, dtype=torch.int32, device=dev); errs = torch.empty(B, 2, mi, device=dev)
    record = torch.empty((mi + 1) * B * (Np * Np + Np * d), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib().conan_fgw_mixup_workspace_bytes(B, K, Np, d)), dtype=torch.uint8, device=dev)
    ins = [ptr(D[n]) for n in ("Ys", "Cs", "ps", "p", "lambdas")]
    call("conan_fgw_mixup_barycenter_fwd_record", *ins, ptr(D["init_C"]), ptr(D["init_Y"]), B, K, Np, d, ctypes.byref(prm), k["rho"], 100, 1e-5,
         ptr(Y), ptr(C), ptr(T), None, ptr(info), ptr(errs), ptr(record), ptr(ws), stream_ptr())
    for a, b in zip((Y, C, T, info, errs), want):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(record[:Np * Np].view(Np, Np).float(), D["init_C"][0])                      # state 0 is the start
    gY, gC = (t32(v)[None].contiguous() for v in R.embed_cotangents(g, "gB", Np))          # (held: the call takes raw pointers)
    dYs = torch.empty(B, K, Np, d, device=dev); dCs = torch.empty(B, K, Np, Np, device=dev)
    T_chk = torch.full((B, K, Np, Np), 7.0, device=dev); ep = torch.full((mi, B, K), 7, dtype=torch.int32, device=dev)
    bws = torch.empty(int(lib().conan_fgw_mixup_barycenter_bwd_workspace_bytes(B, K, Np, d, 100)), dtype=torch.uint8, device=dev)
    call("conan_fgw_mixup_barycenter_bwd", *ins, ptr(D["init_Y"]), B, K, Np, d, ctypes.byref(prm), k["rho"], 100, 1e-5, ptr(info), ptr(record),
         ptr(gY), ptr(gC), ptr(dYs), ptr(dCs), None, None, None, None, None, ptr(T_chk), ptr(ep),
         ptr(bws), stream_ptr())
    assert torch.equal(bits(T_chk), bits(T))
    outer = int(g["outer"])
    assert ep[:outer, 0].cpu().numpy().tolist() == g["epochs"].tolist() and not bool(ep[outer:].any()) and int(ep.sum()) == int(info[0, 1])
    assert R.grad_error(dYs[0, :, :g["Ys"].shape[1]].cpu().numpy(), g["gB_dYs"], R.cotangent_norm(g, "gB")) <= BOUND


# ---------------------------------------------------------------------------------------------- 3. where the gradient goes
def test_zero_weight_and_massless_nodes_get_exact_zeros():
    g = fixture("zero_ps")
    z = int(g["zero_at"])
    L, N, sizes, Np = _op_leaves(g)
    Y, C, *_ = ops.fgw_mixup_barycenter_unrolled(L["Ys"], L["Cs"], ps=L["ps"], p=L["p"], lambdas=L["lambdas"], init_C=L["init_C"], **_kw(g))
    ((Y[0] * t32(g["gw"])).sum() + (C[0] * t32(g["gc"])).sum()).backward()
    assert not bool(L["ps"].grad[0, 0, z]) and not bool(L["Ys"].grad[0, 0, z].any())
    assert not bool(L["Cs"].grad[0, 0, z].any()) and not bool(L["Cs"].grad[0, 0, :, z].any())
    for k in ("Ys", "Cs", "ps", "p", "lambdas", "init_C"):
        assert bool(torch.isfinite(L[k].grad).all()) and bool(L[k].grad.any()), k
    assert bool((L["ps"].grad[0, 1:] != 0).all()) and bool((L["p"].grad != 0).all())
    # the ragged fixture: the embedding's massless nodes, of the barycenter (7 of 9) and of the graphs
    g = fixture("ragged_N7")
    L, N, sizes, Np = _op_leaves(g)
    Y, C, *_ = ops.fgw_mixup_barycenter_unrolled(L["Ys"], L["Cs"], ps=L["ps"], p=L["p"], lambdas=L["lambdas"], init_C=L["init_C"], **_kw(g))
    (Y.sum() + (C * C).sum()).backward()
    assert N < Np and not bool(L["p"].grad[0, N:].any()) and not bool(L["init_C"].grad[0, N:].any()) and not bool(L["init_C"].grad[0, :, N:].any())
    for s, n in enumerate(sizes):
        assert not bool(L["ps"].grad[0, s, n:].any()) and not bool(L["Ys"].grad[0, s, n:].any())
        assert not bool(L["Cs"].grad[0, s, n:].any()) and not bool(L["Cs"].grad[0, s, :, n:].any())
        assert bool(L["ps"].grad[0, s, :n].all())


def test_fixed_starts_receive_their_gradient_and_the_inputs_still_theirs():
    for name, start, other in (("fixedC", "init_C", "Cs"), ("fixedY", "init_Y", "Ys")):
        g = fixture(name)
        L, N, sizes, Np = _op_leaves(g)
        Y, C, *_ = ops.fgw_mixup_barycenter_unrolled(L["Ys"], L["Cs"], ps=L["ps"], p=L["p"], lambdas=L["lambdas"], init_C=L["init_C"],
                                                     init_Y=L["init_Y"], **_kw(g))
        ((Y[0] * t32(g["gw"])).sum() + (C[0] * t32(g["gc"])).sum()).backward()
        assert bool(L[start].grad.any()) and bool(L[other].grad.any()) and bool(torch.isfinite(L[other].grad).all())
        assert R.grad_error(L[start].grad[0].cpu().numpy(), g[f"gB_d{start}"], R.cotangent_norm(g, "gB")) <= BOUND


def test_without_init_C_the_start_is_the_first_graph_and_gets_its_gradient():
    g = fixture("k3_n10_d4")                                             # (its init_C IS Cs[0]: make_fgw_grad_golden.case)
    assert np.array_equal(g["init_C"], g["Cs"][0].astype(np.float32))
    L, N, sizes, Np = _op_leaves(g)
    Y, C, T, info, errs = ops.fgw_mixup_barycenter_unrolled(L["Ys"], L["Cs"], ps=L["ps"], p=L["p"], lambdas=L["lambdas"], **_kw(g))
    _check_counts(g, info)
    ((Y[0] * t32(g["gw"])).sum() + (C[0] * t32(g["gc"])).sum()).backward()
    want = g["gB_dCs"].copy()
    want[0] += g["gB_dinit_C"]
    assert R.grad_error(L["Cs"].grad[0].cpu().numpy(), want, R.cotangent_norm(g, "gB")) <= BOUND


# ---------------------------------------------------------------------------------------------- 4. batches
def _molecule(seed, K=3, n=10, d=4):
    rng = np.random.RandomState(seed)
    Ys = rng.uniform(0.1, 2.0, size=(K, n, d)).astype(np.float32)
    u = np.triu(rng.random_sample((K, n, n)) < 0.35, 1)
    return Ys, (u | u.transpose(0, 2, 1)).astype(np.float32)


def _batch_grads(Ys, Cs, gw, gc, **kw):
    L = [t32(Ys).requires_grad_(True), t32(Cs).requires_grad_(True)]
    B, K, N, d = Ys.shape
    ps = torch.full((B, K, N), 1.0 / N, device=dev, requires_grad=True)
    p = torch.full((B, N), 1.0 / N, device=dev, requires_grad=True)
    lam = torch.full((K,), 1.0 / K, device=dev, requires_grad=True)
    out = ops.fgw_mixup_barycenter_unrolled(L[0], L[1], ps=ps, p=p, lambdas=lam, **kw)
    ((out[0] * t32(gw)).sum() + (out[1] * t32(gc)).sum()).backward()
    return out, [L[0].grad, L[1].grad, ps.grad, p.grad], lam.grad


def test_molecules_with_unequal_outer_counts_equal_their_solo_runs_bit_for_bit():
    """Seeds 510, 500, 516 at tol = 0.15: the fp64 restatement leaves after 4, 5 and 4 outer iterations, every outer error and every compared
    objective change fair (chosen on the CPU; asserted here)."""
    kw = dict(alpha=0.5, rho=4.0, max_iter=6, tol=0.15)
    mols = [_molecule(s) for s in (510, 500, 516)]
    counts = []
    for Ys, Cs in mols:
        _, _, lg = mixup_ref(10, list(Ys), list(Cs), init_C=Cs[0], **kw)
        assert fair(lg["err_feature"] + lg["err_structure"], np.float32(kw["tol"])) and fair(lg["rel"], 1e-5)
        counts.append(len(lg["err_feature"]))
    assert counts == [4, 5, 4]
    Ys, Cs = np.stack([m[0] for m in mols]), np.stack([m[1] for m in mols])
    rng = np.random.RandomState(5)
    gw, gc = rng.normal(size=(3, 10, 4)).astype(np.float32), rng.normal(size=(3, 10, 10)).astype(np.float32)
    out, grads, dlam = _batch_grads(Ys, Cs, gw, gc, **kw)
    assert out[3][:, 0].tolist() == counts
    for b in range(3):
        solo, sg, _ = _batch_grads(Ys[b:b + 1], Cs[b:b + 1], gw[b:b + 1], gc[b:b + 1], **kw)
        for x, y in zip(out[:5], solo[:5]):
            assert torch.equal(bits(x[b]), bits(y[0]))
        for x, y in zip(grads, sg):
            assert torch.equal(bits(x[b]), bits(y[0])) and bool(torch.isfinite(y).all()) and bool(y.any())
    assert bool(torch.isfinite(dlam).all())


def test_a_flagged_molecule_gives_nan_beside_healthy_ones_that_keep_their_bits():
    """test_gpu_fgw_mixup.py's underflow (64-wide features, rho = 1e-2: every exp of the first half-step is 0, a / 0 * 0 is NaN) in molecule 1;
    molecules 0 and 2 carry features scaled down so that they stay finite at the same rho.  The reference's documented NaN, not a fault."""
    rng = np.random.RandomState(3)
    K, N, d = 3, 12, 64
    Ys = rng.uniform(0.1, 2.0, size=(3, K, N, d)).astype(np.float32)
    Ys[0] *= 0.01; Ys[2] *= 0.01
    u = np.triu(rng.random_sample((3, K, N, N)) < 0.4, 1)
    Cs = (u | u.transpose(0, 1, 3, 2)).astype(np.float32) * np.float32(0.02)
    kw = dict(alpha=0.5, rho=1e-2, max_iter=2, tol=1e-9)
    gw, gc = rng.normal(size=(3, N, d)).astype(np.float32), rng.normal(size=(3, N, N)).astype(np.float32)
    out, grads, dlam = _batch_grads(Ys, Cs, gw, gc, **kw)
    assert [int(v) & 4 for v in out[3][:, 3]] == [0, 4, 0]
    assert bool(torch.isnan(dlam).all())
    for x in grads:
        assert bool(torch.isnan(x[1]).all()) and bool(torch.isfinite(x[0]).all()) and bool(torch.isfinite(x[2]).all())
    for b in (0, 2):
        _, sg, sl = _batch_grads(Ys[b:b + 1], Cs[b:b + 1], gw[b:b + 1], gc[b:b + 1], **kw)
        assert bool(torch.isfinite(sl).all())
        for x, y in zip(grads, sg):
            assert torch.equal(bits(x[b]), bits(y[0])) and bool(y.any())


def test_without_a_leaf_nothing_beyond_the_forward_runs_and_nothing_is_saved():
    g = fixture("k3_n10_d4")
    L, N, sizes, Np = _op_leaves(g)
    D = {k: (None if v is None else v.detach()) for k, v in L.items()}
    with Trace() as calls:
        plain = ops.fgw_mixup_barycenter_unrolled(D["Ys"], D["Cs"], ps=D["ps"], p=D["p"], lambdas=D["lambdas"], init_C=D["init_C"], **_kw(g))
    assert calls == ["conan_fgw_mixup_barycenter_fwd"] and all(x.grad_fn is None and not x.requires_grad for x in plain)
    with torch.no_grad(), Trace() as calls:
        off = ops.fgw_mixup_barycenter_unrolled(L["Ys"], L["Cs"], ps=L["ps"], p=L["p"], lambdas=L["lambdas"], init_C=L["init_C"], **_kw(g))
    assert calls == ["conan_fgw_mixup_barycenter_fwd"] and all(x.grad_fn is None for x in off)
    for a, b in zip(plain, off):
        assert torch.equal(bits(a), bits(b))
