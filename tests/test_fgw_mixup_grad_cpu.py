"""CPU-side checks of the differentiable FGWMixup pair (fgw.fgw_barycenters_BAPG with gradients, fgw.fgw_mixup_distance): the plain fp64 formulas
of tests/fgw_mixup_grad_ref.py reproduce every mixup_grad_* fixture's fp64 run, so they can stand in where no fixture exists; the fixture set is
complete and its `grads` lists are what the convention says; the public functions have the documented signatures and still refuse CPU tensors;
the C ABI is untouched.  No compute call: there is no GPU here."""
import inspect
import os

import numpy as np
import pytest
import torch

from fgw_mixup_grad_ref import fixture_problem, mixup_distance, update_steps
from helpers import golden_files, rel

FILES = golden_files("mixup_grad_")
ids = lambda paths: [os.path.basename(p)[11:-4] for p in paths]


def _formula_run(g):
    """The formulas at the fixture's r64 couplings, differentiated by autograd for the fixture's loss -> {name: value} in the fixture's shapes."""
    pr = fixture_problem(g)
    N, Np, sizes = pr["N"], pr["Np"], pr["sizes"]
    n_max = g["Ys"].shape[1]
    given = {"p": "p" in g.files, "lam": "lambdas" in g.files}          # uniform weights that the caller did not pass are no leaves
    leaves = {k: pr[k].clone().requires_grad_(given.get(k, True)) for k in ("Ys", "Cs", "p", "lam", "init_C", "init_Y") if pr[k] is not None}
    Y, C = update_steps(pr["T"], leaves["Ys"], leaves["Cs"], leaves["p"], leaves["lam"], leaves["init_C"], leaves.get("init_Y"), pr["kl"], pr["fs"], pr["ff"])
    Y, C = Y[0, :N], C[0, :N, :N]
    gw = torch.from_numpy(np.random.RandomState(int(g["gw_seed"])).normal(size=tuple(Y.shape)))
    gc = torch.from_numpy(np.random.RandomState(int(g["gc_seed"])).normal(size=tuple(C.shape)))
    ((Y * gw).sum() + (C * gc).sum()).backward()
    out = {"Y": Y.detach().numpy(), "C": C.detach().numpy()}
    cut = {"Ys": lambda v: v[0, :, :n_max], "Cs": lambda v: v[0, :, :n_max, :n_max], "p": lambda v: v[0, :N], "lam": lambda v: v,
           "init_C": lambda v: v[0, :N, :N], "init_Y": lambda v: v[0, :N]}
    for k, leaf in leaves.items():
        if leaf.grad is not None:
            out["d" + ("lambdas" if k == "lam" else k)] = cut[k](leaf.grad).numpy()
    return out, sizes


def test_fixture_set_is_complete():
    """What the committed set must contain, by content, not by file name."""
    gs = [np.load(p) for p in FILES]
    assert len(gs) >= 8
    plain = lambda g: not bool(g["fixed_structure"]) and not bool(g["fixed_features"])
    assert any(str(g["loss_fun"]) == "kl_loss" for g in gs)
    assert any(not np.array_equal(g["Cs"], g["Cs"].transpose(0, 2, 1)) for g in gs)
    assert any(bool(g["fixed_structure"]) for g in gs) and any(bool(g["fixed_features"]) and "init_Y" in g.files for g in gs)
    assert any("p" in g.files and "lambdas" in g.files and len({float(v) for v in g["ps"][0, :int(g["sizes"][0])]}) > 1 for g in gs)
    assert any([int(n) for n in g["sizes"]] == [9, 6, 8] and int(g["N"]) == 7 for g in gs)
    assert any(int(g["N"]) > 64 for g in gs)
    assert any(plain(g) and "p" not in g.files and "lambdas" not in g.files and str(g["loss_fun"]) == "square_loss" for g in gs)
    for p in FILES:
        assert os.path.getsize(p) < 256 * 1024, p
        assert not os.path.basename(p).startswith(("mixup_bary_", "mixup_acc_", "fgw_grad_"))


@pytest.mark.parametrize("path", FILES, ids=ids(FILES))
def test_fixture_is_consistent(path):
    g = np.load(path)
    sizes, N = [int(n) for n in g["sizes"]], int(g["N"])
    K, n_max, d = g["Ys"].shape
    for tag, dt in (("r32", np.float32), ("r64", np.float64)):
        assert g[tag + "_Y"].shape == (N, d) and g[tag + "_C"].shape == (N, N) and g[tag + "_T"].shape == (K, N, n_max) and g[tag + "_Y"].dtype == dt
        for k in g.files:
            if k.startswith(tag + "_"):
                assert np.isfinite(g[k]).all(), k
    for s, n in enumerate(sizes):
        np.testing.assert_allclose(g["r64_T"][s, :, :n].sum(0), g["ps"][s, :n].astype(np.float64), rtol=1e-12)      # the last half-step scales the columns
        assert not g["r64_T"][s, :, n:].any() and not g["ps"][s, n:].any()
    assert 1 <= int(g["outer"]) <= int(g["max_iter"])


@pytest.mark.parametrize("path", FILES, ids=ids(FILES))
def test_grads_lists_follow_the_convention(path):
    """Ys / Cs unless fixed, then init_Y / init_C instead; p and lambdas when given; never ps."""
    g = np.load(path)
    fs, ff = bool(g["fixed_structure"]), bool(g["fixed_features"])
    want = ([] if ff else ["Ys"]) + ([] if fs else ["Cs"]) + [k for k in ("p", "lambdas") if k in g.files] + (["init_C"] if fs else []) + (["init_Y"] if ff else [])
    assert [str(x) for x in g["grads"]] == want
    assert "ps" not in [str(x) for x in g["grads"]] and "r64_dps" not in g.files
    for name in want:
        assert "r64_d" + name in g.files and "r32_d" + name in g.files


def test_formulas_reproduce_every_fixture():
    """fp64 against fp64 with the same formulas in another summation order (einsum against a sum of matrix products).  Measured worst relative
    error over the committed fixtures: 6.1e-16 (Y, C) and 7.5e-16 (gradients); asserted with a factor-10 margin on the rounded-up
    figure, 1e-15 -> 1e-14."""
    worst = {"value": 0.0, "grad": 0.0}
    for path in FILES:
        g = np.load(path)
        out, _ = _formula_run(g)
        assert sorted(k[1:] for k in out if k.startswith("d")) == sorted(str(x) for x in g["grads"]), path
        for k, v in out.items():
            kind = "grad" if k.startswith("d") else "value"
            worst[kind] = max(worst[kind], rel(v, g["r64_" + k]))
    print(f"worst relative error against r64: Y, C {worst['value']:.2e}, gradients {worst['grad']:.2e}")
    assert worst["value"] <= 1e-14 and worst["grad"] <= 1e-14, worst


def test_distance_formula_is_objective_plus_the_constant_term():
    """mixup_distance against its definition written out entry by entry, on a directed rectangular pair."""
    rng = np.random.RandomState(2)
    n1, n2, alpha = 5, 4, 0.6
    M, A, Bm, X = rng.uniform(size=(n1, n2)), rng.uniform(size=(n1, n1)), rng.uniform(size=(n2, n2)), rng.uniform(size=(n1, n2))
    a, b = rng.uniform(size=n1), rng.uniform(size=n2)
    want = 0.0
    for i in range(n1):
        for j in range(n2):
            c1 = sum(A[i, k] ** 2 * a[k] for k in range(n1)) + sum(b[l] * Bm[l, j] ** 2 for l in range(n2))
            axb = sum(A[i, k] * X[k, l] * Bm[l, j] for k in range(n1) for l in range(n2))
            want += ((1 - alpha) * M[i, j] + alpha * (c1 - 2 * axb)) * X[i, j]
    t = lambda v: torch.from_numpy(v)[None]
    got = float(mixup_distance(t(M), t(A), t(Bm), t(a), t(b), t(X), alpha)[0])
    assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(float(mixup_distance(t(M), t(A), t(Bm.T.copy()), t(a), t(b), t(X), alpha)[0]) - want) > 1e-3 * abs(want)


def test_public_names_have_the_documented_signatures():
    from conan_fgw_amd import fgw, ops
    sig = lambda f: [(p.name, p.kind.name, p.default) for p in inspect.signature(f).parameters.values()]
    E, PK, KO = inspect.Parameter.empty, "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY"
    assert sig(ops.fgw_acc_pair_distance) == [("M", PK, E), ("A", PK, E), ("Bm", PK, E), ("a", PK, None), ("b", PK, None), ("X0", PK, None), ("alpha", KO, E),
                                              ("rho", KO, E), ("epoch", KO, 200), ("eps", KO, 1e-5), ("n1", KO, None), ("n2", KO, None), ("return_plan", KO, False)]
    assert sig(fgw.fgw_mixup_distance) == [("M", PK, E), ("A", PK, E), ("B", PK, E), ("a", PK, None), ("b", PK, None), ("X", PK, None), ("alpha", PK, 0),
                                           ("epoch", PK, 200), ("eps", PK, 1e-5), ("rho", PK, 1e-1), ("log", PK, False)]
    assert sig(fgw.fgw_mixup_distance)[:-1] == sig(fgw.fused_ACC_torch)
    # what existed keeps its signature
    assert [n for n, _, _ in sig(ops.fgw_mixup_barycenter_batched)] == ["Ys", "Cs", "ps", "p", "lambdas", "init_C", "init_Y", "alpha", "rho", "max_iter", "tol",
                                                                        "epoch", "eps", "fixed_structure", "fixed_features", "loss_fun", "keep_iterates"]
    assert [n for n, _, _ in sig(ops.fgw_acc_pair_batched)] == ["M", "A", "Bm", "a", "b", "X0", "alpha", "rho", "epoch", "eps", "n1", "n2"]
    for f in (fgw.fgw_barycenters_BAPG, fgw.fgw_mixup_distance, fgw.fused_ACC_torch, ops.fgw_mixup_barycenter_batched, ops.fgw_acc_pair_distance):
        assert "forward only" not in f.__doc__ and "no gradient is carried" not in f.__doc__
    assert "forward only" not in fgw.__doc__
    for f in (fgw.fgw_barycenters_BAPG, fgw.fgw_mixup_distance, ops.fgw_mixup_barycenter_batched, ops.fgw_acc_pair_distance):
        assert "finite difference" in " ".join(f.__doc__.split()) and "held constant" in " ".join(f.__doc__.split())


def test_cpu_tensors_are_still_refused():
    from conan_fgw_amd import fgw, ops
    leaf = lambda *shape: torch.rand(shape).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="fgw_barycenters_BAPG runs on the GPU only: pass CUDA \\(ROCm\\) tensors"):
        fgw.fgw_barycenters_BAPG(5, [leaf(5, 3) for _ in range(2)], [leaf(5, 5) for _ in range(2)], lambdas=[leaf(), leaf()])
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.fgw_mixup_barycenter_batched(leaf(1, 2, 5, 3), leaf(1, 2, 5, 5))
    with pytest.raises(NotImplementedError, match="fgw_mixup_distance runs on the GPU only"):
        fgw.fgw_mixup_distance(leaf(5, 4), leaf(5, 5), leaf(4, 4), alpha=0.5)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.fgw_acc_pair_distance(leaf(1, 5, 4), leaf(1, 5, 5), leaf(1, 4, 4), alpha=0.5, rho=1.0)
    with pytest.raises(ValueError, match="rho must be positive"):
        ops.fgw_acc_pair_distance(leaf(1, 5, 4), leaf(1, 5, 5), leaf(1, 4, 4), alpha=0.5, rho=0.0)


def test_the_c_abi_is_untouched():
    from conan_fgw_amd import _lib
    assert _lib.ABI_VERSION == 6
    assert len(_lib.SIGNATURES) == N_EXPORTS


N_EXPORTS = 141          # len(_lib.SIGNATURES) of the parent commit: this feature adds no export
