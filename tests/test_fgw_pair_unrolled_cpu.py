"""The unrolled pairwise FGW gradient, what needs no GPU: the fp64 restatement tests/fgw_pair_unrolled_ref.py reproduces torch autograd through the
reference's own fgw on every stored fixture (tests/golden/fgw_unrollgrad_*.npz, written by tests/golden/make_fgw_pair_unrolled_golden.py) to
1e-9 (grad_error: the Frobenius norm of the difference over that of the yardstick; worst measured: 1.6e-13, on ppa_dir_n80_false), which pins
both the restatement and the conditioning of the chosen cases; a central finite difference of the restatement's own forward; the fixed-plan
gradient is a different quantity; every header named in _lib.EXT_TABLES agrees with its table and the library; the host-side queries answer;
bad arguments are refused before any launch; the public functions have their signatures and their refusals hold on CPU tensors."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, fgw, ops

from fgw_pair_unrolled_ref import F64, grad_error, pair_distance, pair_forward, pair_grad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INCLUDE = os.path.join(ROOT, "include")
REUSED = ["pgd_1x5", "pgd_model_n20", "pgd_n10", "pgd_n10_cap25", "pgd_n10_g0", "pgd_rect_7x12", "pgd_dir_n12_false", "pgd_dir_n12_none",
          "pgd_undir_n12_none", "pgd_n33", "pgd_n80", "ppa_dir_n80_false"]
NEW = ["ppa_12x9", "zerop_9x11"]
FINITE = REUSED + NEW
NAN = "nan_ppa_n10"
SYM = {1: True, 0: False, -1: None}
HEADER = "conan_fgw_hip_pair_grad.h"
EXPORTS = ("conan_fgw_pair_bwd_lds_resident", "conan_fgw_pair_bwd_workspace_bytes", "conan_fgw_pair_bwd")
KEYS = ("dM", "dC1", "dC2", "dp", "dq", "dG0")


def load(name):
    """The fixture and the file that holds its inputs and parameters (a reused case: tests/golden/fgw_pair_<src>.npz)."""
    z = np.load(os.path.join(GOLDEN, f"fgw_unrollgrad_{name}.npz"))
    f = {k: z[k] for k in z.files}
    src = str(f["src"])
    g = np.load(os.path.join(GOLDEN, f"fgw_pair_{src}.npz")) if src else f
    return f, g


def problem(g):
    return (g["M"], g["C1"].astype(np.float32), g["C2"].astype(np.float32), g["p"], g["q"], g["G0"] if g["G0"].size else None)


def ref_kw(f, g):
    return dict(alpha=float(g["alpha"]), epsilon=float(g["epsilon"]), solver=str(g["solver"]), symmetric=SYM[int(g["symmetric"])], iters=int(f["iters"]),
                num_iter_max=int(g["num_iter_max"]), stop_thr=float(g["stop_thr"]))


def test_fixture_list_is_complete():
    have = sorted(os.path.basename(p)[len("fgw_unrollgrad_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "fgw_unrollgrad_*.npz")))
    assert have == sorted(FINITE + [NAN])
    for name in have:
        assert os.path.getsize(os.path.join(GOLDEN, f"fgw_unrollgrad_{name}.npz")) < 512 * 1024
    for name in REUSED:
        assert str(load(name)[0]["src"]) == name


@pytest.mark.parametrize("name", FINITE)
def test_restatement_reproduces_the_reference_autograd(name):
    f, g = load(name)
    M, C1, C2, p, q, G0 = problem(g)
    assert all(v.dtype == np.float32 for v in (M, p, q, f["W"])) and str(g["loss_fun"]) == "square_loss" and str(g["solver"]) in ("PGD", "PPA")
    if str(f["src"]):
        assert float(f["dist"]) == float(g["r64_fgw_dist"]) and int(f["iters"]) == int(g["r64_it"]) and int(f["sweeps"].sum()) == int(g["r64_sk"])
    assert len(f["sweeps"]) == int(f["iters"]) and (np.abs(f["sk_errs"] - float(g["stop_thr"])) > 1e-6 * float(g["stop_thr"])).all()
    assert ("gT_dG0" in f) == (G0 is not None) == (name == "pgd_n10_g0")
    if name == "ppa_12x9":
        assert M.shape == (12, 9) and int(f["iters"]) == 20 and (C1 == C1.T).all()
    if name == "zerop_9x11":
        assert p[3] == 0 and (p > 0).sum() == 8 and np.isnan(f["ref_full_dp"][:, 3]).all() and float(f["ref_full_gap"]) > 1e-9      # the reference's log(0)
    for tag, kw, cot in (("gT", dict(dT=f["W"]), f["W"]), ("gd", dict(ddist=1.0), 1.0)):
        r = pair_grad_ref(M, C1, C2, p, q, G0, **ref_kw(f, g), **kw)
        assert not r["nan"] and list(r["sweeps"]) == list(f["sweeps"])     # the sweep counts of every Sinkhorn call, decided by the restatement
        assert grad_error(r["T"], f["T"]) <= 1e-12 and abs(r["dist"] - float(f["dist"])) <= 1e-12 * abs(float(f["dist"]))
        for k in KEYS:
            if f"{tag}_{k}" in f:
                e = grad_error(r[k], f[f"{tag}_{k}"], cot)
                print(f"{name} {tag} {k}: {e:.2e}")
                assert e <= 1e-9, (name, tag, k, e)
        if name == "zerop_9x11":                                           # the massless rule: exact zeros, no division by the zero weight
            assert r["dp"][3] == 0 and not r["dM"][3].any() and not r["dC1"][3].any() and not r["dC1"][:, 3].any() and not r["T"][3].any()
            assert all(np.isfinite(r[k]).all() for k in KEYS[:5])


def test_nan_fixture():
    """PPA after entries of the plan have underflowed to exact zero: the reference's autograd gives NaN everywhere, and the restatement names the
    cause (an exact zero of an input plan at an entry with mass) far from the underflow border."""
    f, g = load(NAN)
    assert float(f["log_zero_max"]) < -800.0 and float(f["log_lowest_before"]) > -700.0 and 0 < int(f["first_zero_iter"]) < int(f["iters"]) - 1
    assert np.isfinite(f["T"]).all() and not any(k.startswith(("gT_", "gd_")) for k in f)      # (the reference's gradients: all NaN, not stored)
    r = pair_grad_ref(*problem(g), **ref_kw(f, g), dT=f["W"], ddist=1.0)
    assert r["nan"] and all(np.isnan(r[k]).all() for k in KEYS[:5]) and list(r["sweeps"]) == list(f["sweeps"])


def test_fixed_plan_gradient_is_a_different_quantity():
    f, g = load("pgd_model_n20")
    M, C1, C2, p, q, _ = (None if v is None else torch.from_numpy(v).to(F64) for v in problem(g))
    T, alpha = torch.from_numpy(f["T"]), float(g["alpha"])
    r, c = T.sum(1), T.sum(0)
    fixed = dict(dM=(1 - alpha) * T, dC1=2 * alpha * (C1 * (r[:, None] * p[None, :]) - T @ C2 @ T.T), dC2=2 * alpha * (C2 * (c[:, None] * q[None, :]) - T.T @ C1 @ T),
                 dp=alpha * ((C1 * C1).T @ r), dq=alpha * ((C2 * C2).T @ c))
    for k, v in fixed.items():
        e = grad_error(v.numpy(), f[f"gd_{k}"])
        print(f"fixed-plan {k} against the unrolled gradient: {e:.3f}")
        assert e > 1e-3, (k, e)


def test_restatement_against_a_central_finite_difference():
    """L = sum(W * T) + 0.7 fgw_dist on a 4 x 5 PPA pair with a start, directed graphs (symmetric=False) and given weights, 3 outer iterations
    of 4, 3, 5 sweeps held fixed: <gradient, V> against (L(x + h V) - L(x - h V)) / 2h for a random direction V of every input.  h = 1e-6.  The
    error of a difference quotient is ABSOLUTE: the rounding term eps |L| / h = 2.2e-10 |L|, and the truncation term h^2 L''' / 6, 1e-12 times
    third derivatives of order (4 alpha / epsilon)^3 = 64.  Bound: 10 eps |L| / h (about 2e-9 here), with every directional derivative required
    above 1e-4, five orders more than the bound: a missing or mis-signed term of the walk cannot hide under it."""
    g = np.random.default_rng(13)
    n1, n2, alpha, eps, gd, sweeps = 4, 5, 0.5, 0.5, 0.7, [4, 3, 5]
    x, y = g.uniform(0.1, 1.5, (n1, 3)), g.uniform(0.1, 1.5, (n2, 3))
    ins = dict(M=((x[:, None] - y[None]) ** 2).sum(-1), C1=(g.random((n1, n1)) < 0.5).astype(np.float64) + 0.1 * g.random((n1, n1)),
               C2=(g.random((n2, n2)) < 0.5).astype(np.float64) + 0.1 * g.random((n2, n2)), p=g.uniform(0.5, 1.5, n1), q=g.uniform(0.5, 1.5, n2))
    ins["p"] /= ins["p"].sum(); ins["q"] /= ins["q"].sum()
    ins["G0"] = np.outer(ins["p"], ins["q"]) * g.uniform(0.5, 1.5, (n1, n2))
    W = g.standard_normal((n1, n2))
    kw = dict(alpha=alpha, epsilon=eps, solver="PPA", iters=len(sweeps), num_iter_max=10, stop_thr=0.0, sweeps=sweeps)

    def loss(v):
        t = {k: torch.from_numpy(np.ascontiguousarray(u)).to(F64) for k, u in v.items()}
        T = pair_forward(t["M"], t["C1"], t["C2"], t["p"], t["q"], t["G0"], sym=False, **kw)
        return float((torch.from_numpy(W) * T).sum() + gd * pair_distance(t["M"], t["C1"], t["C2"], t["p"], t["q"], T, alpha))

    r = pair_grad_ref(ins["M"], ins["C1"], ins["C2"], ins["p"], ins["q"], ins["G0"], symmetric=False, dT=W, ddist=gd, **kw)
    assert not r["nan"] and list(r["sweeps"]) == sweeps
    h = 1e-6
    for k, gk in (("M", "dM"), ("C1", "dC1"), ("C2", "dC2"), ("p", "dp"), ("q", "dq"), ("G0", "dG0")):
        V = g.standard_normal(ins[k].shape) * np.abs(ins[k]).mean()
        fd = (loss(dict(ins, **{k: ins[k] + h * V})) - loss(dict(ins, **{k: ins[k] - h * V}))) / (2 * h)
        an = float((r[gk] * V).sum())
        print(f"{k}: analytic {an:+.9e} finite difference {fd:+.9e}")
        assert abs(an) > 1e-4 and abs(fd - an) <= 10 * np.finfo(np.float64).eps * abs(loss(ins)) / h, (k, an, fd)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return {m.group(2): len(m.group(3).split(",")) for m in re.finditer(r"\b(int|long long)\s+(conan_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_every_ext_table_agrees_with_its_header_and_the_library():
    assert list(_lib.EXT_TABLES)[0] == HEADER and set(_lib.EXT_TABLES[HEADER]) == set(EXPORTS)
    raw = ctypes.CDLL(_lib.library_path())
    first = open(os.path.join(INCLUDE, "conan_fgw_hip.h")).read()
    seen = set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES)
    for header, table in _lib.EXT_TABLES.items():
        d = _declared(header)
        assert set(d) == set(table), header
        assert not set(table) & seen, f"{header}: a name appears in two tables"
        seen |= set(table)
        for name, (_res, args) in table.items():
            assert len(args) == d[name], name
            assert hasattr(raw, name), f"{name} declared in {header} but not exported"
            assert not re.search(r"\b" + name + r"\b", first), f"{name} belongs to {header} only"
            assert getattr(_lib.lib(), name).argtypes == args                # lib() binds the table
    assert _lib.lib().conan_abi_version() == _lib.ABI_VERSION == 6          # an added export does not change the version
    I, LL, P, D = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_double
    assert _lib.EXT_TABLES[HEADER]["conan_fgw_pair_bwd"] == (I, [P] * 6 + [I, I, D, D, I, I, D, I, I] + [P] * 13)
    assert _lib.EXT_TABLES[HEADER]["conan_fgw_pair_bwd_workspace_bytes"] == (LL, [I, I, I, I])
    assert _lib.EXT_TABLES[HEADER]["conan_fgw_pair_bwd_lds_resident"] == (I, [I])


def test_every_entry_is_named_by_the_gpu_test_file():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_fgw_pair_unrolled.py")).read()
    for name in _lib.EXT_TABLES[HEADER]:
        assert re.search(r"\b" + name + r"\b", gpu_tests), f"{name}: no GPU test names it"


def test_queries_need_no_gpu():
    L = _lib.lib()
    al = lambda v: (v + 255) // 256 * 256
    for B, N, mi, nim in ((1, 33, 100, 100), (1280, 33, 5, 5), (3, 61, 12, 7), (2, 62, 12, 7), (1, 1, 1, 1), (2, 200, 10, 30), (192, 90, 30, 100)):
        res = ((16 + 8) * N + 16) * 8 + N * (N | 1) * 40 <= 160 * 1024
        assert L.conan_fgw_pair_bwd_lds_resident(N) == int(res)
        per = (mi + 3) * N * N * 8 + (4 * nim + 2) * N * 8 + (mi + 1) // 2 * 8 + (0 if res else 5 * N * (N | 1) * 8)
        assert L.conan_fgw_pair_bwd_workspace_bytes(B, N, mi, nim) == B * al(per)
    assert L.conan_fgw_pair_bwd_lds_resident(61) == 1 and L.conan_fgw_pair_bwd_lds_resident(62) == 0
    assert 0.99e6 < L.conan_fgw_pair_bwd_workspace_bytes(1, 33, 100, 100) < 1.01e6 and 75e3 < L.conan_fgw_pair_bwd_workspace_bytes(1, 33, 5, 5) < 77e3      # the docstring's figures
    assert L.conan_fgw_pair_bwd_lds_resident(0) == 0 and L.conan_fgw_pair_bwd_lds_resident(-4) == 0
    for bad in ((0, 5, 10, 10), (-1, 5, 10, 10), (1, 0, 10, 10), (1, -3, 10, 10), (1, 5, 0, 10), (1, 5, -2, 10), (1, 5, 10, 0), (1, 5, 10, -1), (1, 5000, 10, 10)):
        assert L.conan_fgw_pair_bwd_workspace_bytes(*bad) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """Every pointer is a HOST buffer filled with 7: a launch would fault on it, a refusal leaves it as it is."""
    L = _lib.lib()
    buf = (ctypes.c_float * 256)(*([7.0] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(M=p, C1=p, C2=p, p=p, q=p, G0=p, B=1, N=4, alpha=0.5, eps=0.1, mi=10, nim=10, thr=1e-5, solver=0, sym=1, info=p, dT=p, dd=p, dM=p, dC1=p,
                dC2=p, dp=p, dq=p, dG0=p, chk=p, binfo=p, ws=p)

    def rc(**kw):
        v = dict(good, **kw)
        return L.conan_fgw_pair_bwd(v["M"], v["C1"], v["C2"], v["p"], v["q"], v["G0"], v["B"], v["N"], v["alpha"], v["eps"], v["mi"], v["nim"], v["thr"],
                                    v["solver"], v["sym"], v["info"], v["dT"], v["dd"], v["dM"], v["dC1"], v["dC2"], v["dp"], v["dq"], v["dG0"], v["chk"],
                                    v["binfo"], v["ws"], None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(M=None), dict(C1=None), dict(C2=None), dict(info=None), dict(dM=None), dict(dC1=None), dict(dC2=None), dict(ws=None),
               dict(dT=None, dd=None), dict(p=None), dict(q=None), dict(G0=None), dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(mi=0), dict(mi=-5),
               dict(nim=0), dict(nim=-1), dict(eps=0.0), dict(eps=-1.0), dict(eps=inf), dict(eps=nan), dict(alpha=nan), dict(thr=nan), dict(solver=2),
               dict(solver=-1), dict(sym=2), dict(sym=-2)):
        assert rc(**kw) == -1, kw                                          # (p / q / G0 null with dp / dq / dG0 wanted: refused too)
    assert all(v == 7.0 for v in buf)


def test_python_signatures():
    assert str(inspect.signature(ops.fgw_pair_unrolled)) == str(inspect.signature(ops.fgw_pair_batched)).replace(", with_dist: 'bool' = True", "")
    assert str(inspect.signature(fgw.fgw_unrolled)) == str(inspect.signature(fgw.fgw))
    assert str(inspect.signature(fgw.fgw_distance_unrolled)) == str(inspect.signature(fgw.fgw_distance))
    assert str(inspect.signature(fgw.fgw_pairwise_distances_unrolled)) == str(inspect.signature(fgw.fgw_pairwise_distances))
    doc = ops.fgw_pair_unrolled.__doc__
    assert "((max_iter + 3) N^2 + (4 num_iter_max + 2) N) * 8 bytes" in doc and "1.0 MB" in doc and "76 KB" in doc and 'log["err"]' in doc
    assert "fgw_unrolled" in fgw.__doc__ and "fgw_distance_unrolled" in fgw.__doc__ and "fgw_pairwise_distances_unrolled" in fgw.__doc__


def test_refusals_hold_on_cpu_tensors():
    M, C1, C2 = torch.rand(3, 4), torch.zeros(3, 3), torch.zeros(4, 4)
    for fn in (fgw.fgw_unrolled, fgw.fgw_distance_unrolled):
        with pytest.raises(NotImplementedError, match="'BAPG' is not implemented"):
            fn(M, C1, C2, solver="BAPG")
        with pytest.raises(NotImplementedError, match="'kl_loss' is not implemented"):
            fn(M, C1, C2, loss_fun="kl_loss")
        with pytest.raises(NotImplementedError, match="warmstart=True"):
            fn(M, C1, C2, warmstart=True)
        with pytest.raises(NotImplementedError, match="only method='sinkhorn_log'"):
            fn(M, C1, C2, method="sinkhorn")
        with pytest.raises(NotImplementedError, match="marginal_loss=True is not implemented"):
            fn(M, C1, C2, marginal_loss=True)
        with pytest.raises(ValueError, match="Unknown solver 'XYZ'"):
            fn(M, C1, C2, solver="XYZ")
        with pytest.raises(ValueError, match="Unknown `loss_fun='abs'`"):
            fn(M, C1, C2, loss_fun="abs")
        with pytest.raises(NotImplementedError, match=fn.__name__ + " runs on the GPU only: pass CUDA .ROCm. tensors .M is not one."):
            fn(M, C1, C2)
    for kw, exc, match in ((dict(solver="BAPG"), NotImplementedError, "'BAPG' is not implemented"), (dict(loss_fun="kl_loss"), NotImplementedError, "'kl_loss'"),
                           (dict(solver="XYZ"), ValueError, "Unknown solver"), (dict(), NotImplementedError, "runs on the GPU only: M is a CPU tensor")):
        with pytest.raises(exc, match=match):
            ops.fgw_pair_unrolled(M[None], C1[None], C2[None], **kw)
        with pytest.raises(exc, match=match if kw else "runs on the GPU only"):
            ops.fgw_pair_unrolled_list([M], [C1], [C2], **kw)
    Ys, Cs = [torch.rand(4, 2) for _ in range(3)], [torch.zeros(4, 4) for _ in range(3)]
    with pytest.raises(NotImplementedError, match="'BAPG' is not implemented"):
        fgw.fgw_pairwise_distances_unrolled(Ys, Cs, solver="BAPG")
    with pytest.raises(NotImplementedError, match="'kl_loss'"):
        fgw.fgw_pairwise_distances_unrolled(Ys, Cs, loss_fun="kl_loss")
    with pytest.raises(NotImplementedError, match="fgw_pairwise_distances_unrolled runs on the GPU only"):
        fgw.fgw_pairwise_distances_unrolled(Ys, Cs)
    with pytest.raises(NotImplementedError, match="fgw_pairwise_distances runs on the GPU only"):      # the existing name keeps its message
        fgw.fgw_pairwise_distances(Ys, Cs)
