"""The unrolled FGWMixup gradient, what needs no GPU: the fp64 restatement tests/fgw_acc_grad_ref.py reproduces torch autograd through the
reference's own fused_ACC_torch on every stored fixture (tests/golden/grad_acc_*.npz, written by tests/golden/make_fgw_acc_grad_golden.py) to
1e-9 (fgw_acc_grad_ref.grad_error: the Frobenius norm of the difference over that of the yardstick; worst measured: 2.2e-11, on 5x7), which
pins both the restatement and the conditioning of the chosen cases; a central finite difference of the restatement's own forward; the second
header / table / library triple agrees; the host-side queries answer; bad arguments are refused before any launch; the public functions have
their signatures and refuse CPU tensors."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, fgw, ops

from fgw_acc_grad_ref import F64, acc_distance, acc_forward, acc_grad_ref, grad_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXT_HEADER = os.path.join(ROOT, "include", "conan_fgw_hip_ext.h")
NAMES = ["1x5", "5x7", "5x7_stop", "12x9_directed", "7x7_start", "9x11_zeroa", "33x33", "62x62"]
EXPORTS = ("conan_fgw_acc_pair_bwd_lds_resident", "conan_fgw_acc_pair_bwd_workspace_bytes", "conan_fgw_acc_pair_bwd")


def load(name):
    z = np.load(os.path.join(GOLDEN, f"grad_acc_{name}.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_list_is_complete():
    have = sorted(os.path.basename(p)[len("grad_acc_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "grad_acc_*.npz")))
    assert have == sorted(NAMES)
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, f"grad_acc_{name}.npz")) < 512 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_autograd(name):
    f = load(name)
    n1, n2 = f["M"].shape
    assert f["M"].dtype == f["W"].dtype == np.float32 and all(f[k].dtype == np.float32 for k in ("a", "b", "X0") if k in f)
    epochs, epoch, stored = int(f["epochs"]), int(f["epoch"]), int(f["stored"])
    assert np.isfinite(f["X"]).all() and 1 <= epochs <= epoch
    assert stored == len([ii for ii in range(epochs) if ii > 0 and ii % 10 == 0]) - (1 if epochs < epoch else 0)      # the stopping check is not stored
    if name == "5x7":
        assert (n1, n2) == (5, 7) and epochs == epoch == 25
    if name == "5x7_stop":
        assert float(f["rho"]) == 0.1 and epoch == 200 and 21 <= epochs < 200 and epochs % 10 == 1
    if name == "12x9_directed":
        assert (f["A"] != f["A"].T).any() and (f["B"] != f["B"].T).any()
    if name == "62x62":
        L = _lib.lib()
        assert L.conan_fgw_acc_pair_bwd_lds_resident(n1 - 1) == 1 and L.conan_fgw_acc_pair_bwd_lds_resident(n1) == 0      # just above the bound
    assert ("X0" in f) == (name == "7x7_start")
    if name == "9x11_zeroa":
        assert f["a"][3] == 0 and (f["a"] > 0).sum() == n1 - 1 and abs(f["ref_da_at_zero_weight"]).min() > 0.1      # the reference's da there is no rounding
        assert float(f["ref_max_abs_zeroed"]) < 1e-8
    for tag, kw, cot in (("gX", dict(dX=f["W"]), f["W"]), ("gd", dict(ddist=1.0), 1.0)):
        r = acc_grad_ref(f["M"], f["A"], f["B"], f.get("a"), f.get("b"), f.get("X0"), alpha=float(f["alpha"]), rho=float(f["rho"]), epochs=epochs, **kw)
        assert grad_error(r["X"], f["X"]) <= 1e-12
        assert abs(r["dist"] - float(f["dist"])) <= 1e-12 * abs(float(f["dist"]))
        for k, kf in (("dM", "dM"), ("dA", "dA"), ("dBm", "dB"), ("da", "da"), ("db", "db")) + ((("dX0", "dX0"),) if "X0" in f else ()):
            e = grad_error(r[k], f[f"{tag}_{kf}"], cot)
            print(f"{name} {tag} {k}: {e:.2e}")
            assert e <= 1e-9, (name, tag, k, e)
        if name == "9x11_zeroa":                                           # the massless rule: exact zeros, no division by the zero weight
            assert r["da"][3] == 0 and not r["dM"][3].any() and not r["dA"][3].any() and not r["dA"][:, 3].any() and not r["X"][3].any()
            assert all(np.isfinite(r[k]).all() for k in ("dM", "dA", "dBm", "da", "db"))
    if name == "5x7_stop":                                                 # the fixed-plan gradient (1 - alpha) X is a different quantity: 0.48 away
        assert grad_error((1 - float(f["alpha"])) * f["X"], f["gd_dM"]) > 1e-3      # (5x7 at rho 0.5 ends in a vertex that does not move: 4e-6)


def test_restatement_against_a_central_finite_difference():
    """L = sum(W * X) + 0.7 dist on a 4 x 5 pair with a start, directed graphs and given weights, 7 epochs held fixed: <gradient, V> against
    (L(x + h V) - L(x - h V)) / 2h for a random direction V of every input.  h = 1e-6.  The error of a difference quotient is ABSOLUTE: the
    rounding term eps |L| / h = 2.2e-10 |L|, and the truncation term h^2 L''' / 6, 1e-12 times third derivatives of order (4 alpha / rho)^3 =
    64.  Bound: 10 eps |L| / h (about 2e-9 here), with every directional derivative required above 1e-4, five orders more than the bound: a
    missing or mis-signed term of the walk cannot hide under it."""
    g = np.random.default_rng(11)
    n1, n2, alpha, rho, epochs, gd = 4, 5, 0.5, 0.5, 7, 0.7
    x, y = g.uniform(0.1, 1.5, (n1, 3)), g.uniform(0.1, 1.5, (n2, 3))
    ins = dict(M=((x[:, None] - y[None]) ** 2).sum(-1), A=(g.random((n1, n1)) < 0.5).astype(np.float64) + 0.1 * g.random((n1, n1)),
               Bm=(g.random((n2, n2)) < 0.5).astype(np.float64) + 0.1 * g.random((n2, n2)), a=g.uniform(0.5, 1.5, n1), b=g.uniform(0.5, 1.5, n2))
    ins["a"] /= ins["a"].sum(); ins["b"] /= ins["b"].sum()
    ins["X0"] = np.outer(ins["a"], ins["b"]) * g.uniform(0.5, 1.5, (n1, n2))
    W = g.standard_normal((n1, n2))

    def loss(v):
        t = {k: torch.from_numpy(np.ascontiguousarray(u)).to(F64) for k, u in v.items()}
        X = acc_forward(t["M"], t["A"], t["Bm"], t["a"], t["b"], t["X0"], alpha, rho, epochs)
        return float((torch.from_numpy(W) * X).sum() + gd * acc_distance(t["M"], t["A"], t["Bm"], t["a"], t["b"], X, alpha))

    r = acc_grad_ref(ins["M"], ins["A"], ins["Bm"], ins["a"], ins["b"], ins["X0"], alpha=alpha, rho=rho, epochs=epochs, dX=W, ddist=gd)
    h = 1e-6
    for k, gk in (("M", "dM"), ("A", "dA"), ("Bm", "dBm"), ("a", "da"), ("b", "db"), ("X0", "dX0")):
        V = g.standard_normal(ins[k].shape) * np.abs(ins[k]).mean()
        fd = (loss(dict(ins, **{k: ins[k] + h * V})) - loss(dict(ins, **{k: ins[k] - h * V}))) / (2 * h)
        an = float((r[gk] * V).sum())
        print(f"{k}: analytic {an:+.9e} finite difference {fd:+.9e}")
        assert abs(an) > 1e-4 and abs(fd - an) <= 10 * np.finfo(np.float64).eps * abs(loss(ins)) / h, (k, an, fd)


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(EXT_HEADER).read(), flags=re.S)
    return {m.group(2): len(m.group(3).split(",")) for m in re.finditer(r"\b(int|long long)\s+(conan_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_second_header_table_and_library_agree():
    d = _declared()
    assert set(d) == set(_lib.EXT_SIGNATURES) == set(EXPORTS)
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    raw = ctypes.CDLL(_lib.library_path())
    first = open(os.path.join(ROOT, "include", "conan_fgw_hip.h")).read()
    for name, (_res, args) in _lib.EXT_SIGNATURES.items():
        assert len(args) == d[name], name
        assert hasattr(raw, name), f"{name} declared in the second header but not exported"
        assert not re.search(r"\b" + name + r"\b", first), f"{name} belongs to the second header only"
    assert _lib.lib().conan_abi_version() == _lib.ABI_VERSION == 6          # an added export does not change the version
    I, LL, P, D = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_double
    assert _lib.EXT_SIGNATURES["conan_fgw_acc_pair_bwd"] == (I, [P] * 6 + [I, I, D, D, I] + [P] * 12)
    assert _lib.EXT_SIGNATURES["conan_fgw_acc_pair_bwd_workspace_bytes"] == (LL, [I, I, I])
    assert _lib.EXT_SIGNATURES["conan_fgw_acc_pair_bwd_lds_resident"] == (I, [I])


def test_every_second_table_entry_is_named_by_a_test_file():
    gpu_tests = open(os.path.join(ROOT, "tests", "test_gpu_fgw_acc_grad.py")).read()
    for name in _lib.EXT_SIGNATURES:
        assert re.search(r"\b" + name + r"\b", gpu_tests), f"{name}: no GPU test names it"


def test_queries_need_no_gpu():
    L = _lib.lib()
    al = lambda v: (v + 255) // 256 * 256
    for B, N, epoch in ((1, 33, 200), (7, 33, 100), (3, 61, 12), (2, 62, 12), (1, 1, 1), (2, 200, 10)):
        res = ((8 + 8) * N + 16) * 8 + N * (N | 1) * 40 <= 160 * 1024
        assert L.conan_fgw_acc_pair_bwd_lds_resident(N) == int(res)
        assert L.conan_fgw_acc_pair_bwd_workspace_bytes(B, N, epoch) == B * al((2 * epoch + 3) * N * N * 8 + (0 if res else 5 * N * (N | 1) * 8))
    assert L.conan_fgw_acc_pair_bwd_lds_resident(61) == 1 and L.conan_fgw_acc_pair_bwd_lds_resident(62) == 0      # below the forward's 79
    assert L.conan_fgw_acc_lds_resident(79) == 1 and L.conan_fgw_acc_lds_resident(80) == 0
    record = 2 * 200 * 33 * 33 * 8
    assert 3.4e6 < record < 3.5e6 and record <= L.conan_fgw_acc_pair_bwd_workspace_bytes(1, 33, 200) < 1.01 * record      # "3.5 MB per 33 x 33 pair"
    assert L.conan_fgw_acc_pair_bwd_lds_resident(0) == 0 and L.conan_fgw_acc_pair_bwd_lds_resident(-4) == 0
    for bad in ((0, 5, 10), (-1, 5, 10), (1, 0, 10), (1, -3, 10), (1, 5, 0), (1, 5, -2), (1, 5000, 10)):
        assert L.conan_fgw_acc_pair_bwd_workspace_bytes(*bad) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """Every pointer is a HOST buffer filled with 7: a launch would fault on it, a refusal leaves it as it is."""
    L = _lib.lib()
    buf = (ctypes.c_float * 256)(*([7.0] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(M=p, A=p, Bm=p, a=p, b=p, X0=p, B=1, N=4, alpha=0.5, rho=0.5, epoch=10, info=p, dX=p, dd=p, dM=p, dA=p, dBm=p, da=p, db=p, dX0=p, chk=p, ws=p)

    def rc(**kw):
        v = dict(good, **kw)
        return L.conan_fgw_acc_pair_bwd(v["M"], v["A"], v["Bm"], v["a"], v["b"], v["X0"], v["B"], v["N"], v["alpha"], v["rho"], v["epoch"], v["info"],
                                        v["dX"], v["dd"], v["dM"], v["dA"], v["dBm"], v["da"], v["db"], v["dX0"], v["chk"], v["ws"], None)

    for kw in (dict(M=None), dict(A=None), dict(Bm=None), dict(info=None), dict(dM=None), dict(dA=None), dict(dBm=None), dict(ws=None),
               dict(dX=None, dd=None), dict(a=None), dict(b=None), dict(X0=None), dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(epoch=0),
               dict(epoch=-5), dict(rho=0.0), dict(rho=-1.0), dict(rho=float("inf")), dict(rho=float("nan")), dict(alpha=float("nan"))):
        assert rc(**kw) == -1, kw                                          # (a / b / X0 null with da / db / dX0 wanted: refused too)
    assert all(v == 7.0 for v in buf)


def test_python_signatures():
    assert str(inspect.signature(ops.fgw_acc_pair_unrolled)) == (
        "(M: 'Tensor', A: 'Tensor', Bm: 'Tensor', a: 'Optional[Tensor]' = None, b: 'Optional[Tensor]' = None, X0: 'Optional[Tensor]' = None, *, "
        "alpha: 'float', rho: 'float', epoch: 'int' = 200, eps: 'float' = 1e-05, n1: 'Optional[Tensor]' = None, n2: 'Optional[Tensor]' = None)")
    assert str(inspect.signature(fgw.fused_ACC_unrolled)) == str(inspect.signature(fgw.fused_ACC_torch)) == \
        "(M, A, B, a=None, b=None, X=None, alpha=0, epoch=200, eps=1e-05, rho=0.1)"
    assert str(inspect.signature(fgw.fgw_mixup_distance_unrolled)) == str(inspect.signature(fgw.fgw_mixup_distance)) == \
        "(M, A, B, a=None, b=None, X=None, alpha=0, epoch=200, eps=1e-05, rho=0.1, log=False)"
    doc = ops.fgw_acc_pair_unrolled.__doc__
    assert "2 epoch * N^2 * 8 bytes" in doc and "3.5 MB" in doc and "obj_list" in doc           # the record's size and the deviation are stated
    assert "fgw_acc_pair_unrolled" in ops.fgw_acc_pair_distance.__doc__ and "fused_ACC_unrolled" in fgw.fused_ACC_torch.__doc__
    assert "fgw_mixup_distance_unrolled" in fgw.fgw_mixup_distance.__doc__ and "fused_ACC_unrolled" in fgw.__doc__


def test_cpu_tensors_are_refused():
    M, A, B = torch.rand(3, 4), torch.zeros(3, 3), torch.zeros(4, 4)
    with pytest.raises(NotImplementedError, match="fused_ACC_unrolled runs on the GPU only: pass CUDA .ROCm. tensors .M is not one."):
        fgw.fused_ACC_unrolled(M, A, B, alpha=0.5)
    with pytest.raises(NotImplementedError, match="fgw_mixup_distance_unrolled runs on the GPU only: pass CUDA .ROCm. tensors .M is not one."):
        fgw.fgw_mixup_distance_unrolled(M, A, B, alpha=0.5, log=True)
    with pytest.raises(NotImplementedError, match="the FGWMixup solve runs on the GPU only: M is a CPU tensor"):
        ops.fgw_acc_pair_unrolled(M[None], A[None], B[None], alpha=0.5, rho=0.5)
    with pytest.raises(ValueError, match="rho must be positive"):
        ops.fgw_acc_pair_unrolled(M[None], A[None], B[None], alpha=0.5, rho=0.0)
