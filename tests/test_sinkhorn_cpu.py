"""Entropic OT on its own, what needs no GPU: the stored fixtures of the reference's sinkhorn.py (tests/golden/sinkhorn_*.npz, written by
tests/golden/make_sinkhorn_golden.py) are complete and self-consistent, the fp64 restatement tests/sinkhorn_ref.py reproduces every one of them,
the three C entry points are declared and their host-side queries answer, and the public functions refuse what they do not build."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib
from conan_fgw_amd import sinkhorn as sk

from sinkhorn_ref import fair, sinkhorn_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["1x5", "7x12", "33x33", "64x80", "257x65", "140x140", "9x11col", "zeroa", "warm", "65x257"]
NAMES = [f"{c}_{m}" for c in CASES for m in ("log", "knopp")]


def load(name):
    z = np.load(os.path.join(GOLDEN, f"sinkhorn_{name}.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_list_is_complete():
    have = sorted(os.path.basename(p)[len("sinkhorn_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "sinkhorn_*.npz")))
    assert have == sorted(NAMES)
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, f"sinkhorn_{name}.npz")) < 512 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_self_consistent(name):
    f = load(name)
    n1, n2 = f["M"].shape
    assert f["M"].dtype == f["a"].dtype == f["b"].dtype == f["r32_T"].dtype == np.float32 and f["reg"].dtype == np.float32
    assert f["a"].shape == (n1,) and f["b"].shape == (n2,) and f["r32_T"].shape == f["r64_T"].shape == (n1, n2)
    assert f["r64_T"].dtype == f["r64_err"].dtype == f["r64_log_u"].dtype == f["r64_log_v"].dtype == np.float64
    assert f["r64_log_u"].shape == (n1,) and f["r64_log_v"].shape == (n2,)
    assert str(f["method"]) == ("sinkhorn_log" if name.endswith("_log") else "sinkhorn")
    thr, it, niter, warn, err = float(f["stopThr"]), int(f["numItermax"]), int(f["r64_niter"]), str(f["r64_warn"]), f["r64_err"]
    assert ("warm_u" in f) == name.startswith("warm_")
    if warn == "numerr":
        assert name == "9x11col_knopp" and niter == 0 and len(err) == 0 and int(f["r32_niter"]) == 0
        np.testing.assert_allclose(f["r64_T"], np.exp(f["M"].astype(np.float64) / -float(f["reg"])) / (n1 * n2), rtol=1e-12)
    else:
        assert len(err) == niter // 10 + 1
        # (the fp32 run of Knopp may leave on numerical errors where fp64 does not: fp32 exp underflows earlier; it then holds the checks before that)
        assert len(f["r32_err"]) == int(f["r32_niter"]) // 10 + 1 or (name.endswith("_knopp") and len(f["r32_err"]) == (int(f["r32_niter"]) + 9) // 10)
        assert fair(list(err), niter, it, thr)
        assert (warn == "noconv") == (err[-1] >= thr) and (warn == "noconv") == (name.startswith("7x12"))
        if err[-1] < thr:
            assert np.linalg.norm(f["r64_T"].sum(0) - f["b"]) < thr
        if name.endswith("_log"):
            np.testing.assert_allclose(f["r64_T"].sum(1), f["a"].astype(np.float64), rtol=0, atol=1e-9)
    assert not np.isnan(f["r64_T"]).any()
    assert abs(float(f["r64_loss"]) - float((f["M"].astype(np.float64) * f["r64_T"]).sum())) <= 1e-12 * abs(float(f["r64_loss"]))
    if name.startswith("zeroa"):
        assert f["a"][3] == 0 and not f["r64_T"][3].any()
    if name.startswith("65x257"):
        np.testing.assert_array_equal(f["M"], load("257x65_" + name.split("_")[1])["M"].T)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_fp64_run(name):
    f = load(name)
    warm = (f["warm_u"], f["warm_v"]) if "warm_u" in f else None
    T, log = sinkhorn_ref(f["a"], f["b"], f["M"], float(f["reg"]), str(f["method"]), int(f["numItermax"]), float(f["stopThr"]), warm)
    assert log["niter"] == int(f["r64_niter"]) and log["warn"] == str(f["r64_warn"])
    # err = || colsum - b ||: every column sum adds n1 positive fp64 terms, in an order that depends on the machine (BLAS kernels, threads), so two
    # correct fp64 evaluations differ by up to n1 eps colsum_j per column, n1 eps ||b|| in the norm.  That floor only shows in the cases that
    # converge to 1e-11 (measured across two machines: 2e-18 .. 8e-18 absolute there, 1e-7 of the value); everywhere else rtol 1e-9 decides.
    floor = f["M"].shape[0] * np.finfo(np.float64).eps * float(np.linalg.norm(f["b"].astype(np.float64)))
    np.testing.assert_allclose(np.array(log["err"]), f["r64_err"], rtol=1e-9, atol=floor)
    ref = f["r64_T"]
    assert np.linalg.norm(T.numpy() - ref) <= 1e-12 * np.linalg.norm(ref)
    assert abs(log["loss"] - float(f["r64_loss"])) <= 1e-12 * abs(float(f["r64_loss"]))


def test_signatures_and_host_queries():
    for name in ("conan_sinkhorn_workspace_bytes", "conan_sinkhorn_lds_resident", "conan_sinkhorn_fwd"):
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.conan_abi_version() == 6
    assert L.conan_sinkhorn_lds_resident(33, 33) == 1 and L.conan_sinkhorn_lds_resident(257, 65) == 1
    assert L.conan_sinkhorn_lds_resident(140, 140) == 0 and L.conan_sinkhorn_lds_resident(1000, 1000) == 0
    assert L.conan_sinkhorn_lds_resident(0, 5) == 0 and L.conan_sinkhorn_lds_resident(5, -1) == 0
    # the documented limit: (16 + 3 n1 + 4 n2 + n1 (n2 | 1)) * 8 bytes <= 160 KiB
    for n1, n2 in ((140, 139), (140, 140), (64, 300), (64, 305), (7, 2800)):
        assert L.conan_sinkhorn_lds_resident(n1, n2) == int((16 + 3 * n1 + 4 * n2 + n1 * (n2 | 1)) * 8 <= 160 * 1024)
    for shape in ((33, 33), (200, 300)):
        w = [L.conan_sinkhorn_workspace_bytes(B, *shape) for B in (1, 2, 7, 64)]
        assert all(x > 0 for x in w) and all(x <= y for x, y in zip(w, w[1:]))
    w = [L.conan_sinkhorn_workspace_bytes(B, 200, 300) for B in (1, 2, 7)]
    assert w[0] >= 200 * 301 * 8 and w[0] < w[1] < w[2]                   # streamed: a copy of the matrix per problem
    for bad in ((0, 5, 5), (-1, 5, 5), (1, 0, 5), (1, 5, 0)):
        assert L.conan_sinkhorn_workspace_bytes(*bad) == 0


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(M=p, B=1, N1=4, N2=4, stride=16, reg=0.1, method=0, it=10, T=p, ws=p)

    def rc(**kw):
        a = dict(good, **kw)
        return L.conan_sinkhorn_fwd(a["M"], None, None, None, None, None, None, a["B"], a["N1"], a["N2"], a["stride"], a["reg"], a["method"], a["it"],
                                    1e-5, a["T"], None, None, None, None, None, a["ws"], None)

    for kw in (dict(M=None), dict(T=None), dict(ws=None), dict(B=0), dict(N1=0), dict(N2=-3), dict(it=0), dict(reg=0.0), dict(reg=-1.0),
               dict(reg=float("inf")), dict(reg=float("nan")), dict(method=2), dict(method=-1), dict(stride=-1)):
        assert rc(**kw) == -1, kw


def test_public_refusals_touch_no_tensor():
    a, b, M = torch.ones(3) / 3, torch.ones(4) / 4, torch.rand(3, 4)
    for fn in (sk.sinkhorn, sk.sinkhorn2):
        with pytest.raises(ValueError, match="Unknown method 'nope'"):
            fn(a, b, M, 0.1, method="nope")
    with pytest.raises(ValueError, match="Unknown method"):
        sk.wasserstein_pairwise_distances([M, M], method="nope")
    for m in ("greenkhorn", "sinkhorn_stabilized", "sinkhorn_epsilon_scaling", "Sinkhorn_Stabilized"):
        with pytest.raises(NotImplementedError, match="not implemented"):
            sk.sinkhorn(a, b, M, 0.1, method=m)
    with pytest.raises(NotImplementedError, match="not implemented"):
        sk.sinkhorn2(a, b, M, 0.1, method="sinkhorn_stabilized")
    with pytest.raises(ValueError, match="Unknown method"):               # as the reference's sinkhorn2
        sk.sinkhorn2(a, b, M, 0.1, method="greenkhorn")
    for fn in (sk.sinkhorn, sk.sinkhorn2, sk.sinkhorn_log, sk.sinkhorn_knopp):
        with pytest.raises(NotImplementedError, match="several histograms"):
            fn(a, torch.ones(4, 2) / 4, M, 0.1)
        with pytest.raises(NotImplementedError, match="GPU only"):
            fn(a, b, M, 0.1)
    with pytest.raises(NotImplementedError, match="GPU only"):
        sk.wasserstein_pairwise_distances([M, M])
    from conan_fgw_amd import ops
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.sinkhorn_batched(M[None], reg=0.1)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.sinkhorn_loss(M[None], reg=0.1)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.sinkhorn_list([M], reg=0.1)
    with pytest.raises(ValueError, match="Unknown method"):
        ops.sinkhorn_batched(M[None], reg=0.1, method="greenkhorn")
