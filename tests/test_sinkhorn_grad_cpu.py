"""The unrolled Sinkhorn gradient, what needs no GPU: the fp64 restatement tests/sinkhorn_grad_ref.py reproduces the reference's autograd on
every stored fixture (tests/golden/grad_sinkhorn_*.npz, written by tests/golden/make_sinkhorn_grad_golden.py) to rel <= 1e-9 (rel = Frobenius
norm of the difference over that of the yardstick; worst measured: 8e-12, on the underflowing-row case), which pins both the restatement and
the conditioning of the chosen cases; the host-side workspace query answers; bad arguments are refused before any launch; the public functions
refuse what they do not build."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conan_fgw_amd import _lib, ops
from conan_fgw_amd import sinkhorn as sk

from sinkhorn_grad_ref import sinkhorn_grad_ref, sweeps_of
from sinkhorn_ref import fair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["1x5_log", "1x5_knopp", "7x12_log", "7x12_knopp", "33x33_log", "33x33_knopp", "64x80_log", "64x80_knopp", "zeroa_log", "warm_log",
         "warm_knopp", "9x11col_log", "9x11col_knopp", "9x11row_log"]


def load(name):
    z = np.load(os.path.join(GOLDEN, f"grad_sinkhorn_{name}.npz"))
    return {k: z[k] for k in z.files}


def rel(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


def test_fixture_list_is_complete():
    have = sorted(os.path.basename(p)[len("grad_sinkhorn_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "grad_sinkhorn_*.npz")))
    assert have == sorted(NAMES)
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, f"grad_sinkhorn_{name}.npz")) < 512 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_autograd(name):
    f = load(name)
    n1, n2 = f["M"].shape
    assert f["M"].dtype == f["a"].dtype == f["b"].dtype == f["reg"].dtype == f["dT"].dtype == np.float32
    warn, niter, it, thr = str(f["r64_warn"]), int(f["r64_niter"]), int(f["numItermax"]), float(f["stopThr"])
    assert fair(list(f["r64_err"]), niter, it, thr, warn)
    S = sweeps_of(niter, warn == "numerr")
    assert ("warm_u" in f) == name.startswith("warm_")
    warm = (f["warm_u"], f["warm_v"]) if "warm_u" in f else None
    if name == "7x12_log":
        assert S == it                                                     # runs out its sweeps
    if name == "9x11col_knopp":
        assert S == 0 and not f["g1_da"].any() and not f["g2_db"].any()
    if name == "zeroa_log":
        assert f["a"][3] == 0 and bool(f["ref_nan_at_zero_weight"]) and f["g1_da"][3] == 0 and f["g2_da"][3] == 0
    for tag, dT in (("g1", None), ("g2", f["dT"])):
        r = sinkhorn_grad_ref(f["a"], f["b"], f["M"], float(f["reg"]), S, str(f["method"]), warm, 1.0, dT)
        assert rel(r["T"], f["r64_T"]) <= 1e-12
        keys = ["dM"] + (["da", "db"] if S > 0 else []) + (["dwu"] if warm is not None else [])
        for k in keys:
            e = rel(r[k], f[f"{tag}_{k}"])
            print(f"{name} {tag} {k}: rel {e:.2e}")
            assert e <= 1e-9, (name, tag, k, e)
        if S == 0:                                                         # the plan is u0 K v0: dM = gl T - (Tb o T) / reg, nothing to a, b
            assert not r["da"].any() and not r["db"].any()
            Tb = f["M"].astype(np.float64) + (0.0 if dT is None else dT)
            assert rel(r["dM"], r["T"] - Tb * r["T"] / float(f["reg"])) <= 1e-14
        if name == "zeroa_log":
            assert r["da"][3] == 0.0 and np.isfinite(r["dM"]).all() and not r["T"][3].any()
    if name == "9x11row_log":
        assert np.abs(f["g1_da"]).max() > 50                               # the exact-path case is badly scaled and still finite
    if n1 > 1 and S > 0:                                                   # (one row: the plan is b whatever M is, and dM = T exactly)
        assert rel(f["r64_T"], f["g1_dM"]) > 0.1                           # the fixed-plan gradient is a different quantity


def test_signatures_and_workspace_query():
    for name in ("conan_sinkhorn_bwd_workspace_bytes", "conan_sinkhorn_bwd_lds_resident", "conan_sinkhorn_bwd"):
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.conan_abi_version() == 6
    al = lambda v: (v + 255) // 256 * 256
    for B, n1, n2, it in ((1, 33, 33, 1000), (7, 33, 33, 100), (3, 64, 80, 100), (2, 200, 300, 10), (1, 1, 5, 1)):
        res = (16 + 5 * n1 + 5 * n2 + n1 * (n2 | 1)) * 8 + 16384 <= 160 * 1024
        assert L.conan_sinkhorn_bwd_lds_resident(n1, n2) == int(res)
        assert L.conan_sinkhorn_bwd_workspace_bytes(B, n1, n2, it) == B * al(((2 * it + 1) * (n1 + n2) + (0 if res else n1 * (n2 | 1))) * 8)
    assert 1.0e6 < L.conan_sinkhorn_bwd_workspace_bytes(1, 33, 33, 1000) < 1.1e6      # "about 1 MB per 33 x 33 problem at numItermax = 1000"
    assert L.conan_sinkhorn_bwd_lds_resident(130, 130) == 1 and L.conan_sinkhorn_bwd_lds_resident(131, 131) == 0
    assert L.conan_sinkhorn_bwd_lds_resident(0, 5) == 0 and L.conan_sinkhorn_bwd_lds_resident(5, -1) == 0
    for bad in ((0, 5, 5, 10), (-1, 5, 5, 10), (1, 0, 5, 10), (1, 5, 0, 10), (1, 5, 5, 0), (1, 5, 5, -2), (1, 5000, 5000, 10)):
        assert L.conan_sinkhorn_bwd_workspace_bytes(*bad) == 0


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(M=p, B=1, N1=4, N2=4, stride=16, reg=0.1, method=0, it=10, info=p, gl=p, gT=p, dM=p, ws=p)

    def rc(**kw):
        a = dict(good, **kw)
        return L.conan_sinkhorn_bwd(a["M"], None, None, None, None, None, None, a["B"], a["N1"], a["N2"], a["stride"], a["reg"], a["method"], a["it"],
                                    a["info"], a["gl"], a["gT"], a["dM"], None, None, None, a["ws"], None)

    for kw in (dict(M=None), dict(info=None), dict(dM=None), dict(ws=None), dict(gl=None, gT=None), dict(B=0), dict(N1=0), dict(N2=-3), dict(it=0),
               dict(reg=0.0), dict(reg=-1.0), dict(reg=float("inf")), dict(reg=float("nan")), dict(method=2), dict(method=-1), dict(stride=-1)):
        assert rc(**kw) == -1, kw


def test_public_refusals_touch_no_tensor():
    a, b, M = torch.ones(3) / 3, torch.ones(4) / 4, torch.rand(3, 4)
    for fn in (sk.sinkhorn, sk.sinkhorn2, sk.sinkhorn_log, sk.sinkhorn_knopp):
        with pytest.raises(ValueError, match="grad must be"):
            fn(a, b, M, 0.1, grad="bogus")
        with pytest.raises(NotImplementedError, match="GPU only"):
            fn(a, b, M, 0.1, grad="unrolled")
    with pytest.raises(ValueError, match="grad must be"):
        sk.wasserstein_pairwise_distances([M, M], grad="bogus")
    with pytest.raises(NotImplementedError, match="GPU only"):
        sk.wasserstein_pairwise_distances([M, M], grad="unrolled")
    for m in ("greenkhorn", "sinkhorn_stabilized", "sinkhorn_epsilon_scaling"):
        with pytest.raises(NotImplementedError, match="grad='unrolled' is not implemented"):
            sk.sinkhorn(a, b, M, 0.1, method=m, grad="unrolled")
        with pytest.raises(ValueError, match="grad must be"):
            sk.sinkhorn(a, b, M, 0.1, method=m, grad="bogus")
    with pytest.raises(NotImplementedError, match="grad='unrolled' is not implemented"):
        sk.sinkhorn2(a, b, M, 0.1, method="sinkhorn_stabilized", grad="unrolled")
    for fn in (sk.sinkhorn_stabilized, sk.sinkhorn_epsilon_scaling):     # (greenkhorn takes no **kwargs, in the reference or here)
        with pytest.raises(NotImplementedError, match="grad='unrolled' is not implemented"):
            fn(a, b, M, 0.1, grad="unrolled")
        with pytest.raises(ValueError, match="grad must be"):
            fn(a, b, M, 0.1, grad="bogus")
    with pytest.raises(ValueError, match="grad must be"):
        ops.sinkhorn_loss(M[None], reg=0.1, grad="bogus")
    for fn in (ops.sinkhorn_unrolled, lambda *x, **k: ops.sinkhorn_loss(*x, grad="unrolled", **k)):
        with pytest.raises(NotImplementedError, match="runs on the GPU only"):
            fn(M[None], reg=0.1)
    with pytest.raises(NotImplementedError, match="runs on the GPU only"):
        ops.sinkhorn_unrolled_list([M], reg=0.1)
