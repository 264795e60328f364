"""CPU-side checks of the full FGW barycenter backward: the C ABI exports conan_fgw_barycenter_bwd_full and its workspace query, the ctypes
table declares them, inconsistent requests are refused without launching, and the closed-form adjoint the kernel implements, applied in
numpy fp64 to the reference's own fp64 couplings, reproduces the reference's fp64 autograd gradients (tests/golden/fgw_grad_*.npz, written
by make_fgw_grad_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import golden_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = golden_files("fgw_grad_")
ids = lambda ps: [os.path.basename(p)[9:-4] for p in ps]
ARGS = ["const float *T", "const float *Ys", "const float *Cs", "const float *Y", "const float *C", "const float *dY", "const float *dC",
        "const float *p", "const float *lambdas", "int B", "int K", "int N", "int d", "int loss_fun", "int fixed_structure",
        "int fixed_features", "float *dYs", "float *dCs", "float *dp", "float *dlambdas", "float *dinit_C", "float *dinit_Y",
        "void *workspace", "void *stream"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    return _lib


def _args(hdr, name):
    m = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{name} not declared"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_bwd_full_is_declared_and_exported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "conan_fgw_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(built.library_path())
    assert _args(hdr, "conan_fgw_barycenter_bwd_full") == ARGS
    assert _args(hdr, "conan_fgw_barycenter_bwd_full_workspace_bytes") == ["int B", "int K", "int N", "int d"]
    for name in ("conan_fgw_barycenter_bwd_full", "conan_fgw_barycenter_bwd_full_workspace_bytes"):
        assert hasattr(L, name) and name in built.SIGNATURES
    assert len(built.SIGNATURES["conan_fgw_barycenter_bwd_full"][1]) == len(ARGS)


def test_bwd_full_workspace_query(built):
    L = built.lib()
    for B, K, N, d in ((256, 5, 33, 64), (128, 5, 83, 64), (32, 5, 128, 64)):
        w = L.conan_fgw_barycenter_bwd_full_workspace_bytes(B, K, N, d)
        assert w >= B * K * 4                                   # the dlambdas partials
        if N > 112:                                             # the per-coupling H^T / A scratch of the non-LDS path
            assert w >= B * K * 4 + B * K * 2 * N * N * 4
    assert L.conan_fgw_barycenter_bwd_full_workspace_bytes(0, 5, 33, 64) == 0
    assert L.conan_fgw_barycenter_bwd_full_workspace_bytes(1, 5, 33, 0) == 0


def test_bwd_full_refuses_bad_requests_without_launching(built):
    L = built.lib()
    buf = (ctypes.c_float * 16)()
    X = ctypes.cast(buf, ctypes.c_void_p)           # a host address: none of these calls may get as far as a launch

    def call(T=X, Ys=X, Cs=X, Y=X, C=X, dY=X, dC=X, p=X, lam=X, B=2, K=3, N=5, d=4, loss=0, fs=0, ff=0,
             dYs=None, dCs=None, dp=None, dlam=None, dic=None, diy=None, ws=X):
        return L.conan_fgw_barycenter_bwd_full(T, Ys, Cs, Y, C, dY, dC, p, lam, B, K, N, d, loss, fs, ff, dYs, dCs, dp, dlam, dic, diy,
                                               ws, None)

    bad = [dict(T=None, dYs=X), dict(loss=2, dCs=X), dict(loss=-1, dYs=X), dict(B=0, dYs=X), dict(N=0, dCs=X), dict(d=-1, dp=X),
           dict(Cs=None, dCs=X),                        # dCs wanted without Cs
           dict(ff=1, dYs=X), dict(fs=1, dCs=X),        # gradients the fixed parts do not define
           dict(dic=X), dict(diy=X),                    # init gradients without fixed_structure / fixed_features
           dict(p=None, dp=X), dict(Y=None, dp=X), dict(C=None, dp=X),
           dict(Ys=None, dlam=X), dict(Cs=None, dlam=X), dict(ws=None, dlam=X),
           dict(loss=1, C=None, dCs=X), dict(N=130, ws=None, dCs=X)]
    for kw in bad:
        assert call(**kw) == -1, kw


# ---------------------------------------------------------------------------------------------- the closed-form adjoint, numpy fp64
def adjoint(g):
    """Gradients of sum(Y * gw) + sum(C * gc) through the reference's last update steps, on the recorded fp64 couplings."""
    T, Y, C = g["r64_T"], g["r64_Y"], g["r64_C"]
    K, N, n = T.shape
    Z = g["Ys"].astype(np.float64)
    C2 = g["Cs"].astype(np.float64)
    U = np.random.RandomState(int(g["gw_seed"])).normal(size=Y.shape)
    V = np.random.RandomState(int(g["gc_seed"])).normal(size=C.shape)
    p = g["p"].astype(np.float64) if "p" in g.files else np.full(N, 1.0 / N)
    lam = g["lambdas"].astype(np.float64) if "lambdas" in g.files else np.full(K, 1.0 / K)
    pinv = np.where(p > 0, 1.0 / np.where(p > 0, p, 1.0), 0.0)
    kl = str(g["loss_fun"]) == "kl_loss"
    fs, ff = bool(g["fixed_structure"]), bool(g["fixed_features"])
    out = {}
    dlam, dp = np.zeros(K), np.zeros(N)
    if ff:
        out["init_Y"] = U
    else:
        Up = pinv[:, None] * U
        out["Ys"] = np.stack([lam[s] * T[s].T @ Up for s in range(K)])
        dlam += np.array([np.sum(Up * (T[s] @ Z[s])) for s in range(K)])
        dp += -pinv * np.sum(U * Y, 1)
    if fs:
        out["init_C"] = V
    else:
        if kl:
            W = V * C
            L = np.log(np.maximum(C2, 1e-15))
            Q = np.log(np.where(C > 0, C, 1.0))
            X = np.where(W != 0, W * Q, 0.0)
        else:
            W, L, X = V, C2, V * C
        H = W * pinv[:, None] * pinv[None, :]
        G = np.stack([T[s].T @ H @ T[s] for s in range(K)])
        dC = lam[:, None, None] * G
        if kl:
            dC = np.where(C2 >= 1e-15, dC / np.where(C2 >= 1e-15, C2, 1.0), 0.0)
        out["Cs"] = dC
        dlam += np.sum(G * L, (1, 2))
        dp += -pinv * (X.sum(1) + X.sum(0))
    out["lambdas"], out["p"] = dlam, dp
    return out


@pytest.mark.parametrize("path", ALL, ids=ids(ALL))
def test_closed_form_adjoint_reproduces_the_reference_gradients(path):
    g = np.load(path)
    grads = [str(x) for x in g["grads"]]
    ours = adjoint(g)
    assert "Ys" not in grads if bool(g["fixed_features"]) else "Ys" in grads
    assert "Cs" not in grads if bool(g["fixed_structure"]) else "Cs" in grads
    for name in grads:
        ref = g["r64_d" + name]
        got = ours[name]
        if name in ("Ys", "Cs"):
            got = got[..., :ref.shape[-2], :ref.shape[-1]] if got.ndim == 3 else got
        scale = max(np.abs(ref).max(), 1e-300)
        assert np.abs(got - ref).max() <= 1e-10 * scale, (name, np.abs(got - ref).max(), scale)
