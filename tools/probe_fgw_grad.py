"""Timing of the full FGW barycenter backward (conan_fgw_barycenter_bwd_full: dYs, dCs, dp and dlambdas, square loss) against the same
gradients formed with torch.matmul in fp32, at the cfg2 shape (B=256, K=5, N=33, d=64), the cfg3 shape (B=128, K=5, N=83) and
B=32, K=5, N=128 (the non-LDS path).  HIP events around each launch, warm-up, then the median of 200.  The floors printed next to the
numbers are derived from the shape, not measured: fp32 MFMA at 155 TF for the two N^3 products plus the N^2 d feature product, and HBM at
5.3 TB/s for T, Cs and dCs (the rest is smaller).

    python tools/probe_fgw_grad.py [--iters 200]
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd._lib import call, lib, ptr, stream_ptr  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = [("cfg2", 256, 5, 33, 64), ("cfg3", 128, 5, 83, 64), ("non-LDS", 32, 5, 128, 64)]


def median_us(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ts.append((a, b))
    torch.cuda.synchronize()
    v = sorted(a.elapsed_time(b) * 1e3 for a, b in ts)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    torch.manual_seed(0)
    for name, B, K, N, d in SHAPES:
        T = torch.rand(B, K, N, N, device=dev) / (N * N)
        Ys, Cs = torch.rand(B, K, N, d, device=dev), (torch.rand(B, K, N, N, device=dev) < 0.3).float()
        Y, C = torch.rand(B, N, d, device=dev), torch.rand(B, N, N, device=dev)
        dY, dC = torch.randn(B, N, d, device=dev), torch.randn(B, N, N, device=dev)
        p = torch.full((B, N), 1.0 / N, device=dev)
        lam = torch.full((K,), 1.0 / K, device=dev)
        dYs, dCs, dp, dlam = torch.empty_like(Ys), torch.empty_like(Cs), torch.empty_like(p), torch.empty_like(lam)
        ws = torch.empty(int(lib().conan_fgw_barycenter_bwd_full_workspace_bytes(B, K, N, d)), dtype=torch.uint8, device=dev)

        def ours():
            call("conan_fgw_barycenter_bwd_full", ptr(T), ptr(Ys), ptr(Cs), ptr(Y), ptr(C), ptr(dY), ptr(dC), ptr(p), ptr(lam), B, K, N, d,
                 0, 0, 0, ptr(dYs), ptr(dCs), ptr(dp), ptr(dlam), None, None, ptr(ws), stream_ptr())

        def torch_form():
            pinv = 1.0 / p
            Up = pinv[:, :, None] * dY
            a = torch.matmul(T.transpose(-1, -2), Up[:, None])                      # [B,K,N,d]
            H = dC * pinv[:, :, None] * pinv[:, None, :]
            G = torch.matmul(T.transpose(-1, -2), torch.matmul(H[:, None], T))    # [B,K,N,N]
            out_dYs = lam[None, :, None, None] * a
            out_dCs = lam[None, :, None, None] * G
            out_dlam = (a * Ys).sum((0, 2, 3)) + (G * Cs).sum((0, 2, 3))
            X = dC * C
            out_dp = -pinv * ((dY * Y).sum(2) + X.sum(2) + X.sum(1))
            return out_dYs, out_dCs, out_dp, out_dlam

        ours(); torch.cuda.synchronize()
        ref = torch_form()
        err = max(float(((o - r).norm() / r.norm()).item()) for o, r in zip((dYs, dCs, dp, dlam), ref))
        t_ours, t_torch = median_us(ours, args.iters), median_us(torch_form, args.iters)
        flop = B * K * (4.0 * N ** 3 + 2.0 * N * N * d)
        byts = B * K * N * N * 4 * 3
        print(f"{name}: B={B} K={K} N={N} d={d}  bwd_full {t_ours:8.1f} us   torch fp32 {t_torch:8.1f} us   "
              f"floors: MFMA {flop / 155e12 * 1e6:5.1f} us ({flop / 1e9:.2f} GFLOP)  HBM {byts / 5.3e12 * 1e6:5.1f} us ({byts / 1e6:.0f} MB)  "
              f"max rel diff {err:.1e}")


if __name__ == "__main__":
    main()
