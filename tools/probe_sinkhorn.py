"""What does the batched Sinkhorn kernel cost next to the same iteration written with batched torch ops?

    python tools/probe_sinkhorn.py [--runs 25] [--warmup 5] [--repeats 3] [--out profiles/sinkhorn_probe.txt]

Two shapes, the coupling counts and sizes of the cfg2 and cfg3 batches: B = 1280 problems of 33 x 33 and B = 640 of 83 x 83, with reg 0.1,
stopThr 1e-5, numItermax 100, both methods.  Costs are squared distances of Gaussian clouds over their maximum, marginals random, normalised
(the construction of the stored fixtures).  Per shape and method, HIP events around the call after warm-up, the median of --runs calls, --repeats
times in one process with the two sides interleaved (all repeats are printed; the row's figure is their median):

    kernel_ms   ops.sinkhorn_batched (fp64 inside, every problem stops on its own check)
    torch_ms    the reference's arithmetic on the same GPU: the same iteration as batched fp32 torch ops, the whole batch iterated until every
                problem has passed its check (the count a loop over the reference's function would need for its slowest problem), with one host
                synchronisation per check as in the reference

The iteration counts of both sides are printed beside the times, and the plans are compared (relative Frobenius error), so that the timings are
known to be of the same quantity.  No ratio is promised: the figures are stated."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd import ops  # noqa: E402

REG, THR, ITMAX = 0.1, 1e-5, 100


def problems(B, n, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x, y = torch.randn(B, n, 3, generator=g), torch.randn(B, n, 3, generator=g) + 0.5
    M = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    M = M / M.amax(dim=(1, 2), keepdim=True)
    a, b = torch.rand(B, n, generator=g) + 0.1, torch.rand(B, n, generator=g) + 0.1
    return M.to(dev), (a / a.sum(1, keepdim=True)).to(dev), (b / b.sum(1, keepdim=True)).to(dev)


def torch_log(M, a, b):
    Mr = -M / REG
    u, v = torch.zeros_like(a), torch.zeros_like(b)
    la, lb = torch.log(a), torch.log(b)
    for ii in range(ITMAX):
        v = lb - torch.logsumexp(Mr + u[:, :, None], 1)
        u = la - torch.logsumexp(Mr + v[:, None, :], 2)
        if ii % 10 == 0:
            err = torch.linalg.vector_norm(torch.exp(Mr + u[:, :, None] + v[:, None, :]).sum(1) - b, dim=1)
            if bool((err < THR).all()):
                break
    return torch.exp(Mr + u[:, :, None] + v[:, None, :]), ii


def torch_knopp(M, a, b):
    K = torch.exp(M / -REG)
    Kp = K / a[:, :, None]
    u, v = torch.full_like(a, 1.0 / a.shape[1]), torch.full_like(b, 1.0 / b.shape[1])
    for ii in range(ITMAX):
        v = b / torch.bmm(K.transpose(1, 2), u[:, :, None])[:, :, 0]
        u = 1.0 / torch.bmm(Kp, v[:, :, None])[:, :, 0]
        if ii % 10 == 0:
            err = torch.linalg.vector_norm(v * torch.bmm(K.transpose(1, 2), u[:, :, None])[:, :, 0] - b, dim=1)
            if bool((err < THR).all()):
                break
    return u[:, :, None] * K * v[:, None, :], ii


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    lines = [f"# tools/probe_sinkhorn.py: reg {REG} stopThr {THR} numItermax {ITMAX}; median of {args.runs} calls, {args.repeats} repeats, ms",
             f"# {torch.cuda.get_device_name(0)}",
             "shape            method        kernel_ms  torch_ms   kernel niter (min/median/max)  torch niter  rel(T)    repeats kernel | torch"]
    for B, n in ((1280, 33), (640, 83)):
        M, a, b = problems(B, n, dev, 100 + n)
        for method, tfn in (("sinkhorn_log", torch_log), ("sinkhorn", torch_knopp)):
            kern = lambda: ops.sinkhorn_batched(M, a, b, reg=REG, method=method, num_iter_max=ITMAX, stop_thr=THR)
            tor = lambda: tfn(M, a, b)
            T, _loss, _lu, _lv, info, _errs = kern()
            Tt, tn = tor()
            rel = float((T - Tt).norm() / Tt.norm())
            ni = info[:, 0].float()
            k_ms, t_ms = [], []
            for _ in range(args.repeats):
                k_ms.append(timed(kern, args.runs, args.warmup))
                t_ms.append(timed(tor, args.runs, args.warmup))
            lines.append(f"B={B:<5d}{n:>3d}x{n:<3d}  {method:<12s}  {statistics.median(k_ms):9.3f}  {statistics.median(t_ms):8.3f}   "
                         f"{int(ni.min())}/{int(ni.median())}/{int(ni.max())}".ljust(88) + f"{tn:<11d}  {rel:.2e}  "
                         f"{' '.join(f'{x:.3f}' for x in k_ms)} | {' '.join(f'{x:.3f}' for x in t_ms)}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
