"""What does the unrolled Sinkhorn gradient's backward launch cost, next to the forward launch and to torch autograd through the same iteration?

    python tools/probe_sinkhorn_grad.py [--runs 25] [--warmup 5] [--repeats 3] [--out profiles/sinkhorn_grad_probe.txt]

Two shapes, the coupling counts and sizes of the cfg2 and cfg3 batches: B = 1280 problems of 33 x 33 and B = 640 of 83 x 83, reg 0.1, both
methods, two settings: stopThr 1e-5 / numItermax 100 (every problem stops at its second check) and stopThr 0 (all 100 sweeps).  Problems as in
tools/probe_sinkhorn.py.  The cotangents are a random loss weight per problem and a standard normal dT per plan entry.  Per row, HIP events
around the call after warm-up, the median of --runs calls, --repeats times in one process with the three sides interleaved (all repeats are
printed; the row's figure is their median):

    fwd_ms      ops.sinkhorn_unrolled's forward = ops.sinkhorn_batched's launch
    bwd_ms      its backward: conan_sinkhorn_bwd (recomputes the sweeps, runs them in reverse, one product over the histories) with the
                allocation of its outputs and workspace
    torch_ms    torch autograd's backward through the same iteration written as batched fp32 torch ops on the same GPU, unrolled for the
                kernel's largest sweep count, without checks (the stop decision carries no gradient).  That is the reference's arithmetic,
                not the code under test; its forward is not timed.

The sweep counts of both sides are printed beside the times, and dM, da are compared (relative Frobenius error of the kernel's against
torch's fp32), so that the timings are known to be of the same quantity.  No ratio is promised: the figures are stated."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd import ops  # noqa: E402
from probe_sinkhorn import problems, timed  # noqa: E402

REG, ITMAX = 0.1, 100


def torch_log(M, a, b, sweeps):
    Mr = -M / REG
    u = torch.zeros_like(a)
    la, lb = torch.log(a), torch.log(b)
    for _ in range(sweeps):
        v = lb - torch.logsumexp(Mr + u[:, :, None], 1)
        u = la - torch.logsumexp(Mr + v[:, None, :], 2)
    return torch.exp(Mr + u[:, :, None] + v[:, None, :])


def torch_knopp(M, a, b, sweeps):
    K = torch.exp(M / -REG)
    Kp = K / a[:, :, None]
    u = torch.full_like(a, 1.0 / a.shape[1])
    for _ in range(sweeps):
        v = b / torch.bmm(K.transpose(1, 2), u[:, :, None])[:, :, 0]
        u = 1.0 / torch.bmm(Kp, v[:, :, None])[:, :, 0]
    return u[:, :, None] * K * v[:, None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    lines = [f"# tools/probe_sinkhorn_grad.py: reg {REG} numItermax {ITMAX}; median of {args.runs} calls, {args.repeats} repeats, ms",
             f"# {torch.cuda.get_device_name(0)}",
             "shape            method        stopThr  fwd_ms   bwd_ms   torch_ms  kernel sweeps (min/median/max)  torch sweeps  rel(dM)   rel(da)   "
             "repeats fwd | bwd | torch"]
    for B, n in ((1280, 33), (640, 83)):
        M0, a0, b0 = problems(B, n, dev, 100 + n)
        g = torch.Generator().manual_seed(7)
        gout, gT = (torch.rand(B, generator=g) + 0.5).to(dev), torch.randn(B, n, n, generator=g).to(dev)
        for thr in (1e-5, 0.0):
            for method, tfn in (("sinkhorn_log", torch_log), ("sinkhorn", torch_knopp)):
                kw = dict(reg=REG, method=method, num_iter_max=ITMAX, stop_thr=thr)
                M, a, b = (t.clone().requires_grad_(True) for t in (M0, a0, b0))
                T, loss, _lu, _lv, info, _errs = ops.sinkhorn_unrolled(M, a, b, **kw)
                sweeps = (info[:, 0] + 1 - ((info[:, 1] >> 1) & 1)).float()
                Mt, at, bt = (t.clone().requires_grad_(True) for t in (M0, a0, b0))
                Tt = tfn(Mt, at, bt, int(sweeps.max()))
                lt = (Mt * Tt).sum((1, 2))
                fwd = lambda: ops.sinkhorn_batched(M0, a0, b0, **kw)
                bwd = lambda: torch.autograd.grad([loss, T], [M, a, b], [gout, gT], retain_graph=True)
                tor = lambda: torch.autograd.grad([lt, Tt], [Mt, at, bt], [gout, gT], retain_graph=True)
                gk, gt = bwd(), tor()
                rm, ra = float((gk[0] - gt[0]).norm() / gt[0].norm()), float((gk[1] - gt[1]).norm() / gt[1].norm())
                f_ms, b_ms, t_ms = [], [], []
                for _ in range(args.repeats):
                    f_ms.append(timed(fwd, args.runs, args.warmup))
                    b_ms.append(timed(bwd, args.runs, args.warmup))
                    t_ms.append(timed(tor, args.runs, args.warmup))
                med = statistics.median
                lines.append(f"B={B:<5d}{n:>3d}x{n:<3d}  {method:<12s}  {thr:<7g}  {med(f_ms):7.3f}  {med(b_ms):7.3f}  {med(t_ms):8.3f}  "
                             f"{int(sweeps.min())}/{int(sweeps.median())}/{int(sweeps.max())}".ljust(107) + f"{int(sweeps.max()):<12d}  {rm:.2e}  {ra:.2e}  "
                             f"{' '.join(f'{x:.3f}' for x in f_ms)} | {' '.join(f'{x:.3f}' for x in b_ms)} | {' '.join(f'{x:.3f}' for x in t_ms)}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
