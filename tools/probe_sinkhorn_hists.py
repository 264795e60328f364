"""What does Sinkhorn for several histograms at once (ops.sinkhorn_hists_batched) cost next to the same columns stacked through the 1-D kernel?

    python tools/probe_sinkhorn_hists.py [--runs 15] [--warmup 3] [--repeats 3] [--out profiles/sinkhorn_hists_probe.txt]

Shapes: B = 256 problems of 33 x 33 with H = 5, 16 and 64 target histograms, and B = 64 problems of 83 x 83 with H = 16; beside them H = 1, 2, 4
(33 x 33) and H = 4 (83 x 83), which the kernel runs as per-wavefront dots where H >= 5 runs on the matrix pipe: the rows either side of that
switch show where it belongs.  reg 0.1, numItermax 100 and stopThr 0, so that no form stops early and every form does the same 100 sweeps and
10 checks.  Costs are squared distances of Gaussian
clouds over their maximum, histograms random, normalised (the construction of the stored fixtures).  Per shape, HIP events around the call
after warm-up, the median of --runs calls, --repeats times in one process with the forms interleaved (all repeats are printed; the row's figure
is their median):

    hists_ms     ops.sinkhorn_hists_batched: one workgroup per problem, K staged once, U and V as matrices (the new kernel)
    stacked_ms   the same columns as B H problems through ops.sinkhorn_batched(method="sinkhorn") with M expanded to [B H, n, n] beforehand:
                 the best a caller could do without the new kernel (every column stops on its own there: other semantics)
    +expand_ms   the same with the expansion of M, a and b inside the timed region
    torch_ms     the reference's Knopp iteration as batched fp64 torch ops on the same GPU, one host synchronisation per check as in the reference
    hists_1_ms   the new kernel at numItermax 1 (one sweep, one check, the set-up and the costs): what is not the loop

The costs of the first two forms are compared (largest relative difference), so that the timings are known to be of the same quantity.  No
ratio is promised: the figures are stated."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd import ops  # noqa: E402

REG, THR, ITMAX = 0.1, 0.0, 100


def problems(B, n, H, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x, y = torch.randn(B, n, 3, generator=g), torch.randn(B, n, 3, generator=g) + 0.5
    M = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    M = M / M.amax(dim=(1, 2), keepdim=True)
    a, b = torch.rand(B, n, generator=g) + 0.1, torch.rand(B, n, H, generator=g) + 0.1
    return M.to(dev), (a / a.sum(1, keepdim=True)).to(dev), (b / b.sum(1, keepdim=True)).to(dev)


def expand(M, a, b):
    B, n, H = b.shape
    return (M[:, None].expand(B, H, n, n).reshape(B * H, n, n), a[:, None].expand(B, H, n).reshape(B * H, n), b.transpose(1, 2).reshape(B * H, n))


def torch_knopp(M, a, b):
    M, a, b = M.double(), a.double(), b.double()
    K = torch.exp(M / -REG)
    Kp = K / a[:, :, None]
    u, v = torch.full_like(b, 1.0 / a.shape[1]), torch.full_like(b, 1.0 / b.shape[1])
    for ii in range(ITMAX):
        v = b / torch.bmm(K.transpose(1, 2), u)
        u = 1.0 / torch.bmm(Kp, v)
        if ii % 10 == 0:
            err = torch.linalg.vector_norm(v * torch.bmm(K.transpose(1, 2), u) - b, dim=(1, 2))
            if bool((err < THR).all()):
                break
    return torch.einsum("bik,bij,bjk,bij->bk", u, K, v, M)


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
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    lines = [f"# tools/probe_sinkhorn_hists.py: reg {REG} stopThr {THR} numItermax {ITMAX} (100 sweeps, 10 checks in every form); median of {args.runs} "
             f"calls, {args.repeats} repeats, ms", f"# {torch.cuda.get_device_name(0)}",
             "shape                 hists_ms  stacked_ms  +expand_ms  torch_ms  hists_1_ms  stacked/hists  rel(cost)  repeats hists | stacked | +expand | torch"]
    kw = dict(reg=REG, num_iter_max=ITMAX, stop_thr=THR)
    for B, n, H in ((256, 33, 1), (256, 33, 2), (256, 33, 4), (256, 33, 5), (256, 33, 16), (256, 33, 64), (64, 83, 4), (64, 83, 16)):
        M, a, b = problems(B, n, H, dev, 100 + n + H)
        Me, ae, be = expand(M, a, b)
        forms = {"hists": lambda: ops.sinkhorn_hists_batched(M, a, b, **kw),
                 "stacked": lambda: ops.sinkhorn_batched(Me, ae, be, method="sinkhorn", **kw),
                 "expand": lambda: ops.sinkhorn_batched(*expand(M, a, b), method="sinkhorn", **kw),
                 "torch": lambda: torch_knopp(M, a, b),
                 "hists_1": lambda: ops.sinkhorn_hists_batched(M, a, b, reg=REG, num_iter_max=1, stop_thr=THR)}
        out, st = forms["hists"](), forms["stacked"]()
        assert out[3][:, 0].eq(ITMAX - 1).all() and st[4][:, 0].eq(ITMAX - 1).all() and not out[3][:, 1].any()      # nobody stopped early
        rel = float(((out[0] - st[1].reshape(B, H)).abs() / st[1].reshape(B, H).abs()).max())
        ms = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, fn in forms.items():
                ms[k].append(timed(fn, args.runs, args.warmup))
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append(f"B={B:<4d}{n:>3d}x{n:<3d} H={H:<3d}  {med['hists']:8.3f}  {med['stacked']:10.3f}  {med['expand']:10.3f}  {med['torch']:8.3f}  "
                     f"{med['hists_1']:10.3f}  {med['stacked'] / med['hists']:13.2f}  {rel:.2e}   "
                     + " | ".join(" ".join(f"{x:.3f}" for x in ms[k]) for k in ("hists", "stacked", "expand", "torch")))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
