"""What do the three solvers of csrc/sinkhorn_ext.hip cost per sweep or step, next to the Knopp kernel of csrc/sinkhorn.hip in the same process?

    python tools/probe_sinkhorn_ext.py [--runs 15] [--warmup 3] [--repeats 3] [--out profiles/sinkhorn_ext_probe.txt]

The shapes of tools/probe_sinkhorn.py: B = 1280 problems of 33 x 33 and B = 640 of 83 x 83 (its costs and marginals), at reg 0.1 and 0.01.  Every
run has stopThr = 0, which no error reaches, so the amount of work is its cap and the same for every problem:
    sinkhorn (Knopp)           100 sweeps, a check every 10th
    sinkhorn_stabilized        100 sweeps, print_period 10 (the same number of checks; a sweep is Knopp's two passes plus two maxima)
    sinkhorn_epsilon_scaling   35 outer iterations of 20 inner sweeps (the count is read back from the kernel)
    greenkhorn                 1000 steps
HIP events around the call after warm-up, the median of --runs calls, --repeats times with the methods interleaved (the row's figure is the
median of the repeats).  us_per = launch time over sweeps (steps) of ONE problem: the problems of a launch run side by side, so this is the
latency of a sweep as the batch sees it, set-up, checks and absorptions included.  ratio = us_per over Knopp's at the same shape and reg."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd import ops  # noqa: E402
from probe_sinkhorn import problems, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    lines = [f"# tools/probe_sinkhorn_ext.py: stopThr 0 (every run takes its cap); median of {args.runs} calls, {args.repeats} repeats",
             f"# {torch.cuda.get_device_name(0)}",
             "shape            reg   method                    launch_ms  sweeps/steps  us_per   ratio to Knopp  absorptions (min/median/max)  repeats ms"]
    for B, n in ((1280, 33), (640, 83)):
        M, a, b = problems(B, n, dev, 100 + n)
        for reg in (0.1, 0.01):
            ext = lambda method, **kw: (lambda: ops.sinkhorn_ext_batched(M, a, b, reg=reg, method=method, stop_thr=0.0, **kw))
            runs = [("sinkhorn", lambda: ops.sinkhorn_batched(M, a, b, reg=reg, method="sinkhorn", num_iter_max=100, stop_thr=0.0)),
                    ("sinkhorn_stabilized", ext("sinkhorn_stabilized", num_iter_max=100, print_period=10)),
                    ("sinkhorn_epsilon_scaling", ext("sinkhorn_epsilon_scaling", num_iter_max=35, num_inner_iter_max=20)),
                    ("greenkhorn", ext("greenkhorn", num_iter_max=1000))]
            work, absorbed = {}, {}
            for name, fn in runs:
                out = fn()
                if name == "sinkhorn":
                    x = out[4][:, 0]
                    assert int(x.min()) == int(x.max()), "the problems of the launch did different amounts of work"
                    work[name], absorbed[name] = int(x[0]) + 1, None
                else:
                    x = out[8][:, 0]
                    assert int(x.min()) == int(x.max()), "the problems of the launch did different amounts of work"
                    work[name], absorbed[name] = int(x[0]), None if name == "greenkhorn" else out[8][:, 1].float()
            ms = {name: [] for name, _ in runs}
            for _ in range(args.repeats):
                for name, fn in runs:
                    ms[name].append(timed(fn, args.runs, args.warmup))
            per = {name: 1e3 * statistics.median(ms[name]) / work[name] for name, _ in runs}
            for name, _ in runs:
                ab = absorbed[name]
                lines.append(f"B={B:<5d}{n:>3d}x{n:<3d}  {reg:<5g} {name:<25s} {statistics.median(ms[name]):9.3f}  {work[name]:<12d}  {per[name]:7.3f}  "
                             f"{per[name] / per['sinkhorn']:<14.2f}  " + ("-" if ab is None else f"{int(ab.min())}/{int(ab.median())}/{int(ab.max())}").ljust(28)
                             + "  " + " ".join(f"{x:.3f}" for x in ms[name]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
