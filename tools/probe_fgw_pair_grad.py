"""What does the backward of the pair distance cost next to the solve it follows and next to the same closed form in torch?

    python tools/probe_fgw_pair_grad.py [--runs 25] [--warmup 5] [--repeats 3] [--json OUT.json]

Three shapes — B = 10, N = 33 (the pairs of a K = 5 ESOL-shaped ensemble), B = 10, N = 83 (Lipophilicity-shaped), B = 2560, N = 33 (every pair of a
cfg2 batch) — with the model's literals (alpha 0.1, epsilon 0.1, max_iter 5, tol 1e-4, numItermax 5, stopThr 1e-2).  Per shape, HIP events around
the call after warm-up, the median of --runs calls, --repeats times in one process (all repeats are printed; the row's figure is their median):

    bwd_ms      conan_fgw_pair_dist_bwd, all five gradients, at the plan of the solve below
    solve_ms    ops.fgw_pair_batched of the same batch (the forward the backward follows)
    torch_ms    the same closed form ("Pair form: backward") as torch fp32 bmm expressions on the device

The kernel's gradients are compared with the torch expression's (relative Frobenius error, printed) so that the timings are known to be of the
same quantity."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd import fgw as pfgw  # noqa: E402
from conan_fgw_amd import ops  # noqa: E402
from conan_fgw_amd._lib import call, stream_ptr  # noqa: E402
from probe_fgw_pair import MODEL, problem, timed  # noqa: E402


def torch_closed_form(C1, C2, p, q, T, g, alpha):
    """Square loss, fp32: dM, dC1, dC2, dp, dq."""
    r, c = T.sum(2), T.sum(1)
    ag = (alpha * g)[:, None, None]
    Tt = T.transpose(1, 2)
    dC1 = ag * (2 * C1 * (r[:, :, None] * p[:, None, :]) - 2 * torch.bmm(torch.bmm(T, C2), Tt))
    dC2 = ag * (2 * C2 * (c[:, :, None] * q[:, None, :]) - 2 * torch.bmm(torch.bmm(Tt, C1), T))
    dp = ag[:, :, 0] * torch.bmm((C1 * C1).transpose(1, 2), r[:, :, None])[:, :, 0]
    dq = ag[:, :, 0] * torch.bmm((C2 * C2).transpose(1, 2), c[:, :, None])[:, :, 0]
    return ((1 - alpha) * g)[:, None, None] * T, dC1, dC2, dp, dq


def case(B, N, runs, warmup, repeats, dev):
    Y0, Z, C1, C2 = problem(B, N, 8, 10 + N, dev)
    M = torch.stack([pfgw.feature_cost(Y0[b], Z[b]) for b in range(B)])
    p = torch.full((B, N), 1.0 / N, device=dev)
    q = p.clone()
    g = torch.linspace(0.5, 1.5, B, device=dev)
    solve = lambda: ops.fgw_pair_batched(M, C1, C2, p, q, symmetric=True, **MODEL)
    T = solve()[0]
    out = [torch.empty(B, N, N, device=dev) for _ in range(3)] + [torch.empty(B, N, device=dev) for _ in range(2)]
    bwd = lambda: call("conan_fgw_pair_dist_bwd", C1.data_ptr(), C2.data_ptr(), p.data_ptr(), q.data_ptr(), T.data_ptr(), g.data_ptr(), B, N,
                       MODEL["alpha"], 0, *(o.data_ptr() for o in out), stream_ptr())
    ref = lambda: torch_closed_form(C1, C2, p, q, T, g, MODEL["alpha"])
    bwd()
    err = max(float((a - b).norm() / b.norm()) for a, b in zip(out, ref()))
    reps = dict(bwd_ms=[], solve_ms=[], torch_ms=[])
    for _ in range(repeats):                                       # interleaved: every repeat times all three
        for name, fn in (("bwd_ms", bwd), ("solve_ms", solve), ("torch_ms", ref)):
            reps[name].append(timed(fn, runs, warmup)[0])
    row = dict(case=f"B={B} N={N}", kernel_vs_torch_rel_err=err)
    for name, v in reps.items():
        row[name] = statistics.median(v)
        row[name + "_repeats"] = v
    row["bwd_over_solve"] = row["bwd_ms"] / row["solve_ms"]
    row["bwd_over_torch"] = row["bwd_ms"] / row["torch_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.runs >= 20, "a median of at least 20 runs"
    dev = torch.device("cuda:0")
    rows = [case(10, 33, a.runs, a.warmup, a.repeats, dev), case(10, 83, a.runs, a.warmup, a.repeats, dev), case(2560, 33, a.runs, a.warmup, a.repeats, dev)]
    for r in rows:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), runs=a.runs, repeats=a.repeats, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
