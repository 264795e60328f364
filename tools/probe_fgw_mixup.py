"""What does the FGWMixup barycenter (ops.fgw_mixup_barycenter_batched) cost next to the same iteration written with batched torch ops, and
what does its backward add?

    python tools/probe_fgw_mixup.py [--runs 25] [--warmup 3] [--repeats 3] [--out profiles/fgw_mixup_grad_probe.txt]

Two shapes with max_iter = 5, tol = 1e-9, alpha = 0.5, rho = 8, epoch = 100, eps = 1e-5: cfg2's (B = 256 molecules, K = 5 graphs, N = 33 nodes,
d = 64) and BACE's (B = 64, K = 3, N = 90, d = 64: its matrices are streamed, N > 79).  Inputs are seeded: features uniform in [0.1, 2], random
undirected graphs of density 0.3, init_C the first graph.  Per shape, HIP events around the call after warm-up, the median of --runs calls,
--repeats times with the two sides interleaved (all repeats are printed; the row's figure is their median):

    kernel_ms   ops.fgw_mixup_barycenter_batched (fp64 inside, every coupling stops on its own check, every molecule on its own errors)
    torch_ms    the reference's arithmetic on the same GPU: the same iteration as batched fp32 torch ops over all B * K couplings; a coupling
                that has passed its check keeps its plan while the batch is iterated until the last one has (one host synchronisation per
                check, as in the reference), all five outer iterations

A second row per shape ("grad") times the same call followed by its backward (torch.autograd.backward with fixed output gradients for Y and C,
no loss kernels in between), once with every differentiable input a leaf (Ys, Cs, p, lambdas: conan_fgw_barycenter_bwd_full) and once with Ys alone
(conan_fgw_barycenter_bwd), beside a forward with the same explicit uniform p and lambdas; the backward's own cost is the difference.  The backward
works on the couplings of the last outer iteration only, so it does not grow with max_iter or epoch.  No threshold is set: the figures are stated.

Every shape runs in a process of its own under `timeout -k 10` (this script is the driver; --shape NAME is the worker), and the driver stops
at the first shape that fails.  The epoch counts of both sides are printed beside the times, and so is each side's distance (relative Frobenius
error of Y and of C) from the same torch ops run once in fp64, so that the timings are known to be of the same quantity: five outer iterations on
random graphs amplify rounding, which shows in the fp32 side's distance.  No ratio is promised: the figures are stated."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg2": (256, 5, 33, 64), "bace": (64, 3, 90, 64)}
PRM = dict(alpha=0.5, rho=8.0, max_iter=5, tol=1e-9, epoch=100, eps=1e-5)
GRAD_HEAD = "grad  shape                 fwd_ms  fwd+bwd all leaves_ms  fwd+bwd Ys only_ms  bwd all_ms  bwd Ys_ms  repeats fwd | all leaves | Ys only"
HEAD = "shape                      kernel_ms  torch_ms  kernel epochs (sum / per coupling solve)  torch epochs  kernel rel(Y) rel(C)  torch rel(Y) rel(C)  flags  repeats kernel | torch"


def torch_mixup(Ys, Cs, alpha, rho, max_iter, tol, epoch, eps):
    """fgw_barycenters_BAPG of every molecule at once in fp32 torch ops: Ys [B,K,N,d], Cs [B,K,N,N], uniform weights, init_C = Cs[:, 0]."""
    import torch
    B, K, N, d = Ys.shape
    p = 1.0 / N
    C, Y = Cs[:, 0].clone(), torch.zeros(B, N, d, device=Ys.device, dtype=Ys.dtype)
    z2 = (Ys * Ys).sum(-1)
    epochs = 0
    for _ in range(max_iter):
        M = ((Y * Y).sum(-1)[:, None, :, None] + z2[:, :, None, :] - 2.0 * torch.einsum("bid,bkjd->bkij", Y, Ys)).clamp_min(0)
        Mb, A = (1 - alpha) * M, C[:, None].expand(B, K, N, N)
        X = torch.full((B, K, N, N), p * p, device=Ys.device, dtype=Ys.dtype)
        last, done = None, torch.zeros(B, K, 1, 1, dtype=torch.bool, device=Ys.device)      # a coupling that has stopped keeps its plan
        for ii in range(epoch):
            Xn = X + 1e-10
            Xn = torch.exp((4 * alpha * (A @ Xn @ Cs) - Mb) / rho) * Xn
            Xn = Xn * (p / Xn.sum(3, keepdim=True))
            Xn = torch.exp((4 * alpha * (A @ Xn @ Cs) - Mb) / rho) * Xn
            Xn = Xn * (p / Xn.sum(2, keepdim=True))
            X = torch.where(done, X, Xn)
            epochs += 1
            if ii > 0 and ii % 10 == 0:
                obj = ((Mb - 2 * alpha * (A @ X @ Cs)) * X).sum((2, 3), keepdim=True)
                if last is not None:
                    done = done | (((obj - last) / last).abs() < eps)
                    if bool(done.all()):
                        break
                last = torch.where(done, last, obj) if last is not None else obj
        Yn = torch.einsum("bkij,bkjd->bid", X, Ys) / (K * p)
        Cn = (X @ Cs @ X.transpose(2, 3)).sum(1) / (K * p * p)
        ef, es = (Yn - Y).flatten(1).norm(dim=1), (Cn - C).flatten(1).norm(dim=1)
        Y, C = Yn, Cn
        if not bool(((ef > tol) | (es > tol)).any()):
            break
    return Y, C, epochs


def worker(name, runs, warmup, repeats):
    import torch
    sys.path.insert(0, ROOT)
    from conan_fgw_amd import ops
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    B, K, N, d = SHAPES[name]
    g = torch.Generator().manual_seed(1000 + N)
    Ys = (torch.rand(B, K, N, d, generator=g) * 1.9 + 0.1).to(dev)
    u = torch.triu((torch.rand(B, K, N, N, generator=g) < 0.3).float(), 1)
    Cs = (u + u.transpose(2, 3)).to(dev)

    def timed(fn):
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

    kern = lambda: ops.fgw_mixup_barycenter_batched(Ys, Cs, **PRM)
    tor = lambda: torch_mixup(Ys, Cs, **PRM)
    Y, C, _T, info, _errs = kern()
    Yt, Ct, tn = tor()
    Yd, Cd, _ = torch_mixup(Ys.double(), Cs.double(), **PRM)          # the same ops in fp64: the yardstick of both sides' values (not timed)
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    solves = int(info[:, 0].sum()) * K
    k_ms, t_ms = [], []
    for _ in range(repeats):
        k_ms.append(timed(kern))
        t_ms.append(timed(tor))
    print(f"B={B:<4d}K={K} N={N:<3d}d={d:<4d}  {statistics.median(k_ms):9.3f}  {statistics.median(t_ms):8.3f}  "
          f"{int(info[:, 1].sum())} / {int(info[:, 1].sum()) / max(solves, 1):.1f}".ljust(90) + f"{tn:<12d}  {rel(Y, Yd):.2e} {rel(C, Cd):.2e}  {rel(Yt, Yd):.2e} {rel(Ct, Cd):.2e}  "
          f"{int((info[:, 3] != 0).sum()):<5d}  {' '.join(f'{x:.3f}' for x in k_ms)} | {' '.join(f'{x:.3f}' for x in t_ms)}")
    # forward + backward: explicit uniform weights, so that p and lambdas can be leaves; the output gradients are fixed tensors
    p = torch.full((B, N), 1.0 / N, device=dev)
    lam = torch.full((K,), 1.0 / K, device=dev)
    gen = torch.Generator().manual_seed(7)
    gw, gc = torch.randn(B, N, d, generator=gen).to(dev), torch.randn(B, N, N, generator=gen).to(dev)
    leaf = lambda t: t.clone().requires_grad_(True)
    all_leaves = (leaf(Ys), leaf(Cs), leaf(p), leaf(lam))
    ys_leaf = leaf(Ys)

    def fwd():
        ops.fgw_mixup_barycenter_batched(Ys, Cs, p=p, lambdas=lam, **PRM)

    def fb_all():
        for t in all_leaves:
            t.grad = None
        Yo, Co = ops.fgw_mixup_barycenter_batched(all_leaves[0], all_leaves[1], p=all_leaves[2], lambdas=all_leaves[3], **PRM)[:2]
        torch.autograd.backward((Yo, Co), (gw, gc))

    def fb_ys():
        ys_leaf.grad = None
        Yo = ops.fgw_mixup_barycenter_batched(ys_leaf, Cs, p=p, lambdas=lam, **PRM)[0]
        Yo.backward(gw)

    f_ms, a_ms, y_ms = [], [], []
    for _ in range(repeats):
        f_ms.append(timed(fwd))
        a_ms.append(timed(fb_all))
        y_ms.append(timed(fb_ys))
    assert all(bool(torch.isfinite(t.grad).all()) for t in all_leaves) and bool(torch.isfinite(ys_leaf.grad).all())
    med = statistics.median
    print(f"grad  B={B:<4d}K={K} N={N:<3d}d={d:<4d} {med(f_ms):7.3f}  {med(a_ms):21.3f}  {med(y_ms):18.3f}  {med(a_ms) - med(f_ms):10.3f}  {med(y_ms) - med(f_ms):9.3f}  "
          f"{' '.join(f'{x:.3f}' for x in f_ms)} | {' '.join(f'{x:.3f}' for x in a_ms)} | {' '.join(f'{x:.3f}' for x in y_ms)}")
    print(f"# device: {torch.cuda.get_device_name(0)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds a shape's process may take")
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help="worker: measure this shape in this process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.shape:
        return worker(args.shape, args.runs, args.warmup, args.repeats)
    lines = [f"# tools/probe_fgw_mixup.py: {' '.join(f'{k} {v}' for k, v in PRM.items())}; median of {args.runs} calls, {args.repeats} repeats, ms", HEAD]
    device = ""
    for name in ("cfg2", "bace"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--shape", name, "--runs", str(args.runs),
               "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        print(f"# measuring {name} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:          # a failure ends the probe: nothing more is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"probe_fgw_mixup: shape {name} ended with status {r.returncode}; stopping")
        out = r.stdout.strip().splitlines()
        lines += [l for l in out if not l.startswith("# device")]
        device = next((l for l in out if l.startswith("# device")), device)
    lines = [l for l in lines if not l.startswith("grad")] + [GRAD_HEAD] + [l for l in lines if l.startswith("grad")]
    lines.insert(1, device)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
