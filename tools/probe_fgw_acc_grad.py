"""What does the unrolled FGWMixup gradient (ops.fgw_acc_pair_unrolled, conan_fgw_acc_pair_bwd) cost next to its forward, and next to torch
autograd through the same epochs?

    python tools/probe_fgw_acc_grad.py [--runs 15] [--warmup 2] [--repeats 3] [--parent-lib PATH] [--out profiles/fgw_acc_grad_probe.txt]

The shapes of profiles/fgw_mixup_probe.txt as pairs: cfg2's couplings (B = 256 * 5 = 1280 pairs of N = 33 nodes) and BACE's (B = 64 * 3 = 192 pairs
of N = 90: above both residency bounds, the matrices are streamed), alpha = 0.5, rho = 8, epoch = 100 and eps = 0, so that every pair runs all
100 epochs on every side and the sides do the same work.  Inputs are seeded: squared distances of features uniform in [0.1, 2] (d = 64), random
undirected graphs of density 0.3, random normalised weights.  Per shape, HIP events around the call after warm-up, the median of --runs calls,
--repeats times with the sides interleaved (all repeats are printed; a row's figure is their median, its spread (max - min) / median):

    fwd_ms        ops.fgw_acc_pair_batched: the forward alone
    fwd+bwd_ms    ops.fgw_acc_pair_unrolled with M, A, Bm, a, b as leaves, then ONE backward for the cotangents of X and dist
    bwd_ms        the difference; bwd/fwd is the ratio the product count puts at about four (replay 2 + walk 6 against the forward's 2)
    torch64_ms    the same epochs, the same distance and loss.backward() as batched fp64 torch ops on the same GPU: what a user would otherwise
                  run to get this gradient (no stop checks either)
    agree         the largest relative Frobenius distance between the op's gradients and torch's (fp32 outputs of an fp64 iteration: 1e-7)

With --parent-lib (a libconan_fgw_hip.so built from the parent commit) a second table times conan_fgw_acc_pair_fwd of both libraries through
ctypes on the same buffers, interleaved: the existing forward must not move.  No threshold is set: the figures are stated.

Every shape runs in a process of its own under `timeout -k 10` (this script is the driver; --shape NAME is the worker), and the driver stops at
the first shape that fails."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg2": (1280, 33, 64), "bace": (192, 90, 64)}
PRM = dict(alpha=0.5, rho=8.0, epoch=100, eps=0.0)
HEAD = "shape              fwd_ms  fwd+bwd_ms   bwd_ms  bwd/fwd  torch64_ms  torch64/(fwd+bwd)  agree     spread fwd  fwd+bwd  repeats fwd | fwd+bwd | torch64"
PARENT_HEAD = "parent  shape       this_fwd_ms  parent_fwd_ms  difference  spread this  parent  repeats this | parent"


def torch_loss(M, A, Bm, a, b, W, alpha, rho, epoch):
    """sum(W * X) + sum(dist) after `epoch` epochs from a b^T, every pair at once, in the dtype of the inputs."""
    import torch
    X = a[:, :, None] * b[:, None, :]
    Mb = (1 - alpha) * M
    for _ in range(epoch):
        X = X + 1e-10
        X = torch.exp((4 * alpha * (A @ X @ Bm) - Mb) / rho) * X
        X = X * (a / X.sum(2))[:, :, None]
        X = torch.exp((4 * alpha * (A @ X @ Bm) - Mb) / rho) * X
        X = X * (b / X.sum(1))[:, None, :]
    c1 = ((A * A) @ a[:, :, None]) + (b[:, None, :] @ (Bm * Bm))
    dist = (Mb * X).sum((1, 2)) + alpha * ((c1 * X).sum((1, 2)) - 2 * ((A @ X @ Bm) * X).sum((1, 2)))
    return (W * X).sum() + dist.sum()


def worker(name, runs, warmup, repeats, parent_lib):
    import torch
    sys.path.insert(0, ROOT)
    from conan_fgw_amd import _lib, ops
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    B, N, d = SHAPES[name]
    g = torch.Generator().manual_seed(2000 + N)
    y, z = torch.rand(B, N, d, generator=g) * 1.9 + 0.1, torch.rand(B, N, d, generator=g) * 1.9 + 0.1
    M = ((y[:, :, None, :] - z[:, None, :, :]) ** 2).sum(-1).to(dev)

    def graphs():
        u = torch.triu((torch.rand(B, N, N, generator=g) < 0.3).float(), 1)
        return (u + u.transpose(1, 2)).to(dev)

    def weights():
        w = torch.rand(B, N, generator=g) + 0.5
        return (w / w.sum(1, keepdim=True)).to(dev)
    A, Bm, a, b = graphs(), graphs(), weights(), weights()
    W = torch.randn(B, N, N, generator=g).to(dev)
    ones = torch.ones(B, device=dev)

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

    leaf = lambda t, dt=torch.float32: t.detach().to(dt).clone().requires_grad_(True)
    k_leaves = [leaf(t) for t in (M, A, Bm, a, b)]
    t_leaves = [leaf(t, torch.float64) for t in (M, A, Bm, a, b)]
    W64 = W.double()

    def fwd():
        return ops.fgw_acc_pair_batched(M, A, Bm, a, b, **PRM)

    def fb():
        for t in k_leaves:
            t.grad = None
        X, dist, _objs, _info = ops.fgw_acc_pair_unrolled(*k_leaves, **PRM)
        torch.autograd.backward((X, dist), (W, ones))

    def tor():
        for t in t_leaves:
            t.grad = None
        torch_loss(*t_leaves, W64, PRM["alpha"], PRM["rho"], PRM["epoch"]).backward()

    info = fwd()[2]
    assert int(info[:, 0].min()) == int(info[:, 0].max()) == PRM["epoch"] and not bool((info[:, 2] != 0).any()), "every pair must run all its epochs, unflagged"
    fb(); tor()
    rel = lambda x, y: float((x.double() - y).norm() / y.norm())
    agree = max(rel(k.grad, t.grad) for k, t in zip(k_leaves, t_leaves))
    f_ms, b_ms, t_ms = [], [], []
    for _ in range(repeats):
        f_ms.append(timed(fwd))
        b_ms.append(timed(fb))
        t_ms.append(timed(tor))
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    rep = lambda v: " ".join(f"{x:.3f}" for x in v)
    f, fbm, t = med(f_ms), med(b_ms), med(t_ms)
    print(f"B={B:<5d}N={N:<3d}  {f:9.3f}  {fbm:10.3f}  {fbm - f:7.3f}  {(fbm - f) / f:7.2f}  {t:10.3f}  {t / fbm:17.2f}  {agree:.2e}  {spread(f_ms):10.4f}  {spread(b_ms):7.4f}  "
          f"{rep(f_ms)} | {rep(b_ms)} | {rep(t_ms)}")
    if parent_lib:
        X = torch.empty(B, N, N, device=dev)
        objs = torch.empty(B, (PRM["epoch"] + 9) // 10, device=dev)
        info = torch.empty(B, 4, dtype=torch.int32, device=dev)
        L = _lib.lib()
        ws = torch.empty(int(L.conan_fgw_acc_pair_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)
        P = ctypes.CDLL(os.path.abspath(parent_lib))
        P.conan_fgw_acc_pair_fwd.restype, P.conan_fgw_acc_pair_fwd.argtypes = _lib.SIGNATURES["conan_fgw_acc_pair_fwd"]
        args = (M.data_ptr(), A.data_ptr(), Bm.data_ptr(), a.data_ptr(), b.data_ptr(), None, B, N, PRM["alpha"], PRM["rho"], PRM["epoch"], PRM["eps"],
                X.data_ptr(), objs.data_ptr(), info.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
        outs = []
        for lib_ in (L, P):
            assert lib_.conan_fgw_acc_pair_fwd(*args) == 0
            torch.cuda.synchronize()
            outs.append(X.clone())
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "the forward's bits moved against the parent library"
        m_ms, p_ms = [], []
        for _ in range(repeats):
            m_ms.append(timed(lambda: L.conan_fgw_acc_pair_fwd(*args)))
            p_ms.append(timed(lambda: P.conan_fgw_acc_pair_fwd(*args)))
        print(f"parent  B={B:<5d}N={N:<3d}  {med(m_ms):9.3f}  {med(p_ms):13.3f}  {(med(m_ms) - med(p_ms)) / med(p_ms):+10.4f}  {spread(m_ms):11.4f}  {spread(p_ms):6.4f}  "
              f"{rep(m_ms)} | {rep(p_ms)}")
    print(f"# device: {torch.cuda.get_device_name(0)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds a shape's process may take")
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help="worker: measure this shape in this process")
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: its forward is timed beside this one's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.shape:
        return worker(args.shape, args.runs, args.warmup, args.repeats, args.parent_lib)
    lines = [f"# tools/probe_fgw_acc_grad.py: {' '.join(f'{k} {v}' for k, v in PRM.items())}; median of {args.runs} calls, {args.repeats} repeats, ms", HEAD]
    device = ""
    for name in ("cfg2", "bace"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--shape", name, "--runs", str(args.runs),
               "--warmup", str(args.warmup), "--repeats", str(args.repeats)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
        print(f"# measuring {name} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:          # a failure ends the probe: nothing more is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"probe_fgw_acc_grad: shape {name} ended with status {r.returncode}; stopping")
        out = r.stdout.strip().splitlines()
        lines += [l for l in out if not l.startswith("# device")]
        device = next((l for l in out if l.startswith("# device")), device)
    parent = [l for l in lines if l.startswith("parent")]
    lines = [l for l in lines if not l.startswith("parent")] + ([PARENT_HEAD] + parent if parent else [])
    lines.insert(1, device)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
