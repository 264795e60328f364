"""What does the unrolled gradient of the FGWMixup barycenter (ops.fgw_mixup_barycenter_unrolled, conan_fgw_mixup_barycenter_bwd) cost next to
its forward, and next to torch autograd through the same loop?

    python tools/probe_fgw_mixup_unrolled.py [--runs 7] [--warmup 1] [--repeats 3] [--parent-lib PATH] [--no-torch] [--out profiles/fgw_mixup_unrolled_probe.txt]

The README's two shapes: cfg2 (B = 256 molecules, K = 5 graphs of N = 33 nodes, d = 64) and BACE (B = 64, K = 3, N = 90, d = 64: above both
residency bounds, the matrices are streamed), alpha = 0.5, rho = 8, max_iter = 5 with tol = 0 and epoch = 100 with eps = 0, so that every
molecule runs all 5 outer iterations of 100 epochs on every side and the sides do the same work.  Inputs are seeded: features uniform in
[0.1, 2], random undirected graphs of density 0.3, random normalised weights.  Per shape, HIP events around the call after warm-up, the
median of --runs calls, --repeats times with the sides interleaved (all repeats are printed; a row's figure is their median, its spread
(max - min) / median):

    fwd_ms        ops.fgw_mixup_barycenter_batched: the existing forward
    rec_ms        conan_fgw_mixup_barycenter_fwd_record through the op under grad mode, no backward: the forward with the state copies added
    fwd+bwd_ms    ops.fgw_mixup_barycenter_unrolled with Ys, Cs, ps, p, lambdas as leaves, then ONE backward for the cotangents of Y and C
    bwd_ms        fwd+bwd - rec; bwd/fwd is the ratio the pair measurements put at four to five
    torch64_ms    the same loop and loss.backward() as batched fp64 torch ops on the same GPU, every coupling of every molecule at once (no stop
                  checks): what a user would otherwise run to get this gradient; n/a where it does not fit
    agree         the largest relative Frobenius distance between the op's gradients and torch's (fp32 outputs of an fp64 iteration: 1e-7)

With --parent-lib (a libconan_fgw_hip.so built from the parent commit) a second table times conan_fgw_mixup_barycenter_fwd of both libraries
through ctypes on the same buffers, interleaved: the existing forward must not move.  No threshold is set: the figures are stated.

Every shape runs in a process of its own under `timeout -k 10` (this script is the driver; --shape NAME is the worker), and the driver stops at
the first shape that fails."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg2": (256, 5, 33, 64), "bace": (64, 3, 90, 64)}
PRM = dict(alpha=0.5, rho=8.0, max_iter=5, tol=0.0, epoch=100, eps=0.0)
HEAD = ("shape                    fwd_ms    rec_ms  fwd+bwd_ms   bwd_ms  bwd/fwd  torch64_ms  torch64/(fwd+bwd)  agree     spread fwd  rec  fwd+bwd  "
        "repeats fwd | rec | fwd+bwd | torch64")
PARENT_HEAD = "parent  shape             this_fwd_ms  parent_fwd_ms  difference  spread this  parent  repeats this | parent"


def torch_loss(Ys, Cs, ps, p, lam, gw, gc, alpha, rho, max_iter, epoch):
    """sum(gw * Y) + sum(gc * C) after max_iter outer iterations of `epoch` epochs from C = Cs[:, 0], Y = 0, every molecule at once, in the
    dtype of the inputs."""
    import torch
    C, Y = Cs[:, 0], torch.zeros_like(gw)
    a, pp = p[:, None, :], p[:, :, None] * p[:, None, :]
    z2 = (Ys * Ys).sum(-1)
    for _ in range(max_iter):
        M = torch.clamp((Y * Y).sum(-1)[:, None, :, None] + z2[:, :, None, :] - 2 * torch.einsum("bic,bkjc->bkij", Y, Ys), min=0)
        Mb, A = (1 - alpha) * M, C[:, None]
        X = a[..., None] * ps[:, :, None, :]
        for _ in range(epoch):
            X = X + 1e-10
            X = torch.exp((4 * alpha * (A @ X @ Cs) - Mb) / rho) * X
            X = X * (a / X.sum(3))[..., None]
            X = torch.exp((4 * alpha * (A @ X @ Cs) - Mb) / rho) * X
            X = X * (ps / X.sum(2))[:, :, None, :]
        Y = torch.einsum("k,bkij,bkjc->bic", lam, X, Ys) / p[:, :, None]
        C = torch.einsum("k,bkij,bkjl,bkml->bim", lam, X, Cs, X) / pp
    return (gw * Y).sum() + (gc * C).sum()


def worker(name, runs, warmup, repeats, parent_lib, with_torch):
    import torch
    sys.path.insert(0, ROOT)
    from conan_fgw_amd import _lib, ops
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    B, K, N, d = SHAPES[name]
    g = torch.Generator().manual_seed(3000 + N)
    Ys = (torch.rand(B, K, N, d, generator=g) * 1.9 + 0.1).to(dev)
    u = torch.triu((torch.rand(B, K, N, N, generator=g) < 0.3).float(), 1)
    Cs = (u + u.transpose(2, 3)).to(dev)

    def weights(*shape):
        w = torch.rand(*shape, generator=g) + 0.5
        return (w / w.sum(-1, keepdim=True)).to(dev)
    ps, p, lam = weights(B, K, N), weights(B, N), weights(K)
    gw, gc = torch.randn(B, N, d, generator=g).to(dev), torch.randn(B, N, N, generator=g).to(dev)

    def timed(fn, n=runs):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    leaf = lambda t, dt=torch.float32: t.detach().to(dt).clone().requires_grad_(True)
    k_leaves = [leaf(t) for t in (Ys, Cs, ps, p, lam)]
    run = lambda fn, L: fn(L[0], L[1], ps=L[2], p=L[3], lambdas=L[4], **PRM)

    def fwd():
        return run(ops.fgw_mixup_barycenter_batched, (Ys, Cs, ps, p, lam))

    def rec():
        return run(ops.fgw_mixup_barycenter_unrolled, k_leaves)

    def fb():
        for t in k_leaves:
            t.grad = None
        out = rec()
        torch.autograd.backward((out[0], out[1]), (gw, gc))

    info = fwd()[3]
    assert info[:, 0].tolist() == [PRM["max_iter"]] * B and info[:, 1].tolist() == [PRM["max_iter"] * K * PRM["epoch"]] * B and not bool(info[:, 3].any()), \
        "every molecule must run all its iterations and epochs, unflagged"
    fb()
    agree, t_leaves = float("nan"), None
    if with_torch:
        try:
            t_leaves = [leaf(t, torch.float64) for t in (Ys, Cs, ps, p, lam)]
            torch_loss(*t_leaves, gw.double(), gc.double(), PRM["alpha"], PRM["rho"], PRM["max_iter"], PRM["epoch"]).backward()
            rel = lambda x, y: float((x.double() - y).norm() / y.norm())
            agree = max(rel(k.grad, t.grad) for k, t in zip(k_leaves, t_leaves))
        except torch.cuda.OutOfMemoryError:
            t_leaves = None
            torch.cuda.empty_cache()

    def tor():
        for t in t_leaves:
            t.grad = None
        torch_loss(*t_leaves, gw.double(), gc.double(), PRM["alpha"], PRM["rho"], PRM["max_iter"], PRM["epoch"]).backward()

    f_ms, r_ms, b_ms, t_ms = [], [], [], []
    for _ in range(repeats):
        f_ms.append(timed(fwd))
        r_ms.append(timed(rec))
        b_ms.append(timed(fb))
        if t_leaves is not None:
            t_ms.append(timed(tor, min(runs, 3)))
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    rep = lambda v: " ".join(f"{x:.3f}" for x in v) if v else "n/a"
    f, r, fbm = med(f_ms), med(r_ms), med(b_ms)
    t_txt = f"{med(t_ms):10.3f}  {med(t_ms) / fbm:17.2f}" if t_ms else f"{'n/a':>10s}  {'n/a':>17s}"
    print(f"B={B:<4d}K={K:<2d}N={N:<3d}d={d:<3d}  {f:9.3f} {r:9.3f}  {fbm:10.3f}  {fbm - r:7.3f}  {(fbm - r) / f:7.2f}  {t_txt}  {agree:.2e}  {spread(f_ms):10.4f}  "
          f"{spread(r_ms):.4f}  {spread(b_ms):.4f}  {rep(f_ms)} | {rep(r_ms)} | {rep(b_ms)} | {rep(t_ms)}")
    if parent_lib:
        L = _lib.lib()
        prm = _lib.FgwParams(PRM["alpha"], 0.0, PRM["max_iter"], PRM["tol"], 0.0, 1, 0.0, 0, 0, 0, 0, 0)
        Y = torch.empty(B, N, d, device=dev); C = torch.empty(B, N, N, device=dev); T = torch.empty(B, K, N, N, device=dev)
        info = torch.empty(B, 4, dtype=torch.int32, device=dev); errs = torch.empty(B, 2, PRM["max_iter"], device=dev)
        ws = torch.empty(int(L.conan_fgw_mixup_workspace_bytes(B, K, N, d)), dtype=torch.uint8, device=dev)
        P = ctypes.CDLL(os.path.abspath(parent_lib))
        P.conan_fgw_mixup_barycenter_fwd.restype, P.conan_fgw_mixup_barycenter_fwd.argtypes = _lib.SIGNATURES["conan_fgw_mixup_barycenter_fwd"]
        args = (Ys.data_ptr(), Cs.data_ptr(), ps.data_ptr(), p.data_ptr(), lam.data_ptr(), None, None, B, K, N, d, ctypes.byref(prm), PRM["rho"], PRM["epoch"],
                PRM["eps"], Y.data_ptr(), C.data_ptr(), T.data_ptr(), None, info.data_ptr(), errs.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
        outs = []
        for lib_ in (L, P):
            assert lib_.conan_fgw_mixup_barycenter_fwd(*args) == 0
            torch.cuda.synchronize()
            outs.append((Y.clone(), C.clone(), T.clone()))
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*outs)), "the forward's bits moved against the parent library"
        m_ms, p_ms = [], []
        for _ in range(repeats):
            m_ms.append(timed(lambda: L.conan_fgw_mixup_barycenter_fwd(*args)))
            p_ms.append(timed(lambda: P.conan_fgw_mixup_barycenter_fwd(*args)))
        print(f"parent  B={B:<4d}K={K:<2d}N={N:<3d}  {med(m_ms):9.3f}  {med(p_ms):13.3f}  {(med(m_ms) - med(p_ms)) / med(p_ms):+10.4f}  {spread(m_ms):11.4f}  "
              f"{spread(p_ms):6.4f}  {rep(m_ms)} | {rep(p_ms)}")
    print(f"# device: {torch.cuda.get_device_name(0)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds a shape's process may take")
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help="worker: measure this shape in this process")
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: its forward is timed beside this one's")
    ap.add_argument("--no-torch", action="store_true", help="leave out the torch fp64 autograd side")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.shape:
        return worker(args.shape, args.runs, args.warmup, args.repeats, args.parent_lib, not args.no_torch)
    lines = [f"# tools/probe_fgw_mixup_unrolled.py: {' '.join(f'{k} {v}' for k, v in PRM.items())}; median of {args.runs} calls, {args.repeats} repeats, ms", HEAD]
    device = ""
    for name in ("cfg2", "bace"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--shape", name, "--runs", str(args.runs),
               "--warmup", str(args.warmup), "--repeats", str(args.repeats)] + (["--parent-lib", args.parent_lib] if args.parent_lib else []) \
            + (["--no-torch"] if args.no_torch else [])
        print(f"# measuring {name} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:          # a failure ends the probe: nothing more is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"probe_fgw_mixup_unrolled: shape {name} ended with status {r.returncode}; stopping")
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
