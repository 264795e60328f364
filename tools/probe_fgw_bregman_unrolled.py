"""What does the unrolled BAPG pairwise FGW gradient (ops.fgw_bregman_unrolled, conan_fgw_bregman_bwd) cost next to its forward, and next to torch
autograd through the same iterations?

    python tools/probe_fgw_bregman_unrolled.py [--runs 5] [--warmup 1] [--repeats 3] [--parent-lib PATH] [--ab-lib PATH]
                                               [--out profiles/fgw_bregman_unrolled_probe.txt]

The method of tools/probe_fgw_pair_unrolled.py.  Shapes: cfg2's couplings (B = 256 * 5 = 1280 pairs of N = 33 nodes, LDS-resident) and BACE's
(B = 64 * 3 = 192 pairs of N = 90: above the residency bound, the matrices are streamed), max_iter = 100, alpha 0.5, epsilon 1, symmetric, for
the square loss (random undirected graphs of density 0.3) and kl (positive symmetric structures, uniform in [0.05, 1]).  tol = 0, so that every
pair runs every iteration on every side.  Inputs are seeded: squared distances of features uniform in [0.1, 1.1] (d = 16), random normalised
weights.  Per row, HIP events around the call after warm-up, the median of --runs calls, --repeats times with the sides interleaved (all
repeats are printed; a row's figure is their median, its spread (max - min) / median):

    fwd_ms        ops.fgw_pair_batched(solver="BAPG"): the forward alone
    fwd+bwd_ms    ops.fgw_bregman_unrolled with M, C1, C2, p, q as leaves, then ONE backward for the cotangents of T and fgw_dist
    bwd_ms        the difference; bwd/fwd stands next to the product count: per half-step the forward does 2 N^3-sized products, the backward
                  2 (replay) + 2 (X again) + 4 (walk) = 8 in the symmetric form, all in one workgroup per pair as the forward's
    torch64_ms    the same half-steps, the same distance and loss.backward() as batched fp64 torch ops on the same GPU: what a user would
                  otherwise run to get this gradient
    agree         the largest relative Frobenius distance between the op's gradients and torch's (fp32 outputs of an fp64 iteration: 1e-7)

With --parent-lib (a libconan_fgw_hip.so built from the parent commit) a second table times conan_fgw_pair_fwd with solver BAPG of both
libraries through ctypes on the same buffers, interleaved, and compares the bits of T, fgw_dist, info and errs: the existing forward must not
move.  With --ab-lib (this library built with another register bound: -DCONAN_BREGMAN_BWD_BLOCKS_LDS=.. / -DCONAN_BREGMAN_BWD_BLOCKS_STREAMED=..)
a third table times conan_fgw_bregman_bwd ALONE of both builds, interleaved, on the same buffers.  No threshold is set: the figures are stated.

Every row runs in a process of its own under `timeout -k 10` (this script is the driver; --row NAME is the worker), and the driver stops at the
first row that fails."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg2": (1280, 33, 16), "bace": (192, 90, 16)}
LOSSES = ("square_loss", "kl_loss")
ROWS = [f"{s}:{l}" for l in LOSSES for s in SHAPES]
PRM = dict(alpha=0.5, epsilon=1.0, max_iter=100, tol=0.0, symmetric=True)
HEAD = "row                          fwd_ms  fwd+bwd_ms   bwd_ms  bwd/fwd  torch64_ms  torch64/(fwd+bwd)  agree     spread fwd  fwd+bwd  repeats fwd | fwd+bwd | torch64"
PARENT_HEAD = "parent  row                   this_fwd_ms  parent_fwd_ms  difference  bits   spread this  parent  repeats this | parent"
AB_HEAD = "ab      row                   this_bwd_ms  other_bwd_ms   difference  bits   spread this  other   repeats this | other"


def torch_loss(M, C1, C2, p, q, W, alpha, eps, max_iter, kl):
    """sum(W * T) + sum(fgw_dist) after max_iter BAPG iterations (symmetric form) from p q^T, every pair at once, in the dtype of the inputs."""
    import torch
    T = p[:, :, None] * q[:, None, :]
    h = torch.log(C2 + 1e-15) if kl else 2 * C2
    ht = h.transpose(1, 2)
    for _ in range(max_iter):
        T = T * torch.exp(-(-2 * alpha * (C1 @ T @ ht) + (1 - alpha) * M) / eps)
        T = (p / T.sum(2))[:, :, None] * T
        T = T * torch.exp(-(-2 * alpha * (C1 @ T @ ht) + (1 - alpha) * M) / eps)
        T = T * (q / T.sum(1))[:, None, :]
    f1, f2 = (C1 * torch.log(C1 + 1e-15) - C1, C2) if kl else (C1 * C1, C2 * C2)
    const = (f1 @ p[:, :, None]) + (q[:, None, :] @ f2.transpose(1, 2))
    dist = ((1 - alpha) * M * T).sum((1, 2)) + alpha * ((const - C1 @ T @ ht) * T).sum((1, 2))
    return (W * T).sum() + dist.sum()


def worker(row, runs, warmup, repeats, parent_lib, ab_lib):
    import torch
    sys.path.insert(0, ROOT)
    from conan_fgw_amd import _lib, ops
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    shape, loss = row.split(":")
    kl = loss == "kl_loss"
    B, N, d = SHAPES[shape]
    prm = dict(PRM, loss_fun=loss)
    g = torch.Generator().manual_seed(3000 + N)
    y, z = torch.rand(B, N, d, generator=g) + 0.1, torch.rand(B, N, d, generator=g) + 0.1
    M = ((y[:, :, None, :] - z[:, None, :, :]) ** 2).sum(-1).to(dev)

    def graphs():
        if kl:
            c = 0.05 + 0.95 * torch.rand(B, N, N, generator=g)
            return (0.5 * (c + c.transpose(1, 2))).to(dev)
        u = torch.triu((torch.rand(B, N, N, generator=g) < 0.3).float(), 1)
        return (u + u.transpose(1, 2)).to(dev)

    def weights():
        w = torch.rand(B, N, generator=g) + 0.5
        return (w / w.sum(1, keepdim=True)).to(dev)
    C1, C2, p, q = graphs(), graphs(), weights(), weights()
    W = torch.randn(B, N, N, generator=g).to(dev)
    ones = torch.ones(B, device=dev)

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
    k_leaves = [leaf(t) for t in (M, C1, C2, p, q)]
    t_leaves = [leaf(t, torch.float64) for t in (M, C1, C2, p, q)]
    W64 = W.double()

    def fwd():
        return ops.fgw_pair_batched(M, C1, C2, p, q, solver="BAPG", **prm)

    def fb():
        for t in k_leaves:
            t.grad = None
        T, dist, _info, _errs = ops.fgw_bregman_unrolled(*k_leaves, **prm)
        torch.autograd.backward((T, dist), (W, ones))

    def tor():
        for t in t_leaves:
            t.grad = None
        torch_loss(*t_leaves, W64, prm["alpha"], prm["epsilon"], prm["max_iter"], kl).backward()

    info = fwd()[2]
    assert (int(info[:, 0].min()), int(info[:, 0].max())) == (prm["max_iter"],) * 2, "every pair must run every iteration"
    assert not bool((info[:, 2] != 0).any()), "a pair is flagged"
    fb(); tor()
    rel = lambda x, y: float((x.double() - y).norm() / y.norm())
    agree = max(rel(k.grad, t.grad) for k, t in zip(k_leaves, t_leaves))
    f_ms, b_ms, t_ms = [], [], []
    for _ in range(repeats):
        f_ms.append(timed(fwd))
        b_ms.append(timed(fb))
        t_ms.append(timed(tor, max(2, runs // 2)))
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    rep = lambda v: " ".join(f"{x:.3f}" for x in v)
    f, fbm, t = med(f_ms), med(b_ms), med(t_ms)
    label = f"B={B:<5d}N={N:<3d}{loss.split('_')[0]:>7s}"
    print(f"{label:<25s}  {f:9.3f}  {fbm:10.3f}  {fbm - f:7.3f}  {(fbm - f) / f:7.2f}  {t:10.3f}  {t / fbm:17.2f}  {agree:.2e}  {spread(f_ms):10.4f}  {spread(b_ms):7.4f}  "
          f"{rep(f_ms)} | {rep(b_ms)} | {rep(t_ms)}")
    L = _lib.lib()
    fprm, solver_code, sym_code = ops._pair_params(prm["alpha"], prm["epsilon"], prm["max_iter"], prm["tol"], 1, 1e-9, loss, "BAPG", True)
    T = torch.empty(B, N, N, device=dev)
    dist = torch.empty(B, device=dev)
    info = torch.empty(B, 4, dtype=torch.int32, device=dev)
    errs = torch.empty(B, (prm["max_iter"] + 9) // 10, device=dev)
    ws = torch.empty(int(L.conan_fgw_pair_workspace_bytes(B, N, solver_code, sym_code)), dtype=torch.uint8, device=dev)
    fargs = (M.data_ptr(), C1.data_ptr(), C2.data_ptr(), p.data_ptr(), q.data_ptr(), None, B, N, ctypes.byref(fprm), solver_code, sym_code, T.data_ptr(),
             dist.data_ptr(), info.data_ptr(), errs.data_ptr(), ws.data_ptr(), _lib.stream_ptr())

    def versus(tag, other, name, sig, args, outs_of, reset):
        other = ctypes.CDLL(os.path.abspath(other))
        getattr(other, name).restype, getattr(other, name).argtypes = sig
        outs = []
        for lib_ in (L, other):
            reset()
            assert getattr(lib_, name)(*args) == 0
            torch.cuda.synchronize()
            outs.append([t.clone().view(torch.int32) for t in outs_of])
        same = all(torch.equal(a, b) for a, b in zip(*outs))
        m_ms, o_ms = [], []
        for _ in range(repeats):
            m_ms.append(timed(lambda: getattr(L, name)(*args)))
            o_ms.append(timed(lambda: getattr(other, name)(*args)))
        print(f"{tag:<6s}  {label:<25s}  {med(m_ms):9.3f}  {med(o_ms):13.3f}  {(med(m_ms) - med(o_ms)) / med(o_ms):+10.4f}  {'same' if same else 'DIFFER':6s}  {spread(m_ms):9.4f}  "
              f"{spread(o_ms):6.4f}  {rep(m_ms)} | {rep(o_ms)}")
        return same

    def reset_fwd():
        for t in (T, dist, errs):
            t.fill_(-1.0)
        info.fill_(-1)

    if parent_lib:
        assert versus("parent", parent_lib, "conan_fgw_pair_fwd", _lib.SIGNATURES["conan_fgw_pair_fwd"], fargs, (T, dist, info, errs), reset_fwd), \
            "the forward's bits moved against the parent library"
    if ab_lib:
        assert L.conan_fgw_pair_fwd(*fargs) == 0
        outs = [torch.empty(B, N, N, device=dev) for _ in range(3)] + [torch.empty(B, N, device=dev) for _ in range(2)]
        bws = torch.empty(int(L.conan_fgw_bregman_bwd_workspace_bytes(B, N, prm["max_iter"])), dtype=torch.uint8, device=dev)
        bargs = (M.data_ptr(), C1.data_ptr(), C2.data_ptr(), p.data_ptr(), q.data_ptr(), None, B, N, prm["alpha"], prm["epsilon"], prm["max_iter"], int(kl), 1,
                 info.data_ptr(), W.data_ptr(), ones.data_ptr(), *(t.data_ptr() for t in outs), None, None, None, bws.data_ptr(), _lib.stream_ptr())
        versus("ab", ab_lib, "conan_fgw_bregman_bwd", _lib.EXT_TABLES["conan_fgw_hip_bregman_grad.h"]["conan_fgw_bregman_bwd"], bargs, outs,
               lambda: [t.fill_(-1.0) for t in outs])
    print(f"# device: {torch.cuda.get_device_name(0)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=200, help="seconds a row's process may take")
    ap.add_argument("--row", choices=ROWS, default=None, help="worker: measure this row in this process")
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: its BAPG forward is timed beside this one's")
    ap.add_argument("--ab-lib", default=None, help="this library built with another register bound: its backward launch is timed beside this one's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.row:
        return worker(args.row, args.runs, args.warmup, args.repeats, args.parent_lib, args.ab_lib)
    lines = [f"# tools/probe_fgw_bregman_unrolled.py: BAPG, symmetric, max_iter 100, tol 0; median of {args.runs} calls, {args.repeats} repeats, ms", HEAD]
    device = ""
    for row in ROWS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--row", row, "--runs", str(args.runs),
               "--warmup", str(args.warmup), "--repeats", str(args.repeats)] + (["--parent-lib", args.parent_lib] if args.parent_lib else []) + \
              (["--ab-lib", args.ab_lib] if args.ab_lib else [])
        print(f"# measuring {row} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:          # a failure ends the probe: nothing more is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"probe_fgw_bregman_unrolled: row {row} ended with status {r.returncode}; stopping")
        out = r.stdout.strip().splitlines()
        lines += [l for l in out if not l.startswith("# device")]
        device = next((l for l in out if l.startswith("# device")), device)
    tables = []
    for tag, head in (("parent", PARENT_HEAD), ("ab", AB_HEAD)):
        rows = [l for l in lines if l.startswith(tag + " ")]
        tables += ([head] + rows) if rows else []
    lines = [l for l in lines if not l.startswith(("parent ", "ab "))] + tables
    lines.insert(1, device)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
