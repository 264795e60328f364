"""What does the unrolled pairwise FGW gradient (ops.fgw_pair_unrolled, conan_fgw_pair_bwd) cost next to its forward, and next to torch autograd
through the same iterations?

    python tools/probe_fgw_pair_unrolled.py [--runs 10] [--warmup 2] [--repeats 3] [--parent-lib PATH] [--out profiles/fgw_pair_unrolled_probe.txt]

The shapes of profiles/fgw_acc_grad_probe.txt as pairs: cfg2's couplings (B = 256 * 5 = 1280 pairs of N = 33 nodes) and BACE's (B = 64 * 3 = 192
pairs of N = 90: above the residency bound, the matrices are streamed), each with 5 outer iterations of 5 sweeps (the models' literals: alpha
0.1, epsilon 0.1) and with 30 x 100 (alpha 0.5, epsilon 0.1).  tol = 0 and stop_thr = 0, so that every pair runs every iteration and every sweep on
every side and the sides do the same work.  Inputs are seeded: squared distances of features uniform in [0.1, 1.1] (d = 16), random undirected
graphs of density 0.3, random normalised weights.  Per row, HIP events around the call after warm-up, the median of --runs calls, --repeats
times with the sides interleaved (all repeats are printed; a row's figure is their median, its spread (max - min) / median):

    fwd_ms        ops.fgw_pair_batched: the forward alone
    fwd+bwd_ms    ops.fgw_pair_unrolled with M, C1, C2, p, q as leaves, then ONE backward for the cotangents of T and fgw_dist
    bwd_ms        the difference; bwd/fwd stands next to the product count: the symmetric walk does 7 N^3-sized products per outer iteration (2 of
                  them the replay's, again) + the replay's own 2 against the forward's 2, and about four Sinkhorn solves' worth of matrix-vector
                  passes (replay, again in the walk, and the reverse sweeps at two passes each) against the forward's one
    torch64_ms    the same iterations (scaling-form Sinkhorn from u = 1, so that autograd keeps vectors, not matrices, per sweep), the same
                  distance and loss.backward() as batched fp64 torch ops on the same GPU: what a user would otherwise run to get this gradient
    agree         the largest relative Frobenius distance between the op's gradients and torch's (fp32 outputs of an fp64 iteration: 1e-7)

With --parent-lib (a libconan_fgw_hip.so built from the parent commit) a second table times conan_fgw_pair_fwd of both libraries through ctypes
on the same buffers, interleaved, and compares the bits of T, fgw_dist, info and errs: the existing forward must not move.  (conan_sinkhorn_bwd
is not in that table: its reverse sweeps were not moved, csrc/sinkhorn_grad.hip is the parent's file.)  No threshold is set: the figures are
stated.

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
ITERS = {"5x5": dict(alpha=0.1, epsilon=0.1, max_iter=5, num_iter_max=5), "30x100": dict(alpha=0.5, epsilon=0.1, max_iter=30, num_iter_max=100)}
ROWS = [f"{s}:{i}" for i in ITERS for s in SHAPES]
HEAD = "row                       fwd_ms  fwd+bwd_ms   bwd_ms  bwd/fwd  torch64_ms  torch64/(fwd+bwd)  agree     spread fwd  fwd+bwd  repeats fwd | fwd+bwd | torch64"
PARENT_HEAD = "parent  row                this_fwd_ms  parent_fwd_ms  difference  bits   spread this  parent  repeats this | parent"


def torch_loss(M, C1, C2, p, q, W, alpha, eps, max_iter, num_iter_max):
    """sum(W * T) + sum(fgw_dist) after max_iter PGD iterations of num_iter_max sweeps from p q^T, every pair at once, in the dtype of the inputs."""
    import torch
    T = p[:, :, None] * q[:, None, :]
    c, r = ((C1 * C1) @ p[:, :, None]), (q[:, None, :] @ (C2 * C2).transpose(1, 2))
    const = c + r
    C2t = C2.transpose(1, 2)
    for _ in range(max_iter):
        tens = 2 * alpha * const - 4 * alpha * (C1 @ T @ C2t) + (1 - alpha) * M
        Mr = -tens / eps
        K = torch.exp(Mr - Mr.max(1, keepdim=True).values.detach())
        u = torch.ones_like(p)
        for _ in range(num_iter_max):
            v = q / (K.transpose(1, 2) @ u[:, :, None])[:, :, 0]
            u = p / (K @ v[:, :, None])[:, :, 0]
        T = u[:, :, None] * K * v[:, None, :]
    dist = ((1 - alpha) * M * T).sum((1, 2)) + alpha * ((const - 2 * (C1 @ T @ C2t)) * T).sum((1, 2))
    return (W * T).sum() + dist.sum()


def worker(row, runs, warmup, repeats, parent_lib):
    import torch
    sys.path.insert(0, ROOT)
    from conan_fgw_amd import _lib, ops
    assert torch.cuda.is_available(), "the probe needs a GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    shape, it = row.split(":")
    B, N, d = SHAPES[shape]
    prm = dict(ITERS[it], tol=0.0, stop_thr=0.0, solver="PGD", symmetric=True)
    g = torch.Generator().manual_seed(3000 + N)
    y, z = torch.rand(B, N, d, generator=g) + 0.1, torch.rand(B, N, d, generator=g) + 0.1
    M = ((y[:, :, None, :] - z[:, None, :, :]) ** 2).sum(-1).to(dev)

    def graphs():
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
        return ops.fgw_pair_batched(M, C1, C2, p, q, **prm)

    def fb():
        for t in k_leaves:
            t.grad = None
        T, dist, _info, _errs = ops.fgw_pair_unrolled(*k_leaves, **prm)
        torch.autograd.backward((T, dist), (W, ones))

    def tor():
        for t in t_leaves:
            t.grad = None
        torch_loss(*t_leaves, W64, prm["alpha"], prm["epsilon"], prm["max_iter"], prm["num_iter_max"]).backward()

    info = fwd()[2]
    want = (prm["max_iter"], prm["max_iter"] * prm["num_iter_max"])
    assert (int(info[:, 0].min()), int(info[:, 0].max())) == (want[0],) * 2 and (int(info[:, 1].min()), int(info[:, 1].max())) == (want[1],) * 2, "every pair must run every sweep"
    assert not bool((info[:, 2] != 0).any()), "a pair is flagged"
    fb(); tor()
    rel = lambda x, y: float((x.double() - y).norm() / y.norm())
    agree = max(rel(k.grad, t.grad) for k, t in zip(k_leaves, t_leaves))
    t_runs = runs if it == "5x5" else max(2, runs // 4)                     # (thousands of small launches per call at 30 x 100)
    f_ms, b_ms, t_ms = [], [], []
    for _ in range(repeats):
        f_ms.append(timed(fwd))
        b_ms.append(timed(fb))
        t_ms.append(timed(tor, t_runs))
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    rep = lambda v: " ".join(f"{x:.3f}" for x in v)
    f, fbm, t = med(f_ms), med(b_ms), med(t_ms)
    label = f"B={B:<5d}N={N:<3d}{it:>7s}"
    print(f"{label:<22s}  {f:9.3f}  {fbm:10.3f}  {fbm - f:7.3f}  {(fbm - f) / f:7.2f}  {t:10.3f}  {t / fbm:17.2f}  {agree:.2e}  {spread(f_ms):10.4f}  {spread(b_ms):7.4f}  "
          f"{rep(f_ms)} | {rep(b_ms)} | {rep(t_ms)}")
    if parent_lib:
        L = _lib.lib()
        P = ctypes.CDLL(os.path.abspath(parent_lib))
        P.conan_fgw_pair_fwd.restype, P.conan_fgw_pair_fwd.argtypes = _lib.SIGNATURES["conan_fgw_pair_fwd"]
        fprm, solver_code, sym_code = ops._pair_params(prm["alpha"], prm["epsilon"], prm["max_iter"], prm["tol"], prm["num_iter_max"], prm["stop_thr"], "square_loss",
                                                       prm["solver"], prm["symmetric"])
        T = torch.empty(B, N, N, device=dev)
        dist = torch.empty(B, device=dev)
        info = torch.empty(B, 4, dtype=torch.int32, device=dev)
        errs = torch.empty(B, (prm["max_iter"] + 9) // 10, device=dev)
        ws = torch.empty(int(L.conan_fgw_pair_workspace_bytes(B, N, solver_code, sym_code)), dtype=torch.uint8, device=dev)
        args = (M.data_ptr(), C1.data_ptr(), C2.data_ptr(), p.data_ptr(), q.data_ptr(), None, B, N, ctypes.byref(fprm), solver_code, sym_code, T.data_ptr(),
                dist.data_ptr(), info.data_ptr(), errs.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
        outs = []
        for lib_ in (L, P):
            for t in (T, dist, errs):
                t.fill_(-1.0)
            info.fill_(-1)
            assert lib_.conan_fgw_pair_fwd(*args) == 0
            torch.cuda.synchronize()
            outs.append([t.clone().view(torch.int32) for t in (T, dist, info, errs)])
        same = all(torch.equal(a, b) for a, b in zip(*outs))
        m_ms, p_ms = [], []
        for _ in range(repeats):
            m_ms.append(timed(lambda: L.conan_fgw_pair_fwd(*args)))
            p_ms.append(timed(lambda: P.conan_fgw_pair_fwd(*args)))
        print(f"parent  {label:<22s}  {med(m_ms):9.3f}  {med(p_ms):13.3f}  {(med(m_ms) - med(p_ms)) / med(p_ms):+10.4f}  {'same' if same else 'DIFFER':6s}  {spread(m_ms):9.4f}  "
              f"{spread(p_ms):6.4f}  {rep(m_ms)} | {rep(p_ms)}")
        assert same, "the forward's bits moved against the parent library"
    print(f"# device: {torch.cuda.get_device_name(0)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=200, help="seconds a row's process may take")
    ap.add_argument("--row", choices=ROWS, default=None, help="worker: measure this row in this process")
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: its forward is timed beside this one's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.row:
        return worker(args.row, args.runs, args.warmup, args.repeats, args.parent_lib)
    lines = [f"# tools/probe_fgw_pair_unrolled.py: PGD, symmetric, tol 0, stop_thr 0; median of {args.runs} calls, {args.repeats} repeats, ms", HEAD]
    device = ""
    for row in ROWS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--row", row, "--runs", str(args.runs),
               "--warmup", str(args.warmup), "--repeats", str(args.repeats)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
        print(f"# measuring {row} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:          # a failure ends the probe: nothing more is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"probe_fgw_pair_unrolled: row {row} ended with status {r.returncode}; stopping")
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
