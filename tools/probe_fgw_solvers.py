"""One barycenter solve per coupling solver (PGD / PPA / BAPG) at the cfg2 shape (B=256, K=5, N=33, d=64, the models' radius graphs) and at a
BACE-shaped batch (B=64, K=5, N=90), for kernel timing:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/probe_fgw_solvers.py

Each configuration runs twice (a warm-up, then the timed solve); the per-kernel durations come from the kernel trace (k_fgw_coupling_fast /
_big for PGD, k_fgw_coupling<..., PPA = true> for PPA, k_fgw_coupling_bapg for BAPG).  The script itself prints the wall time of the timed
solve (torch.cuda events) and its iteration counts.  BAPG runs at epsilon = 2.0: at the models' 0.1 it is NaN, in the reference as here.
Every solver runs with symmetric=True and then with symmetric=False (k_fgw_coupling<..., ASYM = true> for PGD / PPA,
k_fgw_coupling_bapg<..., ASYM = true> for BAPG) on the same, symmetric, input: the cost of the second product and of the general kernel
for PGD.  `--sym-only` runs the symmetric=False solves alone."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd import ops  # noqa: E402
from conan_fgw_amd.synthetic import make_batch  # noqa: E402

dev = torch.device("cuda:0")


def batch(shape, B, K):
    b = make_batch(shape, B, K, seed=77)
    pos = torch.from_numpy(b.pos).to(dev); bt = torch.from_numpy(b.batch).to(dev)
    g = ops.RadiusGraph(pos, ops.graph_ptr_from_batch(bt, b.num_graphs), b.num_graphs, 10.0 if shape == "esol" else 5.0, 32)
    torch.manual_seed(3)
    feat = torch.nn.functional.softplus(torch.randn(len(b.z), 64, device=dev))
    Ys, _ = ops.fgw_densify(feat, g, b.max_nodes, 0.5)
    return Ys.view(B, K, b.max_nodes, 64), g


def main():
    for shape, B, K in (("esol", 256, 5), ("bace", 64, 5)):
        Ys, g = batch(shape, B, K)
        runs = [(solver, kw, sym) for sym in (True, False) for solver, kw in (("PGD", {}), ("PPA", {}), ("BAPG", {"epsilon": 2.0}))]
        for solver, kw, sym in runs:      # (BAPG is NaN at the models' epsilon = 0.1)
            if sym and "--sym-only" in sys.argv:
                continue
            kw = dict(kw, symmetric=sym)
            ops.fgw_barycenter_batched(Ys, None, adjacency=g, solver=solver, **kw)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = ops.fgw_barycenter_batched(Ys, None, adjacency=g, solver=solver, **kw)
            e1.record()
            torch.cuda.synchronize()
            info = out[3]
            print(f"{shape} B={B} K={K} N={Ys.shape[2]} {solver:5s} symmetric={sym!s:5s} {e0.elapsed_time(e1):8.3f} ms  outer={int(info[:, 0].sum())} "
                  f"inner={int(info[:, 1].sum())} sinkhorn={int(info[:, 2].sum())} flags={int((info[:, 3] & 4).sum() // 4)} molecules with bit 2",
                  flush=True)


if __name__ == "__main__":
    main()
