"""Every pair kernel of the general coupling solves once, for kernel timing:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/probe_fgw_pair_modes.py

ops.fgw_pair_batched with B = 64 at N = 33 / 80 / 133 — LDS modes 2 / 1 / 0 of k_fgw_coupling_pair; k_fgw_coupling_bapg_pair in LDS (33) and in
the scratch (80, 133) — for PGD, PPA and BAPG, symmetric and not, square loss, max_iter 10 with a tol that never stops it: 7 calls each, the
per-kernel durations come from the kernel trace.  The script prints the iteration counts."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conan_fgw_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
B = 64


def main():
    for N in (33, 80, 133):
        rng = np.random.RandomState(N)
        M = t(rng.uniform(0.0, 1.0, size=(B, N, N)))
        a = np.triu(rng.random_sample((B, N, N)) < 0.3, 1)
        Cs = t(a | a.transpose(0, 2, 1))
        Cd = t((rng.random_sample((B, N, N)) < 0.3) & ~np.eye(N, dtype=bool))
        for solver, sym, eps in (("PGD", True, 0.1), ("PPA", True, 0.1), ("PGD", False, 0.1), ("PPA", False, 0.1), ("BAPG", True, 1.0), ("BAPG", False, 1.0)):
            C = Cs if sym else Cd
            for _ in range(7):
                o = ops.fgw_pair_batched(M, C, C.flip(0).contiguous(), solver=solver, symmetric=sym, epsilon=eps, alpha=0.5, max_iter=10, tol=1e-9)
            torch.cuda.synchronize()
            print(f"N={N} {solver:4s} symmetric={sym!s:5s} iterations={int(o[2][:, 0].sum())}", flush=True)


if __name__ == "__main__":
    main()
