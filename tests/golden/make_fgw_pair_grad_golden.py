"""Generates tests/golden/fgw_distgrad_*.npz: the gradient of the reference's fgw_dist at a FIXED plan, for the cases of make_fgw_pair_golden.py.

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).  For every fgw_pair_<case>.npz with max(n1, n2) <= 80 it loads that fixture's inputs and
recorded plans and differentiates, with torch autograd through the reference's own init_matrix / gwloss (utils.py:4-59),

    (1 - alpha) * sum(M * T) + alpha * gwloss(*init_matrix(C1, C2, p, q, loss_fun), T)          (bregman.py:163-164)

in M, C1, C2, p, q with T held constant: once in fp64 at r64_T ("r64_dM" ... "r64_dq") and once in fp32 at r32_T ("r32_dM" ... "r32_dq").  Only the
gradients and the case name are stored: the inputs stay in the fgw_pair_ fixture of the same name.  This is NOT what log["fgw_dist"].backward() of the
reference gives (it unrolls the Sinkhorn sweeps into the graph); it is the gradient conan_fgw_pair_dist_bwd computes.  No reference source is
copied.  Asserted per case: every fp64 gradient is finite, the file stays under 512 KB (why the two N = 140 cases get none).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_pair_grad_golden.py [name ...]
"""
import glob
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

from conan_fgw.src.model.fgw import utils as ref_utils  # noqa: E402

MAX_N = 80
NAMES = ("dM", "dC1", "dC2", "dp", "dq")


def gradients(g, T, dtype):
    leaf = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
    M, C1, C2, p, q = (leaf(g[k]) for k in ("M", "C1", "C2", "p", "q"))
    T = torch.from_numpy(T).to(dtype)
    alpha = float(g["alpha"])
    constC, hC1, hC2 = ref_utils.init_matrix(C1, C2, p, q, str(g["loss_fun"]))
    dist = (1 - alpha) * torch.sum(M * T) + alpha * ref_utils.gwloss(constC, hC1, hC2, T)
    return [x.numpy() for x in torch.autograd.grad(dist, (M, C1, C2, p, q))]


def save(path):
    name = os.path.basename(path)[len("fgw_pair_"):-len(".npz")]
    g = np.load(path)
    if max(g["M"].shape) > MAX_N:
        return
    rec = dict(case=np.array(name))
    for tag, dtype in (("r64", torch.float64), ("r32", torch.float32)):
        for k, v in zip(NAMES, gradients(g, g[f"{tag}_T"], dtype)):
            rec[f"{tag}_{k}"] = v
    assert all(np.isfinite(rec[f"r64_{k}"]).all() for k in NAMES), (name, "an fp64 gradient is not finite")
    out = os.path.join(HERE, f"fgw_distgrad_{name}.npz")
    np.savez_compressed(out, **rec)
    assert os.path.getsize(out) < 512 * 1024, (name, os.path.getsize(out))
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))
    print(f"{name}: {os.path.getsize(out) // 1024} KB " + " ".join(f"rel32({k})={rel(rec['r32_' + k], rec['r64_' + k]):.1e}" for k in NAMES))


def main():
    only = sys.argv[1:]
    for path in sorted(glob.glob(os.path.join(HERE, "fgw_pair_*.npz"))):
        if not only or os.path.basename(path)[len("fgw_pair_"):-len(".npz")] in only:
            save(path)


if __name__ == "__main__":
    main()
