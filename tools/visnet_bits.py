"""The bits the ViSNet edge kernels give, one SHA-256 per case:  python tools/visnet_bits.py [libconan_fgw_hip.so] > listing

Runs the five graph ops whose forward and backward are the 13 edge-walking kernels of csrc/visnet.hip and csrc/visnet_bwd.hip (neighbor_scale,
edge_embed, attn_message, vec_aggregate, edge_update) through the doors the tests use (tests/test_gpu_visnet_ops.py: IMPL / run_gpu), over every
case of visnet_ref.op_cases and over the `wide` graph at H = 32 and 128, and prints one line per (op, graph, H, flags): the SHA-256 over the bytes
of all outputs and all input gradients (rows up to the edge count), and the first 16 digits of the same over the outputs alone and over the
gradients alone, which tell a difference in a forward kernel from one in its backward kernels.  Two builds of the library whose listings are equal compute the same bits;
the sums run in a fixed order, so a change that only moves code must leave every line as it is."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
from conan_fgw_amd import _lib
if len(sys.argv) > 1 and sys.argv[1]:
    _lib._SO = sys.argv[1]
import visnet_ref as R
import test_gpu_visnet_ops as T

OPS = ["neighbor_scale", "edge_embed", "attn_message", "vec_aggregate", "edge_update"]
OUT_WIDTHS = {"attn_message": lambda H: [(H,), (H,)], "vec_aggregate": lambda H: [(3, H)]}


def digest(name, g, H, fl):
    op, gg = R.OPS[name], T.gpu_graph(g)
    G = gg.ref
    gen = torch.Generator().manual_seed(R.case_seed(name, g, H, fl))
    spec = op.make(gen, G, H, fl)
    gouts = [R.rows(gen, G.E if k == "E" else G.n, *w) for k, w in zip(op.out_kinds, OUT_WIDTHS.get(name, lambda H: [(H,)])(H))]
    res = {"ins": [t for t, _, _ in spec], "diff": [d for _, d, _ in spec], "kinds": [k for _, _, k in spec], "gouts": gouts}
    outs, grads, _, _ = T.run_gpu(name, gg, G, H, fl, res)
    whole, parts = hashlib.sha256(), []
    for group in (outs, grads):
        h = hashlib.sha256()
        for t in group:
            b = t.detach().contiguous().cpu().numpy().tobytes()
            whole.update(b)
            h.update(b)
        parts.append(h.hexdigest()[:16])
    return f"{whole.hexdigest()} outputs={parts[0]} gradients={parts[1]}"


def main():
    for name in OPS:
        cases = R.op_cases(name) + [("wide", H, R.flag_cases(name, H, False)[0]) for H in (32, 128)]
        for g, H, fl in cases:
            if name == "attn_message" and R.attn_branch(H, fl["heads"]) in ("badarg", "unsupported"):
                continue
            flags = ",".join(f"{k}={v}" for k, v in fl.items()) or "-"
            print(f"{name} {g} H{H} {flags} {digest(name, g, H, fl)}", flush=True)


if __name__ == "__main__":
    main()
