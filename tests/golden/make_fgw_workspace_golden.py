"""Generates tests/golden/fgw_workspace_bytes.npz: what the FGW workspace size query of a built libconan_fgw_hip.so returns over a grid of
shapes, structure forms, solvers and symmetric codes, plus the refused codes.  Needs no GPU and no reference: the queries are host arithmetic.

The file pins the public numbers across changes of the host code (tests/test_fgw_workspace_cpu.py), so it is generated from the library of the
commit BEFORE such a change, never from the code under test:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fgw_workspace_golden.py [path/to/libconan_fgw_hip.so [output directory]]

The keys date from the four queries the library once had: `dense` / `ragged` are ragged = 0 / 1 with solver 0 and symmetric 1, `sym` /
`ragged_sym` are ragged = 0 / 1 over the (solver, symmetric) codes.
"""
import ctypes
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SO = os.path.join(os.path.dirname(os.path.dirname(HERE)), "conan-fgw_amd", "libconan_fgw_hip.so")

BS, KS, NS, DS = (1, 4, 104, 256), (1, 3, 5, 20), (1, 7, 33, 64, 65, 90, 132), (3, 64, 128)
SOLVERS, SYMMETRICS = (0, 1, 2), (1, 0, -1)
BAD_CODES = ((0, 2), (1, -2), (3, 0), (-1, 1), (3, 2))            # (solver, symmetric) the query refuses
BAD_DIMS = ((0, 5, 33, 64), (4, 0, 33, 64), (4, 5, 0, 64), (4, 5, 33, 0), (-1, 5, 33, 64), (4, 5, -7, 64))


def queries(so):
    L = ctypes.CDLL(so)
    fn = L.conan_fgw_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_longlong, [ctypes.c_int] * 7
    return {"dense": lambda *dims: fn(*dims, 0, 0, 1), "ragged": lambda *dims: fn(*dims, 1, 0, 1),
            "sym": lambda B, K, N, d, s, y: fn(B, K, N, d, 0, s, y), "ragged_sym": lambda B, K, N, d, s, y: fn(B, K, N, d, 1, s, y)}


def record(so):
    q = queries(so)
    dims = np.array(list(itertools.product(BS, KS, NS, DS)), dtype=np.int64)
    codes = list(itertools.product(SOLVERS, SYMMETRICS))
    both = lambda fn, rows, cds: np.array([[fn(*map(int, r), s, y) for s, y in cds] for r in rows], dtype=np.int64)
    plain = lambda fn, rows: np.array([fn(*map(int, r)) for r in rows], dtype=np.int64)
    return dict(dims=dims, codes=np.array(codes, dtype=np.int64), bad_codes=np.array(BAD_CODES, dtype=np.int64),
                bad_dims=np.array(BAD_DIMS, dtype=np.int64),
                dense=plain(q["dense"], dims), ragged=plain(q["ragged"], dims),
                sym=both(q["sym"], dims, codes), ragged_sym=both(q["ragged_sym"], dims, codes),
                sym_bad_codes=both(q["sym"], dims, BAD_CODES), ragged_sym_bad_codes=both(q["ragged_sym"], dims, BAD_CODES),
                dense_bad_dims=plain(q["dense"], BAD_DIMS), ragged_bad_dims=plain(q["ragged"], BAD_DIMS),
                sym_bad_dims=both(q["sym"], BAD_DIMS, codes), ragged_sym_bad_dims=both(q["ragged_sym"], BAD_DIMS, codes))


if __name__ == "__main__":
    so = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_SO
    rec = record(so)
    np.savez_compressed(os.path.join(sys.argv[2] if len(sys.argv) > 2 else HERE, "fgw_workspace_bytes.npz"), **rec)
    print(f"{len(rec['dims'])} shapes x {len(rec['codes'])} codes from {so}")
