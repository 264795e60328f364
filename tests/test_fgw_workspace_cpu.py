"""The FGW workspace size query returns exactly the numbers recorded in tests/golden/fgw_workspace_bytes.npz, which
tests/golden/make_fgw_workspace_golden.py took from the library built BEFORE the host driver and the workspace layout were unified
(B x K x N x d x solver x symmetric grid, refused codes and non-positive shapes included; it had four queries then: `dense` / `ragged` are
ragged 0 / 1 with solver 0, symmetric 1, `sym` / `ragged_sym` ragged 0 / 1 over the codes).  Host arithmetic only: no GPU."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fgw_workspace_bytes.npz")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from conan_fgw_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def test_grid_is_the_issue_grid(gold):
    dims = gold["dims"]
    assert [sorted(set(dims[:, c].tolist())) for c in range(4)] == [[1, 4, 104, 256], [1, 3, 5, 20], [1, 7, 33, 64, 65, 90, 132], [3, 64, 128]]
    assert len(dims) == 4 * 4 * 7 * 3
    assert sorted(map(tuple, gold["codes"].tolist())) == sorted((s, y) for s in (0, 1, 2) for y in (1, 0, -1))


def test_dense_and_ragged_queries_match_parent(L, gold):
    for row, dense, ragged in zip(gold["dims"].tolist(), gold["dense"].tolist(), gold["ragged"].tolist()):
        assert dense > 0 and ragged > dense
        assert L.conan_fgw_workspace_bytes(*row, 0, 0, 1) == dense, row
        assert L.conan_fgw_workspace_bytes(*row, 1, 0, 1) == ragged, row


def test_sym_queries_match_parent(L, gold):
    codes = gold["codes"].tolist()
    for row, sym, ragged_sym in zip(gold["dims"].tolist(), gold["sym"].tolist(), gold["ragged_sym"].tolist()):
        for (solver, symmetric), w, wr in zip(codes, sym, ragged_sym):
            assert L.conan_fgw_workspace_bytes(*row, 0, solver, symmetric) == w, (row, solver, symmetric)
            assert L.conan_fgw_workspace_bytes(*row, 1, solver, symmetric) == wr, (row, solver, symmetric)


def test_refused_codes_and_shapes_match_parent(L, gold):
    bad_codes, codes = gold["bad_codes"].tolist(), gold["codes"].tolist()
    assert not gold["sym_bad_codes"].any() and not gold["ragged_sym_bad_codes"].any()
    for row in gold["dims"].tolist():
        for solver, symmetric in bad_codes:
            assert L.conan_fgw_workspace_bytes(*row, 0, solver, symmetric) == 0
            assert L.conan_fgw_workspace_bytes(*row, 1, solver, symmetric) == 0
        for ragged in (-1, 2):
            assert L.conan_fgw_workspace_bytes(*row, ragged, 0, 1) == 0
    for k, row in enumerate(gold["bad_dims"].tolist()):
        assert L.conan_fgw_workspace_bytes(*row, 0, 0, 1) == gold["dense_bad_dims"][k] == 0
        assert L.conan_fgw_workspace_bytes(*row, 1, 0, 1) == gold["ragged_bad_dims"][k] == 0
        for c, (solver, symmetric) in enumerate(codes):
            assert L.conan_fgw_workspace_bytes(*row, 0, solver, symmetric) == gold["sym_bad_dims"][k, c] == 0
            assert L.conan_fgw_workspace_bytes(*row, 1, solver, symmetric) == gold["ragged_sym_bad_dims"][k, c] == 0
