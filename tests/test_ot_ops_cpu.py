"""The optimal-transport host layer as a module of its own (conan_fgw_amd/ot_ops.py): ops.py re-exports it name for name, it loads without
ops.py, and the plumbing its solver families share — the operand checker, the embedding, the unstacking — does what each family relied on (no
GPU: the device check lives in the checker alone, so the other helpers run on CPU tensors)."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

from conan_fgw_amd import ops, ot_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the private names tests, tools and the golden generators reach through ops
PRIVATE = ["_pair_prepare", "_pair_params", "_pair_fwd", "_pair_list_stack", "_pair_unrolled_params", "_acc_prepare", "_acc_fwd",
           "_sinkhorn_list_stack", "_LOSS_CODE"]


def test_all_lists_every_public_function_and_constant():
    own = [n for n, v in vars(ot_ops).items() if not n.startswith("_") and (
        (inspect.isfunction(v) and v.__module__ == ot_ops.__name__) or (n.isupper() and isinstance(v, dict)))]
    assert sorted(own) == sorted(ot_ops.__all__) and "fgw_pair_batched" in own and "SINKHORN_EXT_METHODS" in own


@pytest.mark.parametrize("name", ot_ops.__all__ + PRIVATE)
def test_ops_reexports_the_same_object(name):
    assert getattr(ops, name) is getattr(ot_ops, name)


def test_ops_keeps_the_shared_helpers():
    from conan_fgw_amd import _lib
    assert ops._c is _lib._c is ot_ops._c and (ops.f32, ops.i32, ops.i64) == (torch.float32, torch.int32, torch.int64)


def test_each_module_loads_alone_and_ot_ops_without_ops():
    codes = ["import sys; import conan_fgw_amd.ot_ops; assert 'conan_fgw_amd.ops' not in sys.modules; print('ok')",
             "import sys; import conan_fgw_amd.ops as ops; assert ops.fgw_pair_batched is sys.modules['conan_fgw_amd.ot_ops'].fgw_pair_batched; print('ok')"]
    children = [subprocess.Popen([sys.executable, "-c", c], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for c in codes]
    for child in children:                                       # two fresh interpreters, side by side
        out, err = child.communicate(timeout=120)
        assert child.returncode == 0 and out.strip() == "ok", err


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: takes the checker past its device check, so that its shape check runs without a GPU."""
    is_cuda = True


def _gpu(*shape):
    return torch.zeros(*shape).as_subclass(_OnGpu)


# per family: its prepare function on (M, a square operand, a weight vector), and its names for the last two
FAMILIES = {
    "pairwise FGW": (lambda M, sq, v: ot_ops._pair_prepare(M, sq, sq, v, None, None), "C1", "p"),
    "FGWMixup": (lambda M, sq, v: ot_ops._acc_prepare(M, sq, sq, v, None, None, None, None), "A", "a"),
    "Sinkhorn": (lambda M, sq, v: ot_ops._sinkhorn_prepare(M, v, None, None, None, None, "sinkhorn_log"), None, "a"),
}


@pytest.mark.parametrize("family", FAMILIES)
def test_checker_gives_each_familys_message_for_a_cpu_tensor(family):
    prepare, square, vector = FAMILIES[family]
    with pytest.raises(NotImplementedError) as e:
        prepare(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), None)
    assert str(e.value) == f"the {family} solve runs on the GPU only: M is a CPU tensor"
    with pytest.raises(NotImplementedError) as e:
        prepare(_gpu(2, 4, 4), _gpu(2, 4, 4), torch.zeros(2, 4))
    assert str(e.value) == f"the {family} solve runs on the GPU only: {vector} is a CPU tensor"


@pytest.mark.parametrize("family", FAMILIES)
def test_checker_gives_each_familys_message_for_a_wrong_shape(family):
    prepare, square, vector = FAMILIES[family]
    if square is not None:
        with pytest.raises(ValueError) as e:
            prepare(_gpu(2, 4, 4), _gpu(2, 4, 3), None)
        assert str(e.value) == f"{square} must have shape [2, 4, 4], not [2, 4, 3]"
    with pytest.raises(ValueError) as e:
        prepare(_gpu(1, 4, 4), _gpu(1, 4, 4), _gpu(5))
    assert str(e.value) == (f"{vector} must have shape [1, 4] or [4], not [5]" if family == "Sinkhorn" else f"{vector} must have shape [1, 4], not [5]")
    out = prepare(_gpu(1, 4, 4), _gpu(1, 4, 4), _gpu(1, 4).double())                         # the right shapes pass: fp32, contiguous
    M, v = out[0], out[1 if family == "Sinkhorn" else 3]
    assert M.dtype == v.dtype == torch.float32 and M.is_contiguous() and tuple(v.shape) == (1, 4)


def test_embed_keeps_the_leading_block_and_returns_the_sizes():
    g = torch.Generator().manual_seed(0)
    M, C1, C2 = torch.rand(1, 2, 3, generator=g), torch.rand(1, 2, 2, generator=g), torch.rand(1, 3, 3, generator=g)
    q = torch.tensor([[0.2, 0.3, 0.5]])
    Me, C1e, C2e, p, qe, G0, sizes = ot_ops._pair_embed(M, C1, C2, None, q, None)
    assert sizes == (1, 3, 2, 3) and G0 is None
    assert Me.shape == C1e.shape == C2e.shape == (1, 3, 3) and p.shape == qe.shape == (1, 3)
    assert torch.equal(Me[:, :2, :3], M) and torch.equal(C1e[:, :2, :2], C1) and torch.equal(C2e, C2) and torch.equal(qe, q)
    assert (Me[:, 2:] == 0).all() and (C1e[:, 2:] == 0).all() and (C1e[:, :, 2:] == 0).all()
    assert torch.equal(p, torch.tensor([[0.5, 0.5, 0.0]]))                               # uniform over the own nodes, the extra node massless
    # the FGWMixup family: the same embedding, its own uniform weights (mask / count), own sizes inside a square container
    Ma, A, Bm, a, b, X0, sizes = ot_ops._acc_embed(M, C1, C2, None, q, M.clone(), None, None)
    assert sizes == (1, 3, 2, 3) and torch.equal(Ma, Me) and torch.equal(A, C1e) and torch.equal(Bm, C2e) and torch.equal(X0, Me)
    assert torch.equal(a, torch.tensor([[0.5, 0.5, 0.0]])) and torch.equal(b, q)
    sq = torch.rand(1, 3, 3, generator=g)
    out = ot_ops._acc_embed(sq, sq, sq, None, None, None, torch.tensor([2]), None)
    assert out[6] == (1, 3, 3, 3) and torch.equal(out[3], torch.tensor([[0.5, 0.5, 0.0]])) and torch.equal(out[4], torch.full((1, 3), 1 / 3))
    # a square problem without own sizes is passed through untouched
    out = ot_ops._pair_embed(sq, sq, sq, None, None, None)
    assert out[0] is sq and out[3] is None and out[6] == (1, 3, 3, 3)
    assert ot_ops._embed(None, 3) is None


def test_unstack_returns_views_of_the_own_blocks():
    sizes = [(3, 5), (6, 4)]
    T = torch.arange(2 * 6 * 5, dtype=torch.float32).reshape(2, 6, 5)
    plans, rows, cols = ot_ops._unstack(T, sizes), ot_ops._unstack(T[:, :, 0], sizes, (0,)), ot_ops._unstack(T[:, 0, :], sizes, (1,))
    assert [tuple(t.shape) for t in plans] == [(3, 5), (6, 4)]
    assert [tuple(t.shape) for t in rows] == [(3,), (6,)] and [tuple(t.shape) for t in cols] == [(5,), (4,)]
    for b, (n1, n2) in enumerate(sizes):
        assert torch.equal(plans[b], T[b, :n1, :n2]) and torch.equal(rows[b], T[b, :n1, 0]) and torch.equal(cols[b], T[b, 0, :n2])
        assert plans[b].data_ptr() == T[b].data_ptr() and rows[b].data_ptr() == cols[b].data_ptr() == T[b].data_ptr()      # views, not copies
    back = torch.zeros_like(T)
    for b, t in enumerate(plans):
        back[b, :t.shape[0], :t.shape[1]] = t
    assert torch.equal(back[0, :3, :5], T[0, :3, :5]) and torch.equal(back[1, :6, :4], T[1, :6, :4]) and back[0, 3:].eq(0).all()
    assert ot_ops._crop(T, 6, 6) is T and ot_ops._crop(T, 3, 5).shape == (2, 3, 5)


def test_wants_grad_follows_the_grad_mode():
    x, y = torch.zeros(2, requires_grad=True), torch.zeros(2)
    assert ot_ops._wants_grad(y, None, x) and not ot_ops._wants_grad(y, None) and not ot_ops._wants_grad()
    with torch.no_grad():
        assert not ot_ops._wants_grad(x)
