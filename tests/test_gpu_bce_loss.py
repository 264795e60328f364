"""`ops.bce_loss` (k_bce_loss: binary cross-entropy and its gradient in one launch) against torch.nn.functional.binary_cross_entropy in fp64 on the CPU.

Bars: loss within 2e-6 relative, gradient within 2e-6 norm-wise — the project's bar for an fp32 reduction against fp64 (stage2_head, clipping tests);
torch's own fp32 kernel stays below 1e-7 on these inputs, the margin is for differences between logarithm implementations.  Sizes: one element, both
sides of the wavefront (64) and workgroup (256) boundaries, and a multi-trip strided loop."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 257, 1280]


def _inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = 0.001 + 0.998 * torch.rand(n, 1, generator=g)
    y = (torch.rand(n, 1, generator=g) < 0.5).float()
    w_n = 0.25 + 2.0 * torch.rand(n, 1, generator=g)
    return p, y, {"none": None, "one": torch.tensor([2.5]), "each": w_n}


def _reference(p, y, w, seed_scale):
    p64 = p.double().requires_grad_(True)
    ref = F.binary_cross_entropy(p64, y.double(), weight=None if w is None else w.double())
    (seed_scale * ref).backward()
    return ref.detach(), p64.grad


@pytest.mark.parametrize("n", SIZES)
def test_bce_loss_and_its_gradient_match_fp64(n):
    from conan_fgw_amd import ops
    dev = torch.device("cuda:0")
    p, y, weights = _inputs(n, 100 + n)
    for form, w in weights.items():
        pd = p.to(dev).requires_grad_(True)
        loss = ops.bce_loss(pd, y.to(dev), None if w is None else w.to(dev))
        assert loss.shape == () and loss.dtype == torch.float32
        (3.0 * loss).backward()
        ref, gref = _reference(p, y, w, 3.0)
        el = abs(float(loss.detach()) - float(ref)) / abs(float(ref))
        eg = float((pd.grad.cpu().double() - gref).norm() / gref.norm())
        print(f"n={n} weight={form}: loss {float(loss.detach()):.9g} ref {float(ref):.9g} rel {el:.2e}; grad rel {eg:.2e}")
        assert el <= 2e-6, (form, el)
        assert eg <= 2e-6, (form, eg)
        assert pd.grad.shape == pd.shape
        again = ops.bce_loss(pd.detach(), y.to(dev), None if w is None else w.to(dev))
        assert torch.equal(again, loss.detach())                                # fixed summation order: the same bits


def test_bce_loss_edge_values_are_clamped_like_torch():
    """p = 0 and p = 1: both logarithms clamped at -100 BEFORE they meet the label (p = y = 1 and p = y = 0 give 0, not 0 * -inf), the gradient's
    denominator at 1e-12.  Expected (fp64): loss 100.602, gradients 0, 0, +5e11, -5e11, -1.6667."""
    from conan_fgw_amd import ops
    dev = torch.device("cuda:0")
    p = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.3])
    y = torch.tensor([0.0, 1.0, 0.0, 1.0, 1.0])
    w = torch.tensor([2.5])
    pd = p.to(dev).requires_grad_(True)
    loss = ops.bce_loss(pd, y.to(dev), w.to(dev))
    loss.backward()
    ref, gref = _reference(p, y, w, 1.0)
    print("loss", float(loss.detach()), "ref", float(ref), "grad", pd.grad.tolist(), "ref", gref.tolist())
    assert abs(float(ref) - 100.602) < 1e-3 and torch.allclose(gref, torch.tensor([0.0, 0.0, 5e11, -5e11, -5.0 / 3.0], dtype=torch.float64), rtol=1e-4)
    assert torch.isfinite(loss).item()
    assert abs(float(loss.detach()) - float(ref)) <= 2e-6 * abs(float(ref))
    g = pd.grad.cpu().double()
    assert torch.isfinite(g).all()
    assert g[0] == 0.0 and g[1] == 0.0
    assert float((g - gref).norm() / gref.norm()) <= 2e-6
    assert float((g[2:] - gref[2:]).abs().div(gref[2:].abs()).max()) <= 2e-6     # element by element too: the two 5e11 entries own the norm


def test_bce_loss_argument_checks():
    from conan_fgw_amd import ops
    dev = torch.device("cuda:0")
    p = torch.full((5, 1), 0.4, device=dev)
    y = torch.ones(5, 1, device=dev)
    with pytest.raises(RuntimeError):
        ops.bce_loss(p, y[:, 0])                                             # shape mismatch, as ops.mse_loss
    with pytest.raises(ValueError):
        ops.bce_loss(p, y, torch.ones(3, device=dev))                        # neither 1 nor n weights
    with pytest.raises(ValueError):
        ops.bce_loss(p, y, 2.5)                                              # a tensor, not a number


def test_bce_loss_does_not_synchronise_with_the_host():
    from conan_fgw_amd import ops
    dev = torch.device("cuda:0")
    p = torch.full((7, 1), 0.4, device=dev).requires_grad_(True)
    y = torch.ones(7, 1, device=dev)
    w1, wn = torch.tensor([1.7], device=dev), torch.full((7, 1), 0.5, device=dev)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for w in (None, w1, wn):
            loss = ops.bce_loss(p, y, w)
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.isfinite(loss).item() and torch.isfinite(p.grad).all()


def test_classification_loss_is_bce_loss():
    """head.classification_loss(predicted, expected, class_weights) (common.py:210-217) = ops.bce_loss, bit for bit, with and without weights; a
    weight that lives on the host (the reference's torch.tensor([cw[1] / cw[0]])) is moved by the op."""
    from conan_fgw_amd import ops
    from conan_fgw_amd.head import classification_loss
    dev = torch.device("cuda:0")
    p, y, _ = _inputs(65, 9)
    p, y = p.to(dev), y.to(dev)
    w = torch.tensor([1.7])
    for cw in (None, w, w.to(dev)):
        pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
        la, lb = classification_loss(pa, y, cw), ops.bce_loss(pb, y, cw)
        la.backward(); lb.backward()
        assert torch.equal(la, lb) and torch.equal(pa.grad, pb.grad)
    assert torch.equal(classification_loss(p, y, w), classification_loss(p, y, w.to(dev)))
