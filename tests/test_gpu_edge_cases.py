"""Edge cases through the full drop-in path: tiny conformers (1-3 atoms: rows without neighbours, N_max tiny), K=1 and K=2,
a single molecule, and widely ragged batches (padding rows dominate some slabs).  Checked against the fp64 oracle."""
import numpy as np
import pytest
import torch

from helpers import rel
from conan_fgw_amd.schnet import SchNetNoSum
from conan_fgw_amd.synthetic import ConformerBatch
from oracle.schnet import SchNetNoSumOracle

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def _batch(atom_counts, K, seed):
    rng = np.random.RandomState(seed)
    zs, poss, bs = [], [], []
    g = 0
    for n in atom_counts:
        z = rng.choice([1, 6, 7, 8], size=n)
        for _ in range(K):
            zs.append(z); poss.append(rng.uniform(0, 3.0 + n ** (1 / 3), size=(n, 3)).astype(np.float32)); bs.append(np.full(n, g)); g += 1
    return ConformerBatch(z=np.concatenate(zs).astype(np.int64), pos=np.concatenate(poss), batch=np.concatenate(bs).astype(np.int64),
                          y=np.zeros(len(atom_counts), np.float32), num_molecules=len(atom_counts), num_conformers=K,
                          atoms_per_molecule=np.asarray(atom_counts, np.int64))


@pytest.mark.parametrize("atoms,K", [([2, 3, 5], 2), ([7], 1), ([4, 30, 2, 17], 3), ([3, 3], 5)])
def test_tiny_and_ragged_batches(atoms, K):
    b = _batch(atoms, K, seed=sum(atoms) + K)
    torch.manual_seed(1)
    m = SchNetNoSum(dev, hidden_channels=64, num_filters=64, num_interactions=2).to(dev)
    ref = SchNetNoSumOracle(64, 64, 2)
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    ref = ref.double()
    z, pos, batch = torch.from_numpy(b.z), torch.from_numpy(b.pos), torch.from_numpy(b.batch)
    h3, hb = m.forward_w_barycenter(z.to(dev), pos.to(dev), K, batch.to(dev))
    (h3.sum() + hb.sum()).backward()
    r3, rb = ref.forward_w_barycenter(z, pos.double(), K, batch)
    assert h3.shape == (len(atoms) * K, 32) and hb.shape == h3.shape
    assert torch.isfinite(h3).all() and torch.isfinite(hb).all()
    assert rel(h3.detach().cpu().numpy(), r3.detach().numpy()) < 1e-5
    assert rel(hb.detach().cpu().numpy(), rb.detach().numpy()) < 1e-4
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_isolated_atoms_have_no_edges_and_constant_slab_is_nan_like_the_reference():
    """One-atom conformers: the radius graph is empty and the [1,d] slab is normalised over its own min/max.  A slab that
    is constant divides by zero exactly like the reference (Appendix D-13: normalize_tensor has no epsilon)."""
    from conan_fgw_amd import ops
    pos = torch.tensor([[0., 0, 0], [9, 9, 9]], device=dev); batch = torch.tensor([0, 1], device=dev)
    gp = ops.graph_ptr_from_batch(batch, 2)
    g = ops.RadiusGraph(pos, gp, 2, 10.0, 32)
    assert g.num_edges == 0
    feat = torch.full((2, 8), 0.25, device=dev)
    Ys, Cs = ops.fgw_densify(feat, g, 1, 0.5)
    assert torch.isnan(Ys).all() and float(Cs.abs().max()) == 0.0


def _visnet_pair(H, seed=1):
    from conan_fgw_amd.visnet import ViSNet
    from oracle.visnet import ViSNetOracle
    torch.manual_seed(seed)
    m = ViSNet(dev, hidden_channels=H).to(dev)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
    ref = ViSNetOracle(H)
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    return m, ref.double()


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("atoms,K", [([2, 3, 5], 2), ([7], 1), ([4, 30, 2, 17], 3), ([3, 3], 5)])
def test_visnet_tiny_and_ragged_batches(atoms, K, H):
    """The ViSNet twin of test_tiny_and_ragged_batches: forward h3 / hb and every parameter gradient against the fp64 oracle, with the bars of
    test_gpu_visnet.py::test_backward_matches_oracle_autograd (h3 < 2e-5; per parameter gradient rel < 1e-4, and abs max < 1e-6 where the oracle's
    gradient is exactly zero).  hb < 1e-4 is not one of that test's bars and not a measurement: it is the bar test_production_width_vs_oracle_and_invariance
    and the SchNet twin above put on the barycenter branch.

    One case has gradients that are neither: ([3, 3], K = 5).  Every conformer there is a complete 3-atom graph, the transport plans are uniform, all rows
    of the barycenter are equal, and the column-normalised row sum makes hb = sqrt(3) whatever the features are.  The 12 parameter tensors of
    output_model_bary.* and prior_model_bary.atomref then have a gradient that cancels (~1e-14 in the fp64 oracle) instead of being zero term by term,
    so in that case the barycenter head's gradients are only held to the rounding bound below (the `cancelled` branch) and hb to sqrt(3); the other
    three cases test them with rel < 1e-4 and must not take that branch."""
    b = _batch(atoms, K, seed=sum(atoms) + K)
    m, ref = _visnet_pair(H)
    z, pos, batch = torch.from_numpy(b.z), torch.from_numpy(b.pos), torch.from_numpy(b.batch)
    G = len(atoms) * K
    g1 = torch.randn(G, H // 2, generator=torch.Generator().manual_seed(1))
    g2 = torch.randn(G, H // 2, generator=torch.Generator().manual_seed(2))
    h3, hb = m.forward_w_barycenter(z.to(dev), pos.to(dev), K, batch.to(dev))
    ((h3 * g1.to(dev)).sum() + (hb * g2.to(dev)).sum()).backward()
    r3, rb = ref.forward_w_barycenter(z, pos.double(), K, batch)
    ((r3 * g1.double()).sum() + (rb * g2.double()).sum()).backward()
    assert h3.shape == (G, H // 2) and hb.shape == h3.shape
    assert torch.isfinite(h3).all() and torch.isfinite(hb).all()
    assert rel(h3.detach().cpu().numpy(), r3.detach().numpy()) < 2e-5
    assert rel(hb.detach().cpu().numpy(), rb.detach().numpy()) < 1e-4
    refp = dict(ref.named_parameters())
    gmax = max(float(q.grad.norm()) for q in refp.values() if q.grad is not None)
    checked, cancelled = 0, []
    for name, p in m.named_parameters():
        q = refp[name]
        if q.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, name
        gn = float(q.grad.norm())
        if gn == 0.0:
            assert float(p.grad.abs().max()) < 1e-6, name
            continue
        if gn <= 1e-12 * gmax:
            # CANCELLED gradient (see the docstring): not zero term by term, so fp32 leaves rounding residue.  A chain of 64 roundings of 2^-24 on
            # terms of the size of the largest parameter gradient bounds it: 64 * 2^-24 * gmax = 3.8e-6 * gmax (from the number format; the
            # fp32 oracle leaves ~3e-7 * gmax)
            print(f"CANCELLED {name}: |grad| = {float(p.grad.norm()):.3g}, gmax = {gmax:.3g}, bar = {64 * 2.0 ** -24 * gmax:.3g}")
            assert float(p.grad.norm()) < 64 * 2.0 ** -24 * gmax, name
            cancelled.append(name)
            continue
        assert rel(p.grad.detach().cpu().numpy(), q.grad.numpy()) < 1e-4, name
        checked += 1
    assert checked > 100
    if atoms == [3, 3]:
        assert len(cancelled) == 12 and all(c.startswith(("output_model_bary.", "prior_model_bary.")) for c in cancelled), cancelled
        assert rel(hb.detach().cpu().numpy(), np.full(hb.shape, 3 ** 0.5)) < 1e-6
    else:
        assert not cancelled, cancelled


def test_visnet_one_atom_conformers_have_the_oracles_nan_pattern():
    """Conformers of a single atom next to ordinary ones: only a self loop in the ViSNet graph, no edge in the FGW adjacency, a [1,d] slab per
    conformer.  Whatever the reference's normalize_tensor makes of such a slab (it divides by max - min without an epsilon), the GPU path must
    give NaN exactly where the oracle does and agree with it everywhere else."""
    b = _batch([1, 4, 1], 2, seed=5)
    m, ref = _visnet_pair(64)
    z, pos, batch = torch.from_numpy(b.z), torch.from_numpy(b.pos), torch.from_numpy(b.batch)
    with torch.no_grad():
        h3, hb = m.forward_w_barycenter(z.to(dev), pos.to(dev), 2, batch.to(dev))
        r3, rb = ref.forward_w_barycenter(z, pos.double(), 2, batch)
    h3, hb = h3.cpu(), hb.cpu()
    assert torch.isfinite(h3).all() and torch.isfinite(r3).all()
    assert rel(h3.numpy(), r3.numpy()) < 2e-5
    assert torch.equal(torch.isnan(hb), torch.isnan(rb)) and torch.equal(torch.isfinite(hb), torch.isfinite(rb))
    ok = torch.isfinite(rb)
    assert ok.any() and rel(hb[ok].numpy(), rb[ok].numpy()) < 1e-4
