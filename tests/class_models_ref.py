"""fp64 references of the stage-1 classification model and of the GAT-only model (test infrastructure), composed from the classes oracle/ has.

`Stage1ClassificationRef`: EmbeddingsWithGATAggregationClassification.forward (schnet_based_models.py:286-305) on the sub-modules of
`oracle.head.Stage2ClassificationOracle` (same names and shapes, strict load): backbone forward without the barycenter, Lin3d, + Lin_cov(GAT),
SelfAttention over a sequence of length 1 (= `value`: the softmax over one key is 1, attention_layer.py:26-33), conformer mean, MLP, sigmoid — in the
reference's order (value before the mean).
`GATOnlyRef`: EmbeddingsWithGAT (schnet_based_models.py:495-533): Linear(64, 1) on the GAT branch, one row per conformer graph; the backbone the
reference's base class constructs and never uses is there for the strict load."""
import types

import torch
from torch import nn

from oracle.gat import GATBasedOracle
from oracle.head import Stage2ClassificationOracle
from oracle.schnet import SchNetNoSumOracle


class Stage1ClassificationRef(Stage2ClassificationOracle):
    def forward(self, z, pos, node_index, x, edge_index, edge_attr):
        K = self.num_conformers
        x_3d = self.transformation_matrix_3d(self.node_embeddings_model(z, pos, node_index))
        x_cov = self.transformation_matrix_cov(self.gat_embeddings_model(x, edge_index, edge_attr, node_index))
        h = self.self_attention["value"](x_3d + x_cov)
        h = h.view(h.shape[0] // K, K, -1).mean(1)
        return torch.sigmoid(self.molecular_regression_lin(h))


class GATOnlyRef(nn.Module):
    def __init__(self):
        super().__init__()
        self.node_embeddings_model = SchNetNoSumOracle(128, 128, 3)
        self.gat_embeddings_model = GATBasedOracle(64, 3, 9)
        self.molecular_regression_lin = nn.Linear(64, 1)

    def forward(self, x, edge_index, edge_attr, batch):
        return self.molecular_regression_lin(self.gat_embeddings_model(x, edge_index, edge_attr, batch))


def strict_fp64_copy(ref: nn.Module, model: nn.Module) -> nn.Module:
    """`ref` in fp64 with `model`'s parameters, loaded strictly."""
    ref = ref.double()
    res = ref.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return ref


def device_batch(b, g, dev):
    """The model's `batch` argument from a synthetic conformer batch and its bond graph."""
    t = lambda a: torch.from_numpy(a).to(dev)
    return types.SimpleNamespace(z=t(b.z), pos=t(b.pos), x=t(g.x), edge_index=t(g.edge_index), edge_attr=t(g.edge_attr), batch=t(b.batch))


def ref_inputs(b, g):
    """The arguments of the oracle classes' forward (CPU; positions in fp64)."""
    t = torch.from_numpy
    return t(b.z), t(b.pos).double(), t(b.batch), t(g.x), t(g.edge_index), t(g.edge_attr)


def assert_grads_close(model, ref, names):
    """The project's gradient bar (tests/test_gpu_stage2.py): err <= 1e-4 * ||ref|| + 1e-6 * gmax, gmax = the largest reference gradient norm."""
    gp, rp = dict(model.named_parameters()), dict(ref.named_parameters())
    gmax = max(float(q.grad.norm()) for q in rp.values() if q.grad is not None)
    for k in names:
        err = float((gp[k].grad.cpu().double() - rp[k].grad).norm())
        print(f"grad {k}: err {err:.3e}  ||ref|| {float(rp[k].grad.norm()):.3e}  gmax {gmax:.3e}")
        assert err <= 1e-4 * float(rp[k].grad.norm()) + 1e-6 * gmax, (k, err, float(rp[k].grad.norm()))
