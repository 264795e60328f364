"""The stage-1 classification model (`EmbeddingsWithGATAggregationClassification`, schnet_based_models.py:247-305) and the GAT-only model
(`EmbeddingsWithGAT`, :495-533) through the HIP path against fp64 references composed from the oracle classes (tests/class_models_ref.py):
predictions within 1e-4 relative (the bar of BASELINE.json and of the stage-2 classification test), gradients within the stage-2 tests' formula."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from class_models_ref import GATOnlyRef, Stage1ClassificationRef, assert_grads_close, device_batch, ref_inputs, strict_fp64_copy
from helpers import rel
from conan_fgw_amd.synthetic import make_batch, make_bond_graph

pytestmark = pytest.mark.gpu


def _stage1(B, K, seed, shape="esol", **kw):
    from conan_fgw_amd.head import EmbeddingsWithGATAggregationClassification
    dev = torch.device("cuda:0")
    b = make_batch(shape, B, K, seed=seed)
    g = make_bond_graph(b, seed=seed + 1)
    torch.manual_seed(seed + 2)
    m = EmbeddingsWithGATAggregationClassification(K, dev, **kw).to(dev)
    ref = strict_fp64_copy(Stage1ClassificationRef(K, **kw), m)
    return dev, b, g, m, ref


@pytest.fixture(scope="module")
def esol43():
    """make_batch("esol", 4, 3) on SchNet-512: the model, its reference and both forward passes, computed once; tests that follow only read them."""
    dev, b, g, m, ref = _stage1(4, 3, 141)
    batch = device_batch(b, g, dev)
    cidx = m.create_aggregation_index(b.num_graphs, dev)
    p = m(batch, cidx, batch.batch)
    r = ref(*ref_inputs(b, g))
    return dict(dev=dev, b=b, g=g, m=m, ref=ref, batch=batch, cidx=cidx, p=p, r=r)


def test_stage1_classification_prediction_and_gradients_match_fp64(esol43):
    s = esol43
    m, ref, p, r, dev = s["m"], s["ref"], s["p"], s["r"], s["dev"]
    assert m.node_embeddings_model.hidden_channels == 512 and m.self_attention.value.weight.shape == (256, 256)
    assert s["cidx"].tolist() == [i for i in range(4) for _ in range(3)]
    assert p.shape == (4, 1) and float(p.detach().min()) > 0.0 and float(p.detach().max()) < 1.0
    e = rel(p.detach().cpu().double().numpy(), r.detach().numpy())
    print("prediction rel", e)
    assert e < 1e-4
    from conan_fgw_amd import ops
    lab = torch.tensor([[1.0], [0.0], [1.0], [0.0]])
    w = torch.tensor([1.7])
    loss = ops.bce_loss(p, lab.to(dev), weight=w)
    lref = F.binary_cross_entropy(r, lab.double(), weight=w.double())
    assert abs(float(loss.detach()) - float(lref.detach())) <= 1e-4 * abs(float(lref.detach()))
    loss.backward()
    lref.backward()
    assert_grads_close(m, ref, ["molecular_regression_lin.0.weight", "molecular_regression_lin.4.bias", "self_attention.value.weight",
                                "transformation_matrix_3d.weight", "transformation_matrix_cov.weight",
                                "gat_embeddings_model.gat_conv2.lin_src.weight", "node_embeddings_model.interactions.0.conv.lin1.weight"])
    # one key: query and key are not evaluated (the reference leaves exact zeros); the barycenter layers belong to stage 2
    assert m.self_attention.query.weight.grad is None and m.self_attention.key.weight.grad is None
    assert m.transformation_matrix_bary.weight.grad is None and m.node_embeddings_model.lin1_bary.weight.grad is None
    rq = ref.self_attention["query"].weight.grad
    assert rq is None or not rq.any()


def test_stage1_classification_hints_and_index_check(esol43):
    s = esol43
    m, b, batch, cidx = s["m"], s["b"], s["batch"], s["cidx"]
    with torch.no_grad():
        y2 = m(batch, cidx, batch.batch, num_graphs=b.num_graphs, max_nodes=b.max_nodes)
        assert torch.equal(m(batch, cidx, batch.batch), y2)
    with pytest.raises(ValueError):
        m(batch, cidx[:-1], batch.batch)
    t = torch.zeros(3)
    assert m.forward_dummy(t, t.long(), t.long()) is None                    # CPU tensors: the one call made before the model moves to the GPU


def test_stage1_classification_checkpoint_loads_strictly_into_stage2(esol43, tmp_path):
    """The two-stage recipe (train_val.py:175-183): the stage-1 state_dict, saved as a Lightning-style checkpoint, initialises stage 2."""
    from conan_fgw_amd.head import EmbeddingsWithGATAggregationClassificationBaryCenter
    s = esol43
    m1, dev, batch, cidx = s["m"], s["dev"], s["batch"], s["cidx"]
    path = tmp_path / "stage1_class.ckpt"
    torch.save({"state_dict": m1.state_dict()}, path)
    torch.manual_seed(99)
    m2 = EmbeddingsWithGATAggregationClassificationBaryCenter(3, dev).to(dev)
    res = m2.load_state_dict(torch.load(path)["state_dict"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    assert list(sd1) == list(sd2)
    for k in sd1:
        assert sd1[k].shape == sd2[k].shape and torch.equal(sd1[k], sd2[k]), k
    with torch.no_grad():
        p2 = m2(batch, cidx, batch.batch)
    assert p2.shape == (4, 1) and torch.isfinite(p2).all() and float(p2.min()) > 0.0 and float(p2.max()) < 1.0


def test_stage1_classification_with_one_conformer():
    """K = 1: the conformer mean runs over one row."""
    dev, b, g, m, ref = _stage1(2, 1, 151)
    batch = device_batch(b, g, dev)
    with torch.no_grad():
        p = m(batch, m.create_aggregation_index(b.num_graphs, dev), batch.batch)
        r = ref(*ref_inputs(b, g))
    assert p.shape == (2, 1) and 0.0 < float(p.min()) and float(p.max()) < 1.0
    assert rel(p.cpu().double().numpy(), r.numpy()) < 1e-4


def test_stage1_classification_on_visnet_backbone():
    """model_name="visnet", feat_dim=128 (common.py:444-446 -> :542-546), BACE-sized conformers, as for the stage-2 twin."""
    dev, b, g, m, ref = _stage1(2, 2, 161, shape="bace", model_name="visnet", feat_dim=128)
    batch = device_batch(b, g, dev)
    with torch.no_grad():
        p = m(batch, m.create_aggregation_index(b.num_graphs, dev), batch.batch)
        r = ref(*ref_inputs(b, g))
    assert p.shape == (2, 1) and 0.0 < float(p.min()) and float(p.max()) < 1.0
    assert rel(p.cpu().double().numpy(), r.numpy()) < 1e-4


def test_stage1_classification_captured_step_follows_the_eager_loop_bit_for_bit():
    """The classification step (forward, ops.bce_loss, backward, clip, FlatAdam) as HIP graphs — `CapturedTrainStep`, the pattern of
    tests/test_gpu_graph_capture.py at small size — against the same steps run eagerly: K = 2, two same-shaped batches of 3 molecules through a
    static collator, the labels formed inside the loss function.  The model uses no side stream, so the captured step has no parallel branches."""
    from conan_fgw_amd import ops
    from conan_fgw_amd.capture import CapturedTrainStep
    from conan_fgw_amd.collate import DeviceCollator, molecules_from_synthetic
    from conan_fgw_amd.head import EmbeddingsWithGATAggregationClassification
    from conan_fgw_amd.parallel import FlatAdam, FlatGradients
    dev = torch.device("cuda:0")
    K = 2
    cb = make_batch("esol", 3, K, seed=171); bg = make_bond_graph(cb, seed=172)
    base = molecules_from_synthetic(cb, bg)
    rng = np.random.default_rng(7)
    batches = []
    for _ in range(2):
        its = [copy.copy(it) for it in base]
        for it in its:
            it.__dict__.pop("_conan_record", None)
            it.pos = (it.pos + rng.normal(0.0, 0.05, size=it.pos.shape)).astype(np.float32)
        batches.append(its)
    order = [0, 1, 0]

    def build():
        torch.manual_seed(33)
        m = EmbeddingsWithGATAggregationClassification(K, dev).to(dev)
        flat = FlatGradients(m.parameters())
        return m, flat, FlatAdam(flat, lr=1e-3, module=m)

    def loss_of(m, db, y):
        labels = (y[::K][:, None] > 0).float().contiguous()                 # one label per molecule (the collated y is per conformer graph)
        return ops.bce_loss(m(db, db.conformers_index, db.batch), labels)

    me, fe, oe = build()
    coll_e = DeviceCollator(dev, K, depth=2)

    def eager(items):
        db = coll_e(items).wait()
        fe.zero()
        loss = loss_of(me, db, db.y)
        fe.backward(loss)
        fe.all_reduce_mean()
        fe.clip_grad_norm_(1.0)
        oe.step()
        return float(loss.detach())
    for _ in range(3):                                                      # what the captured object does before it captures
        eager(batches[0])
    losses_e = [eager(batches[q]) for q in order]
    torch.cuda.synchronize()

    mg, fg, og = build()
    coll = DeviceCollator(dev, K, depth=2, static=True)
    db = coll(batches[0]).wait()
    y_view = db.y                                                           # fixed views of the static collator
    step = CapturedTrainStep(lambda: loss_of(mg, db, y_view), fg, og, clip_norm=1.0, warmup=3)
    losses_g = []
    for q in order:
        coll(batches[q]).wait()
        losses_g.append(float(step()))
    torch.cuda.synchronize()
    assert losses_e == losses_g, (losses_e, losses_g)
    assert all(l == l and l > 0.0 for l in losses_g)
    for (k, a), (_, c) in zip(me.state_dict().items(), mg.state_dict().items()):
        assert torch.equal(a, c), k
    assert float(oe.step_dev) == float(og.step_dev) == 6.0


def test_gat_only_model_matches_fp64():
    """EmbeddingsWithGAT: Linear(64, 1) on the covalent branch, one row per conformer graph (no conformer mean); the backbone is constructed for
    the strict load and never used."""
    from conan_fgw_amd import ops
    from conan_fgw_amd.head import EmbeddingsWithGAT
    dev = torch.device("cuda:0")
    K = 2
    b = make_batch("esol", 3, K, seed=181)
    g = make_bond_graph(b, seed=182)
    torch.manual_seed(183)
    m = EmbeddingsWithGAT(K, dev).to(dev)
    ref = strict_fp64_copy(GATOnlyRef(), m)
    res = m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)      # and back: the reference's state_dict loads strictly
    assert not res.missing_keys and not res.unexpected_keys
    batch = device_batch(b, g, dev)
    y = m(batch, m.create_aggregation_index(b.num_graphs, dev), batch.batch)
    t = torch.from_numpy
    r = ref(t(g.x), t(g.edge_index), t(g.edge_attr), t(b.batch))
    assert y.shape == (6, 1)
    assert rel(y.detach().cpu().double().numpy(), r.detach().numpy()) < 1e-4
    with torch.no_grad():
        assert torch.equal(m(batch, None, None, num_graphs=b.num_graphs), m(batch, None, None))
    tgt = torch.randn(6, 1, generator=torch.Generator().manual_seed(184))
    ops.mse_loss(y, tgt.to(dev)).backward()
    F.mse_loss(r, tgt.double()).backward()
    assert_grads_close(m, ref, ["gat_embeddings_model.gat_conv1.lin_src.weight", "gat_embeddings_model.gat_conv2.att_src",
                                "molecular_regression_lin.weight"])
    for k, q in m.named_parameters():
        if k.startswith("node_embeddings_model."):
            assert q.grad is None, k
    assert m.forward_dummy(torch.zeros(3), None, None) is None
