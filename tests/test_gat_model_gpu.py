"""GATRec / GATRecModel on the device against gat.py's own training steps (tests/golden/gat_steps.npz, step cases A, B, C)
under tests/step_pins.py's rules (gat_rules.check_steps), the device-drawn dropouts, and the end-to-end train()."""
import numpy as np
import pytest
import torch

import gat_rules as gr
import step_pins as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return gr.load()


def _model(golden, case):
    from recommendation_amd.gat import GATRec, bipartite_edge_index
    cfg = gr.step_config(golden, case)
    model = GATRec(120, 72, cfg["in_channels"], cfg["hidden_channels"], cfg["out_channels"], cfg["num_heads"], cfg["dropout"],
                   cfg["edge_dropout"], cfg["neg_slope"]).cuda().train()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in gr.step_init(golden, case).items()})
    edge_index = bipartite_edge_index(golden["train_user"].astype(np.int64), golden["train_item"].astype(np.int64), 120).cuda()
    return cfg, model, edge_index


@pytest.mark.parametrize("case", gr.STEP_CASES)
def test_training_steps_match_the_reference(golden, case):
    from recommendation_amd.optim import FusedAdam
    cfg, model, edge_index = _model(golden, case)
    graph = model.prepare(edge_index)
    opt = FusedAdam(list(model.parameters()), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    params = dict(model.named_parameters())
    losses, grad0 = [], None
    for step in range(int(golden["steps"])):
        opt.zero_grad(set_to_none=True)
        neg = torch.from_numpy(golden[f"{case}/neg_i"][step].astype(np.int64)).cuda()
        loss = model.loss(edge_index, neg, masks=gr.step_masks(golden, case, step, graph, cfg))
        loss.backward()
        if grad0 is None:
            grad0 = {k: params[k].grad.cpu().numpy().copy() for k in gr.PARAMS}
        opt.step()
        losses.append(float(loss.detach()))
    gr.check_steps(golden, case, losses, grad0, {k: params[k].detach().cpu().numpy() for k in gr.PARAMS})


def test_device_drawn_dropouts(golden):
    from recommendation_amd import functional as Fn
    cfg, model, edge_index = _model(golden, "C")
    graph = model.prepare(edge_index)
    heads, p = cfg["num_heads"], cfg["edge_dropout"]
    count = (graph.nnz + graph.n_rows) * heads
    draws = [Fn.unpack_bits(model.gat1.draw_keep_bits(graph, "cuda"), count) for _ in range(2)]
    assert not torch.equal(draws[0], draws[1])                             # two calls, two draws
    for d in draws:
        assert abs(float(d.float().mean()) - (1 - p)) < 4 * np.sqrt(p * (1 - p) / count)
    from recommendation_amd.gat import GATConv
    other = GATConv(64, 64, heads=heads, dropout=p, seed=12345)
    assert not torch.equal(Fn.unpack_bits(other.draw_keep_bits(graph, "cuda"), count), draws[0])       # two seeds differ
    # the feature dropout of training mode: zeros at rate p, drawn on the device; eval mode is the identity
    x = torch.ones(192, 64, device="cuda")
    y = model._feature_dropout(x, None)
    assert y.is_cuda and abs(float((y == 0).float().mean()) - cfg["dropout"]) < 4 * np.sqrt(0.2 * 0.8 / x.numel())
    model.eval()
    assert model._feature_dropout(x, None) is x
    a, b = model(edge_index), model(edge_index)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])             # no draw in eval mode


def test_gatrecmodel_trains_and_ranks(golden):
    import recommendation_amd as ra
    train = sp.triples(golden)
    test = [[int(u), int(i), 1.0] for u, i in zip(golden["test_user"], golden["test_item"]) if u != 57 and i != 30]
    m = ra.GATRecModel({"num_heads": 2}, train, test, seed=3)
    first = float(m.train_step()[0])
    metrics = m.train()
    assert set(metrics) >= {"Hit Ratio", "Precision", "Recall", "NDCG"} and all(np.isfinite(v) for v in metrics.values())
    assert m.topN == [10]
    last = float(m.model.train().loss(m.edge_index, torch.zeros(1200, dtype=torch.int64, device=m.device)).detach())
    assert np.isfinite(last) and first > 0.6
    scores = m.predict(train[0][0])
    assert scores.shape == (m.data.item_num,) and np.isfinite(scores).all()
