"""DiffNetModel's training step pinned to univariate/diffnet.py's own loop body (:1103-1119) run in float64:
tests/golden/diffnet_steps.npz, written by scripts/gen_golden_diffnet_steps.py.  Six whole-list batches of the reference's
sampler from the fixture's initial parameters, two configurations (2 layers, d = 64; 3 layers, d = 32).

The rule is tests/step_pins.py's (family "diffnet", registered by tests/diffnet_fixture.py): rec / reg / total against the
reference's float64 and float32 runs, each final table within `atol_floor_1` of the reference's own f32 slack, that
tolerance at most 1/50 of what dropping the S X half, the A items addend or the regulariser moves the table."""
import numpy as np
import pytest
import torch

import diffnet_fixture as dfx
import step_pins as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def steps():
    return dfx.load()


def _model(g, c, **kw):
    from recommendation_amd.diffnet import DiffNetModel
    train = sp.triples(g)
    m = DiffNetModel(dfx.conf(g, c), train, train[:10], sp.social(g), device="cuda", **kw)
    sp.assert_dense_id_order(m, g)
    params = dict(m.model.named_parameters())
    assert list(params) == dfx.names(g, c)
    with torch.no_grad():
        for k, v in dfx.init(g, c).items():
            assert params[k].shape == v.shape, k
            params[k].copy_(torch.from_numpy(v))
    return m


def _run(g, c, **kw):
    m = _model(g, c, **kw)
    got = [torch.stack(m.train_step(dfx.batch(g, n))) for n in range(int(g["steps"]))]
    return torch.stack(got).cpu().numpy().astype(np.float64), m


@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("c", [0, 1])
def test_diffnet_trajectory_matches_reference_float64(steps, c, gather):
    g = steps
    got, m = _run(g, c, gather=gather)
    assert m.regU == float(g["hp/reg_lambda"]) and m.maxEpoch == 1
    sp.check(dfx.record(g, c), got, {k: p.detach().cpu().numpy() for k, p in m.model.named_parameters()})


def test_operators_and_predict(steps):
    g = steps
    m = _model(g, 0)
    s, a = m.model.S, m.model.A
    for graph, pre in ((s, "S"), (a, "A")):                            # one entry per pair / triple, in list order per row
        order = np.argsort(g[f"{pre}_row"], kind="stable")
        assert np.array_equal(graph.col.cpu().numpy(), g[f"{pre}_col"][order])
        assert np.array_equal(graph.val.cpu().numpy(), g[f"{pre}_val"][order])
    st = {k: p.detach().cpu().double() for k, p in m.model.named_parameters()}
    n_u, n_i = m.data.user_num, m.data.item_num
    dense = {}
    for pre, cols in (("S", n_u), ("A", n_i)):
        dense[pre] = torch.zeros(n_u, cols, dtype=torch.float64)
        dense[pre].index_put_((torch.from_numpy(g[f"{pre}_row"].astype(np.int64)), torch.from_numpy(g[f"{pre}_col"].astype(np.int64))),
                              torch.from_numpy(g[f"{pre}_val"]).double(), accumulate=True)
    h = st["user_embeddings"]
    for k in range(m.n_layers):
        h = torch.relu(torch.cat([dense["S"] @ h, h], 1) @ st[f"weights.{k}"])
    final = h + dense["A"] @ st["item_embeddings"]
    U, V = m._final()
    assert float((U.cpu().double() - final).abs().max()) <= 1e-5 * float(final.abs().max())
    assert torch.equal(V, m.model.item_embeddings.detach())            # the RAW item table
    raw = int(g["user_ids"][5])
    score = final[m.data.get_user_id(raw)] @ st["item_embeddings"].T
    have = m.predict(raw)
    assert have.shape == (n_i,) and np.abs(have - score.numpy()).max() <= 1e-5 * float(score.abs().max())
    # the composed encoder is the same function
    m2 = _model(g, 0, fused=False)
    with torch.no_grad():
        assert float((m2.model() - U).abs().max()) <= 1e-5 * float(U.abs().max())


def test_train_end_to_end(steps):
    from recommendation_amd.diffnet import DiffNetModel
    g = steps
    train = sp.triples(g)
    conf = dict(dfx.conf(g, 1, batch_size=256), **{"max.epoch": 5})
    m = DiffNetModel(conf, train[:1200], train[1200:], sp.social(g), device="cuda", seed=2)
    before = [p.detach().clone() for p in m.model.parameters()]
    stale = m._final()[0].clone()
    metrics = m.train()                                                # range(1) epochs whatever the conf says
    assert set(metrics) == {"Hit Ratio", "Precision", "Recall", "NDCG"} and all(np.isfinite(v) for v in metrics.values())
    assert m.maxEpoch == 1
    assert all(not torch.equal(b, p.detach()) for b, p in zip(before, m.model.parameters()))
    assert not torch.equal(stale, m._final()[0])                       # the ranking re-encodes with the updated parameters
    other = DiffNetModel(conf, train[:1200], train[1200:], sp.social(g), device="cuda", seed=2)
    assert all(torch.equal(b, p.detach()) for b, p in zip(before, other.model.parameters()))      # a function of the seed
