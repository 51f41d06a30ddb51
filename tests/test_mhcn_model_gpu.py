"""MHCNModel's training step pinned to univariate/mhcn.py's own loop body (mhcn.py:528-539) run in float64:
tests/golden/mhcn_steps.npz, written by scripts/gen_golden_mhcn_steps.py.  Six batches of the reference's sampler with the
recorded torch.randperm draws, from the fixture's initial parameters, two configurations (2 layers at d = 64, 3 at d = 32).

The rule is tests/step_pins.py's (family "mhcn"): terms against the reference's float64 and float32 runs, each of the 20
final parameters within `atol_floor_1` of the reference's own f32 slack, and that tolerance at most 1/50 of what dropping
the self-supervision or the regulariser would move the parameter (exactly 0 for the parameters no term reaches)."""
import numpy as np
import pytest
import torch

import step_pins as sp
from step_pins import MHCN_TERMS as TERMS  # noqa: F401  (tests/test_prepared_models_gpu.py reads it from here)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def steps():
    return sp.load("mhcn")


def _conf(g, c):
    return {"model": {"name": "MHCN", "type": "graph"}, "emb_size": int(g[f"c{c}/d"]), "batch_size": int(g["batch_size"]),
            "lr": float(g["hp/lr"]), "reg_lambda": float(g["hp/reg_lambda"]), "max.epoch": 1, "item.ranking.topN": [10],
            "MHCN": {"n_layer": int(g[f"c{c}/n_layer"]), "ss_rate": float(g["hp/ss_rate"])}}


def _model(g, c):
    from recommendation_amd.mhcn import MHCNModel
    train = sp.triples(g)
    m = MHCNModel(_conf(g, c), train, train[:10], sp.social(g), device="cuda")
    sp.assert_dense_id_order(m, g)                                  # sorted raw ids, mhcn.py:232
    return m


@pytest.mark.parametrize("c", [0, 1])
def test_mhcn_trajectory_matches_reference_float64(steps, c):
    g = steps
    m = _model(g, c)
    names = g[f"c{c}/names"].tolist()
    params = dict(m.model.named_parameters())
    assert list(params) == names and len(names) == 20           # the regulariser sums the norms in this order
    with torch.no_grad():
        for k, p in params.items():
            if k.endswith("_bias.1"):
                assert not bool(p.any())                        # build(): zero biases
            p.copy_(torch.from_numpy(g[f"c{c}/init/{k}"]))
    got = []
    for n in range(int(g["steps"])):
        batch = sp.batch(g, n, ("users", "pos", "neg"))
        perms = [torch.from_numpy(p.astype(np.int64)).cuda() for p in g[f"c{c}/perms"][n]]
        got.append(torch.stack([t.reshape(()) for t in m.train_step(batch, perms)]))
    got = torch.stack(got).cpu().numpy().astype(np.float64)      # [steps, 4]

    sp.check(sp.record("mhcn", g, c), got, {k: p.detach().cpu().numpy() for k, p in params.items()})
    assert not bool(params["sgating_bias.4"].any())             # no term reaches it, and the norm's gradient at 0 is 0
    moved = float((params["sgating_weights.4"].detach().cpu() - torch.from_numpy(g[f"c{c}/init/sgating_weights.4"])).abs().max())
    assert moved > 1e-3                                          # the regulariser alone moves it


def test_operators_built_from_the_raw_lists_equal_the_references(steps):
    """Pairs naming unknown users dropped, the repeated pair and the repeated interaction summed to 2 before the motif
    products: structure exact, values at test_motif_adjacency_matches_reference's bar."""
    g = steps
    m = _model(g, 0)
    assert m.social_pairs[0].tolist() == g["S_row"].tolist() and m.social_pairs[1].tolist() == g["S_col"].tolist()
    enc = m.model
    for name, graph in (("H_s", enc.H_s), ("H_j", enc.H_j), ("H_p", enc.H_p), ("R", enc.R)):
        assert [graph.n_rows, graph.n_cols] == g[f"{name}_shape"].tolist(), name
        assert np.array_equal(np.asarray(graph.rowptr_host), g[f"{name}_indptr"]), name
        assert np.array_equal(graph.col.cpu().numpy(), g[f"{name}_indices"]), name
        np.testing.assert_allclose(graph.val.cpu().numpy(), g[f"{name}_data"], rtol=2e-6, atol=1e-7, err_msg=name)


def test_train_end_to_end_on_a_planted_group_graph():
    from recommendation_amd.evaluate import ranking_evaluation, test as rank_test
    from recommendation_amd.mhcn import MHCNModel
    n_u, n_i = 150, 200
    train, test, social = sp.planted_group_lists(np.random.default_rng(5))
    conf = {"emb_size": 32, "batch_size": 256, "lr": 1e-2, "reg_lambda": 1e-4, "max.epoch": 12, "item.ranking.topN": [10, 20],
            "MHCN": {"n_layer": 2, "ss_rate": 0.01}}
    m = MHCNModel(conf, train, test, social, device="cuda", seed=1)
    before = []
    step = m.train_step

    def recording_step(batch, perms=None):
        before[:] = [{k: p.detach().clone() for k, p in m.model.named_parameters()}]
        return step(batch, perms)

    m.train_step = recording_step
    metrics = m.train()
    assert set(metrics) == {"Hit Ratio", "Precision", "Recall", "NDCG"}
    assert m.bestPerformance and 1 <= m.bestPerformance[0] <= 12 and "Recall" in m.bestPerformance[1]
    g = torch.Generator().manual_seed(0)
    rand = ranking_evaluation(m.data.test_set, rank_test(m.data, torch.randn(n_u, 32, generator=g).cuda(),
                                                         torch.randn(n_i, 32, generator=g).cuda(), m.max_N), m.topN, device="cuda")
    rand = {k: float(v) for line in rand[1:] if ":" in line for k, v in [line.strip().split(":", 1)]}
    print("trained", metrics, "random table", rand)
    assert metrics["Recall"] > rand["Recall"]

    # the kept tables are the LAST batch's forward, before that batch's update (mhcn.py:514, 528): not a re-encode
    u = "u007"
    want = torch.matmul(m.V, m.U[m.data.get_user_id(u)]).cpu().numpy()
    assert np.array_equal(m.predict(u), want) and want.shape == (n_i,)
    with torch.no_grad():
        after = m.model.propagate()[0]
        for k, p in m.model.named_parameters():
            p.copy_(before[0][k])
        pre = m.model.propagate()[0]
    assert float((pre - m.U).abs().max()) <= 1e-6 * float(m.U.abs().max())
    assert float((after - m.U).abs().max()) > 1e-4 * float(m.U.abs().max())
