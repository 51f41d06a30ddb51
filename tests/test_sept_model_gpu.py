"""SEPTModel's training step pinned to univariate/sept_social.py's own loop body (:432-465) run in float64:
tests/golden/sept_steps.npz, written by scripts/gen_golden_sept_steps.py.  Eight batches of the reference's sampler from the
fixture's initial tables, two plain steps and six tri-training steps on the fixture's dropped interaction matrix, two
configurations (2 layers, d = 64, 10 labels; 3 layers, d = 32, 5 labels).

The rule is tests/step_pins.py's (family "sept"): terms against the reference's float64 and float32 runs, each final table
within `atol_floor_1` of the reference's own f32 slack, that tolerance at most 1/50 of what dropping the tri-training term
or the regulariser moves the table.  The kernel's label sets equal the reference's float64 sets (the
generator kept a sampler seed at which every set is decided by a relative gap of at least 1e-5, and a table seed at which no
first-step gradient is of the size of Adam's eps, where one element's rounding would be the whole slack)."""
import numpy as np
import pytest
import torch

import step_pins as sp
from step_pins import SEPT_TABLES as TABLES, SEPT_TERMS as TERMS  # noqa: F401  (read by tests/test_prepared_models_gpu.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def steps():
    return sp.load("sept")


def _conf(g, c, max_epoch=None):
    return {"model": {"name": "SEPT", "type": "graph"}, "emb_size": int(g[f"c{c}/d"]), "batch_size": int(g["batch_size"]),
            "lr": float(g["hp/lr"]), "reg_lambda": float(g["hp/reg_lambda"]), "max.epoch": max_epoch or int(g["max_epoch"]),
            "item.ranking.topN": [10],
            "SEPT": {"n_layer": int(g[f"c{c}/n_layer"]), "ss_rate": float(g["hp/ss_rate"]),
                     "drop_rate": float(g["hp/drop_rate"]), "ins_cnt": int(g[f"c{c}/ins_cnt"])}}


def _model(g, c):
    from recommendation_amd.sept import SEPTModel
    train = sp.triples(g)
    m = SEPTModel(_conf(g, c), train, train[:10], sp.social(g), device="cuda")
    sp.assert_dense_id_order(m, g)
    with torch.no_grad():
        for k in TABLES:
            getattr(m, k).copy_(torch.from_numpy(g[f"c{c}/init/{k}"]))
    return m


def _run(g, c, replay=None):
    """Eight train_steps -> (terms [8, 3] float64, label sets of the six tri-training steps, the model)."""
    m = _model(g, c)
    aug = m.graph_from_kept_pairs(g["kept_user"].astype(np.int64), g["kept_item"].astype(np.int64))
    plain = int(g["plain_steps"])
    got, labels = [], []
    for n in range(int(g["steps"])):
        batch = sp.batch(g, n, ("users", "pos", "neg"), prefix=f"c{c}/")
        tri = n >= plain
        pos = replay[n - plain] if (replay is not None and tri) else None
        got.append(torch.stack([t.reshape(()) for t in m.train_step(batch, tri, aug if tri else None, pos)]))
        if tri:
            labels.append(m.last_positives.clone())
    return torch.stack(got).cpu().numpy().astype(np.float64), labels, m


@pytest.mark.parametrize("c", [0, 1])
def test_sept_trajectory_matches_reference_float64(steps, c):
    g = steps
    got, labels, m = _run(g, c)
    failures = []
    for n, lab in enumerate(labels):                            # the kernel's own label sets are the reference's
        want = g[f"c{c}/labels{n}"].astype(np.int64)
        have = np.sort(lab.cpu().numpy(), axis=2)
        assert have.shape == want.shape, (n, have.shape, want.shape)
        if not np.array_equal(have, want):
            failures.append(f"step {n + 2}: {int((have != want).any(axis=2).sum())} label sets differ from the float64 run's")
    sp.check(sp.record("sept", g, c), got, {k: getattr(m, k).detach().cpu().numpy() for k in TABLES}, failures)

    # a second pass that replays the recorded label sets gives the same losses
    again, labels2, _ = _run(g, c, replay=labels)
    assert all(torch.equal(a, b) for a, b in zip(labels, labels2))
    assert np.all(np.abs(again - got) <= 1e-6 * np.abs(got)), (again - got)


def test_operators_built_from_the_raw_lists_equal_the_references(steps):
    """get_birectional_social_mat + get_social_related_views from the raw lists: structure exact, values at
    tests/test_mhcn_model_gpu.py's bar.  The two operators are not symmetric."""
    g = steps
    m = _model(g, 0)
    assert m.social_pairs[0].tolist() == g["S_row"].tolist() and m.social_pairs[1].tolist() == g["S_col"].tolist()
    assert m.data.uid_dev.cpu().tolist() == g["Y_row"].tolist() and m.data.iid_dev.cpu().tolist() == g["Y_col"].tolist()
    for name, graph in (("social", m.social_mat), ("sharing", m.sharing_mat)):
        assert [graph.n_rows, graph.n_cols] == g[f"{name}_shape"].tolist(), name
        assert np.array_equal(np.asarray(graph.rowptr_host), g[f"{name}_indptr"]), name
        assert np.array_equal(graph.col.cpu().numpy(), g[f"{name}_indices"]), name
        np.testing.assert_allclose(graph.val.cpu().numpy(), g[f"{name}_data"], rtol=2e-6, atol=1e-7, err_msg=name)
        assert not graph.symmetric
    # the model's own dropout keeps exactly int(nnz (1 - drop_rate)) distinct pairs, another subset per epoch
    u3, i3 = m.kept_pairs(3)
    u4, i4 = m.kept_pairs(4)
    n_pairs = m.pair_user.numel()
    assert u3.numel() == u4.numel() == g["kept_user"].size == int(n_pairs * (1 - m.drop_rate))
    k3 = set(zip(u3.tolist(), i3.tolist()))
    assert len(k3) == u3.numel() and k3 <= set(zip(m.pair_user.tolist(), m.pair_item.tolist()))
    assert k3 != set(zip(u4.tolist(), i4.tolist()))
    aug = m.augmented_graph(3)
    assert aug.nnz == 2 * u3.numel()
    assert aug.val is None or bool((aug.val == 1).all())          # un-normalised


def test_train_end_to_end_on_a_planted_group_graph():
    from recommendation_amd.evaluate import ranking_evaluation, test as rank_test
    from recommendation_amd.sept import SEPTModel
    n_u, n_i = 150, 200
    train, test, social = sp.planted_group_lists(np.random.default_rng(5))
    conf = {"emb_size": 32, "batch_size": 300, "lr": 1e-2, "reg_lambda": 1e-4, "max.epoch": 6, "item.ranking.topN": [10, 20],
            "SEPT": {"n_layer": 2, "ss_rate": 0.005, "drop_rate": 0.3, "ins_cnt": 10}}
    # 1800 pairs in batches of 300: no ragged last batch with fewer distinct users than ins_cnt (there the reference's topk
    # raises, and so does the model)
    m = SEPTModel(conf, train, test, social, device="cuda", seed=1)
    before, calls = [], []
    step = m.train_step

    def recording_step(batch, tri_training, aug_graph=None, positives=None):
        before[:] = [[p.detach().clone() for p in m.parameters()]]
        calls.append((bool(tri_training), aug_graph))
        return step(batch, tri_training, aug_graph, positives)

    m.train_step = recording_step
    metrics = m.train()
    assert set(metrics) == {"Hit Ratio", "Precision", "Recall", "NDCG"}
    assert m.bestPerformance and 1 <= m.bestPerformance[0] <= 6 and "Recall" in m.bestPerformance[1]
    # epochs 0-2 plain, 3-5 tri-training on one augmented operator per epoch
    per_epoch = len(calls) // 6
    assert [t for t, _ in calls] == [False] * (3 * per_epoch) + [True] * (3 * per_epoch)
    assert len({id(a) for t, a in calls if t}) == 3 and all(a is not None for t, a in calls if t)
    assert m.last_positives.shape[0] == 3 and m.last_positives.shape[2] == 10
    g = torch.Generator().manual_seed(0)
    rand = ranking_evaluation(m.data.test_set, rank_test(m.data, torch.randn(n_u, 32, generator=g).cuda(),
                                                         torch.randn(n_i, 32, generator=g).cuda(), m.max_N), m.topN, device="cuda")
    rand = {k: float(v) for line in rand[1:] if ":" in line for k, v in [line.strip().split(":", 1)]}
    print("trained", metrics, "random table", rand)
    assert metrics["Recall"] > rand["Recall"]

    # the kept tables are the LAST batch's forward, before that batch's update (:434, 468-469): not a re-encode
    u = "u007"
    want = torch.matmul(m.V, m.U[m.data.get_user_id(u)]).cpu().numpy()
    assert np.array_equal(m.predict(u), want) and want.shape == (n_i,)
    with torch.no_grad():
        after = m.encode(m.norm_adj)[0]
        for p, b in zip(m.parameters(), before[0]):
            p.copy_(b)
        pre = m.encode(m.norm_adj)[0]
    assert float((pre - m.U).abs().max()) <= 1e-6 * float(m.U.abs().max())
    assert float((after - m.U).abs().max()) > 1e-4 * float(m.U.abs().max())
