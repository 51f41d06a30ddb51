"""CPU-side checks of tests/golden/buir_steps.npz (scripts/gen_golden_buir_steps.py) and of BUIRModel's host logic: the
generator's asserts re-checked from the stored arrays, the COO -> CSR mask mapping against a scipy rebuild of one step's
dropped operator, `parse_config`, and a plain NumPy float64 replay of step 0's loss."""
import numpy as np
import pytest
import scipy.sparse as sp

import step_pins
from step_pins import BUIR_TENSORS as TENSORS


@pytest.fixture(scope="module")
def g():
    return step_pins.load("buir")


def _dense_ids(g):
    user = {int(r): k for k, r in enumerate(g["user_ids"])}
    item = {int(r): k for k, r in enumerate(g["item_ids"])}
    return (np.array([user[int(u)] for u in g["train_user"]], dtype=np.int64),
            np.array([item[int(i)] for i in g["train_item"]], dtype=np.int64))


def _keep(g, c, n, e):
    nnz = int(g[f"c{c}/nnz"])
    return np.unpackbits(g[f"c{c}/keep_packed"][n, e], bitorder="little")[:nnz].astype(bool)


def _coo(g):
    """The reference's COO order (buir.py:118-122): (u, i + U) then (i + U, u) per training triple."""
    uid, iid = _dense_ids(g)
    n_u = len(g["user_ids"])
    row, col = np.empty(2 * len(uid), dtype=np.int64), np.empty(2 * len(uid), dtype=np.int64)
    row[0::2], row[1::2] = uid, iid + n_u
    col[0::2], col[1::2] = iid + n_u, uid
    return row, col, n_u + len(g["item_ids"])


def test_fixture_is_self_consistent(g):
    assert int(g["configs"]) == 2 and int(g["steps"]) == 6 and int(g["batch_size"]) == 128
    assert sorted(g["user_ids"].tolist()) == g["user_ids"].tolist() and sorted(g["item_ids"].tolist()) == g["item_ids"].tolist()
    pairs = list(zip(g["train_user"].tolist(), g["train_item"].tolist()))
    assert len(set(pairs)) < len(pairs)                             # duplicate interactions are present
    for n in range(6):
        u, i = g[f"batch{n}_users"], g[f"batch{n}_items"]
        assert u.shape == i.shape == (128,) and (len(set(u.tolist())) < 128 or len(set(i.tolist())) < 128)
    for c, (layers, d, tau) in enumerate([(2, 64, 0.5), (3, 32, 0.1)]):
        assert (int(g[f"c{c}/n_layer"]), int(g[f"c{c}/d"]), float(g[f"c{c}/tau"])) == (layers, d, tau)
        assert float(g[f"c{c}/first_grad"]) >= 1e-7
        l64, l32 = g[f"c{c}/f64/losses"], g[f"c{c}/f32/losses"]
        assert l64.shape == (6,) and np.all(np.abs(l32 - l64) <= step_pins.REL * np.abs(l64))
        rates = g[f"c{c}/rates"]
        assert rates.shape == (6, 2) and np.all((rates >= 0) & (rates < float(g["hp/drop_rate"])))
        assert int(g[f"c{c}/nnz"]) == 2 * len(pairs)
        for n in range(6):
            for e in (0, 1):                                        # a Bernoulli(1 - rate) draw per stored non-zero
                kept = _keep(g, c, n, e).mean()
                assert abs(kept - (1 - rates[n, e])) < 0.03, (n, e, kept, rates[n, e])
        assert not np.array_equal(_keep(g, c, 0, 0), _keep(g, c, 0, 1))
        rec = step_pins.record("buir", g, c)
        assert tuple(rec.tables) == TENSORS and all(set(rec.dropped[k]) == {"update", "iu"} for k in TENSORS)
        rec.assert_sensitivity()                                    # either dropped part: more than DROPPED x atol
        for k in TENSORS:
            assert g[f"c{c}/f64/delta/{k}"].dtype == np.float32 and np.abs(g[f"c{c}/f64/delta/{k}"]).max() > 1e-4
    for k in ("loss", "g_w", "g_bias", "g_on_user", "g_on_item"):
        assert g[f"comp/f64/{k}"].dtype == np.float64 and 0 <= float(g[f"comp/drift/{k}"]) < 1e-5
    u = g["comp/u_idx"]
    assert u.shape == (130,) and (u == 11).sum() >= 40              # recurring ids


def test_coo_to_csr_mask_mapping_matches_a_scipy_rebuild(g):
    from recommendation_amd import CsrGraph
    uid, iid = _dense_ids(g)
    row, col, n = _coo(g)
    graph = CsrGraph.bipartite_raw(uid, iid, len(g["user_ids"]), len(g["item_ids"]), "cpu", want_perm=True)
    perm = graph.coo_perm.numpy()
    assert sorted(perm.tolist()) == list(range(len(row)))
    csr_rows = np.repeat(np.arange(n), np.diff(graph.rowptr_host))
    assert np.array_equal(row[perm], csr_rows) and np.array_equal(col[perm], graph.col.numpy())
    for r in range(n):                                              # the row order is stable: COO order inside a row
        seg = perm[graph.rowptr_host[r]:graph.rowptr_host[r + 1]]
        assert np.all(np.diff(seg) > 0)
    c, step, e = 0, 2, 0
    keep, rate = _keep(g, c, step, e), float(g[f"c{c}/rates"][step, e])
    want = sp.coo_matrix((keep * (1.0 / (1.0 - rate)), (row, col)), shape=(n, n)).tocsr()
    have = sp.csr_matrix((keep[perm] * (1.0 / (1.0 - rate)), graph.col.numpy(), graph.rowptr_host), shape=(n, n))
    have.sum_duplicates()
    assert (want != have).nnz == 0 and 0 < (~keep).sum() < len(keep)


def test_parse_config_defaults_and_tau_is_the_momentum():
    from recommendation_amd.buir import parse_config
    a = parse_config({"BUIR": {"n_layer": "3", "tau": "0.995", "drop_rate": "0.2"}, "lambda": 7, "factors": 9, "max.epoch": 50})
    assert (a.momentum, a.n_layers, a.drop_rate) == (0.995, 3, 0.2)
    assert (a.emb_size, a.lRate, a.batch_size, a.topN) == (64, 0.001, 2048, [10, 20, 30, 50])
    assert not hasattr(a, "maxEpoch") and not hasattr(a, "tau")
    b = parse_config({"BUIR": {"n_layer": 1, "tau": 0.5, "drop_rate": 0}, "emb_size": 32, "lr": 0.01, "batch_size": 64,
                      "item.ranking.topN": ["5", "15"]})
    assert (b.emb_size, b.lRate, b.batch_size, b.topN) == (32, 0.01, 64, [5, 15])
    with pytest.raises(KeyError):
        parse_config({"BUIR": {"n_layer": 1, "drop_rate": 0}})


@pytest.mark.parametrize("c", [0, 1])
def test_numpy_float64_replay_of_the_first_loss(g, c):
    row, col, n = _coo(g)
    n_u = len(g["user_ids"])
    pre = f"c{c}/init/online_encoder.embedding_dict."
    ego = np.concatenate([g[pre + "user_emb"], g[pre + "item_emb"]]).astype(np.float64)
    w, b = g[f"c{c}/init/predictor.weight"].astype(np.float64), g[f"c{c}/init/predictor.bias"].astype(np.float64)
    u, i = g["batch0_users"].astype(np.int64), g["batch0_items"].astype(np.int64)

    def encode(e):                                                  # the targets start as copies of the online tables
        rate = float(g[f"c{c}/rates"][0, e])
        a = sp.coo_matrix((_keep(g, c, 0, e) * (1.0 / (1.0 - rate)), (row, col)), shape=(n, n)).tocsr()
        layers = [ego]
        for _ in range(int(g[f"c{c}/n_layer"])):
            layers.append(a @ layers[-1])
        out = np.mean(layers, axis=0)
        return out[:n_u], out[n_u:]

    def unit(x):
        return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)

    on_u, on_i = encode(0)
    tg_u, tg_i = encode(1)
    p_u, p_i = on_u[u] @ w.T + b, on_i[i] @ w.T + b
    loss = np.mean((2 - 2 * (unit(p_u) * unit(tg_i[i])).sum(-1)) + (2 - 2 * (unit(p_i) * unit(tg_u[u])).sum(-1)))
    assert abs(loss - float(g[f"c{c}/f64/losses"][0])) <= 1e-10 * abs(loss), (loss, float(g[f"c{c}/f64/losses"][0]))
