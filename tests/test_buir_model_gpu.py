"""BUIRModel's training step pinned to univariate/buir.py's own loop body (:194-203) run in float64:
tests/golden/buir_steps.npz, written by scripts/gen_golden_buir_steps.py.  Six batches of the reference's sampler from the
fixture's initial state with the reference's recorded dropout draws, two configurations (2 layers, d = 64, tau 0.5;
3 layers, d = 32, tau 0.1).

The rule is tests/step_pins.py's (family "buir"): the loss against the reference's float64 and float32 runs, each of the six
final tensors within `atol_floor_1` of the reference's own f32 slack, that tolerance at most 1/50 of what dropping
`update_target` or the `loss_iu` term moves the tensor."""
import numpy as np
import pytest
import torch

import step_pins as sp

pytestmark = pytest.mark.gpu

NAMES = dict(zip(sp.BUIR_TENSORS, ("online_user", "online_item", "target_user", "target_item", "weight", "bias")))


@pytest.fixture(scope="module")
def steps():
    return sp.load("buir")


def _conf(g, c, batch_size=None):
    return {"model": {"name": "BUIR", "type": "graph"}, "emb_size": int(g[f"c{c}/d"]), "lr": float(g["hp/lr"]),
            "batch_size": batch_size or int(g["batch_size"]), "item.ranking.topN": [10, 20],
            "BUIR": {"n_layer": int(g[f"c{c}/n_layer"]), "tau": float(g[f"c{c}/tau"]), "drop_rate": float(g["hp/drop_rate"])}}


def _init_state(g, c):
    return {k: sp.buir_init(g, c, k) for k in NAMES}


def _model(g, c):
    from recommendation_amd.buir import BUIRModel
    train = sp.triples(g)
    m = BUIRModel(_conf(g, c), train, train[:10], device="cuda")
    sp.assert_dense_id_order(m, g)
    assert torch.equal(m.target_user, m.online_user.detach()) and torch.equal(m.target_item, m.online_item.detach())
    m.load_reference_state(_init_state(g, c))
    return m


def _views(g, c, m, n):
    """The reference's recorded draws of step n in `draw_views`' layout: COO order -> non-zero order -> bitmaps."""
    import recommendation_amd as ra
    from recommendation_amd import functional as Fn
    adj = m.norm_adj
    coo = ra.CsrGraph.bipartite_raw(m.data.uid_dev, m.data.iid_dev, m.data.user_num, m.data.item_num, "cuda", want_perm=True)
    assert torch.equal(coo.rowptr, adj.rowptr) and torch.equal(coo.col, adj.col)
    nnz = int(g[f"c{c}/nnz"])
    assert nnz == adj.nnz
    keep = np.unpackbits(g[f"c{c}/keep_packed"][n], axis=-1, bitorder="little")[:, :nnz].astype(bool)
    out = []
    for e in (0, 1):
        bits = Fn.pack_bits(torch.from_numpy(keep[e]).cuda()[coo.coo_perm])
        rate = float(g[f"c{c}/rates"][n, e])
        out.append((rate, bits, Fn.mirror_bits(bits, adj.mirror_perm(), nnz)) if e == 0 else (rate, bits))
    return tuple(out)


def _run(g, c):
    m = _model(g, c)
    got = []
    for n in range(int(g["steps"])):
        got.append(m.train_step(sp.batch(g, n, ("users", "items")), views=_views(g, c, m, n)))
    return torch.stack(got).cpu().numpy().astype(np.float64), m


@pytest.mark.parametrize("c", [0, 1])
def test_buir_trajectory_matches_reference_float64(steps, c):
    g = steps
    got, m = _run(g, c)
    sp.check(sp.record("buir", g, c), got, {k: getattr(m, attr).detach().cpu().numpy() for k, attr in NAMES.items()})

    # get_embedding / predict on the final state: the dense float64 formula
    st = {a: getattr(m, a).detach().cpu().double() for a in NAMES.values()}
    n_u = m.data.user_num
    adj = torch.zeros(n_u + m.data.item_num, n_u + m.data.item_num, dtype=torch.float64)
    uid, iid = torch.from_numpy(m.data.uid), torch.from_numpy(m.data.iid) + n_u
    adj.index_put_((uid, iid), torch.ones(len(uid), dtype=torch.float64), accumulate=True)      # duplicates kept (Q1)
    adj.index_put_((iid, uid), torch.ones(len(uid), dtype=torch.float64), accumulate=True)
    e = torch.cat([st["online_user"], st["online_item"]])
    layers = [e]
    for _ in range(m.n_layers):
        layers.append(adj @ layers[-1])
    e = torch.stack(layers, 1).mean(1)
    u_on, i_on = e[:n_u], e[n_u:]
    p_u, p_i = u_on @ st["weight"].T + st["bias"], i_on @ st["weight"].T + st["bias"]
    for have, want in zip(m.get_embedding(), (p_u, u_on, p_i, i_on)):
        assert float((have.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    raw = int(g["user_ids"][5])
    k = m.data.get_user_id(raw)
    score = p_u[k] @ i_on.T + u_on[k] @ p_i.T
    have = m.predict(raw)
    assert have.shape == (m.data.item_num,) and np.abs(have - score.numpy()).max() <= 1e-5 * float(score.abs().max())


def test_the_models_own_draws(steps):
    g = steps
    m = _model(g, 0)
    (r_o, b_o, bt_o), (r_t, b_t) = m.draw_views(3)
    (r_o2, b_o2, bt_o2), (r_t2, b_t2) = m.draw_views(3)
    assert (r_o, r_t) == (r_o2, r_t2) and torch.equal(b_o, b_o2) and torch.equal(bt_o, bt_o2) and torch.equal(b_t, b_t2)
    assert 0 <= r_o < m.drop_rate and 0 <= r_t < m.drop_rate and r_o != r_t
    assert not torch.equal(b_o, b_t)                                # the two encoders draw their own masks
    assert not torch.equal(m.draw_views(4)[0][1], b_o)
    from recommendation_amd import functional as Fn
    adj, nnz = m.norm_adj, m.norm_adj.nnz
    assert torch.equal(bt_o, Fn.mirror_bits(b_o, adj.mirror_perm(), nnz))
    # the dropped operator of one step: kept non-zeros carry 1 / (1 - rate), the others nothing
    e = torch.arange(nnz, device="cuda")
    keep = ((b_o[e >> 5] >> (e & 31)) & 1).bool()
    assert 0 < int((~keep).sum()) < nnz
    x = torch.randn(adj.n_cols, 16, generator=torch.Generator().manual_seed(0)).cuda()
    rows = torch.repeat_interleave(torch.arange(adj.n_rows, device="cuda"), adj.rowptr[1:] - adj.rowptr[:-1])
    want = torch.zeros(adj.n_rows, 16, device="cuda", dtype=torch.float64)
    want.index_add_(0, rows[keep], x.double()[adj.col.long()[keep]] * (1.0 / (1.0 - r_o)))
    have = Fn.spmm(adj, x, keep_bits=b_o, val_scale=1.0 / (1.0 - r_o))
    assert float((have.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_train_end_to_end_and_state_round_trip(steps):
    from recommendation_amd.buir import BUIRModel
    g = steps
    train = sp.triples(g)
    m = BUIRModel(_conf(g, 1, batch_size=256), train[:1200], train[1200:], device="cuda", seed=2)
    before = m.target_user.clone()
    metrics = m.train()
    assert set(metrics) == {"Hit Ratio", "Precision", "Recall", "NDCG"} and all(np.isfinite(v) for v in metrics.values())
    assert m.step_count == 5 and m.bestPerformance[0] == 1          # one epoch (range(1)) of ceil(1200 / 256) batches
    assert not torch.equal(before, m.target_user)
    state = m.reference_state()
    assert set(state) == set(NAMES)
    other = BUIRModel(_conf(g, 1), train[:1200], train[1200:], device="cuda", seed=9)
    assert not torch.equal(other.weight, m.weight)
    other.load_reference_state(state)
    for attr in NAMES.values():
        assert torch.equal(getattr(other, attr).detach(), getattr(m, attr).detach()), attr
    with pytest.raises(ValueError):
        other.load_reference_state({**state, "predictor.bias": np.zeros(3, dtype=np.float32)})
