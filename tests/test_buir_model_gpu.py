"""BUIRModel's training step pinned to univariate/buir.py's own loop body (:194-203) run in float64:
tests/golden/buir_steps.npz, written by scripts/gen_golden_buir_steps.py.  Six batches of the reference's sampler from the
fixture's initial state with the reference's recorded dropout draws, two configurations (2 layers, d = 64, tau 0.5;
3 layers, d = 32, tau 0.1).

Tolerances are those of tests/test_sept_model_gpu.py: a loss within max(1e-5 rel, 4 x the reference's own |f32 - f64|), each
of the six final tensors within 4 x the reference's own f32 slack on it (floored at 1e-7), that tolerance at most 1/50 of
what dropping `update_target` or the `loss_iu` term moves the tensor."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "buir_steps.npz")
NAMES = {"online_encoder.embedding_dict.user_emb": "online_user", "online_encoder.embedding_dict.item_emb": "online_item",
         "target_encoder.embedding_dict.user_emb": "target_user", "target_encoder.embedding_dict.item_emb": "target_item",
         "predictor.weight": "weight", "predictor.bias": "bias"}


@pytest.fixture(scope="module")
def steps():
    return np.load(GOLDEN)


def _conf(g, c, batch_size=None):
    return {"model": {"name": "BUIR", "type": "graph"}, "emb_size": int(g[f"c{c}/d"]), "lr": float(g["hp/lr"]),
            "batch_size": batch_size or int(g["batch_size"]), "item.ranking.topN": [10, 20],
            "BUIR": {"n_layer": int(g[f"c{c}/n_layer"]), "tau": float(g[f"c{c}/tau"]), "drop_rate": float(g["hp/drop_rate"])}}


def _triples(g):
    return [[int(u), int(i), 1.0] for u, i in zip(g["train_user"], g["train_item"])]


def _init_state(g, c):
    state = {}
    for k in NAMES:
        state[k] = g[f"c{c}/init/" + k.replace("target_encoder", "online_encoder")]     # _init_target: copies
    return state


def _model(g, c):
    from recommendation_amd.buir import BUIRModel
    train = _triples(g)
    m = BUIRModel(_conf(g, c), train, train[:10], device="cuda")
    assert [m.data.id2user[k] for k in range(m.data.user_num)] == g["user_ids"].tolist()
    assert [m.data.id2item[k] for k in range(m.data.item_num)] == g["item_ids"].tolist()
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
        batch = tuple(torch.from_numpy(g[f"batch{n}_{s}"].astype(np.int64)).cuda() for s in ("users", "items"))
        got.append(m.train_step(batch, views=_views(g, c, m, n)))
    return torch.stack(got).cpu().numpy().astype(np.float64), m


@pytest.mark.parametrize("c", [0, 1])
def test_buir_trajectory_matches_reference_float64(steps, c):
    g = steps
    got, m = _run(g, c)
    report, failures = [f"config {c}:"], []
    ref, f32 = g[f"c{c}/f64/losses"], g[f"c{c}/f32/losses"]
    tol = np.maximum(1e-5 * np.abs(ref), 4 * np.abs(f32 - ref))
    err = np.abs(got - ref)
    report.append(f"  loss: max err {err.max():.3g} (max rel {np.max(err / np.abs(ref)):.3g})")
    if not np.all(err <= tol):
        failures.append(f"loss: got {got.tolist()} reference {ref.tolist()}")
    init = _init_state(g, c)
    for k, attr in NAMES.items():
        final = getattr(m, attr).detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(final).all(), k
        want = init[k].astype(np.float64) + g[f"c{c}/f64/delta/{k}"].astype(np.float64)
        slack = float(g[f"c{c}/slack/{k}"])
        atol = max(4 * slack, 1e-7)
        err = float(np.abs(final - want).max())
        deltas = {t: float(g[f"c{c}/delta_{t}/{k}"]) for t in ("update", "iu")}
        report.append(f"  {k}: max err {err:.3g} ({err / atol:.2f} x atol {atol:.3g}, reference f32 slack {slack:.3g}); a dropped "
                      "part moves it by " + ", ".join(f"{t} {v:.3g}" for t, v in deltas.items()))
        for t, v in deltas.items():                             # a tolerance that would not see a missing part checks nothing
            assert v > 50 * atol, (k, t, v, atol)
        if err > atol:
            failures.append(f"{k}: max |final - f64| = {err:.3g} > atol {atol:.3g}")
    print("\n".join(report))
    assert not failures, "\n".join(report + failures)

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
    train = _triples(g)
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
