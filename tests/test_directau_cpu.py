"""DirectAU without a GPU: that tests/golden/directau_steps.npz holds what tests/test_directau_gpu.py relies on (the
conditions scripts/gen_golden_directau.py asserted on the reference's runs, re-checked on the stored numbers), the conf
schema of DirectAUModel, the sorted-id maps, and FusedSGD's state layout."""
import numpy as np
import pytest
import torch

import directau_fixture as fx
import step_pins as sp


def test_component_cases_cover_the_grid():
    g, cases, _ = fx.load()
    ds, bs = {c.d for c in cases}, {c.batch for c in cases}
    assert ds == {16, 64, 100, 512} and bs == {1, 2, 127, 512, 2048}
    assert any(c.d == 512 and c.batch == 2048 for c in cases) and any(c.d == 100 for c in cases)
    assert any(c.zero_row for c in cases)
    assert len({c.gamma for c in cases}) >= 3 and len({c.t for c in cases}) >= 3
    for c in cases:
        ut, it, u, i, j = c.inputs()                               # CRC-checked regeneration
        assert ut.shape == c.shape("user_emb") and it.shape == c.shape("item_emb") and ut.dtype == np.float32
        assert u.shape == i.shape == j.shape == (c.batch,) and u.max() < c.n_users and max(i.max(), j.max()) < c.n_items
        if c.batch >= 512:                                         # a table smaller than the batch: ids recur
            assert len(set(u.tolist())) < c.batch and len(set(i.tolist())) < c.batch
        if c.zero_row:
            assert not ut[u].any(axis=1).all() and not it[i].any(axis=1).all() and not it[j].any(axis=1).all()
        assert c.value("sums").shape == (8,)
        for name in fx.VALUES:
            assert np.all(np.isfinite(c.value(name))) and np.all(c.value_slack(name) >= 0)
        for obj in fx.OBJECTIVES:
            for tab in fx.TABLES:
                size = int(np.prod(c.shape(tab)))
                assert c.grad(obj, tab).shape == c.index(tab).shape and 0 <= min(size, fx.SAMPLE) - c.index(tab).size <= c.d * c.zero_row
                if c.zero_row:            # the zero row is held apart: its gradient dwarfs every other row's bound
                    zg, zslack, zmax = c.zero_grad(obj, tab)
                    assert zg.shape == (c.d,) and zmax > 1e6 * c.grad_max(obj, tab) and 0 <= zslack < 1e-4 * zmax
                    assert not np.any(c.index(tab) // c.d == c.zero_index(tab))
                assert np.abs(c.grad(obj, tab)).max() <= c.grad_max(obj, tab) and c.grad_slack(obj, tab) >= 0
        if c.batch == 1:                                           # directau.py:251: no pair, uniformity 0.0
            assert c.value("unif_u") == 0 and c.value("sums")[2:5].tolist() == [0, 0, 0]


def test_component_sums_restate_the_reference_values():
    """sums = [B x alignment, pairs x (exp(uniformity) - 1e-8), ||x||_F^2]: the identities the GPU test leans on when it
    holds `au_sums` to the fixture."""
    _, cases, _ = fx.load()
    for c in cases:
        s, pairs = c.value("sums"), c.batch * (c.batch - 1) / 2
        assert s[0] == pytest.approx(c.value("align_pos") * c.batch, rel=1e-12)
        assert s[1] == pytest.approx(c.value("align_neg") * c.batch, rel=1e-12)
        if c.batch >= 2:
            for k, name in enumerate(("unif_u", "unif_p", "unif_n")):
                assert np.log(s[2 + k] / pairs + 1e-8) == pytest.approx(float(c.value(name)), rel=1e-9, abs=1e-12)
        ut, it, u, i, j = c.inputs()
        for k, x in enumerate((ut[u], it[i], it[j])):
            assert s[5 + k] == pytest.approx(float((x.astype(np.float64) ** 2).sum()), rel=1e-12)
        if c.t == 2:                      # calculate_loss takes uniformity at its default t = 2 (directau.py:242)
            lo = 0.5 * c.gamma * (c.value("unif_u") + c.value("unif_p"))
            assert c.value("calc_pos") == pytest.approx(float(c.value("align_pos") + lo), rel=1e-9)


def test_trajectories_hold_what_the_gpu_test_relies_on():
    g, _, configs = fx.load()
    assert {c.n_layers for c in configs} == {1, 2, 3} and {c.gamma for c in configs} == {0.5, 1.0, 3.0}
    assert {c.emb for c in configs} == {32, 64} and {c.optimizer for c in configs} == {"adam", "sgd"}
    assert int(g["steps"]) == 6 and float(g["learning_rate"]) in (1e-5, 5e-5, 1e-4, 5e-4, 1e-3, 5e-3)
    n_u, n_i = len(g["user_ids"]), len(g["item_ids"])
    assert (n_u, n_i) == (160, 96) and 900 <= len(g["train_user"]) <= 1100
    for u, p, n in fx.batches(g):
        assert u.shape == p.shape == n.shape == (int(g["batch_size"]),) and u.max() < n_u and max(p.max(), n.max()) < n_i
    reg_seen = False
    for c in configs:
        rec = c.record()
        f64 = dict(zip(fx.TERMS, rec.f64.T))
        assert rec.f64.shape == (6, 4) and np.all(np.abs(rec.f32 - rec.f64) <= 2.5e-6 * np.abs(rec.f64) * (1 + 1e-9))
        # loss = pos_loss - neg_loss + l2 / batch.size (directau.py:225-226)
        np.testing.assert_allclose(f64["loss"], f64["pos_loss"] - f64["neg_loss"] + f64["l2"] / int(g["batch_size"]),
                                   rtol=0, atol=1e-12)
        for tab, rows in zip(fx.TABLES, (n_u, n_i)):
            assert c.init(tab).shape == rec.tables[tab].shape == (rows, c.emb) and c.init(tab).dtype == np.float32
        rec.assert_sensitivity()                                    # the MOVED rule, on the reference's own finals
        seen = {term: max(rec.dropped[tab][term] / rec.atol[tab] for tab in fx.TABLES) >= sp.DROPPED_CPU for term in fx.DROPPED}
        assert seen["gamma"] and seen["neg"], (c, seen)
        reg_seen = reg_seen or seen["reg"]
    assert reg_seen                      # some configuration shows the regulariser (the generator says which and why)


def test_conf_schema():
    from recommendation_amd.directau import DirectAUModel
    with pytest.raises(KeyError):
        DirectAUModel({"embedding.size": 16}, [("a", "b", 1.0)], [], device="cpu")
    with pytest.raises(KeyError):
        DirectAUModel({"DirectAU": {"gamma": 1.0}}, [("a", "b", 1.0)], [], device="cpu")
    with pytest.raises(ValueError, match="Unsupported optimizer"):
        DirectAUModel({"DirectAU": {"gamma": 1.0, "n_layers": 2}, "optimizer": "rmsprop"}, [("a", "b", 1.0)], [], device="cpu")


def test_sorted_id_maps():
    """directau.py:116-117: dense ids follow the sorted raw ids (strings by code point), not the order of appearance —
    the order the fixture's batches index."""
    from recommendation_amd.encoders import Interaction
    g, _, _ = fx.load()
    train = fx.train_records(g)
    data = Interaction({}, train, [], device="cpu")
    assert (data.user_num, data.item_num) == (160, 96)
    assert [data.id2user[k] for k in range(data.user_num)] == [str(s) for s in g["user_ids"]] == sorted({t[0] for t in train})
    assert [data.id2item[k] for k in range(data.item_num)] == [str(s) for s in g["item_ids"]] == sorted({t[1] for t in train})
    assert list(dict.fromkeys(t[0] for t in train)) != sorted({t[0] for t in train})     # the two orders do differ here
    assert data.norm_adj.nnz == 2 * len(train)                                           # raw adjacency, duplicates kept


def test_fused_sgd_state_dict_has_torch_sgd_keys():
    from recommendation_amd.optim import FusedSGD
    p = torch.nn.Parameter(torch.zeros(6, 4))
    q = torch.nn.Parameter(torch.zeros(6, 4))
    ours, theirs = FusedSGD([p], lr=0.01, momentum=0.9, weight_decay=1e-2), torch.optim.SGD([q], lr=0.01, momentum=0.9, weight_decay=1e-2)
    a, b = ours.state_dict(), theirs.state_dict()
    assert set(a) == set(b) and len(a["param_groups"]) == len(b["param_groups"]) == 1
    assert set(a["param_groups"][0]) == set(b["param_groups"][0])
    for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"):
        assert a["param_groups"][0][k] == b["param_groups"][0][k]
    # a stepped torch.optim.SGD's state loads into FusedSGD and comes back under the same key
    q.grad = torch.ones_like(q)
    theirs.step()
    ours.load_state_dict(theirs.state_dict())
    st = ours.state_dict()["state"]
    assert list(st) == [0] and set(st[0]) == {"momentum_buffer"} == set(theirs.state_dict()["state"][0])
    assert torch.equal(st[0]["momentum_buffer"], torch.ones(6, 4))
    theirs.load_state_dict(ours.state_dict())
    with pytest.raises(ValueError):
        FusedSGD([p], lr=-1.0)
