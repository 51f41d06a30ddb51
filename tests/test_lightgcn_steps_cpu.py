"""tests/golden/lightgcn_steps.npz without a GPU: its size and keys, the facts the GPU test relies on re-checked from the
stored numbers, and the fixture's first step re-derived in float64 by the numpy oracle (oracle/oracle_np.py), which shows
that the generator's LGConv stand-in and the oracle's `gcn_norm_weights` are one operator."""
import os

import numpy as np
import pytest

import step_pins as sp
from lightgcn_steps_common import (CONFIGS, GOLDEN, HYPER, SIZE_CAP, TABLES, adam_on_weight_decay_only, config, final_table,
                                   fixture, init_table, sensitivity_terms, user_major_perm)
from oracle import oracle_np as onp


def test_size_and_schema():
    assert os.path.getsize(GOLDEN) < SIZE_CAP
    g = fixture()
    want = {"train_user", "train_item", "test_user", "test_item", "num_users", "num_items", "steps", "configs", "iso_user",
            "iso_item", "n_dup", "hub_degree", "neg_seed", "min_first_grad"}
    for d in sorted({int(g[f"{c}/embedding_dim"]) for c in CONFIGS}):
        want |= {f"table_seed_d{d}", f"first_grad_d{d}"} | {f"init_d{d}/{k}" for k in TABLES}
    for c in CONFIGS:
        want |= {f"{c}/{k}" for k in HYPER} | {f"{c}/neg_i", f"{c}/f64/loss", f"{c}/f32/loss"}
        for k in TABLES:
            want |= {f"{c}/f64/grad0/{k}", f"{c}/f64/delta/{k}", f"{c}/slack/{k}", f"{c}/drift/{k}", f"{c}/moved/{k}"}
            want |= {f"{c}/delta_{t}/{k}" for t in sensitivity_terms(g, c)}
    assert set(g.files) == want
    assert g["configs"].tolist() == list(CONFIGS)
    nu, ni, steps, e = int(g["num_users"]), int(g["num_items"]), int(g["steps"]), g["train_user"].size
    for c in CONFIGS:
        cfg = config(g, c)
        d = cfg["embedding_dim"]
        assert g[f"{c}/f64/loss"].shape == g[f"{c}/f32/loss"].shape == (steps,)
        assert g[f"{c}/neg_i"].dtype == np.int32
        assert g[f"{c}/neg_i"].shape == ((steps, e) if cfg["n_neg"] == 1 else (steps, e, cfg["n_neg"]))
        for k, rows in zip(TABLES, (nu, ni)):
            assert init_table(g, c, k).dtype == np.float32 and init_table(g, c, k).shape == (rows, d)
            assert g[f"{c}/f64/grad0/{k}"].dtype == np.float64 and g[f"{c}/f64/grad0/{k}"].shape == (rows, d)
            assert g[f"{c}/f64/delta/{k}"].dtype == np.float32 and g[f"{c}/f64/delta/{k}"].shape == (rows, d)
    # the configurations the fixture was asked to hold
    assert config(g, "A") == dict(embedding_dim=64, num_layers=3, loss_type="bpr", n_neg=1, optimizer="Adam", lr=0.01,
                                  reg_weight=1e-4, weight_decay=0.0)
    assert config(g, "B") == dict(embedding_dim=32, num_layers=2, loss_type="bpr", n_neg=3, optimizer="Adam", lr=0.01,
                                  reg_weight=1e-4, weight_decay=1e-4)
    assert config(g, "C") == dict(embedding_dim=128, num_layers=1, loss_type="bce", n_neg=1, optimizer="Adam", lr=0.01,
                                  reg_weight=1e-3, weight_decay=0.0)
    assert config(g, "D") == dict(embedding_dim=64, num_layers=4, loss_type="bpr", n_neg=1, optimizer="SGD", lr=0.05,
                                  reg_weight=1e-4, weight_decay=0.0)


def test_graph_has_the_edge_cases():
    g = fixture()
    u, i = g["train_user"].astype(np.int64), g["train_item"].astype(np.int64)
    nu, ni = int(g["num_users"]), int(g["num_items"])
    iso_u, iso_i = int(g["iso_user"]), int(g["iso_item"])
    # duplicates: n_dup copies, one pair three times
    uniq, counts = np.unique(np.stack([u, i], 1), axis=0, return_counts=True)
    assert u.size - len(uniq) == int(g["n_dup"]) > 0 and counts.max() == 3
    # isolated ids: inside the id range, only in the test split, and the only ones
    assert 0 < iso_u < nu - 1 and 0 < iso_i < ni - 1
    assert set(range(nu)) - set(u.tolist()) == {iso_u} and iso_u in g["test_user"]
    assert set(range(ni)) - set(i.tolist()) == {iso_i} and iso_i in g["test_item"]
    assert u.max() == nu - 1 and i.max() == ni - 1
    # the file order is not the operator's user-major order, and every row of the operator has ascending columns in file
    # order (what a windowed plan of the hub rows needs): item-major
    perm = user_major_perm(g)
    assert not np.array_equal(perm, np.arange(u.size))
    assert np.array_equal(np.lexsort((u, i)), np.arange(u.size))
    assert np.array_equal(perm, np.argsort(u, kind="stable"))
    # hub rows at the GPU test's forced threshold, on both sides
    hub = int(g["hub_degree"])
    assert (np.bincount(u, minlength=nu) > hub).sum() >= 1 and (np.bincount(i, minlength=ni) > hub).sum() >= 2
    for c in CONFIGS:
        neg = g[f"{c}/neg_i"]
        assert neg.min() >= 0 and neg.max() < ni
        assert (neg == iso_i).any()                      # torch.randint does not know that the item has no edge


def test_tolerances_would_see_a_dropped_term():
    g = fixture()
    for c in CONFIGS:
        rec = sp.record("lightgcn", g, c)
        assert rec.factor == sp.DROPPED_CPU and all(tuple(rec.dropped[k]) == sensitivity_terms(g, c) for k in TABLES)
        rec.assert_sensitivity()                                           # every dropped term: more than DROPPED_CPU x atol
        for k in TABLES:
            moved = float(np.abs(rec.tables[k] - init_table(g, c, k).astype(np.float64)).max())
            assert moved == pytest.approx(float(g[f"{c}/moved/{k}"]), abs=4e-9)
            assert sp.has_moved(moved, max(rec.slack[k], sp.FLOOR)), (c, k, moved, rec.slack[k])
            assert 0 < float(g[f"{c}/drift/{k}"]) < 2.5e-6                 # 4 x drift stays under the 1e-5 of the pin rule
        assert np.all(np.abs(rec.f32 - rec.f64) <= sp.REL * np.abs(rec.f64))
    assert sensitivity_terms(g, "B") == ("reg", "wd")
    # the Adam configurations start without a gradient element of Adam's eps' size (the generator's seed scan)
    for c in "ABC":
        d = int(g[f"{c}/embedding_dim"])
        wd = float(g[f"{c}/weight_decay"])                                # Adam adds weight_decay x the table to the gradient
        seen = {k: g[f"{c}/f64/grad0/{k}"] + wd * init_table(g, c, k).astype(np.float64) for k in TABLES}
        gu = np.delete(seen["user"], int(g["iso_user"]), axis=0)
        smallest = min(np.abs(gu).min(), np.abs(seen["item"]).min())
        assert smallest >= float(g[f"first_grad_d{d}"]) >= float(g["min_first_grad"]) >= 3e-7


def test_isolated_rows():
    """The isolated user has no gradient: its row stays (A, C, D) or moves by weight decay alone (B).  The isolated item is
    drawn as a negative and scored by the BCE branch: it has a gradient, and it moves."""
    g = fixture()
    iso_u, iso_i, steps = int(g["iso_user"]), int(g["iso_item"]), int(g["steps"])
    for c in CONFIGS:
        cfg = config(g, c)
        assert not g[f"{c}/f64/grad0/user"][iso_u].any()
        assert g[f"{c}/f64/grad0/item"][iso_i].all()
        row0 = init_table(g, c, "user")[iso_u].astype(np.float64)
        row = final_table(g, c, "user")[iso_u]
        if cfg["weight_decay"]:
            want = adam_on_weight_decay_only(row0, cfg["lr"], cfg["weight_decay"], steps)
            assert np.median(np.abs(want - row0)) > 0.05                   # it does move: about lr per step
            np.testing.assert_allclose(row, want, rtol=0, atol=4e-9)
        else:
            assert np.array_equal(row, row0)
        assert np.abs(final_table(g, c, "item")[iso_i] - init_table(g, c, "item")[iso_i]).min() > 0


def _first_step(g, c):
    """(loss, d loss / d user table, d loss / d item table) of step 0 by the numpy oracle, float64 throughout."""
    cfg = config(g, c)
    u, i = g["train_user"].astype(np.int64), g["train_item"].astype(np.int64)
    nu, n = int(g["num_users"]), int(g["num_users"]) + int(g["num_items"])
    edge_index = onp.build_edge_index(u, i, nu)
    u0, i0 = init_table(g, c, "user"), init_table(g, c, "item")
    ue, ie = onp.lightgcn_forward(edge_index, u0, i0, cfg["num_layers"], weight_dtype=np.float64)
    if cfg["loss_type"] == "bce":
        loss, gu, gi = onp.lightgcn_bce_loss(ue, ie, u, i, reg_weight=cfg["reg_weight"])
    else:
        neg = g[f"{c}/neg_i"][0].astype(np.int64)
        loss = onp.bpr_loss(ue, ie, u, i, neg, variant=onp.BPR_LOG_SIGMOID) \
            + cfg["reg_weight"] * onp.sq_norm_reg(ue[u], ie[i])          # the MEAN of the BPR terms, the SUM of the norms
        gu, gi = onp.bpr_grads(ue, ie, u, i, neg, variant=onp.BPR_LOG_SIGMOID)
        np.add.at(gu, u, 2.0 * cfg["reg_weight"] * ue[u])
        np.add.at(gi, i, 2.0 * cfg["reg_weight"] * ie[i])
    # back through x0 + A x0 + ... + A^K x0 (A symmetric): Horner on A^T
    w = onp.gcn_norm_weights(edge_index, n, np.float64)
    rowptr, col, _, order = onp.coo_to_csr_stable(edge_index[1], edge_index[0], w, n)
    gfin = np.concatenate([gu, gi])
    h = gfin
    for _ in range(cfg["num_layers"]):
        h = gfin + onp.spmm_backward(rowptr, col, w[order], h, n)
    return loss, h[:nu], h[nu:]


@pytest.mark.parametrize("c", ["A", "C", "B"])
def test_first_step_rederived_by_the_numpy_oracle(c):
    """A and C at 1e-12 relative on the loss (and B, whose three negatives are averaged BEFORE the sigmoid); the step-0
    gradients at 1e-10 of their largest element: a global factor such as 1 / E is visible here and not in a trajectory of
    Adam, whose update does not change when the whole gradient is scaled."""
    g = fixture()
    loss, gu, gi = _first_step(g, c)
    ref = float(g[f"{c}/f64/loss"][0])
    assert abs(loss - ref) <= 1e-12 * abs(ref), (loss, ref)
    for k, got in zip(TABLES, (gu, gi)):
        want = g[f"{c}/f64/grad0/{k}"]
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), k
