"""tests/golden/diffnet_steps.npz re-checked from its stored numbers, and DiffNetModel's host logic against it (no GPU):
self-consistency, step_pins' sensitivity rule, the writer's two seed conditions (Adam, ReLU margin), the float64 composition
against the component cases, the two COO operators, the regU quirk."""
import os

import numpy as np
import pytest
import torch

import diffnet_fixture as dfx
import step_pins as sp


@pytest.fixture(scope="module")
def g():
    return dfx.load()


def test_fixture_is_self_consistent(g):
    assert os.path.getsize(os.path.join(sp.GOLDEN, "diffnet_steps.npz")) < 1_000_000
    steps, batch = int(g["steps"]), int(g["batch_size"])
    assert (steps, int(g["configs"])) == (6, 2) and "regU" in dfx.conf(g, 0)
    assert [(int(g[f"c{c}/n_layer"]), int(g[f"c{c}/d"])) for c in (0, 1)] == [(2, 64), (3, 32)]
    n_u, n_i = g["user_ids"].size, g["item_ids"].size
    for n in range(steps):
        u, i, j = dfx.batch_arrays(g, n)
        assert sorted(g[f"batch{n}_perm"].tolist()) == list(range(batch))       # the whole training list, shuffled
        assert u.shape == i.shape == j.shape == (batch,)
        assert 0 <= u.min() and u.max() < n_u and 0 <= min(i.min(), j.min()) and max(i.max(), j.max()) < n_i
        assert len(set(u.tolist())) < batch                                   # users recur inside a batch
    for c in (0, 1):
        d, layers = int(g[f"c{c}/d"]), int(g[f"c{c}/n_layer"])
        assert dfx.names(g, c) == ["user_embeddings", "item_embeddings"] + [f"weights.{k}" for k in range(layers)]
        shapes = {k: v.shape for k, v in dfx.init(g, c).items()}
        assert shapes["user_embeddings"] == (n_u, d) and shapes["item_embeddings"] == (n_i, d)
        assert all(shapes[f"weights.{k}"] == (2 * d, d) for k in range(layers))
        f64, f32 = g[f"c{c}/f64/losses"], g[f"c{c}/f32/losses"]
        assert f64.shape == f32.shape == (steps, 3) and np.isfinite(f64).all()
        assert np.abs(f64[:, 0] + f64[:, 1] - f64[:, 2]).max() <= 1e-12 * np.abs(f64[:, 2]).max()   # rec + reg = total
        assert (np.abs(f32 - f64) <= 1e-5 * np.abs(f64)).all()
        assert (f64[:, 1] > 0).all()                                           # regU = reg_lambda: 'regU' is in the conf
        rec = dfx.record(g, c)
        for k, t in rec.tables.items():
            assert t.shape == shapes[k] and 0 < np.abs(g[f"c{c}/f64/delta/{k}"]).max() < 1e-1


@pytest.mark.parametrize("c", [0, 1])
def test_sensitivity_rule_holds_from_the_stored_numbers(g, c):
    rec = dfx.record(g, c)
    assert set(next(iter(rec.dropped.values()))) == set(dfx.DROPS)
    rec.assert_sensitivity()
    for k in rec.tables:                       # ... and it is not vacuous: every dropped part moves every table
        assert all(rec.dropped[k][t] > sp.DROPPED * rec.atol[k] for t in dfx.DROPS), k


def test_the_writers_seed_conditions(g):
    assert float(g["min_first_grad"]) == 1e-7 and float(g["relu_margin"]) == 8.0
    for c in (0, 1):
        assert float(g[f"c{c}/first_grad"]) >= 1e-7
        assert float(g[f"c{c}/min_pre"]) >= 8.0 * float(g[f"c{c}/pre_err"]) > 0
    for d in dfx.COMP_WIDTHS:
        assert float(g[f"comp{d}/min_pre"]) >= 8.0 * float(g[f"comp{d}/pre_err"]) > 0


def _cpu_graph(row, col, val, n_rows, n_cols):
    import recommendation_amd as ra
    return ra.CsrGraph.from_coo(row, col, val, n_rows, n_cols, "cpu")


@pytest.mark.parametrize("d", dfx.COMP_WIDTHS)
def test_composed_layer_in_float64_equals_the_component_case(g, d):
    from recommendation_amd import functional as Fn
    c = dfx.component(g, d)
    n = dfx.COMP_N
    deg = np.bincount(c["row"], minlength=n)
    assert deg[0] == 0 and deg[1] == 1 and deg[3] == 300 and deg[-1] > 0 and ((c["row"] == 2) & (c["col"] == 2)).any()
    assert len(set(c["col"][c["row"] == 3].tolist())) < 300 and (c["g"] == 0).any() and not c["g"][5].any()
    graph = _cpu_graph(c["row"], c["col"], c["val"], n, n)
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    w = torch.from_numpy(c["w"]).double().requires_grad_(True)
    for layer in (Fn.diffuse_layer_composed, Fn.diffuse_layer):            # a CPU tensor takes the composition
        x.grad = w.grad = None
        h = layer(graph, x, w)
        h.backward(torch.from_numpy(c["g"]).double())
        for k, have in (("h", h.detach()), ("dx", x.grad), ("dw", w.grad)):
            assert np.abs(have.numpy() - c[k]).max() <= 1e-12 * c[f"scale/{k}"], (d, k)
        assert 0 < c[f"drift/{k}"] < 1e-5


def test_operators_from_the_models_host_logic_equal_the_references(g):
    from recommendation_amd.diffnet import diffusion_values, rating_coo, social_coo
    user = {int(raw): k for k, raw in enumerate(g["user_ids"])}
    item = {int(raw): k for k, raw in enumerate(g["item_ids"])}
    row, col, val = social_coo(sp.social(g), user)
    assert np.array_equal(row, g["S_row"]) and np.array_equal(col, g["S_col"])
    assert val.dtype == np.float32 and np.array_equal(val, g["S_val"])
    assert len(row) == len(g["social_follower"]) - 2                          # the two pairs naming an unknown user are gone
    uid = np.array([user[int(u)] for u in g["train_user"]])
    iid = np.array([item[int(i)] for i in g["train_item"]])
    r, c, v = rating_coo(uid, iid, len(item))
    assert np.array_equal(r, g["A_row"]) and np.array_equal(c, g["A_col"]) and np.array_equal(v, g["A_val"])
    # neither is a row normalisation: a repeated entry counts once in the denominator and twice in the row sum
    s_sum = np.bincount(g["S_row"], weights=g["S_val"].astype(np.float64), minlength=len(user))
    a_sum = np.bincount(g["A_row"], weights=g["A_val"].astype(np.float64), minlength=len(user))
    assert s_sum.max() > 1.0 + 1e-3 and a_sum.max() > 1.0 + 1e-3
    assert np.abs(a_sum[a_sum <= 1.0 + 1e-3] - 1.0).max() < 1e-6
    assert np.array_equal(diffusion_values([0, 0, 0, 2], [1, 1, 3, 0], 4), np.float32([0.5, 0.5, 0.5, 1.0]))
    assert diffusion_values([], [], 4).shape == (0,)


def test_regu_is_reg_lambda_only_when_the_key_regU_is_present():
    import recommendation_amd as ra
    from recommendation_amd.diffnet import DEFAULT_REG_U, DiffNetModel, reg_u
    assert reg_u({"reg_lambda": 0.5}) == DEFAULT_REG_U == 1e-4
    assert reg_u({"reg_lambda": 0.5, "regU": 0}) == 0.5                      # the key's own value is never read
    assert ra.DiffNetModel is DiffNetModel and ra.DiffNetEncoder.__name__ == "DiffNetEncoder"
    with pytest.raises(AttributeError):
        ra.NoSuchModel
