"""GraphSAGE without a device: the float64 restatement (tests/sage_rules.py) and functional.sage_layer_composed against the
fixture's layer cases and step trajectories (tests/golden/sage_steps.npz, written from graphsage.py itself), the fixture's
stored conditions, the mean operator, the module's shapes and quirks, the ABI table, the conditions of the builders that
tests/test_sage_paths_gpu.py runs on the device, and `GraphSAGE.prepare`'s cache."""
import os

import numpy as np
import pytest
import torch

import sage_rules as sr
import step_pins as sp
from gcr_header import header_prototypes

# a float64 result stored as float32 carries at most 2^-24 of its scale; twice that is asked of a float64 recomputation
STORED = 2.0 ** -23
SAGE_EXPORTS = ("gcr_sage_supported", "gcr_sage_workspace_bytes", "gcr_sage_fwd_f32", "gcr_sage_bwd_f32")


@pytest.fixture(scope="module")
def golden():
    return sr.load()


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _close(got, ref, tag):
    for k, want in ref.items():
        scale = float(np.abs(want).max()) or 1.0
        err = float(np.abs(np.asarray(got[k], dtype=np.float64) - want).max()) / scale
        print(f"SAGE cpu {tag} {k}: err/S {err:.3g}")
        assert err <= STORED, (tag, k, err)


@pytest.mark.parametrize("din,dout,act", sr.COMP_CASES)
def test_restatement_and_composed_layer_reproduce_the_fixture(golden, din, dout, act):
    from recommendation_amd import functional as Fn
    case = sr.component(golden, din, dout, act)
    got, _ = sr.restatement(case["src"], case["dst"], case["n"], case["x"], case["wl"], case["wr"], case["bias"], case["g"],
                            act, torch.float64, case["keep"], case["p"])
    _close(got, case["ref"], f"restatement ({din}, {dout}) {act}")
    graph = sr.device_graph(case["src"], case["dst"], case["n"], "cpu")
    got = sr.layer(graph, case, device="cpu", fused=False, fn=Fn.sage_layer, dtype=torch.float64)     # falls back: a CPU tensor
    _close(got, case["ref"], f"sage_layer on CPU ({din}, {dout}) {act}")
    got = sr.layer(graph, case, device="cpu", fused=False, fn=Fn.sage_layer_composed, dtype=torch.float64)
    _close(got, case["ref"], f"composed ({din}, {dout}) {act}")
    # the float32 run of the restatement shows the stored drift's size (the same source in float32)
    f32, _ = sr.restatement(case["src"], case["dst"], case["n"], case["x"], case["wl"], case["wr"], case["bias"], case["g"],
                            act, torch.float32, case["keep"], case["p"])
    sr.check(f32, case["ref"], {k: max(v, 2.0 ** -24) for k, v in case["drift"].items()}, f"restatement f32 ({din}, {dout}) {act}")


@pytest.mark.parametrize("case", sr.STEP_CASES)
def test_composed_module_reproduces_the_step_trajectories_in_float64(golden, case):
    """GraphSAGE on CPU tensors in float64 (every layer through sage_layer_composed), torch's own optimisers, the loss as
    graphsage.py:109-121 writes it: the fixture's float64 losses and final parameters."""
    from recommendation_amd.graphsage import GraphSAGE, bipartite_edge_index
    cfg = sr.step_config(golden, case)
    init = sr.step_init(golden, case)
    model = GraphSAGE(64, cfg["hidden_channels"], 64, cfg["n_layers"], cfg["dropout"], cfg["activation"]).double().train()
    model.load_state_dict({k: torch.from_numpy(v).double() for k, v in init.items() if k != "x"})
    x = torch.from_numpy(init["x"]).double()
    pos_u = torch.from_numpy(golden["train_user"].astype(np.int64))
    pos_i = torch.from_numpy(golden["train_item"].astype(np.int64))
    edge_index = bipartite_edge_index(pos_u, pos_i, 120)
    opt = getattr(torch.optim, cfg["optimizer"])(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    losses = []
    for step in range(int(golden["steps"])):
        opt.zero_grad()
        masks = sr.step_masks(golden, case, step, cfg)
        out = model(x, edge_index, masks=None if masks is None else [torch.from_numpy(m) for m in masks])
        u, v = out[:120], out[120:]
        if cfg["loss_type"] == "bpr":
            neg = torch.from_numpy(golden[f"{case}/neg_i"][step].astype(np.int64))
            loss = -torch.log(torch.sigmoid((u[pos_u] * v[pos_i]).sum(-1) - (u[pos_u] * v[neg]).sum(-1))).mean()
        else:
            logits = u[pos_u] @ v.T
            labels = torch.zeros_like(logits)
            labels[torch.arange(len(pos_u)), pos_i] = 1.0
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    np.testing.assert_allclose(losses, golden[f"{case}/f64/loss"], rtol=1e-9)
    _, tables = sr.step_tables(golden, case)
    params = dict(model.named_parameters())
    for k, (ref, _, _, _) in tables.items():
        # float32(final - initial) is exact to 4e-9 (the writer asserts it); the rest is float64 summation order
        assert float(np.abs(params[k].detach().numpy() - ref).max()) < 1e-8, (case, k)


def test_fixture_conditions_hold_from_its_numbers(golden):
    assert os.path.getsize(sr.GOLDEN) < 1_000_000
    assert golden["cases"].tolist() == list(sr.STEP_CASES)
    for case in sr.STEP_CASES:
        cfg = sr.step_config(golden, case)
        sr.assert_sensitivity(golden, case)
        if cfg["activation"] == "relu":
            assert float(golden[f"{case}/relu_margin"]) >= 8.0, case
        assert golden[f"{case}/neg_i"].shape == (int(golden["steps"]), 1200) and golden[f"{case}/neg_i"].max() < 72
        assert (f"{case}/keep0" in golden.files) == (cfg["dropout"] > 0)
        for k in sr.params_of(cfg):
            assert float(golden[f"{case}/slack/{k}"]) >= float(golden[f"{case}/slack_file_order/{k}"])
    a, b, c = (sr.step_config(golden, k) for k in sr.STEP_CASES)
    assert (a["hidden_channels"], a["n_layers"], a["dropout"], a["activation"], a["optimizer"], a["loss_type"]) == \
        (64, 2, 0.0, "relu", "Adam", "bpr")
    assert (b["hidden_channels"], b["n_layers"], b["dropout"], b["activation"], b["optimizer"], b["lr"]) == \
        (128, 3, 0.5, "gelu", "SGD", 0.05)
    assert (c["hidden_channels"], c["loss_type"], c["dropout"], c["optimizer"], c["weight_decay"]) == (32, "bce", 0.2, "AdamW", 1e-3)


@pytest.mark.parametrize("n,din,dout", sr.MULTI_TRIP_SHAPES)
def test_multi_trip_relu_cases_zero_little_of_g(n, din, dout):
    share, _ = sr.zeroed_share(n, din, dout)
    print(f"SAGE zeroed share n={n} ({din}, {dout}): {share:.3g}")
    assert share <= sr.MAX_ZEROED_SHARE


def test_multi_trip_shapes_exceed_the_caps():
    """The derivation beside sage_rules.MULTI_TRIP_SHAPES, from the kernel's constants restated here."""
    for n, din, dout in sr.MULTI_TRIP_SHAPES:
        fwd_rows = 64 if din <= 64 else 32
        assert -(-n // fwd_rows) == sr.FWD_CAP + 1 and -(-(n - 1) // fwd_rows) == sr.FWD_CAP      # the smallest n over the forward's cap
        assert -(-n // 32) > sr.BWD_CAP and n % 32 == 1
    classes = {((64 if a <= 64 else 32), a * b <= 4096) for a, b in sr.PAIRS}
    assert classes == {((64 if a <= 64 else 32), a * b <= 4096) for _, a, b in sr.MULTI_TRIP_SHAPES}
    # the workspace tells the backward's cap: one partial per workgroup behind [wl^T; wr^T]
    from recommendation_amd import _lib
    w = 2 * 32 * 32
    assert _lib.call("gcr_sage_workspace_bytes", 10 ** 7, 32, 32) == 4 * (w + sr.BWD_CAP * (w + 32))


def test_mean_graph_counts_duplicates_keeps_self_loops_and_leaves_isolated_rows_empty():
    from recommendation_amd import functional as Fn
    # edges j -> i: 0 -> 1 twice (a duplicate), 2 -> 1, 1 -> 1 (a self loop), 1 -> 0, 3 -> 2; node 3 has no in-edge, node 4 none at all
    ei = torch.tensor([[0, 2, 0, 1, 1, 3], [1, 1, 1, 1, 0, 2]])
    g = Fn.sage_mean_graph(ei, 5, "cpu")
    assert (g.n_rows, g.n_cols, g.nnz) == (5, 5, 6)
    assert g.rowptr_host.tolist() == [0, 1, 5, 6, 6, 6]
    assert g.col.tolist() == [1, 0, 2, 0, 1, 3]                        # a row's entries in edge_index order
    np.testing.assert_array_equal(g.val.numpy(), np.float32([1, .25, .25, .25, .25, 1]))
    x = torch.arange(10, dtype=torch.float64).reshape(5, 2)
    z = Fn._sage_mean_torch(g, x)
    want = torch.stack([x[1], (2 * x[0] + x[2] + x[1]) / 4, x[3], torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)])
    assert torch.equal(z, want)
    t = g.t                                                            # built with the graph
    assert (t.n_rows, t.nnz) == (5, 6) and t.rowptr_host.tolist() == [0, 2, 4, 5, 6, 6]
    dense = torch.zeros(5, 5).index_put_((torch.repeat_interleave(torch.arange(5), torch.from_numpy(np.diff(g.rowptr_host))),
                                          g.col.long()), g.val, accumulate=True)
    dense_t = torch.zeros(5, 5).index_put_((torch.repeat_interleave(torch.arange(5), torch.from_numpy(np.diff(t.rowptr_host))),
                                            t.col.long()), t.val, accumulate=True)
    assert torch.equal(dense.T, dense_t)


def test_one_and_two_layers_build_the_same_model():
    from recommendation_amd.graphsage import GraphSAGE
    shapes = [{k: tuple(v.shape) for k, v in GraphSAGE(64, 32, 64, n).state_dict().items()} for n in (1, 2, 3)]
    assert shapes[0] == shapes[1] and len(shapes[0]) == 6 and len(shapes[2]) == 9
    assert shapes[1]["layers.0.lin_l.weight"] == (32, 64) and shapes[1]["layers.1.lin_l.weight"] == (64, 32)
    assert shapes[2]["layers.1.lin_r.weight"] == (32, 32)
    for n in (1, 2, 3):
        cfg = dict(hidden_channels=32, n_layers=n)
        assert {k: tuple(v) for k, v in sr.param_shapes(cfg).items()} == shapes[n - 1]


def test_sageconv_parameter_names_shapes_and_initial_bounds():
    from recommendation_amd.graphsage import SAGEConv
    torch.manual_seed(0)
    conv = SAGEConv(64, 128)
    state = conv.state_dict()
    assert {k: tuple(v.shape) for k, v in state.items()} == \
        {"lin_l.weight": (128, 64), "lin_l.bias": (128,), "lin_r.weight": (128, 64)}
    bound = 1.0 / np.sqrt(64)                                          # kaiming-uniform with a = sqrt(5): +-1 / sqrt(in)
    for v in state.values():
        assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.9 * bound
    assert conv.lin_r.bias is None


def test_unknown_activation_runs_the_composed_layer_with_that_function():
    from recommendation_amd.graphsage import GraphSAGE
    model = GraphSAGE(64, 32, 64, 2, dropout=0.0, activation="elu").double()
    assert model.activation is torch.nn.functional.elu
    src, dst = sr.sweep_graph(12)
    x = torch.from_numpy(sr.inputs(12, 64, 32, 0)[0]).double()
    out = model(x, torch.from_numpy(np.stack([src, dst])))
    conv0, conv1 = model.layers
    z = sr.mean_rows(src, dst, 12, x)
    hid = torch.nn.functional.elu(z @ conv0.lin_l.weight.T + conv0.lin_l.bias + x @ conv0.lin_r.weight.T)
    want = sr.mean_rows(src, dst, 12, hid) @ conv1.lin_l.weight.T + conv1.lin_l.bias + hid @ conv1.lin_r.weight.T
    assert float((out - want).abs().max()) < 1e-12


def test_lazy_exports():
    import recommendation_amd as ra
    from recommendation_amd import GraphSAGE, GraphSAGEModel, SAGEConv
    assert ra.GraphSAGE is GraphSAGE and GraphSAGEModel.DEFAULTS["optimizer"] == "Adam" and SAGEConv is ra.graphsage.SAGEConv


def test_every_sage_declaration_has_its_binding():
    from recommendation_amd import _lib
    protos = header_prototypes()
    for name in SAGE_EXPORTS:
        assert name in protos, f"{name} is not declared in include/gcr.h"
        res, args, names = protos[name]
        assert _lib.SIGNATURES[name] == (res, args), f"{name}: the table disagrees with include/gcr.h"
        assert hasattr(_lib.lib(), name)
    assert sorted(n for n in protos if n.startswith("gcr_sage_")) == sorted(SAGE_EXPORTS)
    assert "gcr_sage_supported" in _lib.INT32_ANSWERS
    assert protos["gcr_sage_fwd_f32"][2][-1] == "stream" and protos["gcr_sage_bwd_f32"][2][-1] == "stream"
    for a in (16, 32, 64, 96, 128, 256):
        for b in (16, 32, 64, 96, 128, 256):
            assert bool(_lib.call("gcr_sage_supported", a, b)) == (a in sr.WIDTHS and b in sr.WIDTHS)
    assert _lib.call("gcr_sage_workspace_bytes", 0, 64, 64) == 0 and _lib.call("gcr_sage_workspace_bytes", 10, 48, 64) == 0
    # [wl^T; wr^T], then one partial of [dwl | dwr] and dbias per workgroup of the backward
    assert _lib.call("gcr_sage_workspace_bytes", 33, 64, 32) == 4 * (2 * 64 * 32 + 2 * (2 * 64 * 32 + 32))


# ---- the builders of tests/test_sage_paths_gpu.py: their conditions, from the restatement alone ----

def test_hub_graph_has_two_hub_rows_in_both_operators_and_out_isolated_nodes():
    from recommendation_amd import functional as Fn
    n = sr.HUB_N
    src, dst = sr.hub_graph(n)
    base_src, base_dst = sr.sweep_graph(n)
    assert np.all(np.diff(dst) >= 0) and src.size == base_src.size + 4 * sr.HUB_EXTRA
    indeg, outdeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    base_in = np.bincount(base_dst, minlength=n)
    hubs = list(sr.hub_nodes(n))
    others = np.setdiff1d(np.arange(n), hubs)
    for hub in hubs:
        assert indeg[hub] >= base_in[hub] + sr.HUB_EXTRA and outdeg[hub] >= sr.HUB_EXTRA
        row = src[dst == hub]
        assert np.all(np.diff(row) >= 0)                                # what the windowed plan asks of a hub row
        targets = dst[src == hub]
        assert np.unique(targets).size >= sr.HUB_EXTRA                  # distinct targets: unequal values 1 / deg(dst) in A^T
        assert np.unique(indeg[targets]).size > 3
    assert indeg[others].max() <= max(sr.DEGREES) + len(hubs) and outdeg[others].max() < 128      # nobody else is a hub
    # every other row keeps sweep_graph's entries in their order, then the hubs' edges
    r = 7
    assert src[dst == r][:base_in[r]].tolist() == base_src[base_dst == r].tolist()
    lonely = sr.out_isolated(src, n)
    print(f"SAGE hub graph: {lonely.size} nodes without out-edges, in-degrees {indeg[hubs]}, out-degrees {outdeg[hubs]}")
    assert lonely.size >= 1
    # the plan's own conditions, on the operator functional.sage_mean_graph builds (a CPU graph plans the same way)
    graph = sr.device_graph(src, dst, n, "cpu")
    for g in (graph, graph.t):
        assert g.hub is not None and g.hub.n_hub == 2 and not g.hub.forced
        assert g.hub.eligible(64) and not g.hub.eligible(32) and not g.hub.eligible(128)
        assert g.rows_p is None
    assert sorted(graph.hub.hub_row_host.tolist()) == hubs == sorted(graph.t.hub.hub_row_host.tolist())
    from recommendation_amd import graph as G
    assert (n - 2) * 4 * 64 < G.HUB_MIN_TABLE_BYTES <= (n - 1) * 4 * 64   # one row above the smallest table that qualifies
    assert Fn.WINDOWED_MAX_D >= 64


@pytest.mark.parametrize("din,dout", sr.HUB_PAIRS)
def test_hub_relu_cases_zero_little_of_g(din, dout):
    share, _ = sr.zeroed_share(sr.HUB_N, din, dout, graph=sr.hub_graph)
    print(f"SAGE hub zeroed share n={sr.HUB_N} ({din}, {dout}): {share:.3g}")
    assert share <= sr.MAX_ZEROED_SHARE


@pytest.mark.parametrize("with_bias", (True, False))
@pytest.mark.parametrize("act", ("none", "relu"))
@pytest.mark.parametrize("din,dout", sr.PAIRS)
def test_exact_cases_are_exact_in_float32(din, dout, act, with_bias):
    case = sr.exact_case(din, dout, act, with_bias)
    assert case["n"] == 70 and case["n"] % 32 and case["n"] % 64
    assert set(np.bincount(case["dst"], minlength=case["n"]).tolist()) == set(sr.EXACT_DEGREES)
    assert case["p"] in (0.5, 0.75) and set(case["ref"]) == set(sr.KEYS if with_bias else sr.KEYS[:-1])
    for k, want in case["ref"].items():
        assert np.array_equal(case["f32"][k], want), k                  # float32 is exact here
    for k in ("dx", "dwl", "dwr"):
        assert np.abs(case["ref"][k]).max() > 0, k
    for k in ("x", "wl", "wr", "g"):
        assert np.array_equal(case[k], np.rint(case[k]))
    pre, g, keep, c = case["pre"], case["g"], case["keep"], case["zero_col"]
    assert np.all(g != 0)
    assert np.all(pre[:, c] == 0) and keep[:, c].any() and not keep[:, c].all()
    if act == "relu":
        assert (pre == 0).mean() > 0.005 and (pre > 0).any() and (pre < 0).any()   # zeros beyond the planted ones, too
        # torch's convention: no gradient at 0, which the column's parameters show
        assert np.all(case["ref"]["dwl"][c] == 0) and np.all(case["ref"]["dwr"][c] == 0)
        if with_bias:
            assert case["ref"]["dbias"][c] == 0
            # ... and `>=` in its place would show: the column's kept g does not sum to 0
            assert (g[:, c] * keep[:, c]).sum() != 0
    if with_bias:
        assert case["zero_row"] is None
    else:
        r = case["zero_row"]
        assert np.all(pre[r] == 0) and keep[r].any() and case["bias"] is None
        assert not np.any(case["dst"] == r) and not np.any(case["x"][r])


@pytest.mark.parametrize("din,dout", ((64, 64), (128, 32)))
def test_tail_cases_reach_past_ten(din, dout):
    case = sr.tail_case(257, din, dout)
    print(f"SAGE tail ({din}, {dout}): pre in [{case['pre'].min():.3g}, {case['pre'].max():.3g}]")
    assert case["pre"].max() >= 10.0 and case["pre"].min() <= -10.0 and case["act"] == "gelu" and case["p"] == 0.5


def test_prepare_holds_its_edge_index_so_that_a_recycled_address_is_not_a_hit():
    """GraphSAGE.prepare on CPU tensors (tests/prepare_cache.py)."""
    from prepare_cache import check_prepare_cache
    from recommendation_amd import functional as Fn
    from recommendation_amd.graphsage import GraphSAGE
    model, n = GraphSAGE(64, 32, 64, 2), 50
    check_prepare_cache(lambda e: model.prepare(e, n), lambda e: Fn.sage_mean_graph(e, n, "cpu"), n)
    e = torch.randint(0, n, (2, 400))
    assert model.prepare(e, n + 1) is not model.prepare(e, n)           # num_nodes is part of the key
