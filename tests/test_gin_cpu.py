"""BGRL / GIN without a device: the conditions of the builders that tests/test_gin_gpu.py and tests/test_gin_paths_gpu.py run
on the device (margins, exactness, the degree cycle, the launch shapes), functional.gin_layer_composed in float64 against the
fixture's layer cases (tests/golden/bgrl_steps.npz, written from bgrl_g2l.py itself), the fixture's stored conditions, the
sum operator and its edge-order maps, BGRLModel on CPU tensors in float64 against the trajectories (which pins the quirks
the module docstring lists), the module's names and the ABI table."""
import os
import re

import numpy as np
import pytest
import torch

import gin_rules as gr
import step_pins as sp
from gcr_header import header_prototypes

# a float64 result stored as float32 carries at most 2^-24 of its scale; twice that is asked of a float64 recomputation
STORED = 2.0 ** -23
GIN_EXPORTS = ("gcr_gin_supported", "gcr_gin_workspace_bytes", "gcr_gin_fwd_f32", "gcr_gin_bwd_f32")
N = 137                     # tests/test_gin_gpu.py's


@pytest.fixture(scope="module")
def golden():
    return gr.load()


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
        print(f"GIN cpu {tag} {k}: err/S {err:.3g}")
        assert err <= STORED, (tag, k, err)


# ---- the builders' own conditions ----

@pytest.mark.parametrize("din,dout,p,edge_p", ((32, 32, 0.0, 0.0), (64, 128, 0.5, 0.3), (128, 64, 0.5, 0.0)))
def test_margin_cases_keep_the_margin_at_both_relus(din, dout, p, edge_p):
    case = gr.margin_case(N, din, dout, p, edge_p)
    assert N % 32 and N % 64
    for pre64, pre32 in zip(case["pre"], case["pre32"]):
        assert pre64.shape == (N, dout) and gr.has_margin(pre64, pre32) and gr.margin_of(pre64, pre32) >= 8.0
    assert (case["keep"] is None) == (p == 0.0) and (case["edge_keep"] is None) == (edge_p == 0.0)
    for k in gr.KEYS:
        assert np.abs(case["ref"][k]).max() > 0 and case["drift"][k] < 1e-5, k
    # the restatement and the composed layer are the same function
    got = gr.layer(gr.device_graph(case["src"], case["dst"], N, "cpu"), case, device="cpu", fused=False, dtype=torch.float64)
    for k in gr.KEYS:
        assert np.abs(got[k] - case["ref"][k]).max() <= 1e-12 * np.abs(case["ref"][k]).max(), k


def test_the_sweep_graph_cycles_through_the_degrees():
    src, dst = gr.sweep_graph(N)
    deg = np.bincount(dst, minlength=N)
    assert deg[1] == 0 and all(deg[r] == gr.DEGREES[r % 10] for r in range(N) if r != 1)
    assert bool((src == dst).any()) and any(np.unique(src[dst == r]).size < deg[r] for r in range(N) if deg[r] >= 2)


@pytest.mark.parametrize("n,din,dout,dense", [(70, a, b, True) for a, b in gr.PAIRS] +
                         [s + (False,) for s in gr.FWD_TRIP_SHAPES[:1] + gr.BWD_TRIP_SHAPES])
def test_exact_cases_are_exact_in_float32(n, din, dout, dense):
    """float32 reproduces float64 bit for bit, `exact_bounds` says why, and the planted zero columns sit on both kinks
    under a non-zero upstream gradient."""
    case = gr.exact_case(n, din, dout, dense=dense)
    assert max(case["bounds"].values()) < gr.EXACT_LIMIT
    for k, want in case["ref"].items():
        assert np.array_equal(case["f32"][k], want) and np.abs(want).max() > 0, k
        assert np.array_equal(want, np.round(want)), k
    zc = case["zero_col"]
    pre1, pre2 = case["pre"]
    assert not pre1[:, zc].any() and not pre2[:, zc + 1].any() and bool(case["g"].all())
    assert not case["ref"]["dw1"][zc].any() and not case["ref"]["db1"][zc] and not case["ref"]["db2"][zc + 1]
    assert (pre1 == 0).mean() < 0.5 and (pre2 > 0).mean() > 0.1


def test_launch_shapes_follow_the_kernels_constants():
    """gin_rules restates csrc/gcr_gin.hip's tile heights, caps and LDS rule; the shapes of tests/test_gin_paths_gpu.py are
    derived from them, one per (tile rows, weights in LDS) class."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "recommendation_amd", "csrc", "gcr_gin.hip")).read()
    for name, value in (("FWD_CAP", gr.FWD_CAP), ("BWD_CAP", gr.BWD_CAP), ("BWD_ROWS", gr.BWD_ROWS)):
        assert re.search(rf"constexpr int {name} = {value};", src), name
    assert "return dout <= 64 ? 64 : 32;" in src and "return (din + dout) * dout <= 8192;" in src
    assert {gr.fwd_class(a, b) for a, b in gr.PAIRS} == {gr.fwd_class(a, b) for a, b in gr.FWD_TRIP_PAIRS}
    assert {gr.bwd_class(a, b) for a, b in gr.PAIRS} == {gr.bwd_class(a, b) for a, b in gr.BWD_TRIP_PAIRS} \
        == {gr.bwd_class(a, b) for a, b in gr.FWD_TRIP_PAIRS}
    for n, din, dout in gr.FWD_TRIP_SHAPES:
        rows = gr.fwd_rows(dout)
        assert -(-n // rows) == gr.FWD_CAP + 1 and -(-(n - 1) // rows) == gr.FWD_CAP and -(-n // gr.BWD_ROWS) > gr.BWD_CAP
    for n, din, dout in gr.BWD_TRIP_SHAPES:
        assert -(-n // gr.BWD_ROWS) == gr.BWD_CAP + 1 and -(-(n - 1) // gr.BWD_ROWS) == gr.BWD_CAP
    # the workspace tells the backward's cap: one partial per workgroup behind [w1^T; w2^T]
    from recommendation_amd import _lib
    for din, dout in ((32, 32), (128, 64)):
        assert _lib.call("gcr_gin_workspace_bytes", 10 ** 7, din, dout) == 4 * gr.workspace_words(10 ** 7, din, dout)
        assert _lib.call("gcr_gin_workspace_bytes", 33, din, dout) == 4 * gr.workspace_words(33, din, dout)
    assert _lib.call("gcr_gin_workspace_bytes", 100, 48, 64) == 0 and _lib.call("gcr_gin_workspace_bytes", 0, 64, 64) == 0


def test_hub_case_is_exact_and_has_hub_rows_in_both_operators():
    n = gr.HUB_N
    case = gr.exact_case(n, 64, 32, graph=gr.hub_graph, edge_p=0.0)
    src, dst = case["src"], case["dst"]
    for hub in gr.hub_nodes(n):
        assert (dst == hub).sum() > 3000 and (src == hub).sum() >= 3000
    assert gr.out_isolated(src, n).size >= 1 and max(case["bounds"].values()) < gr.EXACT_LIMIT
    for k, want in case["ref"].items():
        assert np.array_equal(case["f32"][k], want), k


# ---- the sum operator ----

def test_sum_graph_keeps_duplicates_self_loops_edge_order_and_both_edge_maps():
    from recommendation_amd import functional as Fn
    ei = torch.tensor([[2, 0, 2, 3, 3, 1, 2], [0, 0, 0, 3, 1, 2, 0]])          # (2 -> 0) three times, a self loop at 3, node 4 alone
    g = Fn.gin_sum_graph(ei, 5, "cpu")
    assert g.val is None and g.rowptr_host.tolist() == [0, 4, 5, 6, 7, 7] and g.col.tolist() == [2, 0, 2, 2, 3, 1, 3]
    assert g.edge_of_entry.tolist() == [0, 1, 2, 6, 4, 5, 3]
    gt = g.t
    assert gt.rowptr_host.tolist() == [0, 1, 2, 5, 7, 7] and sorted(gt.edge_of_entry.tolist()) == list(range(7))
    for e, entry_edge in enumerate(gt.edge_of_entry.tolist()):                # entry e of A^T is that edge, transposed
        row = int(np.searchsorted(gt.rowptr_host, e, side="right") - 1)
        assert (row, int(gt.col[e])) == (int(ei[0, entry_edge]), int(ei[1, entry_edge]))
    keep = torch.tensor([True, False, True, True, False, True, False])
    bits, bits_t = Fn.gin_edge_keep_bits(g, keep)
    assert Fn.unpack_bits(bits, 7).tolist() == keep[g.edge_of_entry].tolist()
    assert Fn.unpack_bits(bits_t, 7).tolist() == keep[gt.edge_of_entry].tolist()
    x = torch.arange(10, dtype=torch.float64).view(5, 2) + 1
    w1, w2 = torch.eye(2, dtype=torch.float64), torch.eye(2, dtype=torch.float64)
    zero = torch.zeros(2, dtype=torch.float64)
    h = Fn.gin_layer_composed(g, x, w1, zero, w2, zero, 0.0, None, 0.0, bits, bits_t)
    want = x.clone()
    for e in range(7):
        if keep[e]:
            want[ei[1, e]] += x[ei[0, e]]
    assert torch.equal(h, want)
    everything = x.clone()
    for e in range(7):
        everything[ei[1, e]] += x[ei[0, e]]
    assert torch.equal(Fn.gin_layer_composed(g, x, w1, zero, w2, zero, 0.5), everything + 0.5 * x)       # eps = 0.5, no mask


# ---- the fixture ----

@pytest.mark.parametrize("din,dout", gr.COMP_CASES)
def test_restatement_and_composed_layer_reproduce_the_fixture(golden, din, dout):
    from recommendation_amd import functional as Fn
    case = gr.component(golden, din, dout)
    args = (case["src"], case["dst"], case["n"], case["x"], case["w1"], case["b1"], case["w2"], case["b2"], case["g"])
    got, _ = gr.restatement(*args, torch.float64, case["keep"], case["p"], case["edge_keep"])
    _close(got, case["ref"], f"restatement ({din}, {dout})")
    graph = gr.device_graph(case["src"], case["dst"], case["n"], "cpu")
    got = gr.layer(graph, case, device="cpu", fused=False, fn=Fn.gin_layer, dtype=torch.float64)      # falls back: a CPU tensor
    _close(got, case["ref"], f"gin_layer on CPU ({din}, {dout})")
    got = gr.layer(graph, case, device="cpu", fused=False, fn=Fn.gin_layer_composed, dtype=torch.float64)
    _close(got, case["ref"], f"composed ({din}, {dout})")
    f32, _ = gr.restatement(*args, torch.float32, case["keep"], case["p"], case["edge_keep"])
    gr.check(f32, case["ref"], {k: max(v, 2.0 ** -24) for k, v in case["drift"].items()}, f"restatement f32 ({din}, {dout})")


def test_fixture_conditions_hold_from_its_numbers(golden):
    assert os.path.getsize(gr.GOLDEN) < 1_000_000
    assert golden["cases"].tolist() == list(gr.STEP_CASES)
    for case in gr.STEP_CASES:
        cfg = gr.step_config(golden, case)
        gr.assert_sensitivity(golden, case)
        assert float(golden[f"{case}/kink_margin"]) >= 8.0, case
        steps = int(golden[f"{case}/steps"])
        assert 2 <= steps <= 6 and golden[f"{case}/f64/loss"].shape == (steps,)
        assert golden[f"{case}/node"].shape[:2] == (steps, gr.n_node_masks(cfg))
        assert (f"{case}/edge" in golden.files) == (cfg["edge_p"] > 0) and (f"{case}/feat" in golden.files) == (cfg["feat_p"] > 0)
        assert any(gr.is_unreached(k) for k in gr.tensor_shapes(cfg)) and not gr.is_unreached("online_encoder.layers.0.nn.0.bias")
    a, b, c = (gr.step_config(golden, k) for k in gr.STEP_CASES)
    assert (a["hidden_dim"], a["num_layers"], a["dropout"], a["edge_p"], a["feat_p"]) == (32, 2, 0.0, 0.0, 0.0)
    assert (b["hidden_dim"], b["num_layers"], b["dropout"], b["edge_p"], b["feat_p"]) == (64, 3, 0.5, 0.3, 0.3)
    assert (c["hidden_dim"], c["num_layers"], c["dropout"], c["edge_p"], c["feat_p"]) == (128, 1, 0.2, 0.2, 0.1)
    for cfg in (a, b, c):
        assert (cfg["lr"], cfg["weight_decay"]) == (1e-2, 1e-5)


@pytest.mark.parametrize("case", gr.STEP_CASES)
def test_model_on_cpu_tensors_reproduces_the_trajectories_in_float64(golden, case):
    """Every layer through gin_layer_composed, torch's own Adam: the fixture's float64 losses, final parameters, BatchNorm
    buffers and eval-mode scores.  Case A is the one the issue asks for; B and C replay their recorded masks."""
    model, losses = gr.run_steps(golden, case, "cpu", torch.float64)
    np.testing.assert_allclose(losses, golden[f"{case}/f64/loss"], rtol=1e-9)
    finals = gr.finals_of(model, gr.step_config(golden, case))
    first, tables = gr.step_tables(golden, case)
    for k, (ref, _, _, _) in tables.items():
        # float32(final - initial) is exact to 4e-9, or 2^-24 of its size (the writer asserts it); the rest is float64
        # summation order
        assert float(np.abs(finals[k] - ref).max()) <= max(1e-8, STORED * float(np.abs(ref - first[k]).max())), (case, k)
    want = golden[f"{case}/f64/scores"].astype(np.float64)
    got = np.stack([model.predict(int(u)) for u in golden[f"{case}/score_users"]])
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= STORED * float(np.abs(want).max())


def test_reference_named_state_round_trips_and_the_names_are_the_references():
    from recommendation_amd.bgrl import BGRLModel
    train = [[u, i, 1.0] for u in range(6) for i in range(u % 3, 8, 3)]
    m = BGRLModel(dict(hidden_dim=32, num_layers=2), train, [], device="cpu")
    names = set(m.encoder.state_dict())
    for k in ("online_encoder.layers.0.nn.0.weight", "online_encoder.layers.1.nn.2.bias", "online_encoder.batch_norm.norm.weight",
              "online_encoder.projection_head.0.weight", "online_encoder.projection_head.1.norm.running_var",
              "online_encoder.projection_head.2.weight", "predictor.0.bias", "predictor.1.norm.running_mean", "predictor.2.weight"):
        assert k in names, k
    assert not any(k.startswith("target_encoder") for k in names)
    assert [k for k, _ in m.encoder.named_parameters()] == [k for k in gr.tensor_shapes(m.config, buffers=False)
                                                            if not k.startswith("target_encoder.")]
    lin = m.encoder.online_encoder.layers[0].nn[0]
    assert float(lin.weight.detach().abs().max()) <= 1 / np.sqrt(32) and float(m.encoder.predictor[2].weight.detach()) == 0.25
    m.train_step()                                                       # the target encoder exists from the first forward on
    state = {k: v.clone() for k, v in m.encoder.state_dict().items()}
    assert set(gr.tensor_shapes(m.config)) <= set(state)
    other = BGRLModel(dict(hidden_dim=32, num_layers=2), train, [], device="cpu", seed=5)
    other.load_reference_state({k: v for k, v in state.items() if not k.endswith(".eps")})
    for k, v in other.encoder.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert not any(p.requires_grad for p in other.encoder.target_encoder.parameters())
    with pytest.raises(KeyError):
        other.load_reference_state({"online_encoder.layers.0.nn.0.weight": state["online_encoder.layers.0.nn.0.weight"]})


def test_prepare_holds_its_edge_index_so_that_a_recycled_address_is_not_a_hit():
    from prepare_cache import check_prepare_cache
    from recommendation_amd import functional as Fn
    from recommendation_amd.bgrl import GConv
    conv = GConv(32, 32, 2, 0.2, torch.nn.ReLU)
    check_prepare_cache(lambda e: conv.prepare(e, 50), lambda e: Fn.gin_sum_graph(e, 50, "cpu"), 50)


def test_lazy_exports():
    import recommendation_amd as ra
    from recommendation_amd import BGRLModel, BootstrapContrast, BootstrapLatent, Encoder, GConv, GINConv
    assert ra.BGRLModel is BGRLModel and BGRLModel.DEFAULTS["hidden_dim"] == 32 and GINConv is ra.bgrl.GINConv
    assert all(c.__module__ == "recommendation_amd.bgrl" for c in (BootstrapContrast, BootstrapLatent, Encoder, GConv))


def test_every_gin_declaration_has_its_binding():
    from recommendation_amd import _lib
    protos = header_prototypes()
    for name in GIN_EXPORTS:
        assert name in protos and name in _lib.SIGNATURES, name
    assert "gcr_gin_supported" in _lib.INT32_ANSWERS
    assert [bool(_lib.call("gcr_gin_supported", a, b)) for a, b in ((32, 128), (48, 64), (64, 256), (128, 128))] == \
        [True, False, False, True]
