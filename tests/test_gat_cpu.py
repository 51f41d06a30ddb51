"""The GAT fixture and what can be checked of the GAT path without a GPU: tests/golden/gat_steps.npz's size and schema,
gat_rules' float64 restatement against the reference stand-in's stored runs, functional.gat_aggregate_composed (the path of
CPU tensors and unsupported shapes) under the component rule, GATConv's composition against the whole-layer case, the
operator GATRec.prepare builds, GATRec's float64 forward and step-0 gradients against the step cases (recorded masks
included), and gat_rules.shaped_graph's guarantees with the two float64 statements on the graph tests/test_gat_paths_gpu.py
runs."""
import os

import numpy as np
import pytest
import torch

import gat_rules as gr


@pytest.fixture(scope="module")
def golden():
    return gr.load()


def test_fixture_size_and_schema(golden):
    assert os.path.getsize(gr.GOLDEN) < 1_000_000
    assert golden["cases"].tolist() == list(gr.STEP_CASES) and int(golden["steps"]) == 6
    assert (int(golden["num_users"]), int(golden["num_items"]), golden["train_user"].size) == (120, 72, 1200)
    assert len(gr.PAIRS) == 8
    for heads, c in gr.PAIRS:
        for pe in gr.COMP_PE:
            pre = gr.comp_prefix(heads, c, pe)
            assert golden[pre + "out"].shape == (gr.COMP_N, heads * c) and golden[pre + "da_dst"].shape == (gr.COMP_N, heads)
            assert all(0.0 <= float(golden[pre + "drift/" + k]) < 1e-5 for k in gr.KEYS)
    for case in gr.STEP_CASES:
        cfg = gr.step_config(golden, case)
        shapes = gr.param_shapes(cfg, 120, 72)
        assert golden[f"{case}/neg_i"].shape == (6, 1200) and golden[f"{case}/f64/loss"].shape == (6,)
        for k in gr.PARAMS:
            assert golden[f"{case}/f64/grad0/{k}"].shape == shapes[k] == golden[f"{case}/f64/delta/{k}"].shape
            assert float(golden[f"{case}/slack/{k}"]) < 1e-5
        assert (f"{case}/att0" in golden.files) == (cfg["edge_dropout"] > 0)
    assert gr.step_config(golden, "C")["dropout"] == 0.2 and gr.step_config(golden, "B")["num_heads"] == 4


@pytest.mark.parametrize("heads,c", gr.PAIRS)
@pytest.mark.parametrize("pe", gr.COMP_PE)
def test_restatement_reproduces_the_component_case(golden, heads, c, pe):
    case = gr.component(golden, heads, c, pe)
    got, _ = gr.restatement(case["dst"], case["src"], case["n"], case["h"], case["a_src"], case["a_dst"], case["g"], heads,
                            torch.float64, keep=case["keep"], p=pe, bias=case["bias"])
    for k, want in case["ref"].items():                     # stored as float32 of the float64 run
        assert np.abs(got[k] - want).max() <= 2.0 ** -23 * np.abs(want).max(), k


@pytest.mark.parametrize("heads,c", gr.PAIRS)
@pytest.mark.parametrize("pe", gr.COMP_PE)
def test_composed_on_cpu_tensors_meets_the_rule(golden, heads, c, pe):
    import recommendation_amd as ra
    from recommendation_amd import functional as Fn
    case = gr.component(golden, heads, c, pe)
    graph = ra.CsrGraph.from_coo(case["dst"], case["src"], None, case["n"], case["n"], "cpu")
    got = gr.aggregate(graph, case, device="cpu", fused=False)
    gr.check(got, case["ref"], case["drift"], f"composed cpu heads={heads} c={c} pe={pe}")
    assert Fn.gat_aggregate is not Fn.gat_aggregate_composed


@pytest.mark.parametrize("name", ("PATHS", "FAR", "MIRRORED"))
def test_shaped_graph_keeps_its_guarantees(name):
    """The graphs of tests/test_gat_paths_gpu.py: exact row lengths, exact hub lengths, no other long column, a repeated
    column in every row of two or more entries, no diagonal entry, and `sweep_graph`'s cycle elsewhere."""
    n, rows, hubs = getattr(gr, name)
    dst, src = gr.shaped_graph(n, rows, hubs)
    assert dst.dtype == src.dtype == np.int64 and (np.diff(dst) >= 0).all() and (dst != src).all()
    assert src.min() >= 0 and src.max() < n
    deg, cnt = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    want = np.array([gr.DEGREES[r % len(gr.DEGREES)] for r in range(n)])
    want[1] = 0
    for r, k in rows.items():
        want[r] = k
    assert np.array_equal(deg, want)
    assert all(cnt[s] == k for s, k in hubs.items())
    assert np.delete(cnt, list(hubs)).max() <= gr.LONG_ROW
    start = np.concatenate([[0], np.cumsum(deg)])
    for r in np.flatnonzero(deg >= 2):
        row = src[start[r]:start[r + 1]]
        assert np.unique(row).size < row.size, r
    d2, s2 = gr.shaped_graph(n, rows, hubs)
    assert np.array_equal(dst, d2) and np.array_equal(src, s2)              # a function of its arguments


def test_composed_float64_agrees_with_the_restatement_on_the_paths_graph():
    """The references of tests/test_gat_paths_gpu.py rest on two independent statements: gat_rules.restatement and
    functional.gat_aggregate_composed, both in float64, agree to rounding on the graph with the long rows and columns."""
    import recommendation_amd as ra
    n, rows, hubs = gr.PATHS
    for heads, c, p in ((2, 64, 0.5), (1, 32, 0.0)):
        case = gr.shaped_case(n, rows, hubs, heads, c, p)
        graph = ra.CsrGraph.from_coo(case["dst"], case["src"], None, n, n, "cpu")
        t = {k: torch.from_numpy(case[k]).double().requires_grad_(True) for k in ("h", "a_src", "a_dst", "bias")}
        from recommendation_amd import functional as Fn
        out = Fn.gat_aggregate_composed(graph, t["h"], t["a_src"], t["a_dst"], heads, gr.SLOPE, gr.packed(case["keep"], "cpu"), p,
                                        t["bias"])
        out.backward(torch.from_numpy(case["g"]).double())
        got = dict(out=out.detach(), dh=t["h"].grad, da_src=t["a_src"].grad, da_dst=t["a_dst"].grad, dbias=t["bias"].grad)
        for k, want in case["ref"].items():
            err = np.abs(got[k].numpy() - want).max() / np.abs(want).max()
            print(f"GAT composed f64 against the restatement, heads={heads} c={c} pe={p} {k}: err/S {err:.3g}")
            assert err <= 1e-12, k                                         # 1100-term sums in float64: 1e3 x 2^-53 and room


def test_gatconv_composition_matches_the_whole_layer_case(golden):
    import recommendation_amd as ra
    from recommendation_amd.gat import GATConv
    from recommendation_amd import functional as Fn
    heads, c = gr.CONV_PAIR
    dst, src = golden["conv/dst"].astype(np.int64), golden["conv/src"].astype(np.int64)
    graph = ra.CsrGraph.from_coo(dst, src, None, gr.CONV_N, gr.CONV_N, "cpu")
    conv = GATConv(gr.CONV_IN, c, heads=heads, dropout=gr.CONV_PE, negative_slope=gr.SLOPE).train()
    state = {k: torch.from_numpy(golden[f"conv/{k}"]) for k in ("att_src", "att_dst", "bias")}
    state["lin_src.weight"] = torch.from_numpy(golden["conv/lin.weight"])          # the older PyG name loads too
    conv.load_state_dict(state)
    keep = np.unpackbits(golden["conv/keep"], count=(dst.size + gr.CONV_N) * heads).astype(bool)
    x = torch.from_numpy(golden["conv/x"]).requires_grad_(True)
    out = conv(x, graph, keep_bits=Fn.pack_bits(torch.from_numpy(keep)))
    out.backward(torch.from_numpy(golden["conv/g"]))
    got = dict(out=out.detach(), dx=x.grad, dW=conv.lin.weight.grad, datt_src=conv.att_src.grad, datt_dst=conv.att_dst.grad,
               dbias=conv.bias.grad)
    got = {k: v.numpy() for k, v in got.items()}
    ref = {k: golden[f"conv/{k}"].astype(np.float64) for k in got}
    gr.check(got, ref, {k: float(golden[f"conv/drift/{k}"]) for k in got}, "GATConv cpu")


def test_prepare_strips_the_diagonal_and_keeps_duplicates():
    from recommendation_amd.gat import GATRec
    model = GATRec(2, 3, 8, 4, 4, 2, 0.0, 0.0, 0.2)
    #                        0->1  1->0  2->1  2->1 (duplicate)  3->3 (self loop)  3->0  4->1
    ei = torch.tensor([[0, 1, 2, 2, 3, 3, 4], [1, 0, 1, 1, 3, 0, 1]])
    g = model.prepare(ei)
    assert g is model.prepare(ei)                                          # cached
    assert (g.n_rows, g.n_cols, g.nnz, g.val) == (5, 5, 6, None)
    assert g.rowptr_host.tolist() == [0, 2, 6, 6, 6, 6]                    # rows = edge_index[1]
    assert g.col.tolist() == [1, 3, 0, 2, 2, 4]                            # cols = edge_index[0], edge order inside a row
    assert np.asarray(g.coo_perm).tolist() == [1, 4, 0, 2, 3, 5]           # positions among the kept edges


def test_prepare_holds_its_edge_index_so_that_a_recycled_address_is_not_a_hit():
    """GATRec.prepare on CPU tensors (tests/prepare_cache.py)."""
    from prepare_cache import check_prepare_cache
    from recommendation_amd.gat import GATRec, gat_graph
    model = GATRec(30, 20, 8, 4, 4, 2, 0.0, 0.0, 0.2)
    check_prepare_cache(model.prepare, lambda e: gat_graph(e, 50, "cpu"), 50)


@pytest.mark.parametrize("case", gr.STEP_CASES)
def test_gatrec_float64_forward_and_gradients_match_the_reference(golden, case):
    """GATRec on CPU tensors in float64 (the composition), one step: the loss of gat.py:111-117 and the step-0 gradients."""
    from recommendation_amd.gat import GATRec, bipartite_edge_index
    cfg = gr.step_config(golden, case)
    model = GATRec(120, 72, cfg["in_channels"], cfg["hidden_channels"], cfg["out_channels"], cfg["num_heads"], cfg["dropout"],
                   cfg["edge_dropout"], cfg["neg_slope"]).double().train()
    model.load_state_dict({k: torch.from_numpy(v).double() for k, v in gr.step_init(golden, case).items()})
    u, i = golden["train_user"].astype(np.int64), golden["train_item"].astype(np.int64)
    edge_index = bipartite_edge_index(u, i, 120)
    graph = model.prepare(edge_index)
    user_emb, item_emb = model(edge_index, masks=gr.step_masks(golden, case, 0, graph, cfg, device="cpu"))
    neg = torch.from_numpy(golden[f"{case}/neg_i"][0].astype(np.int64))
    uv = user_emb[torch.from_numpy(u)]
    loss = -torch.log(torch.sigmoid((uv * item_emb[torch.from_numpy(i)]).sum(1) - (uv * item_emb[neg]).sum(1))).mean()
    loss.backward()
    assert abs(float(loss.detach()) - float(golden[f"{case}/f64/loss"][0])) < 1e-12
    params = dict(model.named_parameters())
    for k in gr.PARAMS:
        want = golden[f"{case}/f64/grad0/{k}"].astype(np.float64)           # float32 of the float64 gradient
        assert np.abs(params[k].grad.numpy() - want).max() <= 2.0 ** -23 * np.abs(want).max(), k
