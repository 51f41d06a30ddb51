"""The fused GIN layer (csrc/gcr_gin.hip, functional.gin_layer) off the paths tests/test_gin_gpu.py walks: launches with more
tiles than workgroups, once per (tile height, weights in LDS) class of the forward and of the backward; a graph with hub rows
in A and in A^T (the SpMM's windowed route for s = x + A x and for dx = ds + A^T ds); strided and non-contiguous arguments.

The large cases are gin_rules.exact_case's: small integers, where every sum is a float32 in any order, both ReLU kinks are
unambiguous and equality with float64 is owed (the zeroed-gradient method of sage_rules.large_case cannot reach the inner
ReLU).  The builders' own conditions are asserted in tests/test_gin_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import gin_rules as gr

pytestmark = pytest.mark.gpu

N = 137


def case_graph(case):
    return gr.device_graph(case["src"], case["dst"], case["n"])


# ---- 1. more tiles than workgroups ----

@pytest.mark.parametrize("below", (0, 1))
@pytest.mark.parametrize("n,din,dout", gr.FWD_TRIP_SHAPES + gr.BWD_TRIP_SHAPES)
def test_second_trip_of_each_launch_class_is_exact(n, din, dout, below):
    """n = cap x tile rows + 1 (workgroup 0's second trip holds one row) and n - 1 (one full tile per workgroup), for the
    forward's classes and at the backward's own threshold: every output equals float64's, dropout and edge mask on."""
    forward_threshold = (n, din, dout) in gr.FWD_TRIP_SHAPES
    n -= below
    tiles_f, tiles_b = -(-n // gr.fwd_rows(dout)), -(-n // gr.BWD_ROWS)
    if forward_threshold:
        assert tiles_f == gr.FWD_CAP + 1 - below and tiles_b > gr.BWD_CAP
    else:
        assert tiles_b == gr.BWD_CAP + 1 - below
    case = gr.exact_case(n, din, dout)
    for k, want in case["ref"].items():
        assert np.array_equal(case["f32"][k], want) and np.abs(want).max() > 0, k
    graph = case_graph(case)
    a = gr.layer(graph, case)
    gr.assert_exact(a, case["ref"], f"n={n} ({din}, {dout}) classes {gr.fwd_class(din, dout)} {gr.bwd_class(din, dout)}")
    lean = gr.layer(graph, case, want_dx=False)
    for k in lean:
        assert np.array_equal(a[k], lean[k]), k


# ---- 2. hub rows ----

@pytest.mark.parametrize("din,dout", gr.HUB_PAIRS)
def test_hub_rows_take_the_windowed_route_forward_and_backward(monkeypatch, din, dout):
    """s = x + A x and dx = ds + A^T ds (both the `acc_in` form on a CSR without values) through the hub-windowed launch,
    which sweep_graph's rows (at most 41 entries) never reach; no edge mask, since a masked launch keeps the classic plan."""
    from recommendation_amd import spmm_launch as L
    n = gr.HUB_N
    case = gr.exact_case(n, din, dout, graph=gr.hub_graph, edge_p=0.0)
    assert case["edge_keep"] is None and gr.out_isolated(case["src"], n).size >= 1
    graph = case_graph(case)
    for g in (graph, graph.t):
        assert g.val is None and g.hub is not None and g.hub.eligible(din) and g.hub.n_hub == 2 and g.rows_p is None
    real, seen = L.windowed, []
    monkeypatch.setattr(L, "windowed", lambda *a, **k: seen.append(a[2]) or real(*a, **k))
    a = gr.layer(graph, case)
    assert seen == [graph, graph.t], "s in the forward and dx in the backward: each by the windowed launch"
    gr.assert_exact(a, case["ref"], f"hub n={n} ({din}, {dout})")


# ---- 3. strided and non-contiguous arguments ----

@functools.lru_cache(maxsize=None)
def graph_of(n):
    src, dst = gr.sweep_graph(n)
    return gr.device_graph(src, dst, n)


@pytest.mark.parametrize("din,dout", ((64, 32), (128, 128)))
def test_non_contiguous_arguments_give_the_contiguous_runs_bits(din, dout):
    """x as every second column of a wider tensor, w1 and w2 as transposed storage, b1 as a strided slice, the incoming
    gradient as every second row of a taller tensor (gin_layer's own .contiguous(): libgcr refuses a strided tensor)."""
    case = gr.margin_case(N, din, dout, 0.5, 0.3)
    graph = graph_of(N)
    want = gr.layer(graph, case)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                         # noqa: E731
    wide = torch.zeros(N, 2 * din, device="cuda")
    wide[:, ::2] = dev(case["x"])
    tall = torch.zeros(2 * N, dout, device="cuda")
    tall[::2] = dev(case["g"])
    long = torch.zeros(2 * dout, device="cuda")
    long[::2] = dev(case["b1"])
    odd = dict(x=wide[:, ::2].requires_grad_(True), w1=dev(case["w1"].T).T.requires_grad_(True),
               w2=dev(case["w2"].T).T.requires_grad_(True), b1=long[::2].requires_grad_(True), g=tall[::2])
    assert not any(t.is_contiguous() for t in odd.values())
    got = gr.layer(graph, case, tensors=odd)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    gr.check(got, case["ref"], case["drift"], f"non-contiguous ({din}, {dout})")


def test_strided_keep_bits_and_spare_words():
    from recommendation_amd import functional as Fn
    case = gr.margin_case(N, 64, 64, 0.5, 0.0)
    graph = graph_of(N)
    t = {k: torch.from_numpy(case[k]).cuda() for k in ("x",) + gr.PARAMS}
    bits = gr.packed(case["keep"])
    want = Fn.gin_layer(graph, t["x"], t["w1"], t["b1"], t["w2"], t["b2"], 0.0, bits, 0.5)
    wide = torch.full((2 * bits.numel(),), -1, dtype=torch.int32, device="cuda")
    wide[::2] = bits
    long = torch.cat([bits, torch.full((37,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")])
    for other in (wide[::2], long):
        assert torch.equal(Fn.gin_layer(graph, t["x"], t["w1"], t["b1"], t["w2"], t["b2"], 0.0, other, 0.5), want)
    # a bitmap at p = 0: the mask applied, scale 1; no bitmap: no dropout, whatever p
    plain = Fn.gin_layer(graph, t["x"], t["w1"], t["b1"], t["w2"], t["b2"], 0.0, None, 0.5)
    keep = torch.from_numpy(case["keep"]).cuda()
    assert torch.equal(Fn.gin_layer(graph, t["x"], t["w1"], t["b1"], t["w2"], t["b2"], 0.0, bits, 0.0), plain * keep)
    assert torch.equal(want, plain * keep * 2.0)
