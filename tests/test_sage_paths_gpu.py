"""The fused SAGE layer (csrc/gcr_sage.hip, functional.sage_layer) off the paths tests/test_sage_gpu.py walks: a graph with
hub rows in A and in A^T (the SpMM's windowed route for z and for dx = A^T p + q), cases in which float32 is exact (equality
with float64, and ReLU's gradient at a pre-activation of exactly 0), sentinels behind every output and the workspace, the
wrapper's argument paths and composed fallbacks, and gelu's saturated ends.

Every comparison is sage_rules.check (the float64 restatement and the float32 drift of the same restatement, both computed
on the CPU), exact equality or a sentinel; the builders' own conditions are asserted in tests/test_sage_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import sage_rules as sr

pytestmark = pytest.mark.gpu

N = 257                     # test_sage_gpu.N: a partial last tile for 32- and for 64-row tiles


@functools.lru_cache(maxsize=None)
def graph_of(n, builder=sr.sweep_graph):
    src, dst = builder(n)
    return sr.device_graph(src, dst, n)


def case_graph(case):
    return sr.device_graph(case["src"], case["dst"], case["n"])


# ---- 1. hub rows ----

@pytest.mark.parametrize("act,p", (("gelu", 0.5), ("relu", 0.0)))
@pytest.mark.parametrize("din,dout", sr.HUB_PAIRS)
def test_hub_rows_take_the_windowed_route_forward_and_backward(monkeypatch, din, dout, act, p):
    """z = A x (forward and again in the backward) and dx = A^T p + q (the `acc_in` form, values 1 / deg(dst)) through the
    hub-windowed launch, which sweep_graph's rows (at most 41 entries) never reach; a node without out-edges gets dx = q."""
    from recommendation_amd import spmm_launch as L
    n = sr.HUB_N
    src, dst = sr.hub_graph(n)
    graph = graph_of(n, sr.hub_graph)
    for g in (graph, graph.t):
        assert g.hub is not None and g.hub.eligible(din) and g.hub.n_hub == 2 and g.rows_p is None
    assert sr.out_isolated(src, n).size >= 1
    case = sr.large_case(n, din, dout, act, p, sr.hub_graph)
    assert case["share"] <= sr.MAX_ZEROED_SHARE
    real, seen = L.windowed, []
    monkeypatch.setattr(L, "windowed", lambda *a, **k: seen.append(a[2]) or real(*a, **k))
    a = sr.layer(graph, case)
    assert seen == [graph, graph, graph.t], "z in the forward, z in the backward, dx: each by the windowed launch"
    sr.check(a, case["ref"], case["drift"], f"hub n={n} ({din}, {dout}) {act} p={p} zeroed {case['share']:.2g}")
    b = sr.layer(graph, case)
    assert len(seen) == 6
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 2. exact cases ----

@pytest.mark.parametrize("with_bias", (True, False))
@pytest.mark.parametrize("act", ("none", "relu"))
@pytest.mark.parametrize("din,dout", sr.PAIRS)
def test_exact_integers_give_float64s_every_bit(din, dout, act, with_bias):
    """Where every product and partial sum is a float32 (sage_rules.exact_case) the kernels owe equality, a column (and
    without a bias a row) of pre-activations exactly 0 under non-zero g included: ReLU's gradient there is 0."""
    case = sr.exact_case(din, dout, act, with_bias)
    for k, want in case["ref"].items():
        assert np.array_equal(case["f32"][k], want), k
    for k in ("dx", "dwl", "dwr"):
        assert np.abs(case["ref"][k]).max() > 0
    got = sr.layer(case_graph(case), case)
    assert set(got) == set(case["ref"])
    sr.assert_exact(got, case["ref"], f"({din}, {dout}) {act} {'bias' if with_bias else 'no bias'} p={case['p']}")


# ---- 3. bounds ----

def _untouched(t):
    return t == sr.SENTINEL


@pytest.mark.parametrize("n,din,dout", ((1, 128, 128), (33, 64, 64), (65, 32, 128), (65537, 32, 32), (32769, 128, 64)))
def test_nothing_is_written_out_of_bounds_and_everything_inside_is(n, din, dout):
    """Sentinels in 64 rows behind h, pre, p and q, in 4096 words behind the workspace and all through the outputs: after a
    gelu forward and backward with a keep bitmap of exactly ceil(n dout / 32) words, none outside is touched and none inside
    is left."""
    from recommendation_amd import functional as Fn
    pad_rows, pad_words = 64, 4096
    r = sr.Raw(n=n, din=din, dout=dout, act=2, fill=sr.SENTINEL, pad_rows=pad_rows, pad_words=pad_words)
    assert r.ws_words == 2 * din * dout + min(-(-n // 32), sr.BWD_CAP) * (2 * din * dout + dout)
    assert r.ws.numel() == r.ws_words + pad_words and r.h.shape[0] == n + pad_rows
    keep = Fn.pack_bits(torch.from_numpy(sr.keep_mask(n, dout, 0.5, 3).reshape(-1))).cuda()
    assert keep.numel() == -(-n * dout // 32) and keep.dtype == torch.int32
    wcat = 2 * din * dout
    r.fwd(keep=keep, scale=2.0)
    torch.cuda.synchronize()
    for name in ("h", "pre"):
        t = getattr(r, name)
        assert bool(_untouched(t[n:]).all()), f"forward: {name} is written behind row n"
        assert not bool(_untouched(t[:n]).any()), f"forward: {name} is not written in full"
    assert not bool(_untouched(r.ws[:wcat]).any()), "forward: [wl^T; wr^T] is not written in full"
    assert bool(_untouched(r.ws[wcat:]).all()), "forward: the workspace is written behind [wl^T; wr^T]"
    for name in ("p", "q", "dwl", "dwr", "dbias"):
        assert bool(_untouched(getattr(r, name)).all()), f"forward: {name} is written"
    h, pre = r.h.clone(), r.pre.clone()
    r.bwd(keep=keep, scale=2.0)
    torch.cuda.synchronize()
    assert torch.equal(r.h, h) and torch.equal(r.pre, pre), "the backward writes its inputs"
    for name in ("p", "q"):
        t = getattr(r, name)
        assert bool(_untouched(t[n:]).all()), f"backward: {name} is written behind row n"
        assert not bool(_untouched(t[:n]).any()), f"backward: {name} is not written in full"
    assert not bool(_untouched(r.ws[:r.ws_words]).any()), "backward: a workgroup's partial is not written in full"
    assert bool(_untouched(r.ws[r.ws_words:]).all()), "backward: the workspace is written behind its last word"
    for name in ("dwl", "dwr", "dbias"):
        t = getattr(r, name)
        assert not bool(_untouched(t).any()) and bool(torch.isfinite(t).all()), f"backward: {name} is not written in full"


# ---- 4. the wrapper ----

def _tensors(case, **other):
    """x, wl, wr, bias, g, keep_bits of a case on the device (requires_grad set), `other` in place of some."""
    t = {k: torch.from_numpy(case[k]).cuda().requires_grad_(True) for k in ("x", "wl", "wr", "bias")}
    t["g"], t["keep_bits"] = torch.from_numpy(case["g"]).cuda(), sr.packed(case["keep"])
    t.update(other)
    return t


def _run(graph, case, t, p=None, fused=True):
    from recommendation_amd import functional as Fn
    for k in ("x", "wl", "wr", "bias"):
        t[k].grad = None
    h = Fn.sage_layer(graph, t["x"], t["wl"], t["wr"], t["bias"], case["act"], t["keep_bits"], case["p"] if p is None else p)
    assert sr.is_fused(h) == fused
    h.backward(t["g"])
    return dict(h=h.detach(), dx=t["x"].grad, dwl=t["wl"].grad, dwr=t["wr"].grad, dbias=t["bias"].grad)


@pytest.mark.parametrize("din,dout,act", ((64, 64, "relu"), (128, 32, "gelu")))
def test_a_frozen_parameter_changes_no_other_bit(din, dout, act):
    case = sr.margin_case(N, din, dout, act, 0.5)
    full = sr.layer(graph_of(N), case)
    for frozen in ("wl", "wr", "bias"):
        lean = sr.layer(graph_of(N), case, frozen=(frozen,))              # asserts the fused node
        assert set(full) - set(lean) == {"d" + frozen}
        for k in lean:
            assert np.array_equal(full[k], lean[k]), (frozen, k)


def test_non_contiguous_arguments_give_the_contiguous_runs_bits():
    """wl and wr as transposed storage, the incoming gradient as a stride-0 expand, keep_bits as every second word of a
    wider tensor (sage_layer's own .contiguous(): libgcr refuses a strided tensor)."""
    case = dict(sr.margin_case(N, 64, 32, "gelu", 0.5))
    case["g"] = np.ascontiguousarray(np.broadcast_to(case["g"][:1], case["g"].shape))       # what an expand can carry
    graph = graph_of(N)
    want = _run(graph, case, _tensors(case))
    odd = {k: torch.from_numpy(np.ascontiguousarray(case[k].T)).cuda().T.requires_grad_(True) for k in ("wl", "wr")}
    odd["g"] = torch.from_numpy(case["g"][:1]).cuda().expand(N, 32)
    bits = sr.packed(case["keep"])
    wide = torch.full((2 * bits.numel(),), -1, dtype=torch.int32, device="cuda")
    wide[::2] = bits
    odd["keep_bits"] = wide[::2]
    t = _tensors(case, **odd)
    assert not any(t[k].is_contiguous() for k in ("wl", "wr", "g", "keep_bits")) and t["g"].stride(0) == 0
    got = _run(graph, case, t)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    ref, drift = case["ref"], case["drift"]
    f64, _ = sr.restatement(case["src"], case["dst"], N, case["x"], case["wl"], case["wr"], case["bias"], case["g"], "gelu",
                            torch.float64, case["keep"], 0.5)
    f32, _ = sr.restatement(case["src"], case["dst"], N, case["x"], case["wl"], case["wr"], case["bias"], case["g"], "gelu",
                            torch.float32, case["keep"], 0.5)
    sr.check({k: v.cpu().numpy() for k, v in got.items()}, f64, sr.drift_of(f32, f64), "non-contiguous (64, 32) gelu")
    assert np.array_equal(ref["h"], f64["h"]) and drift["h"] == sr.drift_of(f32, f64)["h"]   # the same forward, another g


def test_keep_bits_and_p_mean_what_the_docstring_says():
    case = sr.margin_case(N, 64, 64, "relu", 0.5)
    graph = graph_of(N)
    keep = torch.from_numpy(case["keep"]).cuda()
    plain = _run(graph, case, _tensors(case, keep_bits=None), p=0.0)["h"]
    # a bitmap at p = 0: the mask applied, scale 1
    assert torch.equal(_run(graph, case, _tensors(case), p=0.0)["h"], plain * keep)
    assert bool((plain * keep != plain).any())
    # no bitmap: no dropout, whatever p
    assert torch.equal(_run(graph, case, _tensors(case, keep_bits=None), p=0.5)["h"], plain)
    # spare words behind the bitmap are not read as bits of it
    want = _run(graph, case, _tensors(case))
    bits = sr.packed(case["keep"])
    long = torch.cat([bits, torch.full((37,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")])
    got = _run(graph, case, _tensors(case, keep_bits=long))
    for k in want:
        assert torch.equal(got[k], want[k]), k
    sr.check({k: v.cpu().numpy() for k, v in got.items()}, case["ref"], case["drift"], "over-long bitmap (64, 64) relu")


def test_argument_errors_leave_earlier_outputs_alone():
    from recommendation_amd import CsrGraph, functional as Fn
    case = sr.margin_case(N, 64, 32, "relu", 0.5)
    graph = graph_of(N)
    t = _tensors(case)
    before = _run(graph, case, t)
    kept = {k: v.clone() for k, v in before.items()}
    x, wl, wr, bias, bits = t["x"], t["wl"], t["wr"], t["bias"], t["keep_bits"]
    words = (N * 32 + 31) // 32
    assert bits.numel() == words
    rect = CsrGraph.from_coo(np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), np.ones(1, dtype=np.float32), N, N + 1, "cuda")
    bad = (("the graph must be", dict(graph=rect)),
           ("wl, wr", dict(wr=wr.detach()[:, :32])),
           ("wl, wr", dict(wr=wr.detach()[:16])),
           ("bias must be", dict(bias=bias.detach()[None, :])),
           ("p must be", dict(p=1.0)),
           ("p must be", dict(p=-0.1)),
           ("keep_bits must be", dict(keep_bits=bits[:words - 1])),
           ("keep_bits must be", dict(keep_bits=bits.to(torch.int64))))
    for fn in (Fn.sage_layer, Fn.sage_layer_composed):
        for match, kw in bad:
            a = dict(graph=graph, x=x, wl=wl, wr=wr, bias=bias, act="relu", keep_bits=bits, p=0.5)
            a.update(kw)
            with pytest.raises(ValueError, match=match):
                fn(a["graph"], a["x"], a["wl"], a["wr"], a["bias"], a["act"], a["keep_bits"], a["p"])
    torch.cuda.synchronize()
    for k in kept:
        assert torch.equal(before[k], kept[k]), k


@pytest.mark.parametrize("what", ("width 48", "float64", "callable"))
def test_composed_fallbacks_on_the_device(what):
    """A width the kernels do not serve, float64 and a callable activation run `sage_layer_composed` on the device: no
    fused node anywhere below h, h the composed layer's, the gradients under the rule (float64: 1e-12 of the scale)."""
    from recommendation_amd import functional as Fn
    din, dtype, act = (48 if what == "width 48" else 64), (torch.float64 if what == "float64" else torch.float32), None
    if what == "callable":
        act = torch.nn.functional.relu
    case = sr.margin_case(N, din, 64, "relu", 0.5)
    graph = graph_of(N)
    assert Fn.sage_supported(din, 64) == (din == 64)
    got = sr.layer(graph, case, fused=False, dtype=dtype, act=act)       # asserts: no fused node below h
    t = {k: torch.from_numpy(case[k]).to("cuda", dtype) for k in ("x", "wl", "wr", "bias")}
    composed = Fn.sage_layer_composed(graph, t["x"], t["wl"], t["wr"], t["bias"], act or "relu", sr.packed(case["keep"]), 0.5)
    assert composed.is_cuda and composed.dtype == dtype and np.array_equal(got["h"], composed.cpu().numpy())
    if dtype == torch.float64:
        for k, want in case["ref"].items():
            assert np.abs(got[k] - want).max() <= 1e-12 * np.abs(want).max(), k
    else:
        sr.check(got, case["ref"], case["drift"], f"composed on the device, {what}")


# ---- 5. gelu's ends ----

@pytest.mark.parametrize("din,dout", ((64, 64), (128, 32)))
def test_gelu_far_from_zero(din, dout):
    """Pre-activations past +-10: erff has saturated and __expf(-pre^2 / 2) runs down to 1e-100-odd, flushed to 0."""
    case = sr.tail_case(N, din, dout)
    assert np.abs(case["pre"]).max() >= 10.0
    got = sr.layer(graph_of(N), case)
    sr.check(got, case["ref"], case["drift"], f"gelu tails ({din}, {dout}) max |pre| {np.abs(case['pre']).max():.3g}")
