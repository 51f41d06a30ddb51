"""The fused GIN layer kernels (csrc/gcr_gin.hip, functional.gin_layer) on the device against the float64 restatement under
the project's rule (tests/gin_rules.py): every width pair with and without dropout and an edge mask, the tile edges, dx
skipped, bitwise reproducibility, exact integers, the ABI's contract, sentinels behind every output, and the composed form
for a width the kernels do not serve."""
import functools

import numpy as np
import pytest
import torch

import gin_rules as gr

pytestmark = pytest.mark.gpu

N = 137                     # no multiple of a tile height (32, 64): five backward tiles, three or five forward tiles


@functools.lru_cache(maxsize=None)
def graph_of(n):
    src, dst = gr.sweep_graph(n)
    return gr.device_graph(src, dst, n)


def test_the_graph_cycles_through_the_degrees_with_duplicates_and_self_loops():
    src, dst = gr.sweep_graph(N)
    deg = np.bincount(dst, minlength=N)
    assert {0, 1, 3, 41} <= set(deg.tolist()) and bool((src == dst).any())
    assert any(np.unique(src[dst == r]).size < deg[r] for r in range(N) if deg[r] >= 2)
    g = graph_of(N)
    assert g.val is None and g.nnz == src.size and g.t.nnz == src.size


@pytest.mark.parametrize("edge_p", (0.0, 0.3))
@pytest.mark.parametrize("p", (0.0, 0.5))
@pytest.mark.parametrize("din,dout", gr.PAIRS)
def test_every_pair_with_and_without_dropout_and_edge_mask(din, dout, p, edge_p):
    case = gr.margin_case(N, din, dout, p, edge_p)
    got = gr.layer(graph_of(N), case)
    gr.check(got, case["ref"], case["drift"], f"n={N} ({din}, {dout}) p={p} edge_p={edge_p}")


@pytest.mark.parametrize("n", (1, 31, 33, 65))
def test_tile_edges(n):
    case = gr.margin_case(n, 64, 64, 0.5, 0.3)
    got = gr.layer(graph_of(n), case)
    gr.check(got, case["ref"], case["drift"], f"n={n} (64, 64)")


@pytest.mark.parametrize("din,dout,p,edge_p", ((64, 64, 0.5, 0.3), (32, 128, 0.5, 0.0), (128, 32, 0.0, 0.3)))
def test_without_dx_the_parameter_gradients_are_the_same_bits(din, dout, p, edge_p):
    """x without requires_grad: the backward gets ds == NULL, skips the product and the SpMM on A^T, and needs no
    transposed edge mask."""
    case = gr.margin_case(N, din, dout, p, edge_p)
    full = gr.layer(graph_of(N), case)
    lean = gr.layer(graph_of(N), case, want_dx=False)
    assert "dx" not in lean
    for k in lean:
        assert np.array_equal(full[k], lean[k]), k
    gr.check(lean, {k: case["ref"][k] for k in lean}, case["drift"], f"no dx ({din}, {dout})")


@pytest.mark.parametrize("din,dout", gr.PAIRS)
def test_two_runs_are_bitwise_equal(din, dout):
    case = gr.margin_case(N, din, dout, 0.5, 0.3)
    a, b = gr.layer(graph_of(N), case), gr.layer(graph_of(N), case)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("din,dout", gr.PAIRS)
def test_exact_integers_give_float64s_every_bit(din, dout):
    """Dense small integers (gin_rules.exact_case): the kernels owe equality, a column of inner and a column of outer
    pre-activations of exactly 0 under non-zero g included."""
    case = gr.exact_case(70, din, dout, dense=True)
    for k in ("dx", "dw1", "db1", "dw2", "db2"):
        assert np.abs(case["ref"][k]).max() > 0
    got = gr.layer(gr.device_graph(case["src"], case["dst"], case["n"]), case)
    gr.assert_exact(got, case["ref"], f"({din}, {dout})")


def test_unsupported_width_runs_the_composition():
    from recommendation_amd import functional as Fn
    case = gr.margin_case(N, 48, 64, 0.5, 0.3)
    assert not Fn.gin_supported(48, 64) and Fn.gin_supported(64, 64)
    got = gr.layer(graph_of(N), case, fused=False)
    composed = gr.layer(graph_of(N), case, fused=False, fn=Fn.gin_layer_composed)
    for k in got:
        assert np.array_equal(got[k], composed[k]), k
    gr.check(got, case["ref"], case["drift"], "composed on the device, width 48")


# ---- the ABI's contract, through the raw exports ----

def test_contract_refusals():
    """Every GCR_EINVAL of include/gcr.h's contract; each call returns before anything is launched."""
    from recommendation_amd._lib import GcrError
    r = gr.Raw()
    odd = torch.zeros(r.n * r.din + 4, device="cuda")[1:1 + r.n * r.din].view(r.n, r.din)        # 4 bytes off a 16-B boundary
    assert odd.data_ptr() % 16 == 4
    bad_fwd = (dict(din=48), dict(dout=96), dict(din=256), dict(n=-1), dict(s=odd), dict(h=odd), dict(h=r.s), dict(s=None),
               dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(h=None), dict(ws=None))
    for kw in bad_fwd:
        with pytest.raises(GcrError, match="invalid or unsupported"):
            r.fwd(**kw)
    bad_bwd = (dict(din=48), dict(dout=16), dict(n=-1), dict(s=odd), dict(ds=odd), dict(ds=r.s), dict(ds=r.g), dict(ds=r.h),
               dict(dw1=None), dict(db1=None), dict(dw2=None), dict(db2=None), dict(g=None), dict(h=None), dict(ws=None))
    for kw in bad_bwd:
        with pytest.raises(GcrError, match="invalid or unsupported"):
            r.bwd(**kw)
    torch.cuda.synchronize()
    assert float(r.h.abs().max()) == 0.0 and float(r.ds.abs().max()) == 0.0
    for t in (r.dw1, r.db1, r.dw2, r.db2):
        assert float((t - 1).abs().max()) == 0.0


def test_no_rows():
    from recommendation_amd import functional as Fn
    r = gr.Raw(n=0)
    r.fwd()
    r.bwd()
    torch.cuda.synchronize()
    for t in (r.dw1, r.db1, r.dw2, r.db2):
        assert float(t.abs().max()) == 0.0                     # the backward zeroes them
    # the wrapper: n == 0 takes the composed form
    g = Fn.gin_sum_graph(torch.zeros(2, 0, dtype=torch.int64), 0, "cpu")
    h = Fn.gin_layer(g, torch.zeros(0, 64), torch.ones(32, 64), torch.ones(32), torch.ones(32, 32), torch.ones(32))
    assert tuple(h.shape) == (0, 32)


def test_dropout_bits_follow_pack_bits_order():
    """s = 0, w1 = 0, b1 = 1, w2 = 0, b2 = 1 gives h = keep_scale exactly where bit r * dout + c is set, for a pattern that
    no transposed or word-swapped reading reproduces."""
    from recommendation_amd import functional as Fn
    n, din, dout = 70, 32, 64
    r = gr.Raw(n=n, din=din, dout=dout)
    keep = (torch.arange(n * dout) * 7 % 13 < 5).view(n, dout)
    r.s.zero_(), r.w1.zero_(), r.w2.zero_(), r.b1.fill_(1.0), r.b2.fill_(1.0)
    r.fwd(keep=Fn.pack_bits(keep.reshape(-1)).cuda(), scale=2.0)
    assert torch.equal(r.h.cpu(), keep.float() * 2.0)


def _untouched(t):
    return t == gr.SENTINEL


@pytest.mark.parametrize("n,din,dout", ((1, 128, 128), (33, 64, 64), (65, 32, 128), (137, 128, 32)))
def test_nothing_is_written_out_of_bounds_and_everything_inside_is(n, din, dout):
    """Sentinels in 64 rows behind h and ds, in 4096 words behind the workspace and all through the outputs: after a forward
    and a backward with a keep bitmap of exactly ceil(n dout / 32) words, none outside is touched and none inside is left."""
    from recommendation_amd import functional as Fn
    pad_rows, pad_words = 64, 4096
    r = gr.Raw(n=n, din=din, dout=dout, fill=gr.SENTINEL, pad_rows=pad_rows, pad_words=pad_words)
    assert r.ws_words == gr.workspace_words(n, din, dout)
    keep = Fn.pack_bits(torch.from_numpy(gr.keep_mask(n, dout, 0.5, 3).reshape(-1))).cuda()
    assert keep.numel() == -(-n * dout // 32)
    wt = (din + dout) * dout
    r.fwd(keep=keep, scale=2.0)
    torch.cuda.synchronize()
    assert bool(_untouched(r.h[n:]).all()), "forward: h is written behind row n"
    assert not bool(_untouched(r.h[:n]).any()), "forward: h is not written in full"
    assert not bool(_untouched(r.ws[:wt]).any()), "forward: [w1^T; w2^T] is not written in full"
    assert bool(_untouched(r.ws[wt:]).all()), "forward: the workspace is written behind [w1^T; w2^T]"
    for name in ("ds", "dw1", "db1", "dw2", "db2"):
        assert bool(_untouched(getattr(r, name)).all()), f"forward: {name} is written"
    h = r.h.clone()
    r.bwd(scale=2.0)
    torch.cuda.synchronize()
    assert torch.equal(r.h, h), "the backward writes its inputs"
    assert bool(_untouched(r.ds[n:]).all()), "backward: ds is written behind row n"
    assert not bool(_untouched(r.ds[:n]).any()), "backward: ds is not written in full"
    assert not bool(_untouched(r.ws[:r.ws_words]).any()), "backward: a workgroup's partial is not written in full"
    assert bool(_untouched(r.ws[r.ws_words:]).all()), "backward: the workspace is written behind its last word"
    for name in ("dw1", "db1", "dw2", "db2"):
        t = getattr(r, name)
        assert not bool(_untouched(t).any()) and bool(torch.isfinite(t).all()), f"backward: {name} is not written in full"
