"""The fused SAGE layer kernels (csrc/gcr_sage.hip) on the device against the float64 restatement under the project's rule
(tests/sage_rules.py): every width pair, activation and dropout setting, the tile edges, the optional pointers, the
multi-trip launches, bitwise reproducibility and the ABI's contract."""
import functools

import numpy as np
import pytest
import torch

import sage_rules as sr

pytestmark = pytest.mark.gpu

N = 257                     # a partial last tile for 32- and for 64-row tiles, nine tiles of 32


@functools.lru_cache(maxsize=None)
def graph_of(n):
    src, dst = sr.sweep_graph(n)
    return sr.device_graph(src, dst, n)


def _ref(case, keys):
    return {k: case["ref"][k] for k in keys}, {k: case["drift"][k] for k in keys}


@pytest.mark.parametrize("p", (0.0, 0.5))
@pytest.mark.parametrize("act", sr.ACTS)
@pytest.mark.parametrize("din,dout", sr.PAIRS)
def test_every_pair_activation_and_dropout(din, dout, act, p):
    case = sr.margin_case(N, din, dout, act, p)
    got = sr.layer(graph_of(N), case)
    sr.check(got, case["ref"], case["drift"], f"n={N} ({din}, {dout}) {act} p={p}")


@pytest.mark.parametrize("act,p", (("relu", 0.5), ("gelu", 0.0), ("none", 0.5)))
@pytest.mark.parametrize("n", (1, 31, 33, 65))
def test_tile_edges(n, act, p):
    case = sr.margin_case(n, 64, 64, act, p)
    got = sr.layer(graph_of(n), case)
    sr.check(got, case["ref"], case["drift"], f"n={n} (64, 64) {act} p={p}")


@pytest.mark.parametrize("din,dout,act,p", ((64, 64, "relu", 0.5), (32, 128, "gelu", 0.5), (128, 32, "none", 0.0)))
def test_without_dx_the_weight_gradients_are_the_same_bits(din, dout, act, p):
    """x without requires_grad: the backward gets p == q == NULL and skips the [p | q] product."""
    case = sr.margin_case(N, din, dout, act, p)
    full = sr.layer(graph_of(N), case)
    lean = sr.layer(graph_of(N), case, want_dx=False)
    assert "dx" not in lean
    for k in ("h", "dwl", "dwr", "dbias"):
        assert np.array_equal(full[k], lean[k]), k
    ref, drift = _ref(case, ("h", "dwl", "dwr", "dbias"))
    sr.check(lean, ref, drift, f"no dx ({din}, {dout}) {act}")


@pytest.mark.parametrize("din,dout,act", ((64, 64, "relu"), (128, 64, "gelu")))
def test_without_bias(din, dout, act):
    case = sr.margin_case(N, din, dout, act, 0.5, with_bias=False)
    assert case["bias"] is None and "dbias" not in case["ref"]
    got = sr.layer(graph_of(N), case)
    sr.check(got, case["ref"], case["drift"], f"no bias ({din}, {dout}) {act}")


def test_strided_x_through_the_wrapper():
    from recommendation_amd import functional as Fn
    case = sr.margin_case(N, 64, 32, "relu", 0.5)
    wide = torch.zeros(N, 128, device="cuda")
    wide[:, ::2] = torch.from_numpy(case["x"]).cuda()
    x = wide[:, ::2].requires_grad_(True)
    assert not x.is_contiguous()
    wl, wr, bias = (torch.from_numpy(case[k]).cuda().requires_grad_(True) for k in ("wl", "wr", "bias"))
    h = Fn.sage_layer(graph_of(N), x, wl, wr, bias, "relu", sr.packed(case["keep"]), 0.5)
    assert type(h.grad_fn).__name__.startswith("_SageLayer")
    h.backward(torch.from_numpy(case["g"]).cuda())
    got = dict(h=h.detach(), dx=x.grad, dwl=wl.grad, dwr=wr.grad, dbias=bias.grad)
    sr.check({k: v.cpu().numpy() for k, v in got.items()}, case["ref"], case["drift"], "strided x")


@pytest.mark.parametrize("act,p", (("gelu", 0.5), ("relu", 0.0)))
@pytest.mark.parametrize("n,din,dout", sr.MULTI_TRIP_SHAPES)
def test_multi_trip(n, din, dout, act, p):
    """More tiles than workgroups in the forward and in the backward (sage_rules.MULTI_TRIP_SHAPES): gelu with dropout, and
    relu through the zeroing rule."""
    case = sr.large_case(n, din, dout, act, p)
    assert case["share"] <= sr.MAX_ZEROED_SHARE
    a = sr.layer(graph_of(n), case)
    sr.check(a, case["ref"], case["drift"], f"multi-trip n={n} ({din}, {dout}) {act} p={p} zeroed {case['share']:.2g}")
    b = sr.layer(graph_of(n), case)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("din,dout,act,p", ((64, 64, "relu", 0.5), (128, 128, "gelu", 0.5), (32, 64, "none", 0.0)))
def test_two_runs_are_bitwise_equal(din, dout, act, p):
    case = sr.margin_case(N, din, dout, act, p)
    a, b = sr.layer(graph_of(N), case), sr.layer(graph_of(N), case)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- the ABI's contract, through the raw exports ----

Raw = sr.Raw                # the arguments of the raw exports (tests/sage_rules.py), shared with test_sage_paths_gpu.py


def test_contract_refusals():
    """Every GCR_EINVAL of include/gcr.h's contract; each call returns before anything is launched."""
    from recommendation_amd._lib import GcrError
    r = Raw()
    odd = torch.zeros(r.n * r.din + 4, device="cuda")[1:1 + r.n * r.din].view(r.n, r.din)        # 4 bytes off a 16-B boundary
    assert odd.data_ptr() % 16 == 4
    bad_fwd = (dict(din=48), dict(dout=96), dict(din=256), dict(n=-1), dict(act=3), dict(act=-1), dict(x=odd), dict(z=odd),
               dict(h=r.x), dict(pre=r.pre), dict(act=2, pre=None), dict(act=0, pre=r.pre), dict(x=None), dict(ws=None))
    for kw in bad_fwd:
        with pytest.raises(GcrError, match="invalid or unsupported"):
            r.fwd(**kw)
    bad_bwd = (dict(din=48), dict(dout=16), dict(n=-1), dict(act=3), dict(x=odd), dict(p=odd), dict(pre=r.pre), dict(act=2, pre=None),
               dict(p=None), dict(q=None), dict(dwl=None), dict(dwr=None), dict(g=None))
    for kw in bad_bwd:
        with pytest.raises(GcrError, match="invalid or unsupported"):
            r.bwd(**kw)
    torch.cuda.synchronize()
    assert float(r.h.abs().max()) == 0.0 and float(r.p.abs().max()) == 0.0 and float((r.dwl - 1).abs().max()) == 0.0


def test_no_rows():
    from recommendation_amd import functional as Fn
    r = Raw(n=0)
    r.fwd()
    r.bwd()
    torch.cuda.synchronize()
    for t in (r.dwl, r.dwr, r.dbias):
        assert float(t.abs().max()) == 0.0                     # the backward zeroes them
    r.dwl.fill_(1.0)
    r.bwd(dbias=None)
    assert float(r.dwl.abs().max()) == 0.0 and float(r.dbias.abs().max()) == 0.0
    # the wrapper: n == 0 takes the composed form
    g = Fn.sage_mean_graph(torch.zeros(2, 0, dtype=torch.int64), 0, "cpu")
    h = Fn.sage_layer(g, torch.zeros(0, 64), torch.ones(32, 64), torch.ones(32, 64), torch.ones(32), "relu")
    assert tuple(h.shape) == (0, 32)


def test_dropout_bits_follow_pack_bits_order():
    """Exact integers: x = 0, wl = wr = 0, bias = 1 gives pre = 1 everywhere, so h is keep_scale exactly where the bit
    r * dout + c is set, for a pattern that no transposed or word-swapped reading reproduces."""
    from recommendation_amd import functional as Fn
    n, din, dout = 70, 32, 64
    r = Raw(n=n, din=din, dout=dout, act=0)
    keep = (torch.arange(n * dout) * 7 % 13 < 5).view(n, dout)
    r.x.zero_(), r.z.zero_(), r.wl.zero_(), r.wr.zero_(), r.bias.fill_(1.0)
    r.fwd(keep=Fn.pack_bits(keep.reshape(-1)).cuda(), scale=2.0)
    assert torch.equal(r.h.cpu(), keep.float() * 2.0)
