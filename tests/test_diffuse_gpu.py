"""The fused social-diffusion layer (gcr_diffuse_fwd_f32 / gcr_diffuse_bwd_f32 behind functional.diffuse_layer) against
float64, in both `gather` modes.

The component cases are the reference's own statements (diffnet.py:1127-1130) run under float64 autograd
(tests/golden/diffnet_steps.npz, comp<d>/); the launch-shape sweep uses a float64 torch restatement on the CPU.  One rule,
the project's (restated from tests/test_buir_gpu.py):  err / S <= max(4 x drift, 2^-20)  and  err / S <= 1e-5,
S = max |f64|, drift = the float32 error of the SAME float64 source (stored for the component cases, computed here for
the restatement).  Inputs of the sweep are drawn until the float64 pre-activations keep a margin of 8 x their float32 error
from zero, as the fixture's are: a gradient pin must not compare two different ReLU masks."""
import numpy as np
import pytest
import torch

import diffnet_fixture as dfx

pytestmark = pytest.mark.gpu

FLOOR, NORTH_STAR = 2.0 ** -20, 1e-5
EINVAL = "code -1"


@pytest.fixture(scope="module")
def golden():
    return dfx.load()


def _graph(row, col, val, n):
    import recommendation_amd as ra
    return ra.CsrGraph.from_coo(row, col, val, n, n, "cuda")


def _layer(graph, x, w, g, gather):
    from recommendation_amd import functional as Fn
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    wt = torch.from_numpy(w).cuda().requires_grad_(True)
    h = Fn.diffuse_layer(graph, xt, wt, gather=gather)
    assert h.grad_fn is not None and type(h.grad_fn).__name__.startswith("_DiffuseLayer"), "the fused node must run"
    h.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    return dict(h=h.detach().cpu().numpy(), dx=xt.grad.cpu().numpy(), dw=wt.grad.cpu().numpy())


def _check(got, ref, drift, tag):
    """drift: relative to the scale, per key."""
    lines, bad = [], []
    for k, want in ref.items():
        scale = float(np.abs(want).max())
        err = float(np.abs(got[k].astype(np.float64) - want).max()) / scale
        bound = max(4.0 * drift[k], FLOOR)
        lines.append(f"DIFFUSE {tag} {k}: err/S {err:.3g} bound {bound:.3g} (drift {drift[k]:.3g}, S {scale:.3g})")
        if not (np.isfinite(got[k]).all() and err <= bound and err <= NORTH_STAR):
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("d", dfx.COMP_WIDTHS)
def test_component_case_matches_the_reference_in_float64(golden, d):
    c = dfx.component(golden, d)
    graph = _graph(c["row"], c["col"], c["val"], dfx.COMP_N)
    ref = {k: c[k] for k in ("h", "dx", "dw")}
    drift = {k: c[f"drift/{k}"] for k in ref}
    for gather in (True, False):
        _check(_layer(graph, c["x"], c["w"], c["g"], gather), ref, drift, f"component d={d} gather={gather}")


def _restatement(row, col, val, n, x, w, g, dtype):
    s = torch.zeros(n, n, dtype=dtype)
    v = torch.ones(len(row), dtype=dtype) if val is None else torch.from_numpy(val).to(dtype)
    s.index_put_((torch.from_numpy(row), torch.from_numpy(col)), v, accumulate=True)
    xt, wt = torch.from_numpy(x).to(dtype).requires_grad_(True), torch.from_numpy(w).to(dtype).requires_grad_(True)
    pre = torch.cat([s @ xt, xt], 1) @ wt
    h = torch.relu(pre)
    h.backward(torch.from_numpy(g).to(dtype))
    return dict(h=h.detach().double().numpy(), dx=xt.grad.double().numpy(), dw=wt.grad.double().numpy()), pre.detach().double().numpy()


def _sweep_case(n, d):
    """Random S (a few entries per row, repeats allowed, an empty row when there is room), x, w, g with a ReLU margin."""
    for seed in range(50):
        rng = np.random.default_rng([n, d, seed])
        deg = rng.integers(0, 9, n)
        deg[-1] = max(deg[-1], 1)
        if n > 2:
            deg[1] = 0
        row = np.repeat(np.arange(n, dtype=np.int64), deg)
        col = rng.integers(0, n, row.size).astype(np.int64)
        val = None if n == 33 else rng.uniform(0.1, 1.0, row.size).astype(np.float32)
        x, w, g = dfx.component_inputs(d, 1000 + seed, n=n)
        ref, pre64 = _restatement(row, col, val, n, x, w, g, torch.float64)
        f32, pre32 = _restatement(row, col, val, n, x, w, g, torch.float32)
        if np.abs(pre64).min() >= 8.0 * np.abs(pre32 - pre64).max():
            drift = {k: float(np.abs(f32[k] - ref[k]).max()) / float(np.abs(ref[k]).max()) for k in ref}
            return row, col, val, x, w, g, ref, drift
    raise AssertionError("no seed with a ReLU margin")


@pytest.mark.parametrize("d", dfx.COMP_WIDTHS)
@pytest.mark.parametrize("n", [1, 33, 64, 257])
def test_launch_shapes(n, d):
    row, col, val, x, w, g, ref, drift = _sweep_case(n, d)
    graph = _graph(row, col, val, n)
    for gather in (True, False):
        _check(_layer(graph, x, w, g, gather), ref, drift, f"n={n} d={d} gather={gather}")


@pytest.mark.parametrize("d", dfx.COMP_WIDTHS)
def test_an_all_zero_row_of_h_gives_exactly_zero_rows_of_p_and_q(d):
    from recommendation_amd import _lib
    n, zero_rows = 100, [0, 37, 99]
    rng = np.random.default_rng(d)
    deg = rng.integers(1, 6, n)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    graph = _graph(row, rng.integers(0, n, row.size).astype(np.int64), rng.uniform(0.1, 1, row.size).astype(np.float32), n)
    x, w, g = (torch.from_numpy(a).cuda() for a in dfx.component_inputs(d, 7, n=n))
    g = g + 3.0                                                       # no zero in g: the zeros below come from the mask alone
    h = torch.relu(torch.randn(n, d, generator=torch.Generator().manual_seed(d))).cuda()
    h[zero_rows] = 0.0
    p, q, dw = torch.full_like(x, 7.0), torch.full_like(x, 7.0), torch.empty_like(w)
    ws = _lib.workspace("gcr_diffuse_workspace_bytes", n, d, device=x.device)
    _lib.call("gcr_diffuse_bwd_f32", graph.rowptr, graph.col, graph.val, n, x, None, w, h, g, d, p, q, dw, ws, on=x)
    torch.cuda.synchronize()
    assert not p[zero_rows].any() and not q[zero_rows].any()
    live = [r for r in range(n) if r not in zero_rows]
    assert p[live].abs().sum(1).min() > 0 and q[live].abs().sum(1).min() > 0
    m = torch.where(h > 0, g, torch.zeros_like(g)).double()
    for have, want in ((p, m @ w[:d].double().T), (q, m @ w[d:].double().T)):
        assert float((have.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("gather", [True, False])
def test_two_runs_are_bitwise_equal(gather):
    n, d = 2100, 64                                                   # 66 backward workgroups fold into dw
    rng = np.random.default_rng(3)
    deg = rng.integers(0, 20, n)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    graph = _graph(row, rng.integers(0, n, row.size).astype(np.int64), rng.uniform(0.1, 1, row.size).astype(np.float32), n)
    x, w, g = dfx.component_inputs(d, 11, n=n)
    a, b = _layer(graph, x, w, g, gather), _layer(graph, x, w, g, gather)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.abs(a["dw"]).max() > 0


def test_error_returns_and_the_empty_problem():
    from recommendation_amd import _lib, functional as Fn
    assert [d for d in (16, 32, 48, 64, 96, 128, 256) if Fn.diffuse_supported(d)] == [32, 64, 128]
    n, d = 8, 32
    row = np.arange(n, dtype=np.int64)
    graph = _graph(row, row[::-1].copy(), np.ones(n, dtype=np.float32), n)
    x, w, g = (torch.from_numpy(a).cuda() for a in dfx.component_inputs(d, 1, n=n))
    h, p, q, dw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x), torch.full_like(w, 5.0)
    ws = _lib.workspace("gcr_diffuse_workspace_bytes", n, d, device=x.device)
    head = (graph.rowptr, graph.col, graph.val)

    def fwd(n_=n, x_=x, w_=w, d_=d, h_=h):
        _lib.call("gcr_diffuse_fwd_f32", *head, n_, x_, None, w_, d_, h_, on=x)

    def bwd(n_=n, x_=x, d_=d, p_=p, dw_=dw):
        _lib.call("gcr_diffuse_bwd_f32", *head, n_, x_, None, w, h, g, d_, p_, q, dw_, ws, on=x)

    fwd()
    bwd()
    off = torch.empty(n * d + 1, device="cuda")[1:].view(n, d)         # 4-byte aligned only
    for bad in (lambda: fwd(d_=48), lambda: fwd(n_=-1), lambda: fwd(x_=off), lambda: fwd(h_=off), lambda: fwd(h_=x),
                lambda: bwd(d_=48), lambda: bwd(n_=-1), lambda: bwd(x_=off), lambda: bwd(p_=off)):
        with pytest.raises(_lib.GcrError, match=EINVAL):
            bad()
    assert _lib.call("gcr_diffuse_workspace_bytes", 0, d) == 0 and _lib.call("gcr_diffuse_workspace_bytes", n, 48) == 0
    h.fill_(3.0)
    fwd(n_=0)                                                          # OK, nothing written
    bwd(n_=0)                                                          # OK: dw zeroed
    torch.cuda.synchronize()
    assert bool((h == 3.0).all()) and not dw.any()
