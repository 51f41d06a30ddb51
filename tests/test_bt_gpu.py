"""The fused Barlow Twins loss through `functional` / `losses`: gcr_col_stats_f32 (`column_stats`), gcr_bt_fwd_f32 /
gcr_bt_bwd_f32 (`bt_loss`), `BarlowTwins` and `WithinEmbedContrast`.

The three cases of tests/golden/bt.npz (scripts/gen_golden_bt.py: the reference's own `WithinEmbedContrast(BarlowTwins())`,
float64 autograd) are checked by tests/f64_pins.py's rule, restated here because f64_pins.FAMILIES is fixed:
    err / S <= max(4 x drift, 2^-20)  and  err / S <= 1e-5,   S = max |f64| (d for the loss: its un-cancelled sum_j 1^2),
drift = the reference's own float32 error.  Every other case uses the same rule against `bt_loss_composed` (the reference's
statements) run in float64 on the CPU, with drift = the float32 error of the SAME composition on the same inputs on the
CPU at test time — never measured on the code under test.

Nothing at module level touches a device: tests/test_bt_geometry_cpu.py imports the shape tables below."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR, NORTH_STAR = 2.0 ** -20, 1e-5
KEYS = ("loss", "c", "g_h1", "g_h2")

WIDTHS = (32, 64, 96, 128, 256)
# n = 7: odd, less than one unrolled group of row pairs, one workgroup; 513: three workgroups, the last holds one row
SWEEP = [(n, d) for d in WIDTHS for n in (7, 513, 4099)]
# above the row count at which the product launch stops adding workgroups (1024 x 256 rows; 256 x 256 at d = 256), odd tails
LARGE = [(300001, 32), (70001, 256)]
OFFSET_CASE = (777, 256)
BRANCH_SHAPE = (513, 64)
REPRO_SHAPE = (4099, 128)
ALL_SHAPES = SWEEP + LARGE + [OFFSET_CASE, BRANCH_SHAPE, REPRO_SHAPE]


def make_views(n, d, offset=1.0, seed=0):
    """scripts/gen_golden_bt.py's recipe: correlated views with a mean in every column (float32)."""
    rng = np.random.default_rng(100003 * d + n + seed)
    m = rng.standard_normal((d, d)) / np.sqrt(d)
    colscale = rng.uniform(0.5, 1.5, d)
    h1 = (rng.standard_normal((n, d)) @ m) * colscale + offset * rng.standard_normal(d)
    h2 = 0.7 * h1 + 0.3 * rng.standard_normal((n, d)) @ m + offset * rng.standard_normal(d)
    return h1.astype(np.float32), h2.astype(np.float32)


def composed(h1, h2, lambda_, batch_norm, eps, g, dtype):
    """`bt_loss_composed` on the CPU at `dtype` -> {key: float64 numpy}."""
    from recommendation_amd import functional as Fn
    a, b = (torch.from_numpy(x).to(dtype).requires_grad_(True) for x in (h1, h2))
    loss = Fn.bt_loss_composed(a, b, lambda_, batch_norm, eps)
    (loss * g).backward()
    with torch.no_grad():
        c = Fn.bt_cross_correlation_composed(a, b, batch_norm, eps)
    return {k: v.detach().double().numpy() for k, v in dict(loss=loss, c=c, g_h1=a.grad, g_h2=b.grad).items()}


@functools.lru_cache(maxsize=None)
def _pinned(n, d, offset, lambda_, batch_norm, g):
    """Inputs, the float64 reference and the float32 drift of one case, computed once per session."""
    h1, h2 = make_views(n, d, offset)
    ref = composed(h1, h2, lambda_, batch_norm, 1e-15, g, torch.float64)
    f32 = composed(h1, h2, lambda_, batch_norm, 1e-15, g, torch.float32)
    return h1, h2, ref, {k: float(np.abs(f32[k] - ref[k]).max()) for k in KEYS}


def fused(h1, h2, lambda_, batch_norm, eps, g, fn=None):
    from recommendation_amd import functional as Fn
    a, b = (torch.from_numpy(x).to(DEV).requires_grad_(True) for x in (h1, h2))
    loss = (fn or Fn.bt_loss)(a, b, lambda_, batch_norm, eps)
    assert loss.dim() == 0 and loss.is_cuda
    (loss * g).backward()
    out = dict(loss=loss.detach(), g_h1=a.grad, g_h2=b.grad)
    if fn is None and Fn.bt_supported(h1.shape[1]):            # c through the raw ABI; the same launches, the same loss
        lam = 1.0 / h1.shape[1] if lambda_ is None else lambda_
        raw_loss, out["c"], _ = Fn.bt_forward_raw(a.detach(), b.detach(), lam, batch_norm, eps)
        assert torch.equal(raw_loss.reshape(()), out["loss"])
    return out


def check(got, ref, drift, tag, d, keys=KEYS, cols=None):
    """The bound rule; prints every figure before asserting.  cols: a column mask applied to the gradients."""
    bad = []
    for k in keys:
        r, x = ref[k], got[k].detach().cpu().double().numpy()
        if cols is not None and k.startswith("g_"):
            r, x = r[:, cols[k]], x[:, cols[k]]
        scale = float(d) if k == "loss" else float(np.abs(r).max())
        err = float(np.abs(x - r).max())
        bound = max(4.0 * drift[k] / scale, FLOOR)
        print(f"BTPIN {tag}:{k} err={err / scale:.3e} bound={bound:.3e} ratio={err / scale / bound:.3f}")
        if not (err / scale <= bound and err / scale <= NORTH_STAR):
            bad.append((k, err / scale, bound))
    assert not bad, (tag, bad)


def pin(n, d, offset=1.0, lambda_=None, batch_norm=True, g=0.37, fn=None):
    h1, h2, ref, drift = _pinned(n, d, offset, lambda_, batch_norm, g)
    got = fused(h1, h2, lambda_, batch_norm, 1e-15, g, fn=fn)
    check(got, ref, drift, f"n{n}_d{d}_off{offset:g}_lam{lambda_}_bn{int(batch_norm)}", d,
          keys=[k for k in KEYS if k in got])
    return got


@pytest.mark.parametrize("case", [0, 1, 2])
def test_fixture_case_matches_reference_float64(case):
    from recommendation_amd import functional as Fn
    from recommendation_amd.losses import BarlowTwins, WithinEmbedContrast
    z = np.load(os.path.join(GOLDEN, "bt.npz"))
    pre = f"case{case}/"
    lam = None if np.isnan(z[pre + "lambda"]) else float(z[pre + "lambda"])
    bn, eps = bool(z[pre + "batch_norm"]), float(z[pre + "eps"])
    a, b = (torch.from_numpy(z[pre + k]).to(DEV).requires_grad_(True) for k in ("h1", "h2"))
    d = a.shape[1]
    loss = WithinEmbedContrast(BarlowTwins(lam, bn))(a, b)
    loss.backward()
    c = Fn.bt_forward_raw(a.detach(), b.detach(), 1.0 / d if lam is None else lam, bn, eps)[1]
    ref = {k: z[f"{pre}f64/{k}"] for k in KEYS}
    for k in KEYS:
        assert float(z[f"{pre}scale/{k}"]) == (float(d) if k == "loss" else float(np.abs(ref[k]).max()))
    drift = {k: float(z[f"{pre}drift/{k}"]) * float(z[f"{pre}scale/{k}"]) for k in KEYS}
    check(dict(loss=loss.detach(), c=c, g_h1=a.grad, g_h2=b.grad), ref, drift, f"fixture{case}", d)


@pytest.mark.parametrize("n, d", SWEEP)
def test_sweep_matches_float64_composition(n, d):
    pin(n, d)                                                      # g = 0.37: the upstream factor is applied


def test_offset_case_column_means_of_tens_of_standard_deviations():
    n, d = OFFSET_CASE
    h1 = make_views(n, d, 20.0)[0]
    assert float((np.abs(h1.mean(0)) / h1.std(0)).max()) > 20.0
    pin(n, d, offset=20.0)


@pytest.mark.parametrize("n, d", LARGE)
def test_rows_above_the_grid_cap(n, d):
    pin(n, d)


@pytest.mark.parametrize("lambda_, batch_norm", [(0.005, True), (None, True), (0.005, False), (None, False)])
def test_branches(lambda_, batch_norm):
    pin(*BRANCH_SHAPE, lambda_=lambda_, batch_norm=batch_norm)


def test_upstream_factor_is_applied():
    n, d = BRANCH_SHAPE
    h1, h2 = make_views(n, d)
    one, scaled = fused(h1, h2, None, True, 1e-15, 1.0), fused(h1, h2, None, True, 1e-15, 0.37)
    assert torch.equal(one["loss"], scaled["loss"])
    for k in ("g_h1", "g_h2"):
        ratio = float(scaled[k].abs().max() / one[k].abs().max())
        assert abs(ratio - 0.37) < 1e-5, (k, ratio)
    pin(n, d, g=0.37)
    pin(n, d, g=1.0)


def test_only_the_view_that_asks_gets_a_gradient():
    from recommendation_amd import functional as Fn
    n, d = BRANCH_SHAPE
    h1, h2, ref, drift = _pinned(n, d, 1.0, None, True, 0.37)
    a = torch.from_numpy(h1).to(DEV).requires_grad_(True)
    b = torch.from_numpy(h2).to(DEV)
    (Fn.bt_loss(a, b) * 0.37).backward()
    assert b.grad is None
    check(dict(g_h1=a.grad), ref, drift, "only_h1", d, keys=["g_h1"])
    a2 = torch.from_numpy(h1).to(DEV)
    b2 = torch.from_numpy(h2).to(DEV).requires_grad_(True)
    (Fn.bt_loss(a2, b2) * 0.37).backward()
    assert a2.grad is None
    check(dict(g_h2=b2.grad), ref, drift, "only_h2", d, keys=["g_h2"])


@pytest.mark.parametrize("d", [48, 1024])
def test_column_stats(d):
    from recommendation_amd import functional as Fn
    x = make_views(513, d, 20.0)[0]
    x64 = torch.from_numpy(x).double()
    ref = dict(mean=x64.mean(0).numpy(), std=x64.std(0).numpy())
    x32 = torch.from_numpy(x)
    f32 = dict(mean=x32.mean(0).double().numpy(), std=x32.std(0).double().numpy())
    mean, std = Fn.column_stats(torch.from_numpy(x).to(DEV))
    again = Fn.column_stats(torch.from_numpy(x).to(DEV))
    assert torch.equal(mean, again[0]) and torch.equal(std, again[1])
    bad = []
    for k, got in (("mean", mean), ("std", std)):
        scale = float(np.abs(ref[k]).max())
        err = float(np.abs(got.cpu().double().numpy() - ref[k]).max()) / scale
        bound = max(4.0 * float(np.abs(f32[k] - ref[k]).max()) / scale, FLOOR)
        print(f"BTPIN column_stats_d{d}:{k} err={err:.3e} bound={bound:.3e} ratio={err / bound:.3f}")
        if not (err <= bound and err <= NORTH_STAR):
            bad.append((k, err, bound))
    assert not bad, bad


def test_constant_column_gets_a_zero_gradient_column():
    n, d, col = 513, 64, 5
    h1, h2 = make_views(n, d)
    h1[:, col] = 3.25                                              # mean exactly 3.25, std exactly 0 in every precision
    ref = composed(h1, h2, None, True, 1e-15, 0.37, torch.float64)
    f32 = composed(h1, h2, None, True, 1e-15, 0.37, torch.float32)
    # the reference differentiates (h - mean) / (0 + eps) there: a column of magnitude 1 / eps (NaN where torch leaves
    # std's backward unmasked at 0); the kernel writes zeros instead (include/gcr.h), so that column is not compared
    assert not (np.abs(ref["g_h1"][:, col]) < 1e6).any() and np.isfinite(np.delete(ref["g_h1"], col, axis=1)).all()
    assert np.isfinite(ref["g_h2"]).all() and np.isfinite(ref["loss"]) and (ref["c"][col] == 0).all()
    cols = dict(g_h1=np.arange(d) != col, g_h2=np.ones(d, dtype=bool))
    drift = {k: float(np.abs((f32[k] - ref[k])[:, cols[k]] if k in cols else f32[k] - ref[k]).max()) for k in KEYS}
    got = fused(h1, h2, None, True, 1e-15, 0.37)
    check(got, ref, drift, "constant_column", d, cols=cols)
    assert bool((got["g_h1"][:, col] == 0).all()) and bool(torch.isfinite(got["g_h1"]).all())
    assert bool((got["c"][col] == 0).all())


@pytest.mark.parametrize("d", [48, 512])
def test_unsupported_width_runs_the_composed_path(d):
    from recommendation_amd import _lib, functional as Fn
    assert not Fn.bt_supported(d) and _lib.lib().gcr_bt_workspace_bytes(513, d) == 0
    assert [Fn.bt_supported(w) for w in WIDTHS] == [True] * len(WIDTHS)
    assert all(bool(_lib.lib().gcr_bt_supported(w)) == Fn.bt_supported(w) for w in (*WIDTHS, 16, 48, 160, 512))
    pin(513, d)
    a = torch.from_numpy(make_views(513, d)[0]).to(DEV)
    with pytest.raises(_lib.GcrError):                              # the C entry refuses what it does not serve
        Fn.bt_forward_raw(a, a, 0.1)


def test_composed_path_on_a_supported_width():
    from recommendation_amd import functional as Fn
    pin(*BRANCH_SHAPE, fn=Fn.bt_loss_composed)


def test_cpu_tensors_are_refused():
    from recommendation_amd import _lib, functional as Fn
    h1, h2 = (torch.from_numpy(x) for x in make_views(7, 32))
    with pytest.raises(_lib.GcrError):
        Fn.bt_loss(h1, h2)


def test_two_calls_are_bitwise_equal():
    h1, h2 = make_views(*REPRO_SHAPE)
    a, b = fused(h1, h2, None, True, 1e-15, 0.37), fused(h1, h2, None, True, 1e-15, 0.37)
    assert all(torch.equal(a[k], b[k]) for k in KEYS)
