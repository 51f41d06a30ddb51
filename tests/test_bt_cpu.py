"""The Barlow Twins fixture and the formulas the kernels implement, on the CPU in float64 (no device).

tests/golden/bt.npz (scripts/gen_golden_bt.py) holds the reference's own `WithinEmbedContrast(BarlowTwins())` of
univariate/gbt.py on three pairs of views: float64 loss, cross-correlation and autograd gradients.  Pinned to it here:
  * `functional.bt_loss_composed` / `bt_cross_correlation_composed` (the reference's statements as this project writes them),
  * a numpy restatement of the ANALYTIC backward documented in include/gcr.h (G, t1, t2: no second reduction over n) and of
    the one-evaluation symmetry (the gradient of (l1 + l2) / 2 is the gradient of l1), before any kernel runs,
  * `losses.WithinEmbedContrast(losses.BarlowTwins())` on CPU tensors."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLDEN, "bt.npz")
KEYS = ("loss", "c", "g_h1", "g_h2")
RTOL = 1e-12


@pytest.fixture(scope="module")
def cases():
    z = np.load(PATH)
    out = []
    for k in range(int(z["cases"])):
        pre = f"case{k}/"
        lam = None if np.isnan(z[pre + "lambda"]) else float(z[pre + "lambda"])
        out.append(dict(h1=z[pre + "h1"], h2=z[pre + "h2"], lambda_=lam, batch_norm=bool(z[pre + "batch_norm"]),
                        eps=float(z[pre + "eps"]), ref={key: z[f"{pre}f64/{key}"] for key in KEYS},
                        drift={key: float(z[f"{pre}drift/{key}"]) for key in KEYS}, offset=float(z[pre + "offset"])))
    return out


def _close(got, ref, what):
    scale = float(np.abs(ref).max())
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    assert err <= RTOL * scale, (what, err, scale)


def test_fixture_is_there_and_small(cases):
    assert os.path.getsize(PATH) < 1_000_000
    assert len(cases) == 3
    assert all(c["h1"].dtype == np.float32 and c["h2"].dtype == np.float32 for c in cases)
    assert all(float(np.abs(c["h1"].mean(0)).min()) > 0 and c["offset"] > 0 for c in cases)    # a mean in every column
    assert any(c["lambda_"] is not None for c in cases) and any(c["lambda_"] is None for c in cases)
    assert any(not c["batch_norm"] for c in cases) and any(c["batch_norm"] for c in cases)
    assert any(c["h1"].shape[0] > 256 for c in cases)               # more than one workgroup along the rows
    assert all(c["eps"] == 1e-5 for c in cases)                     # BarlowTwins' default, not bt_loss's 1e-15
    assert all(0 <= v < 2.5e-6 for c in cases for v in c["drift"].values())


def test_composed_float64_reproduces_the_reference(cases):
    from recommendation_amd import functional as Fn
    for k, c in enumerate(cases):
        a, b = (torch.from_numpy(c[key]).double().requires_grad_(True) for key in ("h1", "h2"))
        loss = Fn.bt_loss_composed(a, b, c["lambda_"], c["batch_norm"], c["eps"])
        loss.backward()
        assert loss.dim() == 0
        _close(loss.detach().numpy(), c["ref"]["loss"], (k, "loss"))
        _close(Fn.bt_cross_correlation_composed(a, b, c["batch_norm"], c["eps"]).detach().numpy(), c["ref"]["c"], (k, "c"))
        _close(a.grad.numpy(), c["ref"]["g_h1"], (k, "g_h1"))
        _close(b.grad.numpy(), c["ref"]["g_h2"], (k, "g_h2"))


def analytic(h1, h2, lambda_, batch_norm, eps, g_loss=1.0):
    """include/gcr.h's forward and backward in float64 numpy -> (loss, c, g_h1, g_h2)."""
    h1, h2 = h1.astype(np.float64), h2.astype(np.float64)
    n, d = h1.shape
    lam = 1.0 / d if lambda_ is None else lambda_
    if batch_norm:
        m1, m2 = h1.mean(0), h2.mean(0)
        s1, s2 = h1.std(0, ddof=1), h2.std(0, ddof=1)
        z1, z2 = (h1 - m1) / (s1 + eps), (h2 - m2) / (s2 + eps)
    else:
        z1, z2 = h1, h2
    c = z1.T @ z2 / n
    diag = np.eye(d, dtype=bool)
    loss = ((1 - np.diag(c)) ** 2).sum() + lam * (c[~diag] ** 2).sum()
    G = g_loss * np.where(diag, -2 * (1 - c), 2 * lam * c)
    t1, t2 = (G * c).sum(1), (G * c).sum(0)
    if batch_norm:
        g1 = (z2 @ G.T) / (n * (s1 + eps)) - t1 * (h1 - m1) / ((s1 + eps) * (n - 1) * s1)
        g2 = (z1 @ G) / (n * (s2 + eps)) - t2 * (h2 - m2) / ((s2 + eps) * (n - 1) * s2)
    else:
        g1, g2 = (z2 @ G.T) / n, (z1 @ G) / n
    return loss, c, g1, g2


def test_the_headers_analytic_backward_reproduces_the_reference(cases):
    for k, c in enumerate(cases):
        got = analytic(c["h1"], c["h2"], c["lambda_"], c["batch_norm"], c["eps"])
        for key, val in zip(KEYS, got):
            _close(val, c["ref"][key], (k, key))
        scaled = analytic(c["h1"], c["h2"], c["lambda_"], c["batch_norm"], c["eps"], g_loss=0.37)
        _close(scaled[2], 0.37 * c["ref"]["g_h1"], (k, "g_h1 x 0.37"))
        _close(scaled[3], 0.37 * c["ref"]["g_h2"], (k, "g_h2 x 0.37"))


def test_within_embed_contrast_on_cpu_tensors(cases):
    from recommendation_amd.losses import BarlowTwins, WithinEmbedContrast

    class Counting(BarlowTwins):
        calls = 0

        def compute(self, *a, **kw):
            Counting.calls += 1
            return super().compute(*a, **kw)

    for k, c in enumerate(cases):
        a, b = (torch.from_numpy(c[key]).double().requires_grad_(True) for key in ("h1", "h2"))
        Counting.calls = 0
        loss = WithinEmbedContrast(Counting(c["lambda_"], c["batch_norm"]))(a, b)
        loss.backward()
        assert Counting.calls == 1                                  # one evaluation serves both directions
        _close(loss.detach().numpy(), c["ref"]["loss"], (k, "loss"))
        _close(a.grad.numpy(), c["ref"]["g_h1"], (k, "g_h1"))
        _close(b.grad.numpy(), c["ref"]["g_h2"], (k, "g_h2"))


def test_any_other_loss_is_called_in_both_directions():
    from recommendation_amd.losses import WithinEmbedContrast
    seen = []

    def other(anchor, sample, weight=1.0):
        seen.append((anchor, sample))
        return (anchor * weight - 2 * sample).sum()

    h1, h2 = torch.arange(6.0).reshape(3, 2), torch.ones(3, 2)
    out = WithinEmbedContrast(other, weight=3.0)(h1, h2)
    assert len(seen) == 2 and seen[0][0] is h1 and seen[1][0] is h2
    assert float(out) == float(((h1 * 3 - 2 * h2).sum() + (h2 * 3 - 2 * h1).sum()) * 0.5)


def test_defaults_are_the_references():
    import inspect
    from recommendation_amd import functional as Fn
    from recommendation_amd.losses import BarlowTwins
    assert inspect.signature(Fn.bt_loss).parameters["eps"].default == 1e-15
    assert inspect.signature(Fn.bt_loss_composed).parameters["eps"].default == 1e-15
    loss = BarlowTwins()
    assert (loss.lambda_, loss.batch_norm, loss.eps) == (None, True, 1e-5)
    assert [Fn.bt_supported(d) for d in (32, 64, 96, 128, 256, 48, 512, 16)] == [True] * 5 + [False] * 3
