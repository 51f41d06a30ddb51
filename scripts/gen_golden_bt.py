#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/bt.npz: the Barlow Twins loss of univariate/gbt.py run by the reference
itself on three small pairs of views.

Runs ONLY where the reference sources are (like scripts/gen_golden_buir_steps.py); the fixture is plain data.  gbt.py
imports torch_geometric, so nothing of it is imported: `bt_loss` (:203-217), `Loss.__call__` (:198-200),
`BarlowTwins.compute` (:226-228) and `WithinEmbedContrast.forward` (:392-395) are lifted with
`oracle.gen_golden.load_defs` and executed unchanged; the two shells below only hold the attributes the reference's
constructors store (:221-224, :387-390).  The cross-correlation c is what the statements :208-213 of `bt_loss` leave behind
(`load_stmts`).

Inputs, so that the views are correlated as real views are and every column has a mean:
    M = randn(d, d) / sqrt(d),  colscale ~ U[0.5, 1.5]
    h1 = (randn(n, d) @ M) * colscale + offset * randn(d)
    h2 = 0.7 * h1 + 0.3 * randn(n, d) @ M + offset * randn(d)
Per case: the float32 inputs, lambda_ (NaN = None), batch_norm, eps; the float64 loss, c, g_h1, g_h2 of
`WithinEmbedContrast(BarlowTwins(lambda_, batch_norm))(h1, h2)` by autograd; the float32 drift of each,
max |f32 - f64| / S with S = max |f64| (d for the loss: its un-cancelled constant sum_j 1^2).
Asserted when the file is written: every drift < 2.5e-6 (then 4 x drift stays under the 1e-5 cap) — the seed is scanned
upward from the case's first until that holds; the file stays under 1,000,000 bytes.

Usage:  python scripts/gen_golden_bt.py [--out DIR]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle.gen_golden import REF, load_defs, load_stmts  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden")
PATH = os.path.join(REF, "univariate", "gbt.py")
MAX_DRIFT = 2.5e-6
KEYS = ("loss", "c", "g_h1", "g_h2")
# n = 300 > 256: the launches over the rows use more than one workgroup
CASES = [dict(n=70, d=32, lambda_=None, batch_norm=True, offset=1.0, seed=11),
         dict(n=300, d=64, lambda_=0.005, batch_norm=True, offset=2.0, seed=21),
         dict(n=45, d=96, lambda_=None, batch_norm=False, offset=0.5, seed=31)]

NS = load_defs(PATH, {"bt_loss"}, ("Loss.__call__", "BarlowTwins.compute", "WithinEmbedContrast.forward"))
C_STMTS = load_stmts(PATH, "bt_loss", 208, 213)


class BarlowTwinsShell:
    compute, __call__ = NS["compute"], NS["__call__"]

    def __init__(self, lambda_=None, batch_norm=True, eps=1e-5):
        self.lambda_, self.batch_norm, self.eps = lambda_, batch_norm, eps


class WithinEmbedContrastShell:
    forward = NS["forward"]

    def __init__(self, loss):
        self.loss, self.kwargs = loss, {}


def make_views(n, d, offset, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    m = r(d, d) / d ** 0.5
    colscale = 0.5 + torch.rand(d, generator=g, dtype=torch.float64)
    h1 = (r(n, d) @ m) * colscale + offset * r(d)
    h2 = 0.7 * h1 + 0.3 * r(n, d) @ m + offset * r(d)
    return h1.float().numpy(), h2.float().numpy()


def reference(h1, h2, lambda_, batch_norm, dtype):
    a, b = (torch.from_numpy(x).to(dtype).requires_grad_(True) for x in (h1, h2))
    loss_obj = BarlowTwinsShell(lambda_, batch_norm)
    loss = WithinEmbedContrastShell(loss_obj).forward(a, b)
    loss.backward()
    env = dict(h1=a.detach(), h2=b.detach(), batch_norm=batch_norm, eps=loss_obj.eps, batch_size=a.size(0), torch=torch)
    exec(C_STMTS, env)
    out = dict(loss=loss.detach(), c=env["c"], g_h1=a.grad, g_h2=b.grad)
    return {k: v.double().numpy() for k, v in out.items()}, loss_obj.eps


def main(out_dir):
    out = dict(cases=len(CASES))
    for k, case in enumerate(CASES):
        for seed in range(case["seed"], case["seed"] + 200):
            h1, h2 = make_views(case["n"], case["d"], case["offset"], seed)
            f64, eps = reference(h1, h2, case["lambda_"], case["batch_norm"], torch.float64)
            f32, _ = reference(h1, h2, case["lambda_"], case["batch_norm"], torch.float32)
            scale = {key: float(case["d"]) if key == "loss" else float(np.abs(f64[key]).max()) for key in KEYS}
            drift = {key: float(np.abs(f32[key] - f64[key]).max()) / scale[key] for key in KEYS}
            print(f"case {k} seed {seed}: " + "  ".join(f"{key} drift {drift[key]:.3g}" for key in KEYS))
            if max(drift.values()) < MAX_DRIFT:
                break
        else:
            raise AssertionError("no seed keeps the reference's float32 drift under the rule")
        assert np.abs(h1.mean(0)).min() > 0 and np.isfinite(f64["loss"])
        pre = f"case{k}/"
        out.update({pre + "h1": h1, pre + "h2": h2, pre + "seed": seed, pre + "offset": case["offset"], pre + "eps": eps,
                    pre + "lambda": np.nan if case["lambda_"] is None else case["lambda_"],
                    pre + "batch_norm": case["batch_norm"]})
        for key in KEYS:
            assert drift[key] < MAX_DRIFT
            out[f"{pre}f64/{key}"], out[f"{pre}scale/{key}"], out[f"{pre}drift/{key}"] = f64[key], scale[key], drift[key]
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "bt.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", os.path.abspath(path), size, "bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT)
