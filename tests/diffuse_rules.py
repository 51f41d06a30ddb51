"""What the diffusion-layer tests share (tests/test_diffuse_gpu.py, tests/test_diffuse_paths_gpu.py and
tests/test_diffuse_rules_cpu.py): the comparison rule, the float64 restatements of the layer, and the case builders.

The rule, the project's (restated from tests/test_buir_gpu.py):  err / S <= max(4 x drift, 2^-20)  and  err / S <= 1e-5,
S = max |f64|, drift = the float32 error of the SAME float64 source.

The layer, diffnet.py:1127-1130, four statements:  z = sparse.mm(S, x);  c = cat([z, x], 1);  pre = c @ w;  h = relu(pre).
`dense_restatement` writes S as a dense [n, n] matrix; `sparse_restatement` keeps it a COO tensor (duplicates sum in
both), which is what a case of 32833 rows needs.

A small case is drawn until every float64 pre-activation keeps 8 x the float32 error from zero (`margin_case`): a gradient
pin must not compare two different ReLU masks.  With about 2 M pre-activations no seed does that, so `large_case` makes
the mask irrelevant where it is ambiguous instead: g = 0 wherever |pre64| < 8 x max |pre32 - pre64|.  g is an input, so
every element of h, dx and dw is still compared; the share of g zeroed this way must stay <= MAX_ZEROED_SHARE."""
import functools

import numpy as np
import torch

import diffnet_fixture as dfx

FLOOR, NORTH_STAR = 2.0 ** -20, 1e-5
KEYS = ("h", "dx", "dw")
# a row's entry count against fill_tile's 8-deep gather: no block, a tail alone, blocks with and without a tail
UNROLL_DEGREES = (0, 1, 7, 8, 9, 15, 16, 17, 24, 41)
# the smallest n with 514 forward tiles over 512 workgroups at every width (1027 backward tiles over 512, 514 over 256);
# the last tile holds one row
MULTI_TRIP_SHAPES = ((32833, 32), (32833, 64), (16417, 128))
MAX_ZEROED_SHARE = 1e-3


def check(got, ref, drift, tag):
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


def drift_of(f32, ref):
    return {k: float(np.abs(f32[k] - ref[k]).max()) / float(np.abs(ref[k]).max()) for k in ref}


def _values(val, nnz, dtype):
    return torch.ones(nnz, dtype=dtype) if val is None else torch.from_numpy(val).to(dtype)


def _finish(xt, wt, pre, g, dtype):
    h = torch.relu(pre)
    h.backward(torch.from_numpy(g).to(dtype))
    return dict(h=h.detach().double().numpy(), dx=xt.grad.double().numpy(), dw=wt.grad.double().numpy()), pre.detach().double().numpy()


def dense_restatement(row, col, val, n, x, w, g, dtype):
    """(dict of h, dx, dw, pre), all float64 arrays, computed in `dtype` with S a dense matrix."""
    s = torch.zeros(n, n, dtype=dtype)
    s.index_put_((torch.from_numpy(row), torch.from_numpy(col)), _values(val, len(row), dtype), accumulate=True)
    xt, wt = torch.from_numpy(x).to(dtype).requires_grad_(True), torch.from_numpy(w).to(dtype).requires_grad_(True)
    pre = torch.cat([s @ xt, xt], 1) @ wt
    return _finish(xt, wt, pre, g, dtype)


def _sparse_forward(row, col, val, n, x, w, dtype):
    s = torch.sparse_coo_tensor(torch.stack([torch.from_numpy(row), torch.from_numpy(col)]), _values(val, len(row), dtype), (n, n))
    xt, wt = torch.from_numpy(x).to(dtype).requires_grad_(True), torch.from_numpy(w).to(dtype).requires_grad_(True)
    return xt, wt, torch.cat([torch.sparse.mm(s, xt), xt], 1) @ wt


def sparse_restatement(row, col, val, n, x, w, g, dtype):
    """`dense_restatement` with S a COO tensor under torch.sparse.mm."""
    return _finish(*_sparse_forward(row, col, val, n, x, w, dtype), g, dtype)


def margin_case(draw, restatement=dense_restatement, seeds=50):
    """The first of `draw(seed)` = (row, col, val, n, x, w, g), seed = 0, 1, ..., whose float64 pre-activations keep 8 x
    their float32 error from zero: (row, col, val, x, w, g, ref, drift)."""
    for seed in range(seeds):
        row, col, val, n, x, w, g = draw(seed)
        ref, pre64 = restatement(row, col, val, n, x, w, g, torch.float64)
        f32, pre32 = restatement(row, col, val, n, x, w, g, torch.float32)
        if np.abs(pre64).min() >= 8.0 * np.abs(pre32 - pre64).max():
            return row, col, val, x, w, g, ref, drift_of(f32, ref)
    raise AssertionError("no seed with a ReLU margin")


def unroll_case(d, ones, n=64):
    """Row r has UNROLL_DEGREES[r % 10] entries (so the two rows a wave walks together at d = 32 always differ in length),
    with a repeated column in every row of two or more entries and a self-loop in every third row."""
    deg = np.array([UNROLL_DEGREES[r % len(UNROLL_DEGREES)] for r in range(n)])
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    start = np.concatenate([[0], np.cumsum(deg)])

    def draw(seed):
        rng = np.random.default_rng([n, d, int(ones), seed])
        col = rng.integers(0, n, row.size).astype(np.int64)
        for r in range(n):
            if deg[r] >= 2:
                col[start[r] + 1] = col[start[r]]
            if deg[r] >= 1 and r % 3 == 0:
                col[start[r + 1] - 1] = r
        val = None if ones else rng.uniform(0.1, 1.0, row.size).astype(np.float32)
        return (row, col, val, n) + dfx.component_inputs(d, 2000 + seed, n=n)

    return margin_case(draw)


def large_graph(n, rng):
    """Row 0 has 1000 entries, row 1 none, the last row 9; every other row 0..4, one in twenty a draw from UNROLL_DEGREES.
    Columns are uniform over [0, n) and n - 1 occurs."""
    deg = rng.integers(0, 5, n)
    special = rng.random(n) < 0.05
    deg[special] = rng.choice(UNROLL_DEGREES, int(special.sum()))
    deg[0], deg[1], deg[-1] = 1000, 0, 9
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    col = rng.integers(0, n, row.size).astype(np.int64)
    col[0] = n - 1
    val = rng.uniform(0.1, 1.0, row.size).astype(np.float32)
    return row, col, val


@functools.lru_cache(maxsize=None)
def large_case(n, d):
    """A case of `large_graph` with g zeroed where the ReLU mask is ambiguous (module docstring), as a dict the tests
    share and do not write to: row, col, val, x, w, g, ref (float64 h, dx, dw by `sparse_restatement`), drift, share (of g
    zeroed)."""
    rng = np.random.default_rng([n, d])
    row, col, val = large_graph(n, rng)
    x, w, g = dfx.component_inputs(d, 3000, n=n)
    with torch.no_grad():
        pre64 = _sparse_forward(row, col, val, n, x, w, torch.float64)[2].numpy()
        pre32 = _sparse_forward(row, col, val, n, x, w, torch.float32)[2].double().numpy()
    ambiguous = np.abs(pre64) < 8.0 * np.abs(pre32 - pre64).max()
    share = float(ambiguous.mean())
    assert share <= MAX_ZEROED_SHARE, f"n={n} d={d}: {share:.3g} of g would be zeroed"
    g[ambiguous] = 0.0
    ref, _ = sparse_restatement(row, col, val, n, x, w, g, torch.float64)
    f32, _ = sparse_restatement(row, col, val, n, x, w, g, torch.float32)
    return dict(row=row, col=col, val=val, x=x, w=w, g=g, ref=ref, drift=drift_of(f32, ref), share=share)


def exact_case(d, ones, n=257):
    """Small integers: x in [-3, 3], w in {-1, 0, 1}, g in [-2, 2], val in {1, 2} or None, row degrees from UNROLL_DEGREES.
    |z| <= 41 * 2 * 3, |pre| <= 2 d * 246, |p|, |q| <= 2 d, |dw| <= n * 246 * 2 and dx sums at most nnz p's: every product
    and partial sum is an integer far below 2^24, exact in float32 in any order.  Row 1 has no entries and x[1] = 0, and
    column 3 of w is zero, so pre is 0 on all of row 1 and of column 3 (a wrong mask at 0 shows in dx there, resp. in dw).
    Returns (row, col, val, x, w, g)."""
    rng = np.random.default_rng([n, d, int(ones), 7])
    deg = rng.choice(UNROLL_DEGREES, n)
    deg[1] = 0
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    col = rng.integers(0, n, row.size).astype(np.int64)
    val = None if ones else rng.integers(1, 3, row.size).astype(np.float32)
    x = rng.integers(-3, 4, (n, d)).astype(np.float32)
    w = rng.integers(-1, 2, (2 * d, d)).astype(np.float32)
    g = rng.integers(-2, 3, (n, d)).astype(np.float32)
    x[1], w[:, 3] = 0.0, 0.0
    g[1], g[:, 3] = 1.0, 2.0
    return row, col, val, x, w, g


def device_graph(row, col, val, n):
    import recommendation_amd as ra
    return ra.CsrGraph.from_coo(row, col, val, n, n, "cuda")


def fused_layer(graph, x, w, g, gather):
    """h, dx, dw of functional.diffuse_layer on the device, as float32 arrays; the node must be the fused one."""
    from recommendation_amd import functional as Fn
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    wt = torch.from_numpy(w).cuda().requires_grad_(True)
    h = Fn.diffuse_layer(graph, xt, wt, gather=gather)
    assert h.grad_fn is not None and type(h.grad_fn).__name__.startswith("_DiffuseLayer"), "the fused node must run"
    h.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    return dict(h=h.detach().cpu().numpy(), dx=xt.grad.cpu().numpy(), dw=wt.grad.cpu().numpy())
