"""What the GraphSAGE tests and the writer of tests/golden/sage_steps.npz (scripts/gen_golden_sage_steps.py) share: the
comparison rule, the float64 restatement of one layer, the case builders and the fixture's key layout.

The rule, the project's (restated from tests/diffuse_rules.py `check`):  err / S <= max(4 x drift, 2^-20)  and
err / S <= 1e-5,  S = max |f64|, drift = the float32 error of the SAME float64 source.  Training steps are held to
tests/step_pins.py's rules (`check_steps`: `term_tol` with the float32 run for the loss, `atol_floor_1` for a final
parameter, `has_moved` and `sees_dropped` for what the tolerance sees).

The layer, graphsage.py:28-30 over torch_geometric's SAGEConv (mean aggregation, root weight, bias), for edges j -> i
(src, dst), duplicates and self loops counted as they come:
    z_i = mean over the edges into i of x_j (0 without one);  pre = z wl^T + bias + x wr^T;  a = act(pre);
    h = a * keep / (1 - p).
`restatement` runs these in a given dtype under autograd.  ReLU has a kink at zero, so a relu case is drawn until every
float64 pre-activation keeps 8 x the float32 error from zero (`margin_case`, `has_margin`: gat_rules.has_margin's rule).
With millions of pre-activations no seed does that, so `large_case` makes the mask irrelevant where it is ambiguous
instead (diffuse_rules.large_case's method): g = 0 wherever |pre64| < 8 x max |pre32 - pre64|; g is an input, so every
element of every output is still compared, and the share of g zeroed this way must stay <= MAX_ZEROED_SHARE.

For tests/test_sage_paths_gpu.py: `hub_graph` (long rows in A and in A^T, for the SpMM's windowed route), `exact_case`
(integers, where float32 is exact and equality is owed; `assert_exact`), `tail_case` (gelu far from zero), `Raw` (the raw
exports' arguments, with sentinels for the bounds tests).  tests/test_sage_cpu.py asserts each builder's conditions."""
import functools
import os

import numpy as np
import torch

import step_pins as sp

FLOOR, NORTH_STAR = 2.0 ** -20, 1e-5
MAX_ZEROED_SHARE = 1e-3                      # diffuse_rules.MAX_ZEROED_SHARE
KEYS = ("h", "dx", "dwl", "dwr", "dbias")
WIDTHS = (32, 64, 128)
PAIRS = tuple((a, b) for a in WIDTHS for b in WIDTHS)          # every (din, dout) the kernels serve
ACTS = ("none", "relu", "gelu")
# a node's in-degree cycle: none, one, a few, many
DEGREES = (0, 1, 3, 8, 2, 17, 5, 1, 41, 4)
# Multi-trip: the smallest n at which each launch's tile count exceeds its workgroup cap, once per width class
# (csrc/gcr_sage.hip: the forward walks 64-row tiles for din <= 64 and 32-row tiles for din = 128, the backward 32-row
# tiles, each under a cap of 1024 workgroups; W sits in LDS where din * dout <= 4096 and is read through the caches
# elsewhere, which are different kernels).
#   din <= 64:  n = 1024 * 64 + 1 = 65537 gives 1025 forward tiles over 1024 workgroups (workgroup 0 takes a second trip,
#               whose tile holds one row; n - 1 gives 1024) and 2049 backward tiles over 1024;
#   din = 128:  n = 1024 * 32 + 1 = 32769 gives 1025 forward and 1025 backward tiles over 1024 (n - 1 gives 1024 of each).
# One pair per (forward tile rows, W in LDS) class: (32, 32) 64 / yes, (64, 128) 64 / no, (128, 64) 32 / no, (128, 32) 32 / yes.
FWD_CAP = BWD_CAP = 1024
MULTI_TRIP_SHAPES = ((65537, 32, 32), (65537, 64, 128), (32769, 128, 64), (32769, 128, 32))
# Hub rows: the smallest width at which the SpMM's windowed hub plan (graph.HubPlan) both exists and is used, for z = A x
# and for dx = A^T p + q, at the multi-trip n (one row above the smallest table that qualifies).  The plan is eligible when
# the gathered table is at least 16 MiB and one 16384-row window at most 4 MiB: at d = 64, 65537 x 256 B >= 16 MiB and
# 16384 x 256 B = 4 MiB; at d = 32 the table is too small, at d = 128 the window too large.  A hub row has more than max(128, 8 x 5 windows) entries.  (64, 32): W in LDS; (64, 128): W through the
# caches.
HUB_N, HUB_EXTRA, HUB_PAIRS = 65537, 3000, ((64, 32), (64, 128))
# Exact cases: in-degrees whose reciprocals are powers of two, 70 rows = a partial tile for 32- and for 64-row tiles
EXACT_N, EXACT_DEGREES = 70, (0, 1, 2, 4, 8)
SENTINEL = -1.2345678e30                     # no kernel output: what the bounds tests fill with and look for
COMP_N, COMP_P = 12, 0.5                     # the fixture's layer cases
COMP_CASES = ((32, 64, "gelu"), (64, 32, "relu"), (32, 32, "none"))
STEP_CASES = ("A", "B", "C")
GOLDEN = os.path.join(sp.GOLDEN, "sage_steps.npz")
IN_CHANNELS = OUT_CHANNELS = 64


def check(got, ref, drift, tag):
    """drift: relative to the scale, per key."""
    lines, bad = [], []
    for k, want in ref.items():
        scale = float(np.abs(want).max()) or 1.0
        err = float(np.abs(np.asarray(got[k], dtype=np.float64) - want).max()) / scale
        bound = max(4.0 * drift[k], FLOOR)
        lines.append(f"SAGE {tag} {k}: err/S {err:.3g} bound {bound:.3g} (drift {drift[k]:.3g}, S {scale:.3g})")
        if not (np.isfinite(got[k]).all() and err <= bound and err <= NORTH_STAR):
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


def drift_of(f32, ref):
    return {k: float(np.abs(f32[k] - ref[k]).max()) / (float(np.abs(ref[k]).max()) or 1.0) for k in ref}


def has_margin(pre64, pre32):
    """Every float64 pre-activation keeps 8 x the float32 error from ReLU's kink."""
    return bool(np.abs(pre64).min() >= 8.0 * np.abs(pre32 - pre64).max())


def margin_of(pre64, pre32):
    return float(np.abs(pre64).min() / max(np.abs(pre32 - pre64).max(), 1e-300))


def activation(name, pre):
    if name == "relu":
        return torch.where(pre > 0, pre, torch.zeros_like(pre))
    if name == "gelu":
        return 0.5 * pre * (1.0 + torch.erf(pre / np.sqrt(2.0)))
    assert name == "none", name
    return pre


def mean_rows(src, dst, n, xt):
    """z [n, d]: the mean of x over the edges into each node, in xt's dtype."""
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    deg = torch.zeros(n, dtype=xt.dtype).index_add_(0, d, torch.ones(d.numel(), dtype=xt.dtype))
    return torch.zeros(n, xt.shape[1], dtype=xt.dtype).index_add_(0, d, xt[s]) / deg.clamp(min=1.0)[:, None]


def forward_pre(src, dst, n, x, wl, wr, bias, dtype):
    """The pre-activation alone, a float64 array computed in `dtype`."""
    with torch.no_grad():
        t = [None if v is None else torch.from_numpy(v).to(dtype) for v in (x, wl, wr, bias)]
        pre = mean_rows(src, dst, n, t[0]) @ t[1].T + t[0] @ t[2].T
        return (pre if t[3] is None else pre + t[3]).double().numpy()


def restatement(src, dst, n, x, wl, wr, bias, g, act, dtype, keep=None, p=0.0, root=True):
    """(dict of h, dx, dwl, dwr and, with a bias, dbias; pre), float64 arrays computed in `dtype`.  keep: bool [n, dout]
    or None.  root=False drops the x wr^T term (what the step fixture's sensitivity figures and the mutation run drop)."""
    xt, lt, rt = (torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (x, wl, wr))
    bt = None if bias is None else torch.from_numpy(bias).to(dtype).requires_grad_(True)
    pre = mean_rows(src, dst, n, xt) @ lt.T
    if bt is not None:
        pre = pre + bt
    if root:
        pre = pre + xt @ rt.T
    h = activation(act, pre)
    if keep is not None:
        h = h * torch.from_numpy(keep).to(dtype) / (1.0 - p)
    h.backward(torch.from_numpy(g).to(dtype))
    res = dict(h=h.detach(), dx=xt.grad, dwl=lt.grad, dwr=rt.grad if root else torch.zeros_like(rt))
    if bt is not None:
        res["dbias"] = bt.grad
    return {k: v.double().numpy() for k, v in res.items()}, pre.detach().double().numpy()


def sweep_graph(n, seed=0):
    """(src, dst) int64, dst ascending: node r has DEGREES[r % 10] in-edges (node 1 none), uniform sources; every node
    with two or more has a repeated source, every third node with one or more a self loop."""
    rng = np.random.default_rng([n, seed])
    deg = np.array([DEGREES[r % len(DEGREES)] for r in range(n)])
    if n > 1:
        deg[1] = 0
    else:
        deg[0] = 1                                             # a single node: its self loop
    dst = np.repeat(np.arange(n, dtype=np.int64), deg)
    src = rng.integers(0, n, dst.size).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(deg)])
    for r in range(n):
        if deg[r] >= 2:
            src[start[r] + 1] = src[start[r]]
        if deg[r] >= 1 and r % 3 == 0:
            src[start[r + 1] - 1] = r
    return src, dst


def inputs(n, din, dout, seed):
    """x ~ N(0, 1) [n, din], wl, wr ~ U(+-1 / sqrt(din)) [dout, din], bias ~ U(+-1 / sqrt(din)), g ~ N(0, 1) [n, dout]."""
    rng = np.random.default_rng([n, din, dout, seed])
    b = 1.0 / np.sqrt(din)
    x = rng.standard_normal((n, din)).astype(np.float32)
    wl, wr = (rng.uniform(-b, b, (dout, din)).astype(np.float32) for _ in range(2))
    bias = rng.uniform(-b, b, dout).astype(np.float32)
    g = rng.standard_normal((n, dout)).astype(np.float32)
    return x, wl, wr, bias, g


def keep_mask(n, dout, p, seed):
    """bool [n, dout], `rand >= p` as F.dropout keeps; None at p = 0."""
    return None if p == 0.0 else np.random.default_rng([n, dout, seed, 77]).random((n, dout)) >= p


def _case(src, dst, n, din, dout, act, p, seed, with_bias, x, wl, wr, bias, g, keep):
    bias = bias if with_bias else None
    ref, _ = restatement(src, dst, n, x, wl, wr, bias, g, act, torch.float64, keep, p)
    f32, _ = restatement(src, dst, n, x, wl, wr, bias, g, act, torch.float32, keep, p)
    return dict(src=src, dst=dst, n=n, din=din, dout=dout, act=act, p=p, seed=seed, x=x, wl=wl, wr=wr, bias=bias, g=g,
                keep=keep, ref=ref, drift=drift_of(f32, ref))


@functools.lru_cache(maxsize=None)
def margin_case(n, din, dout, act, p, with_bias=True, seeds=200):
    """A case on `sweep_graph(n)`: the first seed's inputs (for relu: whose pre-activations keep the margin), with ref
    (float64) and drift; shared among the tests that need it and never written to."""
    src, dst = sweep_graph(n)
    for seed in range(seeds):
        x, wl, wr, bias, g = inputs(n, din, dout, seed)
        b = bias if with_bias else None
        if act == "relu" and not has_margin(forward_pre(src, dst, n, x, wl, wr, b, torch.float64),
                                            forward_pre(src, dst, n, x, wl, wr, b, torch.float32)):
            continue
        return _case(src, dst, n, din, dout, act, p, seed, with_bias, x, wl, wr, bias, g, keep_mask(n, dout, p, seed))
    raise AssertionError("no seed with a ReLU margin")


def hub_nodes(n):
    return n // 3, 2 * (n // 3) + 1


@functools.lru_cache(maxsize=None)
def hub_graph(n, seed=0):
    """`sweep_graph(n)` plus two hub nodes (`hub_nodes`), each with HUB_EXTRA more in-edges from uniform sources and
    HUB_EXTRA more out-edges to distinct targets, stable-sorted by dst: a popular node is a long row of A (values 1 / its
    in-degree) and a long row of A^T (the unequal values 1 / deg(dst) of its targets).  The hubs' own rows list their
    sources in ascending order, which the windowed plan asks of a hub row (graph.HubPlan.build); A^T's rows do by
    construction."""
    src, dst = sweep_graph(n, seed)
    rng = np.random.default_rng([n, seed, HUB_EXTRA])
    assert n > HUB_EXTRA
    for hub in hub_nodes(n):
        src = np.concatenate([src, rng.integers(0, n, HUB_EXTRA), np.full(HUB_EXTRA, hub)]).astype(np.int64)
        dst = np.concatenate([dst, np.full(HUB_EXTRA, hub), rng.choice(n, HUB_EXTRA, replace=False)]).astype(np.int64)
    order = np.argsort(dst, kind="stable")
    src, dst = src[order], dst[order]
    for hub in hub_nodes(n):
        lo, hi = np.searchsorted(dst, [hub, hub + 1])
        src[lo:hi] = np.sort(src[lo:hi])
    return src, dst


def zeroed_share(n, din, dout, seed=0, graph=sweep_graph):
    """(share of g that `large_case` zeroes for relu, the ambiguous mask), from the restatement alone."""
    src, dst = graph(n)
    x, wl, wr, bias, _ = inputs(n, din, dout, seed)
    pre64 = forward_pre(src, dst, n, x, wl, wr, bias, torch.float64)
    pre32 = forward_pre(src, dst, n, x, wl, wr, bias, torch.float32)
    ambiguous = np.abs(pre64) < 8.0 * np.abs(pre32 - pre64).max()
    return float(ambiguous.mean()), ambiguous


@functools.lru_cache(maxsize=None)
def large_case(n, din, dout, act, p, graph=sweep_graph):
    """A case too large for a margin scan (module docstring): for relu, g is zeroed where the mask is ambiguous.  graph:
    `sweep_graph` or `hub_graph`."""
    src, dst = graph(n)
    x, wl, wr, bias, g = inputs(n, din, dout, 0)
    share = 0.0
    if act == "relu":
        share, ambiguous = zeroed_share(n, din, dout, graph=graph)
        assert share <= MAX_ZEROED_SHARE, f"n={n} ({din}, {dout}): {share:.3g} of g would be zeroed"
        g[ambiguous] = 0.0
    case = _case(src, dst, n, din, dout, act, p, 0, True, x, wl, wr, bias, g, keep_mask(n, dout, p, 0))
    case["share"] = share
    return case


def out_isolated(src, n):
    """The nodes without an out-edge: empty rows of A^T, whose dx is q alone."""
    return np.flatnonzero(np.bincount(src, minlength=n) == 0)


@functools.lru_cache(maxsize=None)
def exact_case(din, dout, act, with_bias):
    """A case in which float32 is exact, so that the kernels owe float64's every bit: x in -2 .. 2, weights in {-1, 0, 1},
    bias in -2 .. 2, g in {-2, -1, 1, 2} (never zero), in-degrees from EXACT_DEGREES (1 / deg a power of two), keep masks
    with p = 0.5 (with a bias; scale 2) or 0.75 (without; scale 4).  Every z is a multiple of 1/8 below 2 in size, every
    pre-activation a multiple of 1/8 below 2 * 2 * 128 + 2, every gradient a multiple of 1/8 far below 2^21: each product
    and each partial sum, in any order, is a float32.  Column `zero_col` of the pre-activations is exactly 0 (zero rows of
    wl and wr, zero bias entry) and, without a bias, so is row `zero_row` (a node without in-edges whose x row is zero),
    both under non-zero g: torch's ReLU gives such an element gradient 0.  Also carries `f32`, the float32 restatement."""
    assert act in ("none", "relu")
    n = EXACT_N
    rng = np.random.default_rng([n, din, dout, ACTS.index(act), int(with_bias)])
    deg = np.array([EXACT_DEGREES[r % len(EXACT_DEGREES)] for r in range(n)])
    dst = np.repeat(np.arange(n, dtype=np.int64), deg)
    src = rng.integers(0, n, dst.size).astype(np.int64)
    x = rng.integers(-2, 3, (n, din)).astype(np.float32)
    wl, wr = (rng.integers(-1, 2, (dout, din)).astype(np.float32) for _ in range(2))
    bias = rng.integers(-2, 3, dout).astype(np.float32)
    g = rng.choice(np.float32([-2, -1, 1, 2]), (n, dout))
    zero_col, zero_row = dout // 2 + 1, 35                     # 35 % 5 == 0: no in-edge; in the second 32-row tile
    wl[zero_col], wr[zero_col], bias[zero_col] = 0.0, 0.0, 0.0
    if not with_bias:
        assert deg[zero_row] == 0
        x[zero_row] = 0.0
    p = 0.5 if with_bias else 0.75
    keep = keep_mask(n, dout, p, 0)
    case = _case(src, dst, n, din, dout, act, p, 0, with_bias, x, wl, wr, bias, g, keep)
    case["f32"], _ = restatement(src, dst, n, x, wl, wr, case["bias"], g, act, torch.float32, keep, p)
    _, case["pre"] = restatement(src, dst, n, x, wl, wr, case["bias"], g, act, torch.float64, keep, p)
    case["zero_col"], case["zero_row"] = zero_col, zero_row if not with_bias else None
    return case


def assert_exact(got, ref, tag):
    """Every element equal; the first differing index otherwise."""
    for k, want in ref.items():
        have = np.asarray(got[k], dtype=np.float64)
        assert have.shape == want.shape, (tag, k, have.shape, want.shape)
        if not np.array_equal(have, want):
            at = tuple(int(v) for v in np.argwhere(have != want)[0])
            raise AssertionError(f"SAGE exact {tag} {k}: {int((have != want).sum())} of {want.size} elements differ, the first "
                                 f"at {at}: got {have[at]!r}, float64 {want[at]!r}")


TAIL_SCALE = 8.0


@functools.lru_cache(maxsize=None)
def tail_case(n, din, dout, p=0.5):
    """gelu far from zero: `inputs` with x scaled by TAIL_SCALE, which puts pre-activations past +-10, where erf has
    saturated in float32 and exp(-pre^2 / 2) is below 2e-22.  Carries `pre`, the float64 pre-activations."""
    src, dst = sweep_graph(n)
    x, wl, wr, bias, g = inputs(n, din, dout, 0)
    x *= np.float32(TAIL_SCALE)
    case = _case(src, dst, n, din, dout, "gelu", p, 0, True, x, wl, wr, bias, g, keep_mask(n, dout, p, 0))
    case["pre"] = forward_pre(src, dst, n, x, wl, wr, bias, torch.float64)
    return case


def checksum(*arrays):
    return float(sum(np.abs(np.asarray(a, dtype=np.float64)).sum() for a in arrays if a is not None))


# ---- the device side ----

def device_graph(src, dst, n, device="cuda"):
    from recommendation_amd import functional as Fn
    return Fn.sage_mean_graph(torch.from_numpy(np.stack([src, dst])), n, device)


def packed(keep, device="cuda"):
    from recommendation_amd import functional as Fn
    return None if keep is None else Fn.pack_bits(torch.from_numpy(keep.reshape(-1))).to(device)


def is_fused(h):
    return h.grad_fn is not None and type(h.grad_fn).__name__.startswith("_SageLayer")


def no_fused_node_below(h):
    """Walks the autograd graph under h: the fused node is nowhere in it."""
    todo, seen = [h.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is not None and f not in seen:
            seen.add(f)
            if type(f).__name__.startswith("_SageLayer"):
                return False
            todo += [nf for nf, _ in f.next_functions]
    return h.grad_fn is not None


def layer(graph, case, device="cuda", fused=True, fn=None, dtype=torch.float32, want_dx=True, act=None, frozen=()):
    """h, dx, dwl, dwr (and dbias) of functional.sage_layer (or `fn`) for a case, as arrays; with `fused` the node must be
    the fused one, without it the node must be nowhere below h.  act: given instead of the case's (a callable with the
    same meaning); frozen: the parameters among wl, wr, bias without requires_grad."""
    from recommendation_amd import functional as Fn
    t = {k: torch.from_numpy(case[k]).to(device=device, dtype=dtype).requires_grad_((k != "x" or want_dx) and k not in frozen)
         for k in ("x", "wl", "wr")}
    bias = None if case["bias"] is None else \
        torch.from_numpy(case["bias"]).to(device=device, dtype=dtype).requires_grad_("bias" not in frozen)
    h = (fn or Fn.sage_layer)(graph, t["x"], t["wl"], t["wr"], bias, act or case["act"], packed(case["keep"], device), case["p"])
    if fused:
        assert is_fused(h), "the fused node must run"
    elif fn is None:
        assert no_fused_node_below(h), "the composed layer must run"
    h.backward(torch.from_numpy(case["g"]).to(device=device, dtype=dtype))
    if frozen:
        res = dict(h=h.detach(), dx=t["x"].grad, dwl=t["wl"].grad, dwr=t["wr"].grad, dbias=None if bias is None else bias.grad)
        return {k: v.cpu().numpy() for k, v in res.items() if v is not None}
    res = dict(h=h.detach(), dwl=t["wl"].grad, dwr=t["wr"].grad)
    if want_dx:
        res["dx"] = t["x"].grad
    if bias is not None:
        res["dbias"] = bias.grad
    return {k: v.cpu().numpy() for k, v in res.items()}


class Raw:
    """The arguments of gcr_sage_fwd_f32 / gcr_sage_bwd_f32 for n rows of (din, dout), every buffer its own, the workspace
    of the size gcr_sage_workspace_bytes gives for (n, din, dout).  fill (the bounds tests): every output and the workspace
    hold that value, h, pre, p, q over pad_rows more rows and the workspace over pad_words more words than the call is told
    of; the kernels get the same pointers and the same n."""

    def __init__(self, n=40, din=64, dout=64, act=1, fill=None, pad_rows=0, pad_words=0):
        from recommendation_amd import _lib
        self.lib, self.n, self.din, self.dout, self.act = _lib, n, din, dout, act
        f = functools.partial(torch.randn, device="cuda")
        self.x, self.z, self.g = f(n, din), f(n, din), f(n, dout)
        self.wl, self.wr, self.bias = f(dout, din), f(dout, din), f(dout)
        out = functools.partial(torch.full, fill_value=0.0 if fill is None else fill, device="cuda")
        self.h, self.pre = out((n + pad_rows, dout)), out((n + pad_rows, dout))
        self.p, self.q = out((n + pad_rows, din)), out((n + pad_rows, din))
        grad = functools.partial(torch.full, fill_value=1.0 if fill is None else fill, device="cuda")
        self.dwl, self.dwr, self.dbias = grad((dout, din)), grad((dout, din)), grad((dout,))
        self.ws_words = int(_lib.call("gcr_sage_workspace_bytes", max(n, 1), din, dout)) // 4
        self.ws = torch.empty(max(self.ws_words, 1) + pad_words, device="cuda")
        if fill is not None:
            self.ws.fill_(fill)

    def fwd(self, **kw):
        a = dict(n=self.n, x=self.x, z=self.z, wl=self.wl, wr=self.wr, bias=self.bias, din=self.din, dout=self.dout, act=self.act,
                 keep=None, scale=1.0, h=self.h, pre=self.pre if self.act == 2 else None, ws=self.ws)
        a.update(kw)
        self.lib.call("gcr_sage_fwd_f32", a["n"], a["x"], a["z"], a["wl"], a["wr"], a["bias"], a["din"], a["dout"], a["act"],
                      a["keep"], a["scale"], a["h"], a["pre"], a["ws"], on=self.g)

    def bwd(self, **kw):
        a = dict(n=self.n, x=self.x, z=self.z, wl=self.wl, wr=self.wr, h=self.h, pre=self.pre if self.act == 2 else None, g=self.g,
                 din=self.din, dout=self.dout, act=self.act, keep=None, scale=1.0, p=self.p, q=self.q, dwl=self.dwl, dwr=self.dwr,
                 dbias=self.dbias, ws=self.ws)
        a.update(kw)
        self.lib.call("gcr_sage_bwd_f32", a["n"], a["x"], a["z"], a["wl"], a["wr"], a["h"], a["pre"], a["g"], a["din"], a["dout"],
                      a["act"], a["keep"], a["scale"], a["p"], a["q"], a["dwl"], a["dwr"], a["dbias"], a["ws"], on=self.g)


# ---- the fixture's layout ----

def load():
    return np.load(GOLDEN, allow_pickle=False)


def comp_prefix(din, dout, act):
    return f"comp/{din}x{dout}/{act}/"


def component(g, din, dout, act):
    """One layer case of the fixture as `margin_case`'s dict: the inputs redrawn from the stored seed (and checked against
    the writer's checksum), ref = the reference stand-in's float64 run (stored as float32 of it) and the float32 run's
    drift."""
    pre = comp_prefix(din, dout, act)
    src, dst = g["comp/src"].astype(np.int64), g["comp/dst"].astype(np.int64)
    seed = int(g[pre + "seed"])
    x, wl, wr, bias, gr = inputs(COMP_N, din, dout, seed)
    keep = keep_mask(COMP_N, dout, COMP_P, seed)
    assert abs(checksum(x, wl, wr, bias, gr, keep) - float(g[pre + "checksum"])) < 1e-6, "the inputs' streams changed"
    return dict(src=src, dst=dst, n=COMP_N, din=din, dout=dout, act=act, p=COMP_P, seed=seed, x=x, wl=wl, wr=wr, bias=bias,
                g=gr, keep=keep, ref={k: g[pre + k].astype(np.float64) for k in KEYS},
                drift={k: float(g[pre + "drift/" + k]) for k in KEYS})


# ---- training steps: step_pins' rules on the fixture's step cases ----

def step_config(g, case):
    pre = f"{case}/"
    cfg = {k: int(g[pre + k]) for k in ("hidden_channels", "n_layers")}
    cfg.update({k: float(g[pre + k]) for k in ("dropout", "lr", "weight_decay")})
    cfg.update({k: str(g[pre + k]) for k in ("activation", "optimizer", "loss_type")})
    return cfg


def n_convs(cfg):
    return max(int(cfg["n_layers"]), 2)             # graphsage.py:22: n_layers 1 and 2 build the same two layers


def params_of(cfg):
    return tuple(f"layers.{k}.{name}" for k in range(n_convs(cfg)) for name in ("lin_l.weight", "lin_l.bias", "lin_r.weight"))


def param_shapes(cfg):
    hid, out = int(cfg["hidden_channels"]), {}
    widths = [IN_CHANNELS] + [hid] * (n_convs(cfg) - 1) + [OUT_CHANNELS]
    for k in range(n_convs(cfg)):
        out[f"layers.{k}.lin_l.weight"] = (widths[k + 1], widths[k])
        out[f"layers.{k}.lin_l.bias"] = (widths[k + 1],)
        out[f"layers.{k}.lin_r.weight"] = (widths[k + 1], widths[k])
    return out


def init_arrays(cfg, n_nodes, seed):
    """The step cases' node features x ~ N(0, 1) [n, 64] (graphsage.py:46) and initial parameters, float32, functions of
    the seed (numpy's PCG64): torch.nn.Linear's default bounds, uniform(+-1 / sqrt(in)) for weights (kaiming-uniform with
    a = sqrt(5)) and biases alike.  The reference's own draws are overwritten with these."""
    rng = np.random.default_rng([int(seed), n_nodes])
    out = {"x": rng.standard_normal((n_nodes, IN_CHANNELS)).astype(np.float32)}
    for k, shape in param_shapes(cfg).items():
        b = 1.0 / np.sqrt(shape[-1] if len(shape) == 2 else param_shapes(cfg)[k.replace("bias", "weight")][1])
        out[k] = rng.uniform(-b, b, shape).astype(np.float32)
    return out


def step_init(g, case):
    init = init_arrays(step_config(g, case), int(g["num_users"]) + int(g["num_items"]), int(g[f"{case}/init_seed"]))
    assert abs(checksum(*init.values()) - float(g[f"{case}/init_checksum"])) < 1e-6, "the initial parameters' stream changed"
    return init


def step_masks(g, case, step, cfg):
    """The recorded keep masks of one step, bool arrays [n, hidden] per hidden layer, or None for a case without dropout."""
    if f"{case}/keep0" not in g.files:
        return None
    n, hid = int(g["num_users"]) + int(g["num_items"]), int(cfg["hidden_channels"])
    return [np.unpackbits(g[f"{case}/keep{k}"][step], count=n * hid).reshape(n, hid).astype(bool) for k in range(n_convs(cfg) - 1)]


def step_tables(g, case):
    """{parameter: (float64 final, slack, atol, what dropping the root term moves it by)} of a step case."""
    init, pre = step_init(g, case), f"{case}/"
    out = {}
    for k in params_of(step_config(g, case)):
        slack = float(g[f"{pre}slack/{k}"])
        out[k] = (init[k].astype(np.float64) + g[f"{pre}f64/delta/{k}"].astype(np.float64), slack, sp.atol_floor_1(slack),
                  float(g[f"{pre}delta_root/{k}"]))
    return init, out


def assert_sensitivity(g, case):
    """The fixture's side of step_pins' rule, from stored numbers alone: the float64 run without the root term
    (x wr^T dropped in every layer) ends more than DROPPED x atol away in every parameter, and every parameter moved by
    more than MOVED x max(slack, FLOOR)."""
    init, tables = step_tables(g, case)
    for k, (ref, slack, atol, d_root) in tables.items():
        assert sp.sees_dropped(d_root, atol), (case, k, d_root, atol)
        moved = float(np.abs(ref - init[k]).max())
        assert sp.has_moved(moved, max(slack, sp.FLOOR)), (case, k, moved, slack)


def check_steps(g, case, losses, grad0, finals):
    """losses [steps]; grad0, finals: {parameter: array}.  Loss: `term_tol` with the float32 run; a step-0 gradient: the
    layer rule (`check`) with the stored drift; a final parameter: `atol_floor_1` of the stored float32 slack; and the
    tolerance sees the training (`assert_sensitivity`, and `has_moved` of the model's own finals)."""
    pre = f"{case}/"
    l64, l32 = g[pre + "f64/loss"], g[pre + "f32/loss"]
    tol = sp.term_tol(l64, l32)
    err = np.abs(np.asarray(losses, dtype=np.float64) - l64)
    report = [f"STEPPIN sage case {case}", f"  loss: max err {err.max():.3g} ({(err / tol).max():.2f} x tol)"]
    failures = [] if np.all(err <= tol) else [f"loss: got {list(losses)} reference {l64.tolist()}"]
    assert_sensitivity(g, case)
    init, tables = step_tables(g, case)
    for k, (ref, slack, atol, d_root) in tables.items():
        got = np.asarray(finals[k], dtype=np.float64)
        e = float(np.abs(got - ref).max())
        moved = float(np.abs(got - init[k]).max())
        report.append(f"  {k}: max err {e:.3g} ({e / atol:.2f} x atol), atol {atol:.3g}, reference f32 slack {slack:.3g}, "
                      f"moved {moved:.3g}; dropping the root term moves it by {d_root:.3g}")
        if not (np.isfinite(got).all() and e <= atol):
            failures.append(f"{k}: max |final - f64| = {e:.3g} > atol {atol:.3g}")
        if not sp.has_moved(moved, max(slack, sp.FLOOR)):
            failures.append(f"{k}: moved {moved:.3g}, which the tolerance does not see")
    print("\n".join(report))
    assert not failures, "\n".join(report + failures)
    check(grad0, {k: g[f"{pre}f64/grad0/{k}"].astype(np.float64) for k in tables},
          {k: float(g[f"{pre}drift/{k}"]) for k in tables}, f"case {case} step-0 gradient")
