"""What the GAT tests and the writer of tests/golden/gat_steps.npz (scripts/gen_golden_gat_steps.py) share: the comparison
rule, GAT's constants, the float64 restatement of the aggregation, the case builders and the fixture's key layout.

The rule, the project's (tests/diffuse_rules.py):  err / S <= max(4 x drift, 2^-20)  and  err / S <= 1e-5,  S = max |f64|,
drift = the float32 error of the SAME float64 source.  Training steps are held to tests/step_pins.py's rules (`check_steps`:
`term_tol` with the float32 run for the loss, `atol_floor_1` for a final parameter, `has_moved` for what the tolerance
sees).

The aggregation, torch_geometric's GATConv with the defaults gat.py leaves in place, for terms = the graph's entries (edge
j -> i; no diagonal) followed by one self loop per node:
    z = a_src[j] + a_dst[i];  e = leaky_relu(z);  alpha = exp(e - max_i) / (sum_i + 1e-16) per target and head;
    alpha~ = alpha * keep / (1 - p);  out_i = sum_j alpha~_ij h_j + bias.
`restatement` runs these in a given dtype under autograd.  LeakyReLU has a kink at zero, so a case is drawn until every
float64 z keeps 8 x its float32 error from zero (`margin_case`): a gradient pin must not compare two different slopes.

Two graph builders: `sweep_graph` (the DEGREES cycle, uniform sources, one optional long row 0) and `shaped_graph`
(prescribed row and column lengths, for the paths a uniform draw never reaches: tests/test_gat_paths_gpu.py).

A component case's inputs are functions of a seed (`inputs`, `keep_mask`: numpy's PCG64 streams); the fixture stores the
seed and a checksum of what the writer drew, and `component` re-checks it."""
import functools
import os

import numpy as np
import torch

import step_pins as sp

FLOOR, NORTH_STAR = 2.0 ** -20, 1e-5
KEYS = ("out", "dh", "da_src", "da_dst")
# every (heads, c) the kernels serve: c in {32, 64, 128}, heads in {1, 2, 4}, heads * c <= 256
PAIRS = tuple((h, c) for h in (1, 2, 4) for c in (32, 64, 128) if h * c <= 256)
# a row's entry count against the kernel's 8-deep gather (the self loop makes it one term more): a tail alone, blocks with
# and without a tail
DEGREES = (0, 1, 7, 8, 9, 15, 16, 17, 24, 41)
LONG_ROW = 512                      # csrc/gcr_gat.hip: a row with more entries is walked by a whole workgroup
SLOPE = 0.2
# `shaped_graph`'s dictionaries of tests/test_gat_paths_gpu.py (n, rows, hubs), which tests/test_gat_cpu.py holds to the
# builder's guarantees: second 64-term batches of a one-wave row (64, 65, 128, 129 terms with the self loop), both sides
# of LONG_ROW in the CSR and in the transpose, long rows whose waves get no term (513, 600), one batch each (1023) and
# one wave a second batch (1024); n = 1200 gives the long launch two workgroups, each with two or more long rows
PATHS = (1200, {2: 63, 3: 64, 4: 65, 6: 127, 8: 128, 9: 200, 12: 511, 13: 512, 0: 513, 7: 1023, 700: 1024, 701: 600, 1199: 1100},
         {20: 513, 21: 512, 640: 1100, 1198: 600})
FAR = (257, {0: 513, 5: 600}, {9: 513})                        # embedded behind 2^20 isolated nodes
MIRRORED = (300, {0: 513}, {})                                 # symmetrised: node 0 is long as a row and as a column
COMP_N, COMP_PE = 8, (0.0, 0.5)    # the fixture's component cases
CONV_PAIR, CONV_IN, CONV_N, CONV_PE = (2, 64), 64, 12, 0.5
STEP_CASES = ("A", "B", "C")
PARAMS = ("user_embedding.weight", "item_embedding.weight", "gat1.lin.weight", "gat1.att_src", "gat1.att_dst", "gat1.bias",
          "gat2.lin.weight", "gat2.att_src", "gat2.att_dst", "gat2.bias")
GOLDEN = os.path.join(sp.GOLDEN, "gat_steps.npz")


def check(got, ref, drift, tag):
    """drift: relative to the scale, per key."""
    lines, bad = [], []
    for k, want in ref.items():
        scale = float(np.abs(want).max()) or 1.0               # an all-zero reference (one isolated node): absolute
        err = float(np.abs(np.asarray(got[k], dtype=np.float64) - want).max()) / scale
        bound = max(4.0 * drift[k], FLOOR)
        lines.append(f"GAT {tag} {k}: err/S {err:.3g} bound {bound:.3g} (drift {drift[k]:.3g}, S {scale:.3g})")
        if not (np.isfinite(got[k]).all() and err <= bound and err <= NORTH_STAR):
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


def drift_of(f32, ref):
    return {k: float(np.abs(f32[k] - ref[k]).max()) / (float(np.abs(ref[k]).max()) or 1.0) for k in ref}


def terms_of(dst, src, n):
    """(src, dst) of the aggregation's terms: the entries, then one self loop per node."""
    loops = np.arange(n, dtype=np.int64)
    return np.concatenate([src, loops]), np.concatenate([dst, loops])


def restatement(dst, src, n, h, a_src, a_dst, g, heads, dtype, slope=SLOPE, keep=None, p=0.0, bias=None):
    """(dict of out, dh, da_src, da_dst and, with a bias, dbias; z), float64 arrays computed in `dtype`.  dst / src int64
    [nnz] without diagonal entries; keep: bool [nnz + n, heads] or None."""
    s, d = (torch.from_numpy(t) for t in terms_of(dst, src, n))
    ht, at, bt = (torch.from_numpy(t).to(dtype).requires_grad_(True) for t in (h, a_src, a_dst))
    bias_t = None if bias is None else torch.from_numpy(bias).to(dtype).requires_grad_(True)
    z = at[s] + bt[d]
    e = torch.where(z > 0, z, slope * z)
    top = torch.full((n, heads), -np.inf, dtype=dtype).scatter_reduce(0, d[:, None].expand(-1, heads), e.detach(), "amax")
    w = torch.exp(e - top[d])
    alpha = w / (torch.zeros(n, heads, dtype=dtype).index_add_(0, d, w) + 1e-16)[d]
    if keep is not None:
        alpha = alpha * torch.from_numpy(keep).to(dtype) / (1.0 - p)
    c = h.shape[1] // heads
    out = torch.zeros(n, heads, c, dtype=dtype).index_add_(0, d, alpha[:, :, None] * ht.view(n, heads, c)[s]).reshape(n, -1)
    if bias_t is not None:
        out = out + bias_t
    out.backward(torch.from_numpy(g).to(dtype))
    res = dict(out=out.detach(), dh=ht.grad, da_src=at.grad, da_dst=bt.grad)
    if bias_t is not None:
        res["dbias"] = bias_t.grad
    return {k: v.double().numpy() for k, v in res.items()}, z.detach().double().numpy()


def has_margin(z64, z32):
    """Every float64 z keeps 8 x the float32 error from LeakyReLU's kink.  A z that is exactly 0 in both runs is exempt: it
    is 0 + 0 of a node whose every input was dropped (step case C has one), exact in any arithmetic, and every
    implementation takes the same side of `z > 0` there."""
    live = ~((z64 == 0.0) & (z32 == 0.0))
    return bool(not live.any() or np.abs(z64[live]).min() >= 8.0 * np.abs(z32 - z64).max())


def inputs(n, heads, c, seed, big_dst=False):
    """h ~ 0.3 N(0, 1) [n, heads * c], a_src, a_dst ~ N(0, 1) [n, heads], g ~ N(0, 1), bias ~ 0.1 N(0, 1), float32.
    big_dst: a_dst[::3] += 100, which a softmax without the max shift turns into inf / inf."""
    rng = np.random.default_rng([n, heads, c, seed])
    h = (0.3 * rng.standard_normal((n, heads * c))).astype(np.float32)
    a_src, a_dst = (rng.standard_normal((n, heads)).astype(np.float32) for _ in range(2))
    g = rng.standard_normal((n, heads * c)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(heads * c)).astype(np.float32)
    if big_dst:
        a_dst[::3] += 100.0
    return h, a_src, a_dst, g, bias


def keep_mask(nterm, heads, p, seed):
    """bool [nterm, heads], `rand >= p` as F.dropout keeps; None at p = 0."""
    return None if p == 0.0 else np.random.default_rng([nterm, heads, seed]).random((nterm, heads)) >= p


def sweep_graph(n, seed=0, long_row=0):
    """(dst, src) int64, dst ascending: row r has DEGREES[r % 10] entries, row 1 none, row 0 `long_row` when given; no
    diagonal entry; every row of two or more entries has a repeated column."""
    rng = np.random.default_rng([n, seed, long_row])
    deg = np.array([DEGREES[r % len(DEGREES)] for r in range(n)])
    if long_row:
        deg[0] = long_row
    if n > 1:
        deg[1] = 0
    else:
        deg[:] = 0
    dst = np.repeat(np.arange(n, dtype=np.int64), deg)
    src = rng.integers(0, max(n - 1, 1), dst.size).astype(np.int64)
    src += src >= dst                                           # skips the diagonal
    start = np.concatenate([[0], np.cumsum(deg)])
    for r in np.flatnonzero(deg >= 2):
        src[start[r] + 1] = src[start[r]]
    return dst, src


def shaped_graph(n, rows, hubs, seed=0):
    """(dst, src) int64, dst ascending, no diagonal entry, with prescribed row AND column lengths: row r has exactly
    rows[r] entries (the other rows follow `sweep_graph`'s DEGREES cycle, row 1 empty), source s appears exactly hubs[s]
    times, no other source more than LONG_ROW times, and every row of two or more entries has a repeated column (its
    first two entries).  A hub takes the place of one entry per row, round by round over the rows that still have an
    entry to give (never a row's first two, never its own row), so a hub longer than the graph has rows gets several
    entries in the longest rows; nothing is appended, so no row length changes."""
    rng = np.random.default_rng([n, seed, len(rows), len(hubs)])
    deg = np.array([DEGREES[r % len(DEGREES)] for r in range(n)])
    if n > 1:
        deg[1] = 0
    for r, k in rows.items():
        deg[r] = k
    dst = np.repeat(np.arange(n, dtype=np.int64), deg)
    start = np.concatenate([[0], np.cumsum(deg)])
    # the plain sources: non-hub nodes, uniformly, without the row's own
    pool = np.array([s for s in range(n) if s not in hubs], dtype=np.int64)
    where = np.full(n, -1, dtype=np.int64)
    where[pool] = np.arange(pool.size)
    own = where[dst]
    k = (rng.random(dst.size) * (pool.size - (own >= 0))).astype(np.int64)
    src = pool[k + ((own >= 0) & (k >= own))]
    for r in np.flatnonzero(deg >= 2):
        src[start[r] + 1] = src[start[r]]
    free = np.where(deg == 1, 0, 2)                             # the next entry a row can give to a hub
    for s in sorted(hubs):
        left = hubs[s]
        while left:
            cand = np.flatnonzero((free < deg) & (np.arange(n) != s))
            assert cand.size, f"hub {s}: no row has an entry left for it"
            take = rng.permutation(cand)[:left]
            src[start[take] + free[take]] = s
            free[take] += 1
            left -= take.size
    count = np.bincount(src, minlength=n)
    assert (dst != src).all() and all(count[s] == hubs[s] for s in hubs)
    assert count[pool].max(initial=0) <= LONG_ROW, "a plain source became a long row of the transpose"
    return dst, src


def margin_case(dst, src, n, heads, c, p, seed0=0, seeds=200, big_dst=False, with_bias=True, slope=SLOPE):
    """The first seed's inputs whose z keep the margin: dict of dst, src, n, heads, c, p, slope, h, a_src, a_dst, g, bias,
    keep, seed, ref (float64) and drift."""
    for seed in range(seed0, seed0 + seeds):
        h, a_src, a_dst, g, bias = inputs(n, heads, c, seed, big_dst)
        z64 = a_src.astype(np.float64)[terms_of(dst, src, n)[0]] + a_dst.astype(np.float64)[terms_of(dst, src, n)[1]]
        z32 = (a_src[terms_of(dst, src, n)[0]] + a_dst[terms_of(dst, src, n)[1]]).astype(np.float64)
        if not has_margin(z64, z32):
            continue
        keep = keep_mask(dst.size + n, heads, p, seed)
        kw = dict(keep=keep, p=p, bias=bias if with_bias else None, slope=slope)
        ref, _ = restatement(dst, src, n, h, a_src, a_dst, g, heads, torch.float64, **kw)
        f32, _ = restatement(dst, src, n, h, a_src, a_dst, g, heads, torch.float32, **kw)
        return dict(dst=dst, src=src, n=n, heads=heads, c=c, p=p, slope=slope, h=h, a_src=a_src, a_dst=a_dst, g=g,
                    bias=kw["bias"], keep=keep, seed=seed, ref=ref, drift=drift_of(f32, ref))
    raise AssertionError("no seed with a LeakyReLU margin")


@functools.lru_cache(maxsize=None)
def sweep_case(n, heads, c, p, long_row=0, big_dst=False):
    """A `margin_case` on `sweep_graph`, shared among the tests that need it and never written to."""
    dst, src = sweep_graph(n, long_row=long_row)
    return margin_case(dst, src, n, heads, c, p, big_dst=big_dst)


@functools.lru_cache(maxsize=None)
def _shaped_case(n, rows, hubs, heads, c, p, slope):
    dst, src = shaped_graph(n, dict(rows), dict(hubs))
    return margin_case(dst, src, n, heads, c, p, slope=slope)


def shaped_case(n, rows, hubs, heads, c, p, slope=SLOPE):
    """A `margin_case` on `shaped_graph(n, rows, hubs)` (dicts), shared among the tests that need it and never written to."""
    return _shaped_case(n, tuple(sorted(rows.items())), tuple(sorted(hubs.items())), heads, c, p, slope)


def checksum(*arrays):
    return float(sum(np.abs(np.asarray(a, dtype=np.float64)).sum() for a in arrays if a is not None))


# ---- the fixture's layout ----

def load():
    return np.load(GOLDEN, allow_pickle=False)


def comp_prefix(heads, c, pe):
    return f"comp/h{heads}c{c}/pe{int(round(pe * 100)):02d}/"


def component(g, heads, c, pe):
    """One component case of the fixture as `margin_case`'s dict: the inputs redrawn from the stored seed (and checked
    against the writer's checksum), ref = the reference stand-in's float64 run (stored as float32 of it, which puts at
    most 2^-24 S on a measured error) and the float32 run's drift."""
    pre = comp_prefix(heads, c, pe)
    dst, src = g["comp/dst"].astype(np.int64), g["comp/src"].astype(np.int64)
    seed = int(g[pre + "seed"])
    h, a_src, a_dst, gr, bias = inputs(COMP_N, heads, c, seed)
    keep = keep_mask(dst.size + COMP_N, heads, pe, seed)
    assert abs(checksum(h, a_src, a_dst, gr, bias, keep) - float(g[pre + "checksum"])) < 1e-6, "the inputs' streams changed"
    return dict(dst=dst, src=src, n=COMP_N, heads=heads, c=c, p=pe, h=h, a_src=a_src, a_dst=a_dst, g=gr, bias=bias, keep=keep,
                seed=seed, ref={k: g[pre + k].astype(np.float64) for k in KEYS + ("dbias",)},
                drift={k: float(g[pre + "drift/" + k]) for k in KEYS + ("dbias",)})


# ---- the device side ----

def device_graph(dst, src, n):
    """dst ascending, so the CSR's entry order is the arrays' order."""
    import recommendation_amd as ra
    assert (np.diff(dst) >= 0).all()
    return ra.CsrGraph.from_coo(dst, src, None, n, n, "cuda", hub_window_rows=0)


def packed(keep, device="cuda"):
    from recommendation_amd import functional as Fn
    return None if keep is None else Fn.pack_bits(torch.from_numpy(keep.reshape(-1))).to(device)


def aggregate(graph, case, device="cuda", fused=True, fn=None, slope=None):
    """out, dh, da_src, da_dst (and dbias) of functional.gat_aggregate (or `fn`) for a case, as arrays; with `fused` the
    node must be the fused one.  slope: None = the case's own, SLOPE where it names none."""
    from recommendation_amd import functional as Fn
    slope = case.get("slope", SLOPE) if slope is None else slope
    t = {k: torch.from_numpy(case[k]).to(device).requires_grad_(True) for k in ("h", "a_src", "a_dst")}
    bias = None if case["bias"] is None else torch.from_numpy(case["bias"]).to(device).requires_grad_(True)
    out = (fn or Fn.gat_aggregate)(graph, t["h"], t["a_src"], t["a_dst"], case["heads"], slope, packed(case["keep"], device),
                                   case["p"], bias)
    if fused:
        assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_GatAggregate"), "the fused node must run"
    out.backward(torch.from_numpy(case["g"]).to(device))
    res = dict(out=out.detach(), dh=t["h"].grad, da_src=t["a_src"].grad, da_dst=t["a_dst"].grad)
    if bias is not None:
        res["dbias"] = bias.grad
    return {k: v.cpu().numpy() for k, v in res.items()}


# ---- training steps: step_pins' rules on the fixture's step cases ----

def step_config(g, case):
    pre = f"{case}/"
    cfg = {k: int(g[pre + k]) for k in ("in_channels", "hidden_channels", "out_channels", "num_heads")}
    cfg.update({k: float(g[pre + k]) for k in ("dropout", "edge_dropout", "neg_slope", "lr", "weight_decay")})
    return cfg


def param_shapes(cfg, num_users, num_items):
    heads, hid, cin, out = (int(cfg[k]) for k in ("num_heads", "hidden_channels", "in_channels", "out_channels"))
    return {"user_embedding.weight": (num_users, cin), "item_embedding.weight": (num_items, cin),
            "gat1.lin.weight": (heads * hid, cin), "gat1.att_src": (1, heads, hid), "gat1.att_dst": (1, heads, hid),
            "gat1.bias": (heads * hid,), "gat2.lin.weight": (out, heads * hid), "gat2.att_src": (1, 1, out),
            "gat2.att_dst": (1, 1, out), "gat2.bias": (out,)}


def init_arrays(cfg, num_users, num_items, seed):
    """The step cases' initial parameters, float32, a function of the seed (numpy's PCG64): uniform(-a, a) with the
    xavier / glorot bound a = sqrt(6 / (size(-2) + size(-1))) of gat.py:28-29 and of PyG's GATConv, zero biases.  The
    reference's own draws are overwritten with these, as the LightGCN writer overwrites the tables."""
    rng = np.random.default_rng([int(seed), num_users, num_items])
    out = {}
    for k, shape in param_shapes(cfg, num_users, num_items).items():
        if k.endswith("bias"):
            out[k] = np.zeros(shape, dtype=np.float32)
        else:
            a = np.sqrt(6.0 / (shape[-2] + shape[-1]))
            out[k] = rng.uniform(-a, a, shape).astype(np.float32)
    return out


def step_init(g, case):
    init = init_arrays(step_config(g, case), int(g["num_users"]), int(g["num_items"]), int(g[f"{case}/init_seed"]))
    assert abs(checksum(*init.values()) - float(g[f"{case}/init_checksum"])) < 1e-6, "the initial parameters' stream changed"
    return init


def step_masks(g, case, step, graph, cfg, device="cuda"):
    """The recorded draws of one step of a case as GATRec.forward's `masks`, or None for a case without dropout.  The
    writer stores the attention keep masks in PyG's term order (the kept edges in edge_index order, then the self
    loops); `graph.coo_perm` brings them into the CSR's."""
    if f"{case}/feat0" not in g.files:
        return None
    from recommendation_amd import functional as Fn
    n = graph.n_rows
    heads, hid, cin = int(cfg["num_heads"]), int(cfg["hidden_channels"]), int(cfg["in_channels"])
    feat = [np.unpackbits(g[f"{case}/feat{k}"][step], count=n * w).reshape(n, w).astype(bool)
            for k, w in ((0, cin), (1, heads * hid))]
    perm = np.asarray(graph.coo_perm.cpu().numpy() if hasattr(graph.coo_perm, "cpu") else graph.coo_perm)
    order = np.concatenate([perm, graph.nnz + np.arange(n)])
    att = []
    for k, hh in ((0, heads), (1, 1)):
        keep = np.unpackbits(g[f"{case}/att{k}"][step], count=(graph.nnz + n) * hh).reshape(-1, hh).astype(bool)[order]
        att.append(Fn.pack_bits(torch.from_numpy(np.ascontiguousarray(keep).reshape(-1))).to(device))
    return {"feat": tuple(torch.from_numpy(f).to(device) for f in feat), "att": tuple(att)}


def check_steps(g, case, losses, grad0, finals):
    """losses [steps]; grad0, finals: {parameter: array}.  Loss: `term_tol` with the float32 run; a step-0 gradient: the
    component rule (`check`) with the stored drift; a final parameter: `atol_floor_1` of the stored float32 slack; and the
    tolerance sees the training: every parameter moved by more than MOVED x max(slack, FLOOR) (`has_moved`)."""
    pre = f"{case}/"
    l64, l32 = g[pre + "f64/loss"], g[pre + "f32/loss"]
    tol = sp.term_tol(l64, l32)
    err = np.abs(np.asarray(losses, dtype=np.float64) - l64)
    report = [f"STEPPIN gat case {case}", f"  loss: max err {err.max():.3g} ({(err / tol).max():.2f} x tol)"]
    failures = [] if np.all(err <= tol) else [f"loss: got {list(losses)} reference {l64.tolist()}"]
    init = step_init(g, case)
    for k in PARAMS:
        ref = init[k].astype(np.float64) + g[f"{pre}f64/delta/{k}"].astype(np.float64)
        slack = float(g[f"{pre}slack/{k}"])
        atol = sp.atol_floor_1(slack)
        got = np.asarray(finals[k], dtype=np.float64)
        e = float(np.abs(got - ref).max())
        moved = float(np.abs(got - init[k]).max())
        report.append(f"  {k}: max err {e:.3g} ({e / atol:.2f} x atol), atol {atol:.3g}, reference f32 slack {slack:.3g}, moved {moved:.3g}")
        if not (np.isfinite(got).all() and e <= atol):
            failures.append(f"{k}: max |final - f64| = {e:.3g} > atol {atol:.3g}")
        if not sp.has_moved(moved, max(slack, sp.FLOOR)):
            failures.append(f"{k}: moved {moved:.3g}, which the tolerance does not see")
    print("\n".join(report))
    assert not failures, "\n".join(report + failures)
    check(grad0, {k: g[f"{pre}f64/grad0/{k}"].astype(np.float64) for k in PARAMS},
          {k: float(g[f"{pre}drift/{k}"]) for k in PARAMS}, f"case {case} step-0 gradient")
