"""Every backward path of the fused BPR loss (csrc/gcr_bpr.hip behind `functional.bpr_sums` / `functional.bpr_edge_sums`)
against a float64 restatement, across widths, batch edges, grid-stride trips, id patterns and score regimes.

Reference: `_restated`, the formulas of include/gcr.h in torch on the CPU — gather the rows, x = <u, p> - mean_k <u, n_k>,
the variant's loss, the four sums, autograd of (sums[:4] * w).sum().  Samples with any id out of range are removed before the
restatement and counted against sums[4].  It runs in float64 (the reference) and in float32 (the drift); the drift is computed
on the CPU at test time, never from the code under test (the arrangement of tests/test_buir_gpu.py).

Bound rule (tests/f64_pins.py's, restated here because f64_pins.FAMILIES is fixed):

    err / S <= max(4 x drift, 2^-20),  and  err / S <= 1e-5  unless 4 x drift > 1e-5 (ill-conditioned: drift bound only)

S = max |f64| for the two gradients, the f64 value for the three squared-norm sums, sum_b max(1, |l_b|) for the loss sum (the
log's argument is O(1) per sample).  A reference that is all zero asks for exactly zero.  Every figure is printed as a
`BPRPIN tag:key err= bound= ratio=` line before anything is asserted.

Paths (monkeypatch on `functional`): atomic (bpr_bwd_kernel), sorted_payload (bpr_bwd_sorted_kernel sides 0 and 1 +
bpr_neg_block_kernel + gcr_sort_pairs_u64 + bpr_neg_items_sorted_kernel), sorted_index (bpr_bwd_sorted_kernel sides 0, 1, 2),
edge_payload / edge_index (`bpr_edge_sums` on a raw bipartite CsrGraph whose user-major edges are the batch:
gcr_bpr_edge_values_f32 + two SpMMs, the negatives' item rows by either sort).

Case tables (module-level: tests/test_launch_geometry_cpu.py asserts on the host that each shape lies where it says):

  WIDTHS       B = 130; both forward templates (d % 4 == 0 or not) and NV = 1 .. 4 of the four templated backward kernels, with
               (variant, n_neg) rotating so that each NV meets ONE_NEG true and false.  70 and 250 stand for the scalar forward
               at NV = 2 and NV = 4.
  BATCH_EDGES  batches one below, at and one above a gather group (8 / 4 in bpr_bwd_sorted_kernel, 16 / 8 in
               bpr_neg_items_sorted_kernel) and the 64-entry chunk of a wave.
  TRIPS        the second grid-stride trip of bpr_bwd_kernel (B > 8192 x 4) and of bpr_fwd_kernel (B > 4096 x 16): dloss_dx of
               the second trip is checked through the gradients, not only the loss.  The 65 536-block caps of the sorted, the
               neg-block and the edge-values kernels need more than 16 M entries (65 536 x 4 waves x 64 entries; 65 536 x 256
               slots) and are not reached here.
  PATTERNS     B = 257: one user everywhere, all ids distinct, a run of equal keys across the 64-entry chunk boundary, x = 0,
               a twin negative, bad ids in every index vector at the first / last sample and at lane 63 of chunk 0, every
               sample bad; each once with the default weights and once with the regulariser only (w = [0, 1, 2, 3]), where the
               run length `run_n` and the `c_self` index show at full scale instead of under the loss gradient.
  REGIMES      B = 257, loss only (w = [1/B, 0, 0, 0]: with the regulariser in, its gradient hides the loss gradient), scores
               shifted to x ~ shift: converged (+8, +12, +20), anti-converged (-12, -30, -80).  Left out: variants 0 and 2 at
               +20 — the reference's own float32 gradient is 100 % off there (4 x drift = 4.0), which pins nothing; variant 2
               at -80 and beyond — sigmoid underflows and the float32 reference is not finite.  Variants 0 and 2 at +8 and +12
               are ill-conditioned in the reference's own float32 (4 x drift ~ 1.8e-4 and ~ 6e-3): drift bound only.  Every kept
               case's reference bound is asserted <= 1e-2 before the GPU is touched."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, NORTH_STAR = 2.0 ** -20, 1e-5
KEYS = ("loss", "su", "sp", "sn", "gu", "gi")
SUMS_PATHS = ("atomic", "sorted_payload", "sorted_index")
EDGE_PATHS = ("edge_payload", "edge_index")
N_USERS, N_ITEMS, SCALE = 50, 41, 0.3
ROTATION = ((0, 1), (1, 2), (2, 3))                       # (variant, n_neg)

WIDTH_BATCH = 130
WIDTHS = (1, 3, 4, 50, 64, 68, 100, 128, 130, 160, 192, 196, 256, 70, 250)
EDGE_WIDTHS = (64, 160)
# (d, batch, unit, k, off): batch = k * unit + off, unit a gather group or the chunk of the kernels that d selects
BATCH_EDGES_64 = ((1, 8, 0, 1), (7, 8, 1, -1), (8, 8, 1, 0), (9, 8, 1, 1), (15, 16, 1, -1), (16, 16, 1, 0), (17, 16, 1, 1),
                  (63, 64, 1, -1), (64, 64, 1, 0), (65, 64, 1, 1), (127, 64, 2, -1), (128, 64, 2, 0), (129, 64, 2, 1),
                  (257, 64, 4, 1))
BATCH_EDGES_100 = ((3, 4, 1, -1), (4, 4, 1, 0), (5, 4, 1, 1), (65, 64, 1, 1))
BATCH_EDGES = tuple((64, b, n_neg, unit, k, off) for b, unit, k, off in BATCH_EDGES_64 for n_neg in (1, 3)) + \
    tuple((100, b, 2, unit, k, off) for b, unit, k, off in BATCH_EDGES_100)
TRIP_USERS, TRIP_ITEMS = 3000, 700
# (batch, path, variant, the kernel whose second grid-stride trip the batch reaches)
TRIPS = ((32773, "atomic", 1, "bwd"), (65539, "atomic", 2, "fwd"), (65539, "sorted_payload", 2, "fwd"))
PATTERN_BATCH = 257
REGIME_SHIFTS = {0: (0, 8, 12, -12, -30), 1: (0, 8, 12, 20, -12, -30, -80), 2: (0, 8, 12, -12, -30)}
REGIME_PATHS = ("atomic", "sorted_payload")
REGIME_MAX_BOUND = 1e-2


def width_cases():
    return [(d, *ROTATION[k % 3]) for k, d in enumerate(WIDTHS)]


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _case(tag, batch, d, n_neg, n_users=N_USERS, n_items=N_ITEMS):
    """Tables and ids drawn from a seed of the tag: the same inputs on every path, a fresh seed per case."""
    rng = _rng(tag)
    return dict(tag=tag, ut=(rng.standard_normal((n_users, d)) * SCALE).astype(np.float32),
                it=(rng.standard_normal((n_items, d)) * SCALE).astype(np.float32),
                u=rng.integers(0, n_users, batch), i=rng.integers(0, n_items, batch),
                j=rng.integers(0, n_items, (batch, n_neg)))


def _valid(c):
    n_u, n_i = c["ut"].shape[0], c["it"].shape[0]
    return (c["u"] >= 0) & (c["u"] < n_u) & (c["i"] >= 0) & (c["i"] < n_i) & ((c["j"] >= 0) & (c["j"] < n_i)).all(1)


def _restated(ut, it, u, i, j, variant, w, dtype):
    """include/gcr.h's BPR formulas in torch on the CPU at `dtype`; j: [B, n_neg], every id in range -> {key: float64}."""
    tu = torch.from_numpy(ut).to(dtype).requires_grad_(True)
    ti = torch.from_numpy(it).to(dtype).requires_grad_(True)
    u, i, j = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)) for a in (u, i, j))
    ur, pr, nr = tu[u], ti[i], ti[j]
    x = (ur * pr).sum(-1) - (ur[:, None, :] * nr).sum(-1).mean(-1)
    if variant == 0:
        per = -torch.log(10e-6 + torch.sigmoid(x))
    elif variant == 1:
        per = -F.logsigmoid(x)
    else:
        per = -torch.log(torch.sigmoid(x))
    sums = torch.stack([per.sum(), ur.square().sum(), pr.square().sum(), nr.square().sum()])
    (sums * torch.tensor(w, dtype=dtype)).sum().backward()
    gu = tu.grad if tu.grad is not None else torch.zeros_like(tu)
    gi = ti.grad if ti.grad is not None else torch.zeros_like(ti)
    out = dict(loss=sums[0], su=sums[1], sp=sums[2], sn=sums[3], gu=gu, gi=gi, per=per)
    return {k: v.detach().double().numpy() for k, v in out.items()}


_REFS = {}


def _reference(c, variant, w):
    """(f64 values, their scales S, the float32 restatement's absolute drift, #samples removed), computed once per case."""
    key = (c["tag"], variant, tuple(w))
    if key not in _REFS:
        ok = _valid(c)
        args = (c["ut"], c["it"], c["u"][ok], c["i"][ok], c["j"][ok], variant, w)
        ref, f32 = _restated(*args, torch.float64), _restated(*args, torch.float32)
        scale = dict(loss=float(np.maximum(1.0, np.abs(ref["per"])).sum()), su=float(ref["su"]), sp=float(ref["sp"]),
                     sn=float(ref["sn"]), gu=float(np.abs(ref["gu"]).max()), gi=float(np.abs(ref["gi"]).max()))
        drift = {k: float(np.abs(f32[k] - ref[k]).max()) for k in KEYS}
        assert all(np.isfinite(f32[k]).all() and np.isfinite(ref[k]).all() for k in KEYS), c["tag"]
        _REFS[key] = (ref, scale, drift, int((~ok).sum()))
    return _REFS[key]


def _bounds(scale, drift):
    return {k: max(4.0 * drift[k] / scale[k], FLOOR) for k in KEYS if scale[k] != 0.0}


def _fused(path, c, variant, w, monkeypatch):
    """The library on one path -> ({key: float64 numpy}, sums[4])."""
    import recommendation_amd as ra
    from recommendation_amd import functional as Fn
    monkeypatch.setattr(Fn, "BPR_SORTED_MIN_BATCH", 1 << 40 if path == "atomic" else 1)
    monkeypatch.setattr(Fn, "BPR_NEG_PAYLOAD_SORT", not path.endswith("_index"))
    n_u, n_i = c["ut"].shape[0], c["it"].shape[0]
    j = c["j"][:, 0] if c["j"].shape[1] == 1 else c["j"]
    w5 = torch.tensor([*w, 0.0], dtype=torch.float32, device=DEV)
    if path in EDGE_PATHS:
        graph = ra.CsrGraph.bipartite_raw(c["u"], c["i"], n_u, n_i, DEV)
        uu, ii = graph.user_major_edges(n_u)
        order = np.argsort(c["u"], kind="stable")                  # the batch is the edge list in user-major order
        assert np.array_equal(uu.cpu().numpy(), c["u"][order]) and np.array_equal(ii.cpu().numpy(), c["i"][order])
        table = torch.from_numpy(np.concatenate([c["ut"], c["it"]])).to(DEV).requires_grad_(True)
        sums = Fn.bpr_edge_sums(graph, table, n_u, torch.from_numpy(np.ascontiguousarray(j[order])).to(DEV), variant)
        (sums * w5).sum().backward()
        gu, gi = table.grad[:n_u], table.grad[n_u:]
    else:
        tu = torch.from_numpy(c["ut"]).to(DEV).requires_grad_(True)
        ti = torch.from_numpy(c["it"]).to(DEV).requires_grad_(True)
        sums = Fn.bpr_sums(tu, ti, c["u"], c["i"], j, variant)
        (sums * w5).sum().backward()
        gu, gi = tu.grad, ti.grad
    s = sums.detach().cpu().double().numpy()
    got = dict(loss=s[0], su=s[1], sp=s[2], sn=s[3], gu=gu.cpu().double().numpy(), gi=gi.cpu().double().numpy())
    return got, float(s[4])


def _check(got, ref, scale, drift, tag):
    """The bound rule; prints every figure before asserting."""
    bad = []
    for k in KEYS:
        err = float(np.abs(got[k] - ref[k]).max())
        if scale[k] == 0.0:
            print(f"BPRPIN {tag}:{k} reference is all zero, err={err:.3e}")
            if not err == 0.0:
                bad.append((k, err, 0.0))
            continue
        err /= scale[k]
        bound = max(4.0 * drift[k] / scale[k], FLOOR)
        print(f"BPRPIN {tag}:{k} err={err:.3e} bound={bound:.3e} ratio={err / bound:.3f}")
        if not err <= bound or (4.0 * drift[k] / scale[k] <= NORTH_STAR and not err <= NORTH_STAR):
            bad.append((k, err, bound))
    assert not bad, (tag, bad)


def _default_w(c):
    return (1.0 / len(c["u"]), 3e-4, 2e-4, 1e-4)


def _pin(path, c, variant, w, monkeypatch, table):
    ref, scale, drift, n_bad = _reference(c, variant, w)
    got, skipped = _fused(path, c, variant, w, monkeypatch)
    assert skipped == n_bad, (c["tag"], skipped, n_bad)
    _check(got, ref, scale, drift, f"{table}/{c['tag']}/{path}")
    return got, ref


# ---- WIDTHS ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", SUMS_PATHS)
@pytest.mark.parametrize("d, variant, n_neg", width_cases())
def test_widths(monkeypatch, path, d, variant, n_neg):
    c = _case(f"d{d}_v{variant}_n{n_neg}", WIDTH_BATCH, d, n_neg)
    _pin(path, c, variant, _default_w(c), monkeypatch, "WIDTHS")


@pytest.mark.parametrize("path", EDGE_PATHS)
@pytest.mark.parametrize("d, variant, n_neg", [wc for wc in width_cases() if wc[0] in EDGE_WIDTHS])
def test_widths_over_a_graphs_edges(monkeypatch, path, d, variant, n_neg):
    c = _case(f"d{d}_v{variant}_n{n_neg}", WIDTH_BATCH, d, n_neg)
    _pin(path, c, variant, _default_w(c), monkeypatch, "WIDTHS")


# ---- BATCH_EDGES -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", SUMS_PATHS)
@pytest.mark.parametrize("k", range(len(BATCH_EDGES)))
def test_batch_edges(monkeypatch, path, k):
    d, batch, n_neg = BATCH_EDGES[k][:3]
    variant = k % 3
    c = _case(f"B{batch}_d{d}_v{variant}_n{n_neg}", batch, d, n_neg)
    _pin(path, c, variant, _default_w(c), monkeypatch, "BATCH_EDGES")


# ---- TRIPS -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch, path, variant, trip", TRIPS)
def test_second_grid_stride_trip(monkeypatch, batch, path, variant, trip):
    c = _case(f"B{batch}_v{variant}", batch, 64, 1, TRIP_USERS, TRIP_ITEMS)
    _pin(path, c, variant, _default_w(c), monkeypatch, "TRIPS")


# ---- PATTERNS --------------------------------------------------------------------------------------------------------------
BAD_IDS = (-1, None, 2 ** 32 + 3)            # None: one past the table; the last would alias id 3 if cut to 32 bits


def _chunk0_end(keys, per_sample=1):
    """The sample that owns position 63 of the sorted order of `keys`: lane 63 of the first wave's chunk."""
    return int(np.argsort(np.asarray(keys).reshape(-1), kind="stable")[63]) // per_sample


def _spoil(c, name):
    """Bad ids in one index vector at the first sample, the last sample and a sample that sits at the end of chunk 0 of
    another vector's order (its own bad key sorts last): of the user order for i and j, of the positive-item order and of
    the negative order for u."""
    n_neg = c["j"].shape[1]
    vec, n = (c["u"], c["ut"].shape[0]) if name == "u" else (c["i"], c["it"].shape[0]) if name == "i" else \
        (c["j"][:, int(name[1])], c["it"].shape[0])
    where = [0, len(vec) - 1] + ([_chunk0_end(c["i"]), _chunk0_end(c["j"], n_neg)] if name == "u" else [_chunk0_end(c["u"])])
    for k, b in enumerate(where):
        bad = BAD_IDS[min(k, 2)]
        vec[b] = n if bad is None else bad


def pattern(name):
    """-> (case, variant, whether the batch can be a graph's edge list)."""
    b = PATTERN_BATCH
    c = _case(name, b, 64, 1 if name == "x_zero" else 2, *((300, 800) if name == "distinct" else (N_USERS, N_ITEMS)))
    rng = _rng(name + "/ids")
    if name == "same_user":
        c["u"][:] = 7
    elif name == "distinct":
        items = rng.permutation(800)
        c["u"], c["i"], c["j"] = rng.permutation(300)[:b], items[:b], items[b:3 * b].reshape(b, 2)
    elif name == "straddle":                                   # sorted: the run of 1s lies on entries 60 .. 69
        ids = np.array([0] * 60 + [1] * 10 + [2] * 187)
        c["u"], c["i"] = rng.permutation(ids), rng.permutation(ids)
    elif name == "x_zero":
        c["j"] = c["i"][:, None].copy()
    elif name == "twin_negative":
        c["j"][:, 1] = c["j"][:, 0]
    elif name.startswith("bad_"):
        _spoil(c, name[4:])
    elif name == "all_bad":                                    # the bad id rotates through u, i, j[:, 0], j[:, 1]
        for k, vec in enumerate((c["u"], c["i"], c["j"][:, 0], c["j"][:, 1])):
            vec[k::4] = -1 - k if k % 2 else N_ITEMS + N_USERS + k
    elif name == "all_bad_negatives":
        c["j"][0::2, 0], c["j"][1::2, 1] = N_ITEMS, -1
    else:
        raise KeyError(name)
    variant = PATTERNS.index(name) % 3
    return c, variant, name not in ("bad_u", "bad_i", "all_bad")


PATTERNS = ("same_user", "distinct", "straddle", "x_zero", "twin_negative", "bad_u", "bad_i", "bad_j0", "bad_j1", "all_bad",
            "all_bad_negatives")
PATTERN_WEIGHTS = {"default": None, "reg_only": (0.0, 1.0, 2.0, 3.0)}


def pattern_cases():
    return [(name, wkey, path) for name in PATTERNS for wkey in PATTERN_WEIGHTS
            for path in SUMS_PATHS + (EDGE_PATHS if name not in ("bad_u", "bad_i", "all_bad") else ())]


@pytest.mark.parametrize("name, wkey, path", pattern_cases())
def test_patterns(monkeypatch, name, wkey, path):
    c, variant, edge_ok = pattern(name)
    assert edge_ok or path in SUMS_PATHS
    w = PATTERN_WEIGHTS[wkey] or _default_w(c)
    c["tag"] = f"{name}/{wkey}"
    got, ref = _pin(path, c, variant, w, monkeypatch, "PATTERNS")
    n_bad = int((~_valid(c)).sum())
    if name == "same_user":
        rest = np.delete(got["gu"], 7, axis=0)
        assert (got["gu"][7] != 0).any() and (rest == 0).all()
    elif name == "straddle":
        order = np.sort(c["u"])
        assert order[59] == 0 and order[60] == 1 and order[69] == 1 and order[70] == 2
    elif name == "x_zero":
        assert (np.abs(ref["per"] - np.log(2.0) if variant else ref["per"] + np.log(10e-6 + 0.5)) < 1e-12).all()
    elif name.startswith("bad_"):
        assert n_bad == (3 if name != "bad_u" else 4)
    elif name.startswith("all_bad"):
        assert n_bad == PATTERN_BATCH and got["loss"] == 0.0 and not got["gu"].any() and not got["gi"].any()


# ---- REGIMES ---------------------------------------------------------------------------------------------------------------
def regime_case(variant, shift):
    """x ~ shift: column 0 of every user row is 1; of the first half of the items (the positives) + shift / 2, of the second
    half (the negatives) - shift / 2."""
    tag = f"v{variant}_shift{shift}"
    c = _case(tag, PATTERN_BATCH, 64, 2)
    rng, half = _rng(tag + "/ids"), N_ITEMS // 2
    c["ut"][:, 0] = 1.0
    c["it"][:half, 0], c["it"][half:, 0] = shift / 2.0, -shift / 2.0
    c["i"] = rng.integers(0, half, PATTERN_BATCH)
    c["j"] = rng.integers(half, N_ITEMS, (PATTERN_BATCH, 2))
    return c


@pytest.mark.parametrize("path", REGIME_PATHS)
@pytest.mark.parametrize("variant, shift", [(v, s) for v in (0, 1, 2) for s in REGIME_SHIFTS[v]])
def test_score_regimes(monkeypatch, path, variant, shift):
    """Variant 1 at shift 8, 12 and 20 is what failed while bpr_point took 1 - sigmoid(x) by subtraction at every x
    (err / bound 32, 704 and 166 472 on the user gradient: exactly zero at 20)."""
    c = regime_case(variant, shift)
    w = (1.0 / PATTERN_BATCH, 0.0, 0.0, 0.0)
    ref, scale, drift, _ = _reference(c, variant, w)
    bounds = _bounds(scale, drift)
    assert set(bounds) == set(KEYS) and max(bounds.values()) <= REGIME_MAX_BOUND, bounds
    x = -np.log(np.expm1(ref["per"])) if variant else None
    assert x is None or abs(float(np.median(x)) - shift) < 1.0
    _pin(path, c, variant, w, monkeypatch, "REGIMES")
