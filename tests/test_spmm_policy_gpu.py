"""Cache-policy hints change no word: the kernels around `walk_partition` and `sum_partials` load the CSR words, acc_in
and the partial rows, and store the output and partial rows, with `nt`; the generic kernel (`spmm_parts`, behind
gcr_spmm_csr_acc2_f32) keeps plain accesses and is the reference.

On small bipartite sym-norm operators (users first, as bench.py builds them) every word of y, acc_out, both split-row
workspaces and the hub partials, all NaN-filled beforehand, must be `torch.equal` to what the generic kernel writes on the
same plan: the plain launch (gcr_spmm_rows_f32) on the graph's plan, the windowed launch (gcr_spmm_windowed_f32) on the
main plan for every row that is no hub and on the companion for the window partials.  A hub row is the sum of its window
partials in `sum_partials`' fixed order (wave w adds partials w, w + 4, ... from 0, then ((w0 + w1) + w2) + w3) and the
two-rounding epilogue: that is restated in float32 numpy.  A second launch must equal the first.

Shapes: 300 users x 40 items x 3 000 interactions with partitions of 64 non-zeros (items above 64 users are split rows,
those above 100 hubs of a forced 64-row-window plan; users without interactions are empty rows) and 5 x 3; d = 64, 48, 4;
with values and all-ones; acc_in given, absent and in place.  The probe that measured the hints (gcr_probe_policy_rows_f32)
is checked against torch for every combination of its three flags."""
import functools

import numpy as np
import pytest
import torch

from spmm_raw import Out, assert_words_equal as _equal, generic, nan as _nan

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = {"300x40": (300, 40, 3000, 100), "5x3": (5, 3, None, 3)}        # users, items, interactions, hub_min_degree
# (y, acc_in: None | 'given' | 'inplace', acc_out, val_scale, acc_scale)
FORMS = {"y_only": (True, None, False, 1.0, 1.0), "horner": (False, "given", True, 1.0, 1.0),
         "both_scaled": (True, "given", True, 1.0 / 0.65, 0.25), "in_place": (False, "inplace", True, 1.0, 0.5),
         "acc_in_none": (True, None, True, 0.7, 3.0)}


def _pairs(shape):
    n_u, n_i, e, _ = SHAPES[shape]
    if e is None:
        return np.array([0, 1, 2, 4, 1, 4, 2]), np.array([0, 0, 0, 0, 1, 2, 2])          # user 3 has no interaction
    rng = np.random.default_rng(20251)
    p = 1.0 / np.arange(1, n_i + 1) ** 0.8                                               # a few items most users name
    u = rng.integers(0, n_u - 7, e)                                                      # the last users: empty rows
    i = rng.choice(n_i, e, p=p / p.sum())
    keep = np.unique(u * n_i + i)
    return keep // n_i, keep % n_i


@functools.lru_cache(maxsize=None)
def _graph(shape, has_val, hub):
    import recommendation_amd as ra
    n_u, n_i, _, min_deg = SHAPES[shape]
    u, i = _pairs(shape)
    n = n_u + n_i
    rows, cols = np.concatenate([u, i + n_u]), np.concatenate([i + n_u, u])
    order = np.lexsort((cols, rows))                                                     # sorted columns inside a row
    rows, cols = rows[order], cols[order]
    deg = np.bincount(rows, minlength=n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    val = (1.0 / np.sqrt(deg[rows] * deg[cols])).astype(F32) if has_val else None
    kw = dict(hub_window_rows=64, hub_min_degree=min_deg) if hub else dict(hub_window_rows=0)
    g = ra.CsrGraph(rowptr, cols.astype(np.int32), val, n, n, "cuda", symmetric=True, nnz_per_part=64, **kw)
    assert (g.hub is not None) == hub
    if shape == "300x40":
        assert int((deg == 0).sum()) >= 7 and g.plan.n_long > 0
        if hub:
            assert g.hub.main.n_long > 0 and g.hub.n_hub > 1 and g.hub.n_windows == 6
    return g


@functools.lru_cache(maxsize=None)
def _inputs(shape, d):
    n = SHAPES[shape][0] + SHAPES[shape][1]
    rng = np.random.default_rng(31 * d + n)
    return (torch.from_numpy(rng.standard_normal((n, d)).astype(F32)).cuda(),
            torch.from_numpy(rng.standard_normal((n, d)).astype(F32)).cuda())


@pytest.mark.parametrize("has_val", [True, False], ids=["val", "ones"])
@pytest.mark.parametrize("d", [64, 48, 4])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_plain_launch_equals_the_generic_kernel(shape, d, has_val):
    from recommendation_amd import spmm_launch as L
    g = _graph(shape, has_val, False)
    xt, a_in = _inputs(shape, d)
    for form in FORMS:
        ref, ref_ws = Out(g.n_rows, d, FORMS[form], a_in), _nan(g.plan.n_slots, d)
        generic(g, g.plan, xt, d, ref_ws, **ref.kw())
        assert not any(bool(torch.isnan(t).any()) for t in (ref.y, ref.acc_out) if t is not None), "the reference left a word unwritten"
        runs = []
        for _ in range(2):
            o, ws = Out(g.n_rows, d, FORMS[form], a_in), _nan(g.plan.n_slots, d)
            L.rows(g, g.plan, x=xt, d=d, partials=ws, on=xt, **o.kw())
            torch.cuda.synchronize()
            runs.append((o.y, o.acc_out, ws))
        for k, what in enumerate(("y", "acc_out", "workspace")):
            _equal(runs[0][k], (ref.y, ref.acc_out, ref_ws)[k], f"{shape} {form} {what}")
            _equal(runs[1][k], runs[0][k], f"{shape} {form} {what}, second launch")


def _hub_rows_f32(part, n_hub, n_win, val_scale, acc_in_rows, acc_scale):
    """The hub rows' reduction restated: `sum_partials`' order, then store_row's two roundings; (y rows, acc_out rows)."""
    p = part.cpu().numpy().reshape(n_win, n_hub, -1)
    waves = []
    for w in range(4):
        acc = np.zeros(p.shape[1:], F32)
        for k in range(w, n_win, 4):
            acc = acc + p[k]
        waves.append(acc)
    total = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    yv = total * F32(val_scale)
    prev = F32(0.0) if acc_in_rows is None else acc_in_rows
    return yv, (prev + yv) * F32(acc_scale)


@pytest.mark.parametrize("has_val", [True, False], ids=["val", "ones"])
@pytest.mark.parametrize("d", [64, 48, 4])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_windowed_launch_equals_the_generic_kernel(shape, d, has_val):
    from recommendation_amd import spmm_launch as L
    g = _graph(shape, has_val, True)
    hub, H, main = g.hub, g.hub.H, g.hub.main
    xt, a_in = _inputs(shape, d)
    hub_rows = hub.hub_row.long()
    rest = torch.ones(g.n_rows, dtype=torch.bool, device="cuda")
    rest[hub_rows] = False
    # the window partials are H x as the generic kernel writes it with y only and a val_scale of 1
    ref_part, ref_hws = _nan(H.n_rows, d), _nan(H.plan.n_slots, d)
    generic(H, H.plan, xt, d, ref_hws, y=ref_part)
    assert not bool(torch.isnan(ref_part).any())
    for form in FORMS:
        ref, ref_mws = Out(g.n_rows, d, FORMS[form], a_in), _nan(main.n_slots, d)
        generic(g, main, xt, d, ref_mws, **ref.kw())
        acc_rows = None if FORMS[form][1] is None else a_in[hub_rows].cpu().numpy()
        hub_y, hub_acc = _hub_rows_f32(ref_part, hub.n_hub, hub.n_windows, ref.val_scale, acc_rows, ref.acc_scale)
        runs = []
        for _ in range(2):
            o, part, hws, mws = Out(g.n_rows, d, FORMS[form], a_in), _nan(H.n_rows, d), _nan(H.plan.n_slots, d), _nan(main.n_slots, d)
            L.windowed(H, H.plan, g, main, hub, hub_split=hws, partials=mws, hub_partials=part, x=xt, d=d,
                       main_first=int(hub.main_first), on=xt, **o.kw())
            torch.cuda.synchronize()
            runs.append((o.y, o.acc_out, part, hws, mws))
        y, acc_out, part, hws, mws = runs[0]
        _equal(part, ref_part, f"{shape} {form} hub partials")
        _equal(hws, ref_hws, f"{shape} {form} companion workspace")
        _equal(mws, ref_mws, f"{shape} {form} main workspace")
        for got, want, hub_want, what in ((y, ref.y, hub_y, "y"), (acc_out, ref.acc_out, hub_acc, "acc_out")):
            assert (got is None) == (want is None)
            if got is None:
                continue
            assert not bool(torch.isnan(got).any()), f"{shape} {form} {what}: a word was left unwritten"
            _equal(got[rest], want[rest], f"{shape} {form} {what}, rows of the main plan")
            _equal(got[hub_rows], torch.from_numpy(np.ascontiguousarray(hub_want, dtype=F32)).cuda(), f"{shape} {form} {what}, hub rows")
        for k, what in enumerate(("y", "acc_out", "hub partials", "companion workspace", "main workspace")):
            _equal(runs[1][k], runs[0][k], f"{shape} {form} {what}, second launch")


@pytest.mark.parametrize("n_idx", [64, 64 * 9])
def test_policy_probe_sums_what_it_says(n_idx):
    from recommendation_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(n_idx)
    n_hot, n_cold = 37, 1001
    hot = torch.rand(n_hot, 64, device="cuda", generator=g)
    cold = torch.rand(n_cold, 64, device="cuda", generator=g)
    idx = torch.randint(-3, n_cold + 3, (n_idx,), device="cuda", dtype=torch.int32, generator=g)   # ids out of range are clamped
    stream_in = torch.rand(n_idx // 16, 64, 4, device="cuda", generator=g)
    ids = idx.long().view(-1, 8, 2)
    want = (hot[ids[:, :, 0].clamp(0, n_hot - 1)].sum(1) + cold[ids[:, :, 1].clamp(0, n_cold - 1)].sum(1) + stream_in.sum(2))
    first = None
    for flags in range(8):
        out = _nan(n_idx // 16, 64)
        _lib.call("gcr_probe_policy_rows_f32", hot, n_hot, cold, n_cold, idx, n_idx, stream_in, out, flags, on=out)
        torch.cuda.synchronize()
        # 20 addends in [0, 1): every partial sum is below 32, so an addition rounds by at most 2^-20, in either order
        assert torch.allclose(out, want, rtol=0.0, atol=2 * 20 * 2.0 ** -20), f"nt_flags {flags}"
        first = out if first is None else first
        assert torch.equal(out, first), f"nt_flags {flags} computes other words than plain loads and stores"
    assert _lib.lib().gcr_probe_policy_rows_f32(_lib.dptr(hot), n_hot, _lib.dptr(cold), n_cold, _lib.dptr(idx), n_idx,
                                                _lib.dptr(stream_in), _lib.dptr(first), 8, None) == -1
