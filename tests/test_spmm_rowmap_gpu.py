"""A row order changes no word.

A graph with a row order (graph.RowOrder: a row-permuted copy of the CSR, a plan over it and a row map) runs its plain
launches at d <= 64 through the mapped instantiations of `walk_partition` (gcr_spmm_rows_mapped_f32,
gcr_spmm_windowed_mapped_f32), which take the row of a flush and of an acc_in load from the row map instead of stepping a
pointer.  Every row keeps its non-zeros in stored order and the split rows keep their slots, so every word of y, acc_out,
both split-row workspaces and the hub partials, all NaN-filled beforehand, must be `torch.equal` to what the same launch
writes on the same graph built with row_order=False.  A second launch must equal the first.

Graphs: those of tests/test_spmm_walk_gpu.py, built here -- the 300 users x 40 items and the 5 x 3 bipartite sym-norm
operators; a hand-built CSR (34 rows x 700 columns) whose first partition holds exactly 512 non-zeros in whole rows, with
empty rows first, in the middle and last, a row ending exactly at non-zero 64 and one at 65, five degree-1 rows inside one
batch of 16, followed by a row of 1 300 non-zeros and one of 600 (split rows; the first is the hub row when the hub plan
is on); and a one-non-zero matrix.  Orders, each forced: the coldest-column order (of the user rows of a bipartite
operator, of every row otherwise), a seeded random permutation, the reversal, the identity.  d = 64, 48, 4; with values
and all-ones; hub plan forced with a 64-row window, and off."""
import functools

import numpy as np
import pytest
import torch

from spmm_raw import Out, assert_words_equal, nan as _nan

pytestmark = pytest.mark.gpu

F32 = np.float32
HAND_COLS = 700
# (y, acc_in: None | 'given' | 'inplace', acc_out, val_scale, acc_scale)
FORMS = {"horner": (False, "given", True, 1.0, 1.0), "horner_scaled": (False, "given", True, 0.75, 0.25),
         "horner_in_place": (False, "inplace", True, 1.0, 0.5), "y_only": (True, None, False, 1.0 / 0.65, 1.0),
         "y_and_acc": (True, "given", True, 1.0 / 0.65, 1.0 / 3.0), "acc_without_acc_in": (False, None, True, -1.5, 0.5)}
# graph, hub plan on; a graph without a row above its hub degree has no hub plan to force
CASES = [("300x40", False), ("300x40", True), ("5x3", False), ("5x3", True), ("hand", False), ("hand", True), ("one_nnz", False)]
BIPARTITE = {"300x40": (300, 40, 3000, 100), "5x3": (5, 3, None, 3)}         # users, items, interactions, hub_min_degree
ORDERS = ("coldest", "random", "reversed", "identity")


def _bipartite(shape, has_val):
    """rowptr, col, val, n_rows, n_cols, hub_min_degree, nnz_per_part: users first, sym-norm values, sorted columns."""
    n_u, n_i, e, min_deg = BIPARTITE[shape]
    if e is None:
        u, i = np.array([0, 1, 2, 4, 1, 4, 2]), np.array([0, 0, 0, 0, 1, 2, 2])           # user 3 has no interaction
    else:
        rng = np.random.default_rng(20251)
        p = 1.0 / np.arange(1, n_i + 1) ** 0.8                                            # a few items most users name
        u = rng.integers(0, n_u - 7, e)                                                   # the last users: empty rows
        i = rng.choice(n_i, e, p=p / p.sum())
        keep = np.unique(u * n_i + i)
        u, i = keep // n_i, keep % n_i
    n = n_u + n_i
    rows, cols = np.concatenate([u, i + n_u]), np.concatenate([i + n_u, u])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    deg = np.bincount(rows, minlength=n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    val = (1.0 / np.sqrt(deg[rows] * deg[cols])).astype(F32) if has_val else None
    return rowptr, cols.astype(np.int32), val, n, n, min_deg, 64


HAND_HEAD = [0, 0, 0, 30, 34, 1, 1, 1, 1, 1, 1, 0, 0, 10, 9, 11, 12, 8, 13, 16, 17, 2]      # 168 non-zeros
HAND_DEG = HAND_HEAD + [512 - sum(HAND_HEAD)] + [1300, 3, 0, 5, 600, 1, 7, 0, 0]


def _hand(has_val):
    deg = np.asarray(HAND_DEG, dtype=np.int64)
    rng = np.random.default_rng(97 + int(has_val))
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.integers(0, HAND_COLS, k)) for k in deg]).astype(np.int32)   # sorted inside a row
    val = rng.standard_normal(col.size).astype(F32) if has_val else None
    return rowptr, col, val, deg.size, HAND_COLS, 1000, 512


def _row_order(name, order, n_rows):
    if order == "coldest":
        return (0, BIPARTITE[name][0]) if name in BIPARTITE else (0, n_rows)
    if order == "random":
        return torch.from_numpy(np.random.default_rng(4099 + n_rows).permutation(n_rows))
    if order == "reversed":
        return torch.arange(n_rows - 1, -1, -1)
    return torch.arange(n_rows)


@functools.lru_cache(maxsize=None)
def _graph(name, has_val, hub, order):
    """The operator with a forced row order, or (order None) with row_order=False: the reference."""
    import recommendation_amd as ra
    if name in BIPARTITE:
        rowptr, col, val, n_rows, n_cols, min_deg, npp = _bipartite(name, has_val)
    elif name == "hand":
        rowptr, col, val, n_rows, n_cols, min_deg, npp = _hand(has_val)
    else:
        rowptr, col, val = np.array([0, 1], dtype=np.int64), np.array([5], dtype=np.int32), (np.array([0.5], F32) if has_val else None)
        n_rows, n_cols, min_deg, npp = 1, 9, None, 512
    kw = dict(hub_window_rows=64, hub_min_degree=min_deg) if hub else dict(hub_window_rows=0)
    kw["row_order"] = False if order is None else _row_order(name, order, n_rows)
    g = ra.CsrGraph(rowptr, col, val, n_rows, n_cols, "cuda", symmetric=n_rows == n_cols, nnz_per_part=npp, **kw)
    assert (g.hub is not None) == hub and (g.rows_p is not None) == (order is not None)
    if order is not None:
        rp, base = g.rows_p, (g.hub.main if hub else g.plan)
        assert rp.n_p == n_rows - (g.hub.n_hub if hub else 0) and rp.plan.n_slots == base.n_slots and rp.eligible(4)
        if name == "hand":
            assert rp.plan.n_long == (1 if hub else 2), "the rows of 1 300 and 600 non-zeros are split rows of P as well"
        if order != "identity" and n_rows > 1:
            assert not np.array_equal(rp.order_host, np.sort(rp.order_host)), "the order moves a row"
    return g


@functools.lru_cache(maxsize=None)
def _inputs(name, d):
    g = _graph(name, True, False, None)
    rng = np.random.default_rng(31 * d + g.n_rows)
    return (torch.from_numpy(rng.standard_normal((g.n_cols, d)).astype(F32)).cuda(),
            torch.from_numpy(rng.standard_normal((g.n_rows, d)).astype(F32)).cuda())


def _launch(g, xt, d, form, a_in):
    """[y, acc_out, main workspace, hub partials, companion workspace] of the plain launch `functional.spmm_into` makes at
    d <= 64: mapped when the graph carries a row order, unmapped when it does not."""
    from recommendation_amd import spmm_launch as L
    o = Out(g.n_rows, d, FORMS[form], a_in)
    rp = g.rows_p
    if g.hub is None:
        ws = _nan(g.plan.n_slots, d)
        if rp is not None:
            L.rows_mapped(rp, rp.plan, x=xt, d=d, partials=ws, on=xt, **o.kw())
        else:
            L.rows(g, g.plan, x=xt, d=d, partials=ws, on=xt, **o.kw())
        torch.cuda.synchronize()
        return [o.y, o.acc_out, ws, None, None]
    hub, H, main = g.hub, g.hub.H, g.hub.main
    part, hws, mws = _nan(H.n_rows, d), _nan(H.plan.n_slots, d), _nan(main.n_slots, d)
    kw = dict(hub_split=hws, partials=mws, hub_partials=part, x=xt, d=d, main_first=int(hub.main_first), on=xt, **o.kw())
    if rp is not None:
        L.windowed_mapped(H, H.plan, rp, rp.plan, hub, **kw)
    else:
        L.windowed(H, H.plan, g, main, hub, **kw)
    torch.cuda.synchronize()
    return [o.y, o.acc_out, mws, part, hws]


WHAT = ("y", "acc_out", "main workspace", "hub partials", "companion workspace")


def _equal(got, want, what):
    for g, w, name in zip(got, want, WHAT):
        assert_words_equal(g, w, f"{what} {name}")


@functools.lru_cache(maxsize=None)
def _reference(name, hub, d, has_val, form):
    """The launch on the graph without a row order: computed once per case, shared by the four orders, never written to."""
    xt, a_in = _inputs(name, d)
    ref = _launch(_graph(name, has_val, hub, None), xt, d, form, a_in)
    for t, nm in zip(ref[:2], WHAT):
        assert t is None or not bool(torch.isnan(t).any()), f"{name} hub={hub} d={d} {form}: the reference left a word of {nm} unwritten"
    return ref


@pytest.mark.parametrize("has_val", [True, False], ids=["val", "ones"])
@pytest.mark.parametrize("d", [64, 48, 4])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,hub", CASES, ids=[f"{n}-{'hub' if h else 'plain'}" for n, h in CASES])
def test_every_word_equals_the_launch_without_a_row_order(name, hub, order, d, has_val):
    g = _graph(name, has_val, hub, order)
    xt, a_in = _inputs(name, d)
    for form in FORMS:
        what = f"{name} hub={hub} order={order} d={d} {form}"
        ref = _reference(name, hub, d, has_val, form)
        first = _launch(g, xt, d, form, a_in)
        _equal(first, ref, what)
        _equal(_launch(g, xt, d, form, a_in), first, what + ", second launch")


@pytest.mark.parametrize("hub", [False, True], ids=["plain", "hub"])
def test_spmm_into_takes_the_mapped_route_and_writes_the_same_words(hub, monkeypatch):
    """`functional.spmm_into` on a graph with a row order against the same graph without one, Horner layer and y only: the
    mapped launch function runs, once, and only for the graph that carries the order.  A view with other values
    (`with_values`) drops the row order with the values it copied."""
    from recommendation_amd import functional as F
    from recommendation_amd import spmm_launch as L
    g, ref = _graph("300x40", True, hub, "coldest"), _graph("300x40", True, hub, None)
    xt, a_in = _inputs("300x40", 64)
    mapped = "windowed_mapped" if hub else "rows_mapped"
    real, seen = getattr(L, mapped), []
    monkeypatch.setattr(L, mapped, lambda *a, **k: seen.append(mapped) or real(*a, **k))
    for form in ("horner", "y_only"):
        outs = []
        for graph, want in ((g, [mapped]), (ref, [])):
            o = Out(g.n_rows, 64, FORMS[form], a_in)
            seen.clear()
            F.spmm_into(graph, xt, **o.kw())
            torch.cuda.synchronize()
            assert seen == want, f"hub={hub} {form}: the route"
            outs.append([o.y, o.acc_out])
        for a, b, nm in zip(outs[0], outs[1], WHAT):
            assert_words_equal(a, b, f"spmm_into hub={hub} {form} {nm}")
    v2 = g.val * 2.0
    g2 = g.with_values(v2)
    assert g2.rows_p is None and g2.hub is None
    y2, y1 = _nan(g.n_rows, 64), _nan(g.n_rows, 64)
    seen.clear()
    F.spmm_into(g2, xt, y=y2)
    F.spmm_into(ref.with_values(v2), xt, y=y1)
    torch.cuda.synchronize()
    assert seen == [] and not bool(torch.isnan(y2).any())
    assert_words_equal(y2, y1, "with_values y")
