"""The windowed companion's own kernel (gcr_spmm_hub_parts_f32, step 1 of a windowed launch at d <= 64) against the launch
it replaces.

Step 1 used to be `spmm_parts` on the companion CSR `H`.  The new kernel runs the same partitions, one wave each, and differs
in the partition body only (no epilogue; what is left of a 64-non-zero block below a batch of 16 is gathered in batches of 8,
4, 2, 1), so every word of `hub.partials(d)` must equal the generic launch `Fn.spmm_into(H, x, y=...)`, and the whole launch
must stay on the bits of tests/spmm_window_common.py's replay.  The matrices are that file's (n_cols = 700, 64-row windows,
hubs above 40), once as they are and once as a stack of copies (other seeds, rows appended), which gives partitions of every
tail length, padded partitions and several blocks per XCD list."""
import numpy as np
import pytest
import torch

from spmm_raw import nan
from spmm_window_common import F32, HUB_MIN_DEGREE, N_COLS, WINDOW_ROWS, make_matrix, replay_windowed

pytestmark = pytest.mark.gpu

STACK = {"base": 10, "empty_window": 20, "dup": 8}


def stacked(kind, copies):
    mats = [make_matrix(kind, seed=s) for s in range(copies)]
    deg = np.concatenate([np.diff(m[0]) for m in mats])
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return rowptr, np.concatenate([m[1] for m in mats]), np.concatenate([m[2] for m in mats])


def build(rowptr, col, val):
    import recommendation_amd as ra
    n_rows = rowptr.size - 1
    g = ra.CsrGraph(rowptr, col, val, n_rows, N_COLS, "cuda", hub_window_rows=WINDOW_ROWS, hub_min_degree=HUB_MIN_DEGREE)
    assert g.hub is not None
    return g


def generic_partials(hub, xt):
    """H x by the launch the new kernel replaces (`spmm_parts`), before the hub reduction."""
    from recommendation_amd import functional as Fn
    ref = nan(hub.H.n_rows, xt.shape[1])
    assert hub.H.hub is None
    Fn.spmm_into(hub.H, xt, y=ref)
    return ref


def nan_workspaces(hub, d):
    hub.partials(d).fill_(float("nan"))
    ws = hub.H.workspace(d)
    if ws is not None:
        ws.fill_(float("nan"))


def check(g, rowptr, col, w, d, seed):
    """Partials against the generic launch (a skipped or doubly written row shows as NaN or a wrong word), the whole launch
    against the replay, and a second launch against the first."""
    from recommendation_amd import functional as Fn
    hub, n_rows = g.hub, rowptr.size - 1
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N_COLS, d)).astype(F32)
    acc_in = rng.standard_normal((n_rows, d)).astype(F32)
    xt, a_in = torch.from_numpy(x).cuda(), torch.from_numpy(acc_in).cuda()
    raw = replay_windowed(g, rowptr, col, w, x)
    want_y, want_acc, want_half = torch.from_numpy(raw).cuda(), torch.from_numpy(acc_in + raw).cuda(), \
        torch.from_numpy((acc_in + raw) * F32(0.5)).cuda()
    ref = generic_partials(hub, xt)
    assert bool(torch.isfinite(ref).all())
    empty = lambda: nan(n_rows, d)
    nan_workspaces(hub, d)
    y = empty()
    Fn.spmm_into(g, xt, y=y)                                                             # y only
    part = hub.partials(d)
    assert bool(torch.isfinite(part).all()), "a row of the companion was not written"
    assert torch.equal(part, ref), f"{int((part != ref).sum())} words of the partials differ"
    assert torch.equal(y, want_y), "y only"
    nan_workspaces(hub, d)
    y2 = empty()
    Fn.spmm_into(g, xt, y=y2)
    assert torch.equal(y2, y) and torch.equal(hub.partials(d), ref), "two launches differ"
    out = empty()
    Fn.spmm_into(g, xt, acc_in=a_in, acc_out=out)                                        # acc_out only (the Horner layer)
    assert torch.equal(out, want_acc), "acc_out only"
    inplace = a_in.clone()
    Fn.spmm_into(g, xt, acc_in=inplace, acc_out=inplace, acc_scale=0.5)                  # in place
    assert torch.equal(inplace, want_half), "in place"


@pytest.mark.parametrize("has_val", [True, False], ids=["val", "ones"])
@pytest.mark.parametrize("d", [64, 48])
@pytest.mark.parametrize("kind", ["base", "empty_window", "one_hub", "dup"])
def test_partials_have_the_generic_launch_bits(kind, d, has_val):
    rowptr, col, val, _ = make_matrix(kind)
    g = build(rowptr, col, val if has_val else None)
    if kind == "one_hub":
        assert g.hub.n_hub == 1
    if kind == "dup":
        assert g.hub.H.plan.n_long > 0
    check(g, rowptr, col, val if has_val else np.ones(col.size, F32), d, 31 * d + int(has_val) + len(kind))


@pytest.mark.parametrize("has_val", [True, False], ids=["val", "ones"])
@pytest.mark.parametrize("d", [64, 48])
@pytest.mark.parametrize("kind", sorted(STACK))
def test_stacked_matrices(kind, d, has_val):
    rowptr, col, val = stacked(kind, STACK[kind])
    g = build(rowptr, col, val if has_val else None)
    desc = g.hub.H.plan.desc_host
    n = desc[:, 1] - desc[:, 0]
    assert ((n == 0) & (desc[:, 2] == 0)).any(), "no padded partition"
    assert desc.shape[0] >= 8 * 4 * 3                                  # several blocks in every XCD's list
    # every tail the batches of 8, 4, 2, 1 can be asked for: all 16 residues of a block's length
    assert set(((n[n > 0] - 1) % 64 + 1) % 16) == set(range(16))
    if kind == "dup":
        assert g.hub.H.plan.n_long > 0
    check(g, rowptr, col, val if has_val else np.ones(col.size, F32), d, 57 * d + int(has_val) + len(kind))


def test_wider_launches_keep_the_generic_companion():
    from recommendation_amd import _lib, spmm_launch
    from recommendation_amd import functional as Fn
    d = 128
    rowptr, col, val, _ = make_matrix("dup")
    g = build(rowptr, col, val)
    hub, H = g.hub, g.hub.H
    x = np.random.default_rng(5).standard_normal((N_COLS, d)).astype(F32)
    xt = torch.from_numpy(x).cuda()
    part = hub.partials(d).fill_(7.0)
    with pytest.raises(_lib.GcrError, match="code -2"):              # GCR_EUNSUPPORTED
        spmm_launch.hub_parts(H, H.plan, x=xt, d=d, y=part, partials=H.workspace(d), on=xt)
    torch.cuda.synchronize()
    assert bool((part == 7.0).all()), "a refused call launched something"
    nan_workspaces(hub, d)
    y = nan(rowptr.size - 1, d)
    Fn.spmm_into(g, xt, y=y)
    assert torch.equal(hub.partials(d), generic_partials(hub, xt))
    assert torch.equal(y, torch.from_numpy(replay_windowed(g, rowptr, col, val, x)).cuda())


def empty_run_then_long_segment():
    """70 hub rows; only the last one has anything in window 3: 600 non-zeros (repeated columns).  In H, window 3 is 69 empty
    rows -- they close the running partition at its 64-row cap and leave one of empty rows only -- and then a row cut into
    five chunks."""
    rng = np.random.default_rng(77)
    keep = np.arange(N_COLS)
    keep = keep[keep // WINDOW_ROWS != 3]
    rows = [np.sort(rng.choice(keep, 45, replace=False)) for _ in range(70)]
    rows[69] = np.sort(np.concatenate([rows[69], rng.choice(np.arange(192, 256), 600, replace=True)]))
    rows += [np.sort(rng.choice(N_COLS, k, replace=False)) for k in (3, 0, 40, 12)]
    deg = np.asarray([r.size for r in rows], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    return rowptr, col, rng.standard_normal(col.size).astype(F32)


@pytest.mark.parametrize("d", [64, 48])
def test_empty_partitions_in_front_of_a_chunked_segment(d):
    rowptr, col, val = empty_run_then_long_segment()
    g = build(rowptr, col, val)
    hub, desc = g.hub, g.hub.H.plan.desc_host
    assert hub.n_hub == 70 and hub.H.plan.n_long >= 1
    n, nrows, slot = desc[:, 1] - desc[:, 0], desc[:, 2] >> 32, desc[:, 3]
    assert ((slot < 0) & (nrows == 64)).any(), "no partition that the 64-row cap closed"
    assert ((slot < 0) & (nrows > 0) & (n == 0)).any(), "no partition of empty rows only"
    assert (slot >= 0).sum() >= 5
    check(g, rowptr, col, val, d, 9 + d)


@pytest.mark.parametrize("d", [64, 48])
def test_single_non_empty_window(d):
    rng = np.random.default_rng(3)
    rows = [np.sort(rng.choice(np.arange(128, 192), k, replace=k > 64)) for k in (41, 64, 150, 45, 300, 90)]
    rows += [np.sort(rng.choice(np.arange(128, 192), k, replace=False)) for k in (3, 0, 40)]
    deg = np.asarray([r.size for r in rows], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    val = rng.standard_normal(col.size).astype(F32)
    g = build(rowptr, col, val)
    seg = np.diff(g.hub.H.rowptr.cpu().numpy()).reshape(g.hub.n_windows, g.hub.n_hub)
    assert g.hub.n_hub == 6 and int((seg.sum(1) > 0).sum()) == 1 and g.hub.H.plan.n_long >= 2
    check(g, rowptr, col, val, d, 40 + d)
