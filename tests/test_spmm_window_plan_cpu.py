"""The windowed companion of the heaviest rows (graph.HubPlan), checked on the host: which rows are hubs, what the
companion CSR holds and where, what the main plan keeps, and how the companion's partitions are laid out over the XCDs.
No GPU: the graph lives on the CPU device, the plans are host arrays."""
import numpy as np
import pytest

from spmm_window_common import HUB_MIN_DEGREE, N_COLS, N_WIN, WINDOW_ROWS, make_matrix


def _graph(kind, **kw):
    import recommendation_amd as ra
    rowptr, col, val, notes = make_matrix(kind)
    kw.setdefault("hub_window_rows", WINDOW_ROWS)
    kw.setdefault("hub_min_degree", HUB_MIN_DEGREE)
    g = ra.CsrGraph(rowptr, col, val, rowptr.size - 1, N_COLS, "cpu", **kw)
    return g, rowptr, col, val, notes


def _covered(desc, nnz):
    c = np.zeros(nnz, np.int64)
    for a, b, _, _ in desc.tolist():
        c[a:b] += 1
    return c


@pytest.mark.parametrize("kind", ["base", "empty_window", "one_hub", "dup"])
def test_companion_holds_every_hub_non_zero_once_in_its_window(kind):
    g, rowptr, col, val, notes = _graph(kind)
    hub = g.hub
    assert hub is not None and hub.n_windows == N_WIN == -(-N_COLS // WINDOW_ROWS)
    deg = np.diff(rowptr)
    hubs = np.flatnonzero(deg > HUB_MIN_DEGREE)
    if kind == "base":
        assert {0, 1, 39, 40, 41, 700} <= set(deg.tolist())
        assert deg[notes["one_window"]] > HUB_MIN_DEGREE and deg[notes["edge"]] > HUB_MIN_DEGREE
    if kind == "one_hub":
        assert hubs.size == 1
    assert np.array_equal(hub.hub_row_host, hubs) and hub.n_hub == hubs.size      # 40 is not a hub, 41 is
    assert np.array_equal(hub.hub_row.numpy(), hubs)
    H = hub.H
    assert H.n_rows == N_WIN * hub.n_hub and H.n_cols == N_COLS and H.nnz == deg[hubs].sum() == hub.hub_nnz
    h_rp, h_col, h_val = H.rowptr.numpy(), H.col.numpy(), H.val.numpy()
    bounds = hub.bounds.numpy()
    assert bounds.shape == (hub.n_hub, N_WIN + 1)
    for w in range(N_WIN):
        empties = 0
        for h, r in enumerate(hubs):
            slot = w * hub.n_hub + h                                                # slots are w * n_hub + h
            cols, vals = col[rowptr[r]:rowptr[r + 1]], val[rowptr[r]:rowptr[r + 1]]
            sel = (cols // WINDOW_ROWS) == w
            assert np.array_equal(h_col[h_rp[slot]:h_rp[slot + 1]], cols[sel])      # exactly its window, stored order
            assert np.array_equal(h_val[h_rp[slot]:h_rp[slot + 1]], vals[sel])
            assert bounds[h, w + 1] - bounds[h, w] == sel.sum()
            empties += not sel.any()
        if kind == "empty_window" and w == 3:
            assert empties == hub.n_hub                                             # an empty window for every hub row
    if kind == "base":
        h = int(np.flatnonzero(hubs == notes["one_window"])[0])
        lens = np.diff(h_rp)[h::hub.n_hub]
        assert lens[2] == deg[notes["one_window"]] and lens.sum() == lens[2]        # all its columns in window 2
        h = int(np.flatnonzero(hubs == notes["edge"])[0])
        assert h_col[h_rp[0 * hub.n_hub + h + 1] - 1] == 63 and h_col[h_rp[1 * hub.n_hub + h]] == 64
    # every non-zero exactly once across the main plan and the companion
    main = _covered(hub.main.desc_host, col.size)
    is_hub = np.repeat(np.isin(np.arange(deg.size), hubs), deg)
    assert np.array_equal(main, (~is_hub).astype(np.int64))
    assert (_covered(H.plan.desc_host, H.nnz) == 1).all()
    for a, b, rowinfo, slot in hub.main.desc_host.tolist():                         # no hub row in the main plan
        row0, nrows = rowinfo & 0xFFFFFFFF, rowinfo >> 32
        assert not np.isin(np.arange(row0, row0 + nrows), hubs).any()
    assert hub.main.n_long == 0 or not np.isin(hub.main.long_row.numpy()[: hub.main.n_long], hubs).any()
    # the classic plan is still there, whole
    assert (_covered(g.plan.desc_host, col.size) == 1).all()


@pytest.mark.parametrize("kind", ["base", "dup"])
def test_every_window_runs_on_one_xcd(kind):
    g, *_ = _graph(kind)
    hub = g.hub
    desc = hub.H.plan.desc_host
    xcd = (np.arange(desc.shape[0]) // 4) % 8                 # workgroup b = partitions 4 b .. 4 b + 3, round-robin over 8
    real = (desc[:, 1] > desc[:, 0]) | ((desc[:, 2] >> 32) > 0) | (desc[:, 3] >= 0)
    window = (desc[:, 2] & 0xFFFFFFFF) // hub.n_hub
    seen = 0
    for w in range(N_WIN):
        on = np.unique(xcd[real & (window == w)])
        assert on.size <= 1, f"window {w} is spread over XCDs {on}"
        seen += on.size
        # ... and consecutively inside that XCD's sequence
        idx = np.flatnonzero(real & (window == w))
        if idx.size:
            seq = np.flatnonzero(xcd == on[0])
            pos = np.searchsorted(seq, idx)
            assert np.array_equal(pos, np.arange(pos[0], pos[0] + pos.size))
    # a partition belongs to the window of its first row: a run of short or empty segments may carry it into the next one
    assert seen == N_WIN if kind == "base" else seen >= 1


def test_unsorted_hub_row_falls_back_to_the_classic_plan():
    g, *_ = _graph("unsorted")
    assert g.hub is None and g.plan.n_parts > 0                 # not an error: CsrGraph accepts unsorted rows


def test_keyword_disables_and_small_tables_are_left_alone():
    g, *_ = _graph("base", hub_window_rows=0)
    assert g.hub is None
    g, *_ = _graph("base", hub_window_rows=None, hub_min_degree=None)
    assert g.hub is None                                        # 700 rows of table: nothing a window could save
    g, rowptr, *_ = _graph("base", hub_min_degree=None)        # forced window, default bound max(nnz_per_part, 8 W)
    from recommendation_amd.graph import HUB_NNZ_PER_PART
    thr = max(HUB_NNZ_PER_PART, 8 * N_WIN)
    assert np.array_equal(g.hub.hub_row_host, np.flatnonzero(np.diff(rowptr) > thr))
    assert g.hub.eligible(64) and g.hub.eligible(256)


def test_size_conditions_of_an_automatic_plan():
    from recommendation_amd import graph as G
    hub = G.HubPlan()
    hub.forced, hub.window_rows = False, G.HUB_WINDOW_ROWS
    hub.H = type("H", (), {"n_cols": 1_100_000})()
    assert hub.eligible(64) and hub.eligible(48)                # 282 MB of table, windows of at most one XCD's L2
    assert G.HUB_WINDOW_ROWS * 4 * 64 <= G.HUB_MAX_WINDOW_BYTES < G.HUB_WINDOW_ROWS * 4 * 128
    assert not hub.eligible(128)                                # a window larger than an L2
    hub.H.n_cols = 60_000
    assert not hub.eligible(64)                                 # 15 MB of table: under 4 x one XCD's L2
