"""Matrices and the order replay shared by tests/test_spmm_window_plan_cpu.py and tests/test_spmm_window_gpu.py: the
windowed companion of the heaviest rows (recommendation_amd.graph.HubPlan) at sizes a test can afford.

n_cols = 700 and window_rows = 64 give W = 11 column windows (the last one 60 columns wide); rows with more than 40
non-zeros are hubs."""
import numpy as np

from test_spmm_order_cpu import fma32

F32 = np.float32
N_COLS = 700
WINDOW_ROWS = 64
N_WIN = 11
HUB_MIN_DEGREE = 40


def _sorted_cols(rng, deg, lo=0, hi=N_COLS, avoid=None):
    pool = np.arange(lo, hi)
    if avoid is not None:
        pool = pool[(pool // WINDOW_ROWS) != avoid]
    return np.sort(rng.choice(pool, deg, replace=False))


def make_matrix(kind, seed=0):
    """(rowptr int64, col int32, val float32, notes): sorted columns inside every row unless kind == 'unsorted'.
    kinds: base | unsorted | empty_window | one_hub | dup"""
    rng = np.random.default_rng(1000 + seed + sum(map(ord, kind)))
    rows, notes = [], {}
    if kind in ("base", "unsorted"):
        for deg in (0, 1, 39, 40, 41, 700, 3, 0, 120):
            rows.append(_sorted_cols(rng, deg))
        notes["one_window"] = len(rows)
        rows.append(_sorted_cols(rng, 45, 128, 192))                      # a hub row inside window 2
        edge = np.union1d(_sorted_cols(rng, 48), [63, 64])                 # a column on either side of a window edge
        notes["edge"] = len(rows)
        rows.append(edge)
        for deg in (300, 5, 64, 0, 200, 41, 7, 513, 12, 40):
            rows.append(_sorted_cols(rng, deg))
        if kind == "unsorted":
            r = notes["unsorted"] = 8                                       # the degree-120 row
            rows[r] = rng.permutation(rows[r])
            assert (np.diff(rows[r]) < 0).any()
    elif kind == "empty_window":
        for deg in (0, 41, 2, 600, 39, 100, 40, 0, 77):
            rows.append(_sorted_cols(rng, deg, avoid=3))                  # nobody has a column in [192, 256)
    elif kind == "one_hub":
        for deg in (3, 0, 40, 100, 17, 1, 39):
            rows.append(_sorted_cols(rng, deg))
    elif kind == "dup":
        # repeated columns (the raw multigraph keeps duplicates): segments longer than a partition of the companion
        for deg in (5, 700, 0, 41, 420, 30):
            rows.append(np.sort(rng.choice(np.r_[0:40, 130:150, 640:700], deg, replace=True)))
    else:
        raise ValueError(kind)
    deg = np.asarray([r.size for r in rows], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    val = rng.standard_normal(col.size).astype(F32)
    return rowptr, col, val, notes


def replay_plan(rowptr, col, w, x, desc, long_row, long_slot0, n_rows, skip=None):
    """Raw float32 row sums of one gcr_spmm_csr_f32 launch in the kernel's order (tests/test_spmm_pipeline_gpu.py): per
    partition the non-zeros of a row (or chunk) in stored order, one fma each from 0; chunk partials of a split row summed
    per wave (chunks v, v+4, ...) and the four wave sums added in wave order.  Returns (raw [n_rows, d], covered bool [nnz]);
    rows in `skip` must not appear in the plan."""
    d = x.shape[1]
    seg_a, seg_b, seg_row, seg_slot = [], [], [], []
    for a, b, rowinfo, slot in np.asarray(desc).tolist():
        row0, nrows = rowinfo & 0xFFFFFFFF, rowinfo >> 32
        if slot < 0:
            for r in range(row0, row0 + nrows):
                seg_a.append(rowptr[r]); seg_b.append(rowptr[r + 1]); seg_row.append(r); seg_slot.append(-1)
        else:
            seg_a.append(a); seg_b.append(b); seg_row.append(row0); seg_slot.append(slot)
    seg_a, seg_b = np.asarray(seg_a, np.int64), np.asarray(seg_b, np.int64)
    seg_row, seg_slot = np.asarray(seg_row, np.int64), np.asarray(seg_slot, np.int64)
    if skip is not None and seg_row.size:
        assert not np.isin(seg_row, skip).any(), "a skipped row has a partition"
    seg_of = np.repeat(np.arange(seg_a.size), seg_b - seg_a)
    e_all = np.concatenate([np.arange(a, b) for a, b in zip(seg_a, seg_b)] + [np.zeros(0, np.int64)]).astype(np.int64)
    covered = np.zeros(col.size, np.int64)
    np.add.at(covered, e_all, 1)
    assert covered.max(initial=0) <= 1, "a non-zero is in two partitions"
    first = np.searchsorted(seg_of, np.arange(seg_a.size))
    rank = np.arange(e_all.size) - first[seg_of]
    acc = np.zeros((seg_a.size, d), F32)
    for k in range(int(rank.max()) + 1 if rank.size else 0):
        sel = rank == k
        s, e = seg_of[sel], e_all[sel]
        acc[s] = fma32(w[e][:, None], x[col[e]], acc[s])
    raw = np.zeros((n_rows, d), F32)
    whole = seg_slot < 0
    raw[seg_row[whole]] = acc[whole]
    n_slots = int(long_slot0[-1]) if len(long_row) else 0
    partial = np.zeros((max(n_slots, 1), d), F32)
    partial[seg_slot[~whole]] = acc[~whole]
    for i in range(len(long_row)):
        raw[long_row[i]] = wave_sums(partial, range(long_slot0[i], long_slot0[i + 1]))
    return raw, covered.astype(bool)


def wave_sums(partial, slots):
    """((s0 + s1) + s2) + s3 with s_v = the partials at slots[v], slots[v + 4], ... added in that order from 0."""
    slots = list(slots)
    waves = []
    for v in range(4):
        t = np.zeros(partial.shape[1], F32)
        for s in slots[v::4]:
            t = t + partial[s]
        waves.append(t)
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def replay_windowed(graph, rowptr, col, w, x):
    """Raw row sums of a windowed launch: the companion's partials (segment sums from 0 in stored order), per-wave window
    sums of every hub row, the four wave sums in wave order; every other row from the main plan."""
    hub, H = graph.hub, graph.hub.H
    n_rows = rowptr.size - 1
    pl = hub.main
    raw, cov_main = replay_plan(rowptr, col, w, x, pl.desc_host, pl.long_row.cpu().numpy()[: pl.n_long],
                                pl.long_slot0.cpu().numpy(), n_rows, skip=hub.hub_row_host)
    h_rowptr, h_col = H.rowptr.cpu().numpy(), H.col.cpu().numpy()
    h_w = np.ones(h_col.size, F32) if H.val is None else H.val.cpu().numpy()
    part, cov_h = replay_plan(h_rowptr, h_col, h_w, x, H.plan.desc_host, H.plan.long_row.cpu().numpy()[: H.plan.n_long],
                              H.plan.long_slot0.cpu().numpy(), H.n_rows)
    assert cov_h.all()
    is_hub = np.zeros(n_rows, bool)
    is_hub[hub.hub_row_host] = True
    assert np.array_equal(cov_main, ~np.repeat(is_hub, np.diff(rowptr))), "main plan + companion must cover every non-zero once"
    for h, r in enumerate(hub.hub_row_host):
        raw[r] = wave_sums(part, [wd * hub.n_hub + h for wd in range(hub.n_windows)])
    return raw
