"""Graphs shared by tests/test_spmm_fused_gpu.py and tests/test_spmm_fused_plan_cpu.py: the four kinds of
tests/spmm_window_common.make_matrix and three small graphs that put the one-launch windowed SpMM (gcr_spmm_windowed_f32) on
the paths those four do not take."""
import numpy as np

from spmm_window_common import F32, HUB_MIN_DEGREE, N_COLS, WINDOW_ROWS, make_matrix

KINDS = ("base", "empty_window", "one_hub", "dup")
CASES = KINDS + ("all_hub", "main_split", "odd_counts")
ODD_COPIES = 7                       # copies of `base` in odd_counts: see the counts asserted in the tests
NARROW = np.r_[0:40, 130:150, 640:700]     # the column pool of the `dup` kind: long segments in three windows


def _csr(rows, rng):
    deg = np.asarray([r.size for r in rows], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    return rowptr, col, rng.standard_normal(col.size).astype(F32)


def case_matrix(case):
    """(rowptr, col, val, keywords of CsrGraph)."""
    kw = dict(hub_window_rows=WINDOW_ROWS, hub_min_degree=HUB_MIN_DEGREE)
    if case in KINDS:
        return make_matrix(case)[:3] + (kw,)
    rng = np.random.default_rng(4000 + sum(map(ord, case)))
    if case == "all_hub":
        # every row is a hub: the main plan has no partition and its range of the grid is empty
        rows = [np.sort(rng.choice(N_COLS, k, replace=False)) for k in (41, 300, 77, 700, 120)]
        return _csr(rows, rng) + (kw,)
    if case == "main_split":
        # partitions of 64 non-zeros, hubs above 200: rows of 65 .. 200 non-zeros are split rows of the MAIN plan, and the
        # two rows with repeated columns have segments longer than a partition of the companion (128)
        rows = [np.sort(rng.choice(N_COLS, k, replace=False)) for k in (3, 100, 150, 64, 65, 0, 199, 700, 250, 12, 130,
                                                                         5, 7, 2, 9, 1, 4, 70)]
        rows += [np.sort(rng.choice(NARROW, k, replace=True)) for k in (500, 610)]
        return _csr(rows, rng) + (dict(hub_window_rows=WINDOW_ROWS, hub_min_degree=200, nnz_per_part=64),)
    if case == "odd_counts":
        mats = [make_matrix("base", seed=s) for s in range(ODD_COPIES)]
        deg = np.concatenate([np.diff(m[0]) for m in mats])
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        return rowptr, np.concatenate([m[1] for m in mats]), np.concatenate([m[2] for m in mats]), dict(kw, nnz_per_part=64)
    raise ValueError(case)


def build_graph(case, has_val, device):
    import recommendation_amd as ra
    rowptr, col, val, kw = case_matrix(case)
    g = ra.CsrGraph(rowptr, col, val if has_val else None, rowptr.size - 1, N_COLS, device, **kw)
    assert g.hub is not None
    return g


def companion_plan(g, case):
    """The companion's plan a case runs with: the graph's own (laid out per XCD, so a multiple of 8 blocks) except in
    odd_counts, where it is the same partitions in row order, without the padding."""
    from recommendation_amd.graph import SpmmPlan
    H = g.hub.H
    if case != "odd_counts":
        return H.plan
    return SpmmPlan(H.rowptr_host, H.device, H.plan.nnz_per_part)
