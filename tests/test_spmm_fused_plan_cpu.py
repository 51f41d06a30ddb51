"""graph.long_rows_first_order / SpmmPlan.permuted (host only): the order of `HubPlan.main`'s descriptors is a permutation of
the same partitions, few-row partitions first, and the split rows' tables are left alone."""
import numpy as np
import pytest

from spmm_fused_common import CASES, build_graph


@pytest.mark.parametrize("case", CASES)
def test_long_rows_first_is_a_stable_permutation_and_keeps_the_split_rows(case):
    from recommendation_amd.graph import long_rows_first_order
    main = build_graph(case, True, "cpu").hub.main
    order = long_rows_first_order(main.desc_host)
    assert np.array_equal(np.sort(order), np.arange(main.n_parts))
    q = main.permuted(order)
    nrows = q.desc_host[:, 2] >> 32
    assert (np.diff(nrows) >= 0).all(), "not ascending by rows per partition"
    ties = np.diff(nrows) == 0
    assert (np.diff(order)[ties] > 0).all(), "not stable"
    # the same descriptors, each with its own slot: as a multiset of rows
    assert np.array_equal(np.sort(q.desc_host.view("i8,i8,i8,i8").ravel()), np.sort(main.desc_host.view("i8,i8,i8,i8").ravel()))
    assert np.array_equal(q.desc.numpy()[: q.n_parts], q.desc_host)
    chunks = q.desc_host[:, 3] >= 0
    assert np.array_equal(np.sort(q.desc_host[chunks, 3]), np.arange(main.n_slots)), "a split row's slot moved"
    assert (q.n_parts, q.n_long, q.n_slots) == (main.n_parts, main.n_long, main.n_slots)
    assert q.long_row is main.long_row and q.long_slot0 is main.long_slot0
    if case == "main_split":
        # a chunk counts as one row: the chunks lead together with the one-row partitions, ahead of every other one
        assert main.n_long > 0 and (nrows[chunks] == 1).all() and (nrows > 1).any()
        assert np.flatnonzero(chunks).max() < np.flatnonzero(nrows > 1).min(), "the chunks of split rows do not lead"


def test_a_non_permutation_is_refused():
    main = build_graph("base", True, "cpu").hub.main
    with pytest.raises(ValueError):
        main.permuted(np.zeros(main.n_parts, dtype=np.int64))


def test_the_default_plan_keeps_plan_order_and_puts_the_main_range_first():
    from recommendation_amd import graph as G
    assert G.HUB_MAIN_FIRST is True and G.HUB_MAIN_LONG_ROWS_FIRST is False
    hub = build_graph("odd_counts", True, "cpu").hub
    assert hub.main_first is True
    assert (np.diff(hub.main.desc_host[:, 0]) >= 0).all()
