"""The launch geometry that tests/test_bt_gpu.py's shapes rely on, asserted on the host: csrc/gcr_bt.hip's `bt_blocks` /
`bt_rows` (the product launch) and `stat_blocks` (the statistics launch) restated in Python for every (n, d) run there.

  (a) the restated workspace size is what gcr_bt_workspace_bytes / gcr_col_stats_workspace_bytes return: the layout holds
      one d x d partial per product workgroup and one (mean, M2) pair per statistics workgroup and view, so equality pins
      both restated workgroup counts to the library;
  (b) the shapes lie on both sides of the single-workgroup boundary and of each grid cap, and include the odd tails, the
      single-row last workgroup and the empty trailing workgroup that the even rows-per-workgroup rounding can leave.

The backward's grid (one workgroup per tile of 32 x RT rows, capped) is restated only: no workspace depends on it.
The workspace functions are host-only: no device is touched here."""
import os

import pytest

import test_bt_gpu as bt

MIN_ROWS = 256                                               # rows a workgroup takes before another is added
CAP, CAP_256 = 1024, 256                                     # bt_blocks()'s caps (d <= 128, d = 256: times four quadrants)
STAT_CAP = 1024                                              # stat_blocks()'s cap
LOSS_PARTS = 1024                                            # kBtLossParts
BWD_ROWS = {32: 128, 64: 64, 96: 32, 128: 32, 256: 32}       # rows per tile of bt_bwd_kernel (32 x waves / (d / 32))
BWD_CAP = {32: 1024, 64: 1024, 96: 1024, 128: 1024, 256: 512}


@pytest.fixture(scope="module")
def lib():
    from recommendation_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib.lib()


def ceil_div(a, b):
    return -(-a // b)


def bt_blocks(n, d):
    return max(1, min(CAP_256 if d == 256 else CAP, ceil_div(n, MIN_ROWS)))


def bt_rows(n, nb):
    return max(MIN_ROWS, (ceil_div(n, nb) + 1) & ~1)          # below the cap: whole chunks of 256, the last one short


def stat_blocks(n):
    return max(1, min(STAT_CAP, ceil_div(n, MIN_ROWS)))


def workspace_floats(n, d):
    return bt_blocks(n, d) * d * d + 2 * stat_blocks(n) * 2 * d + LOSS_PARTS + 2 * d * d + 4 * d


def test_restated_geometry_is_the_librarys(lib):
    for n, d in bt.ALL_SHAPES:
        assert lib.gcr_bt_workspace_bytes(n, d) == 4 * workspace_floats(n, d), (n, d)
        assert lib.gcr_col_stats_workspace_bytes(n, d) == 4 * stat_blocks(n) * 2 * d, (n, d)
        nb = bt_blocks(n, d)
        per = bt_rows(n, nb)
        assert per % 2 == 0 and nb * per >= n                       # the workgroups cover every row, pairs never straddle
    assert lib.gcr_bt_workspace_bytes(513, 48) == 0 and lib.gcr_bt_workspace_bytes(0, 64) == 0
    assert lib.gcr_col_stats_workspace_bytes(513, 1024) == 4 * 3 * 2 * 1024
    assert lib.gcr_col_stats_workspace_bytes(513, 1028) == 0 and lib.gcr_col_stats_workspace_bytes(513, 50) == 0


def test_shapes_lie_on_both_sides_of_every_boundary():
    for d in bt.WIDTHS:
        rows = [n for n, w in bt.ALL_SHAPES if w == d]
        cap = CAP_256 if d == 256 else CAP
        assert any(bt_blocks(n, d) == 1 for n in rows) and any(1 < bt_blocks(n, d) < cap for n in rows), d
    for d, cap in ((32, CAP), (256, CAP_256)):                      # the capped launches: one narrow, the quadrant form
        rows = [n for n, w in bt.ALL_SHAPES if w == d]
        assert any(ceil_div(n, MIN_ROWS) > cap for n in rows) and any(ceil_div(n, MIN_ROWS) < cap for n in rows), d
        assert any(ceil_div(n, MIN_ROWS) > STAT_CAP for n in rows) or d == 256
    # n = 7: less than one unrolled group of eight row pairs, odd; n = 513: the last workgroup holds a single row
    assert (7, 32) in bt.SWEEP and bt_blocks(513, 64) == 3 and 513 - 2 * bt_rows(513, 3) == 1
    # the capped shapes have odd tails; 70001 rows at d = 256 leave the last workgroup short
    for n, d in bt.LARGE:
        nb = bt_blocks(n, d)
        assert n % 2 == 1 and nb == (CAP_256 if d == 256 else CAP) and n - (nb - 1) * bt_rows(n, nb) < bt_rows(n, nb)
    # the backward walks more than one tile per workgroup only above its own cap: reached at d = 32 and d = 256
    for d in (32, 256):
        assert any(ceil_div(n, BWD_ROWS[d]) > BWD_CAP[d] for n, w in bt.ALL_SHAPES if w == d)
        assert any(ceil_div(n, BWD_ROWS[d]) < BWD_CAP[d] for n, w in bt.ALL_SHAPES if w == d)
