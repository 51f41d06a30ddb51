"""The launch geometry that the large-shape GPU cases rely on, asserted on the host: csrc/gcr_tri.hip's `splits_for` /
`tri_layout` and csrc/gcr_mim.hip's `mim_blocks` / `mim_layout` restated in Python for every shape of
tests/test_tri_gpu.py (`rows_for(MAX_K)`, `SPLIT_CASES`) and tests/test_mim_gpu.py (`FOLD_CASES`):

  (a) the restated split count / workgroup count / rows per workgroup are the ones the case tables name;
  (b) the restated workspace size is what gcr_tri_workspace_bytes / gcr_mim_workspace_bytes return — both layouts depend on
      the split and workgroup counts, so equality pins the restatement to the library;
  (c) the waves and workgroups wanted lie on the intended side of each grid cap.

A constant retuned in a kernel file fails this test at the GPU case that no longer reaches its branch.  The workspace
functions are host-only: no device is touched here."""
import os

import pytest

# the case tables are read from the GPU test modules themselves, so the shapes asserted here are the shapes run there.  Those
# modules must stay importable without a device: nothing at their module level may touch one (their tests are marked gpu)
import test_mim_gpu as mim
import test_ssl4rec_gpu as drop
import test_tri_gpu as tri

TILE, MAX_SPLITS, ROW_BLOCKS = 32, 8, 8192                 # gcr_tri.hip: kTile, kMaxSplits, row_blocks()'s cap (4 waves each)
MIM_MAX_BLOCKS, MIM_BWD_BLOCKS = 1024, 16384               # gcr_mim.hip: kMaxBlocks, the grid cap of mim_bwd_kernel
FOLD_LOADS, WAVE = 16, 64                                  # gcr_mim.hip: kFoldLoads, the lanes of the loss fold
DROPOUT_BLOCKS = 8192                                      # gcr_dropout.hip: dropout_grid()'s cap (4 rows each)


@pytest.fixture(scope="module")
def lib():
    from recommendation_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib.lib()


def ceil_div(a, b):
    return -(-a // b)


def align64(x):
    return (x + 63) & ~63


def splits_for(n_tiles):
    return max(1, min(MAX_SPLITS, n_tiles, ceil_div(256, n_tiles)))


def tri_workspace_bytes(m, d, k, ns=None):
    """tri_layout().total in bytes: every array padded to 64 four-byte words."""
    ns = splits_for(ceil_div(m, TILE)) if ns is None else ns
    words = (align64(4 * m * d) + align64(4 * m)                       # xhat, inv_norm
             + align64(ns * 3 * m) + align64(2 * ns * 3 * m) + align64(3 * m)      # z1, zt (doubles), row_loss
             + 2 * align64(3 * m * 2 * ns * k)                         # cand_val, cand_col
             + 2 * align64(ns * 3 * m * d))                            # part_e, part_a
    return 4 * words


def mim_blocks(n):
    return max(1, min(MIM_MAX_BLOCKS, ceil_div(n, 256)))


def mim_workspace_bytes(n, d):
    """mim_layout().total: 64 bytes of tickets, then every array padded to 64 bytes."""
    nb = mim_blocks(n)
    return 64 + 2 * align64(nb * d * 8) + align64(nb * 8) + align64(3 * n * 8)


def test_tri_cases_reach_the_split_counts_they_name(lib):
    cases = [(m, d, k, ns) for m, d, k, ns in tri.SPLIT_CASES]
    cases += [(m, d, tri.MAX_K, ns) for d in tri.WIDTHS for m, ns in zip(tri.rows_for(tri.MAX_K), (1, 2, 4, 8))]
    assert tri.rows_for(tri.MAX_K) == [32, 33, 97, 257]
    for m, d, k, ns in cases:
        tiles = ceil_div(m, TILE)
        assert splits_for(tiles) == ns, (m, tiles)
        assert lib.gcr_tri_supported(d, k)
        assert tri_workspace_bytes(m, d, k) == lib.gcr_tri_workspace_bytes(m, d, k), (m, d, k)
        # the layout does depend on the split count: one split more or fewer is another size
        assert all(tri_workspace_bytes(m, d, k, other) != tri_workspace_bytes(m, d, k) for other in (ns - 1, ns + 1))
    # between them the old and the new shapes run every split count
    old = {splits_for(ceil_div(m, TILE)) for k in tri.KS for m in tri.rows_for(k)}
    assert old == {1, 2, 4, 8}
    assert old | {ns for _, _, _, ns in tri.SPLIT_CASES} == set(range(1, MAX_SPLITS + 1))
    # tiles per split: at most two in the old shapes, up to 342 here
    assert max(ceil_div(ceil_div(m, TILE), splits_for(ceil_div(m, TILE))) for k in tri.KS for m in tri.rows_for(k)) == 2
    per_split = {m: ceil_div(ceil_div(m, TILE), ns) for m, _, _, ns in tri.SPLIT_CASES}
    assert per_split == {1000: 4, 1100: 5, 1200: 6, 1500: 8, 2000: 13, 2100: 17, 2900: 31, 4100: 65, 10940: 342}
    assert ceil_div(1100, TILE) % 8 == 3                                           # uneven: 3 splits of 5 tiles, 5 of 4
    # k = 32 with 8 splits fills the finish kernel's 2 * kMaxSplits * kMaxK candidate slots per wave
    assert {k for m, _, k, ns in cases if ns == MAX_SPLITS} >= {tri.MAX_K} and tri.MAX_K == 32


def test_tri_grid_caps(lib):
    """row_blocks(): at most 8192 workgroups of four waves.  tri_prepare_kernel and tri_bwd_rows_kernel want 4 m waves,
    tri_finish_kernel 3 m: only the last case takes a second grid-stride trip, and it takes it in all three."""
    cap = 4 * ROW_BLOCKS
    assert cap == 32768
    big = max(m for m, _, _, _ in tri.SPLIT_CASES)
    assert big == 10940
    assert 3 * big > cap and 4 * big > cap
    for m, _, _, _ in tri.SPLIT_CASES:
        if m != big:
            assert 4 * m <= cap
    assert 4 * max(tri.rows_for(tri.MAX_K)) <= cap


def test_mim_cases_reach_the_folds_they_name(lib):
    assert max(mim_blocks(n) for n in mim.ROWS) == 4
    for n, d, nb, per in mim.FOLD_CASES:
        assert mim_blocks(n) == nb and ceil_div(n, nb) == per, (n, d)
        assert (nb - 1) * per < n                                                   # the last workgroup has rows
        assert lib.gcr_mim_supported(d)
        assert mim_workspace_bytes(n, d) == lib.gcr_mim_workspace_bytes(n, d), (n, d)
    chain_len = {(n, d): ceil_div(nb, 256 // d) for n, d, nb, _ in mim.FOLD_CASES}
    assert chain_len[(4353, 256)] == 18 > FOLD_LOADS and 256 // 256 == 1            # one chain, a second batch of loads
    assert chain_len[(4353, 128)] == 9 and 256 // 128 == 2                          # two chains
    assert chain_len[(16641, 64)] == 17 > FOLD_LOADS and 256 // 64 == 4
    assert chain_len[(33025, 32)] == 17 > FOLD_LOADS and 256 // 32 == 8
    # the 64-lane loss fold: loads per lane
    assert ceil_div(66, WAVE) == 2 and 66 - WAVE == 2                               # lanes 0-1 load twice
    assert ceil_div(130, WAVE) == 3
    assert all(ceil_div(mim_blocks(n), WAVE) == 1 for n in mim.ROWS)


def test_mim_grid_caps(lib):
    for n, d, nb, per in mim.FOLD_CASES:
        capped = ceil_div(n, 256) > MIM_MAX_BLOCKS
        assert capped == (n == 263000) and (per > 256) == capped
        groups = 256 // (d // 4)
        assert (ceil_div(n, 2 * groups) > MIM_BWD_BLOCKS) == ((n, d) == (131080, 256)), (n, d)
    assert ceil_div(131080, 2 * 4) == MIM_BWD_BLOCKS + 1
    assert all(ceil_div(n, 256) <= MIM_MAX_BLOCKS and ceil_div(n, 2 * 256 // (d // 4)) <= MIM_BWD_BLOCKS
               for n in mim.ROWS for d in mim.WIDTHS)


def test_dropout_grid_cap():
    """dropout_grid(): one wave per batch row, four per workgroup, at most 8192 workgroups."""
    assert ceil_div(max(drop.NS), 4) <= DROPOUT_BLOCKS < ceil_div(drop.N_CAPPED, 4)
    assert drop.N_CAPPED == 4 * DROPOUT_BLOCKS + 37
