"""The launch geometry that the large-shape GPU cases rely on, asserted on the host: csrc/gcr_tri.hip's `splits_for` /
`tri_layout` and csrc/gcr_mim.hip's `mim_blocks` / `mim_layout` restated in Python for every shape of
tests/test_tri_gpu.py (`rows_for(MAX_K)`, `SPLIT_CASES`) and tests/test_mim_gpu.py (`FOLD_CASES`):

  (a) the restated split count / workgroup count / rows per workgroup are the ones the case tables name;
  (b) the restated workspace size is what gcr_tri_workspace_bytes / gcr_mim_workspace_bytes return — both layouts depend on
      the split and workgroup counts, so equality pins the restatement to the library;
  (c) the waves and workgroups wanted lie on the intended side of each grid cap.

A constant retuned in a kernel file fails this test at the GPU case that no longer reaches its branch.  The workspace
functions are host-only: no device is touched here.

csrc/gcr_bpr.hip's geometry for tests/test_bpr_paths_gpu.py (`WIDTHS`, `BATCH_EDGES`, `TRIPS`): `fwd_blocks` is pinned to the
library through gcr_bpr_workspace_floats (five partials per block); the atomic backward's grid cap and the sorted kernels'
chunk and gather-group sizes are restated only — no workspace function exposes them, so these restatements are NOT pinned to
the library and a retuned constant there has to be carried over here by hand."""
import os

import pytest

# the case tables are read from the GPU test modules themselves, so the shapes asserted here are the shapes run there.  Those
# modules must stay importable without a device: nothing at their module level may touch one (their tests are marked gpu)
import test_bpr_paths_gpu as bpr
import test_mim_gpu as mim
import test_ssl4rec_gpu as drop
import test_tri_gpu as tri

TILE, MAX_SPLITS, ROW_BLOCKS = 32, 8, 8192                 # gcr_tri.hip: kTile, kMaxSplits, row_blocks()'s cap (4 waves each)
MIM_MAX_BLOCKS, MIM_BWD_BLOCKS = 1024, 16384               # gcr_mim.hip: kMaxBlocks, the grid cap of mim_bwd_kernel
FOLD_LOADS, WAVE = 16, 64                                  # gcr_mim.hip: kFoldLoads, the lanes of the loss fold
DROPOUT_BLOCKS = 8192                                      # gcr_dropout.hip: dropout_grid()'s cap (4 rows each)
BPR_FWD_GROUPS, BPR_FWD_BLOCKS = 16, 4096                  # gcr_bpr.hip: kGroups (samples per block), fwd_blocks()'s cap
# gcr_bpr.hip, NOT pinned to the library (no workspace function depends on them): a retuned constant must be restated here
BPR_BWD_BLOCKS, BPR_BWD_WAVES = 8192, 4                    # gcr_bpr_bwd_f32's grid cap, one sample per wave
BPR_CHUNK = 64                                             # entries a wave of the sorted kernels walks
BPR_GATHER_SORTED = {1: 8, 2: 4, 3: 4, 4: 4}               # kGather of bpr_bwd_sorted_kernel by NV
BPR_GATHER_NEG_ITEMS = {1: 16, 2: 8, 3: 8, 4: 8}           # kGather of bpr_neg_items_sorted_kernel by NV
BPR_SORTED_BLOCKS = 65536                                  # grid cap of the sorted, neg-block and edge-values kernels


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


def bpr_fwd_blocks(batch):
    return max(1, min(BPR_FWD_BLOCKS, ceil_div(batch, BPR_FWD_GROUPS)))


def bpr_nv(d):
    return ceil_div(d, 64)


def bpr_batches():
    return sorted({bpr.WIDTH_BATCH, bpr.PATTERN_BATCH} | {c[1] for c in bpr.BATCH_EDGES} | {t[0] for t in bpr.TRIPS})


def test_bpr_forward_blocks_are_the_librarys(lib):
    """gcr_bpr_workspace_floats is five partial sums per forward block: equality pins `bpr_fwd_blocks` to fwd_blocks()."""
    for batch in bpr_batches() + [0, 16 * 4096, 16 * 4096 + 1, 2_000_000]:
        assert lib.gcr_bpr_workspace_floats(batch) == 5 * bpr_fwd_blocks(batch), batch
    assert bpr_fwd_blocks(16 * 4096) == 4096 == bpr_fwd_blocks(16 * 4096 + 1)


def test_bpr_trips_lie_past_the_cap_they_name():
    fwd_cap, bwd_cap = BPR_FWD_GROUPS * BPR_FWD_BLOCKS, BPR_BWD_WAVES * BPR_BWD_BLOCKS
    assert (fwd_cap, bwd_cap) == (65536, 32768)
    for batch, path, variant, trip in bpr.TRIPS:
        assert path in bpr.SUMS_PATHS and trip in ("fwd", "bwd")
        if trip == "bwd":                                      # the atomic backward alone: the forward still takes one trip
            assert path == "atomic" and bwd_cap < batch <= fwd_cap
        else:
            assert batch > fwd_cap and ceil_div(batch, BPR_FWD_GROUPS) > BPR_FWD_BLOCKS
        assert 0 < batch % bwd_cap < 16                        # the last trip has few samples: most waves and groups idle
        # the sorted kernels' cap is out of reach of a quick test: one trip covers 16 M entries
        assert ceil_div(ceil_div(batch, BPR_CHUNK), 4) <= BPR_SORTED_BLOCKS and ceil_div(batch, 256) <= BPR_SORTED_BLOCKS
    assert {t[3] for t in bpr.TRIPS} == {"fwd", "bwd"}
    assert {t[1] for t in bpr.TRIPS if t[3] == "fwd"} == {"atomic", "sorted_payload"}
    assert BPR_SORTED_BLOCKS * 4 * BPR_CHUNK == 1 << 24
    # every other table stays within one trip of every kernel
    assert max(b for b in bpr_batches() if b not in {t[0] for t in bpr.TRIPS}) <= min(fwd_cap, bwd_cap)


def test_bpr_batch_edges_lie_where_the_table_says():
    """Each row names a unit (a gather group of one of the two sorted kernels at the row's NV, or the 64-entry chunk), a
    multiple k and an offset: batch = k * unit + off, off in -1, 0, +1 (the single-sample batch: +1 past zero)."""
    seen = {}
    for d, batch, n_neg, unit, k, off in bpr.BATCH_EDGES:
        nv = bpr_nv(d)
        assert unit in (BPR_GATHER_SORTED[nv], BPR_GATHER_NEG_ITEMS[nv], BPR_CHUNK), (d, unit)
        assert batch == k * unit + off and off in (-1, 0, 1) and batch >= 1
        seen.setdefault((nv, unit), set()).add(off)
    assert seen[(1, 8)] == seen[(1, 16)] == seen[(1, 64)] == seen[(2, 4)] == {-1, 0, 1}
    assert 1 in seen[(2, 64)]
    # NV = 2's group of 8 in bpr_neg_items_sorted_kernel is met by the negatives' batch * n_neg entries
    slots = {batch * n_neg for d, batch, n_neg, *_ in bpr.BATCH_EDGES if d == 100}
    assert {BPR_GATHER_NEG_ITEMS[2] - 2, BPR_GATHER_NEG_ITEMS[2], BPR_GATHER_NEG_ITEMS[2] + 2} <= slots
    # both ONE_NEG branches at d = 64; a last chunk that is full, one entry long and one short of full
    assert {n for d, _, n, *_ in bpr.BATCH_EDGES if d == 64} == {1, 3}
    assert {batch % BPR_CHUNK for _, batch, *_ in bpr.BATCH_EDGES} >= {0, 1, BPR_CHUNK - 1}
    # the straddling run of PATTERNS: entries 60 .. 69 of the sorted order cross the first chunk boundary
    assert 60 < BPR_CHUNK < 70 and bpr.PATTERN_BATCH == 4 * BPR_CHUNK + 1


def test_bpr_widths_reach_every_template():
    cases = bpr.width_cases()
    assert [c[0] for c in cases] == list(bpr.WIDTHS) and all(1 <= d <= 256 for d in bpr.WIDTHS)
    pairs = {(d % 4 == 0, bpr_nv(d)) for d in bpr.WIDTHS}
    assert pairs == {(vec4, nv) for vec4 in (True, False) for nv in (1, 2, 3, 4)}
    for nv in (1, 2, 3, 4):
        n_negs = {n_neg for d, _, n_neg in cases if bpr_nv(d) == nv}
        assert 1 in n_negs and max(n_negs) > 1, nv                 # ONE_NEG true and false
        assert 64 * nv in bpr.WIDTHS                               # every lane of the last column group live
    assert {bpr_nv(d) for d in bpr.WIDTHS if d % 64} == {1, 2, 3, 4}   # a last column group that is partly masked
    assert {v for _, v, _ in cases} == {0, 1, 2}
    assert set(bpr.EDGE_WIDTHS) <= set(bpr.WIDTHS) and {bpr_nv(d) for d in bpr.EDGE_WIDTHS} == {1, 3}
