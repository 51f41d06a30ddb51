"""The workspace size queries of the all-pairs kernels (csrc/gcr_pairs.h: one launch plan per family, shared by the launcher
and the query) against tests/golden/pairs_workspace.json, recorded by scripts/gen_pairs_workspace_golden.py from the commit
before the plans existed: the sizes callers see are what they were, for every width, for empty problems, for every shape of
the case tables of tests/test_infonce_gpu.py and tests/test_bce_gpu.py, and for shapes on both sides of each branch of
plan_fwd / plan_bwd_rows.  Those branch conditions are restated here (as in tests/test_launch_geometry_cpu.py) so that the
shapes are known to reach them.  The queries are host-only: no device is touched."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("gen_pairs_workspace_golden",
                                               os.path.join(ROOT, "scripts", "gen_pairs_workspace_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

TILE = 32                                                  # gcr_tile.h: kTileJ
CUS = 256                                                  # gcr_pairs.h: kCUs (resident_blocks(n) = n workgroups per CU)
EIGHT_WAVE_TILES = 256                                     # gcr_pairs.h: kEightWaveTiles


@pytest.fixture(scope="module")
def lib():
    from recommendation_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    with open(gen.GOLDEN) as f:
        return json.load(f)


def ceil_div(a, b):
    return -(-a // b)


def plan_fwd(m, n, rows_per_block, resident):
    """gcr_pairs.h plan_fwd -> (nsplit, tiles_per_split, m_blocks, branch taken, whether the 16-tile floor cut it)"""
    m_blocks, tiles = ceil_div(m, rows_per_block), ceil_div(n, TILE)
    if 2 * m_blocks <= resident:
        nsplit, branch = resident // m_blocks, "one_wave"
    else:
        nsplit, branch = ceil_div(tiles, 320), "320_tiles"
        if m_blocks * nsplit < 3 * resident:
            nsplit, branch = ceil_div(3 * resident, m_blocks), "three_rounds"
    floored = nsplit > max(tiles // 16, 1)
    nsplit = min(nsplit, max(tiles // 16, 1))
    nsplit = max(1, min(nsplit, tiles))
    per = ceil_div(tiles, nsplit)
    return max(1, ceil_div(tiles, per)), per, m_blocks, branch, floored


def plan_bwd_rows(mx, ny, d, rows_per_block, resident):
    """gcr_pairs.h plan_bwd_rows -> (nsplit, tiles_per_split, m_blocks, halvings by row blocks, halvings by bytes)"""
    nsplit, per, m_blocks, _, _ = plan_fwd(mx, ny, rows_per_block, resident)
    tiles, by_blocks, by_bytes = ceil_div(ny, TILE), 0, 0
    while nsplit > 1 and (m_blocks >= 3 * resident or nsplit * mx * d * 4 > 1 << 30):
        by_blocks += m_blocks >= 3 * resident
        by_bytes += m_blocks < 3 * resident
        per *= 2
        nsplit = ceil_div(tiles, per)
    return nsplit, per, m_blocks, by_blocks, by_bytes


def test_sizes_are_the_recorded_ones(lib, golden):
    assert tuple(golden["exports"]) == gen.SIZE_EXPORTS
    rows = golden["sizes"]
    for m, n, d, *want in rows:
        got = [getattr(lib, name)(m, n, d) for name in gen.SIZE_EXPORTS]
        assert got == want, (m, n, d)
    # nothing is trivially equal: every export is non-zero somewhere, and zero for empty problems and the unsupported width
    assert all(any(r[3 + k] > 0 for r in rows) for k in range(len(gen.SIZE_EXPORTS)))
    assert all(r[3:] == [0] * 5 for r in rows if r[0] == 0 or r[1] == 0 or r[2] == gen.UNSUPPORTED)
    assert {r[2] for r in rows} >= set(gen.WIDTHS) | {gen.UNSUPPORTED}
    assert {(0, 100), (100, 0), (0, 0)} <= {(r[0], r[1]) for r in rows}


def test_fwd_o_supported_is_the_recorded_one(lib, golden):
    assert len(golden["fwd_o_supported"]) == len(gen.FLAGS) * (len(gen.WIDTHS) + 1)
    for d, flags, want in golden["fwd_o_supported"]:
        assert lib.gcr_infonce_fwd_o_supported(d, flags) == want, (d, flags)
    assert {w for _, _, w in golden["fwd_o_supported"]} == {0, 1}


def test_recorded_shapes_cover_the_gpu_case_tables(golden):
    """A shape added to a GPU case table has to be recorded too (rerun the generator on a build whose sizes are trusted)."""
    have = {tuple(r[:3]) for r in golden["sizes"]}
    assert set(gen.cases()) <= have
    assert len(gen.table_shapes()) >= 150
    assert {(1, 1, 64), (130, 4097, 32), (50, 300, 48), (40, 90, 100), (40, 90, 128), (70, 40000, 64), (1280, 2, 32),
            (257, 1682, 256), (130, 4100, 48), (1025, 1025, 128), (2000, 300_000, 64), (2348, 600_011, 64)} <= have
    # shapes built in test bodies, in both orientations (the gradient of the other side swaps the roles)
    assert gen.body_shapes() <= have
    assert {(45, 1, 64), (45, 1025, 64), (1025, 45, 64), (1 << 15, 4096, 64), (4096, 1 << 15, 64), (70, 300, 64), (23, 25, 64),
            (89, 57, 128), (57, 90, 32), (943, 1682, 64), (900, 70, 64)} <= have


def test_branch_shapes_reach_the_branches_they_name():
    B = gen.BRANCH_SHAPES
    two, one = 2 * CUS, CUS
    # plan_fwd on the split-operand lse forward at d = 64: 256 anchors per workgroup, two workgroups per CU
    assert plan_fwd(*B["one_resident_wave"][:2], 256, two) == (250, 25, 2, "one_wave", False)
    assert plan_fwd(*B["one_resident_wave_cut_by_the_floor"][:2], 256, two) == (9, 18, 2, "one_wave", True)
    assert 2 * ceil_div(B["one_resident_wave"][0], 256) <= two
    assert plan_fwd(*B["many_row_blocks_320_tiles"][:2], 256, two) == (10, 313, 391, "320_tiles", False)
    assert plan_fwd(*B["many_row_blocks_three_rounds"][:2], 256, two) == (6, 105, 274, "three_rounds", False)
    m, n, _ = B["floor_16_tiles_per_split"]
    assert n < 512 and plan_fwd(m, n, 256, two) == (1, 16, 2, "one_wave", True)
    assert plan_fwd(m, 512, 256, two)[0] == 1 and plan_fwd(m, 1024, 256, two)[0] == 2
    # plan_bwd_rows at 128 rows per workgroup: the halving loop by row blocks ...
    mx, ny, d = B["halving_by_row_blocks"]
    assert mx == 196_608 == 3 * two * 128
    nsplit, per, m_blocks, by_blocks, by_bytes = plan_bwd_rows(mx, ny, d, 128, two)
    assert m_blocks >= 3 * two and by_blocks >= 1 and by_bytes == 0 and nsplit == 1
    assert plan_fwd(mx, ny, 128, two)[0] > 1                                     # there was something to halve
    mx, ny, d = B["below_halving_by_row_blocks"]
    nsplit, per, m_blocks, by_blocks, by_bytes = plan_bwd_rows(mx, ny, d, 128, two)
    assert m_blocks == 3 * two - 1 and (by_blocks, by_bytes) == (0, 0) and nsplit > 1
    # ... and by the 1 GiB cap on the partials
    mx, ny, d = B["halving_by_partial_bytes"]
    nsplit, per, m_blocks, by_blocks, by_bytes = plan_bwd_rows(mx, ny, d, 128, two)
    assert m_blocks < 3 * two and by_blocks == 0 and by_bytes >= 1
    assert plan_fwd(mx, ny, 128, two)[0] * mx * d * 4 > 1 << 30 >= nsplit * mx * d * 4
    # the 512-thread lse forward: d = 64, m >= 512 anchors, >= 256 tiles per split of plan_fwd(512 anchors, one per CU)
    for name, m_ok, tiles_ok in (("eight_waves_lse", True, True), ("eight_waves_lse_256_tiles", True, True),
                                 ("eight_waves_lse_255_tiles", True, False), ("eight_waves_lse_511_anchors", False, True),
                                 ("eight_waves_lse_512_anchors", True, True)):
        m, n, d = B[name]
        per = plan_fwd(m, n, 512, one)[1]
        assert d == 64 and (m >= 512) == m_ok and (per >= EIGHT_WAVE_TILES) == tiles_ok, (name, per)
    assert plan_fwd(*B["eight_waves_lse_256_tiles"][:2], 512, one)[1] == 256
    assert plan_fwd(*B["eight_waves_lse_255_tiles"][:2], 512, one)[1] == 255
    # the 512-thread flash forward: d = 64, >= 256 tiles per split of plan_bwd_rows(256 rows, one per CU)
    assert plan_bwd_rows(*B["eight_waves_flash"], 256, one)[1] == 293
    assert plan_bwd_rows(*B["eight_waves_flash_256_tiles"], 256, one)[1] == 256
    assert plan_bwd_rows(*B["eight_waves_flash_255_tiles"], 256, one)[1] == 255
    assert B["eight_waves_lse"] == (2348, 600_011, 64) and B["eight_waves_flash"] == (2000, 300_000, 64)


def test_restated_plans_are_the_librarys(lib):
    """The restatement above is pinned to the library where a size is a plain function of one plan: the flash forward at
    d = 128 has a single path (plan_bwd_rows at 128 rows), nsplit * m * (8 + 4 d) bytes; the backward at d = 256 a single
    path too (128 rows per workgroup), nsplit * mx * d * 4 bytes past one split."""
    for m, n, d in gen.cases():
        if m <= 0 or n <= 0:
            continue
        nsplit = plan_bwd_rows(m, n, 128, 128, 2 * CUS)[0]
        assert lib.gcr_infonce_fwd_o_workspace_bytes(m, n, 128) == nsplit * m * (8 + 4 * 128), (m, n)
        nsplit = plan_bwd_rows(m, n, 256, 128, 2 * CUS)[0]
        assert lib.gcr_infonce_bwd_workspace_bytes(m, n, 256) == (nsplit * m * 256 * 4 if nsplit > 1 else 0), (m, n)
