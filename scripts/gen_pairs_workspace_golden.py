#!/usr/bin/env python3
"""Writes tests/golden/pairs_workspace.json: what the host-only size queries of the all-pairs kernels (InfoNCE forward,
flash forward, backward; BCE forward, backward) return for the shapes of `cases()`, and gcr_infonce_fwd_o_supported for
every width and engine flag.  Only exports are called, so the script runs against any build of the library; the committed
file was recorded from the commit BEFORE the launch plans moved into one function per family, and
tests/test_pairs_workspace_cpu.py holds every later build to it.

    python scripts/gen_pairs_workspace_golden.py [--check]

`cases()` = every (m, n, d) of the case tables of tests/test_infonce_gpu.py and tests/test_bce_gpu.py (read from their
parametrize marks: a table without `d` runs at every width, one without `m` or `n` as a square problem), the shapes those
modules build in a test body, empty problems, an unsupported width, and the shapes that reach each branch of plan_fwd /
plan_bwd_rows (tests/test_pairs_workspace_cpu.py restates the branch conditions and names the shapes)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pairs_workspace.json")
WIDTHS = (32, 64, 128, 256)
UNSUPPORTED = 48
SIZE_EXPORTS = ("gcr_infonce_fwd_workspace_bytes", "gcr_infonce_fwd_o_workspace_bytes", "gcr_infonce_bwd_workspace_bytes",
                "gcr_bce_fwd_workspace_bytes", "gcr_bce_bwd_workspace_bytes")
FLAGS = (0, 1, 2, 3, 4, 7)                                  # GCR_INFONCE_EXCLUDE_DIAGONAL | ENGINE_F32 | UNIT_ROWS

# Shapes built inside test bodies, (stationary rows, streamed rows, d); body_shapes() adds each with the roles swapped, as
# the gradient of the other side runs it.  tests/test_infonce_gpu.py: the eight-wave test, the two-views test, the exponent-range
# test; test_every_tile_count_parity_forward_and_backward runs 45 anchors against its table of n (TILE_COUNT_M).
# tests/test_bce_gpu.py: the three score regimes, the rows far below zero, the golden tables (40 users x 25 items, and a
# batch of 23 gathered rows), the edge loss (90 users of which at most 89 have an edge, 57 items) and the cfg1 step.
TILE_COUNT_M = 45
BODY_SHAPES = [(2000, 300_000, 64), (2048 + 300, 600_011, 64), (50_000, 50_000, 64), (100_000, 100_000, 64), (70, 900, 64),
               (1 << 15, 4096, 64), (70, 300, 64), (40, 25, 64), (23, 25, 64), (943, 1682, 64)]
BODY_SHAPES += [(users, 57, d) for users in (89, 90) for d in (32, 64, 128)]

# name -> (m, n, d): one shape per branch of plan_fwd / plan_bwd_rows (the test asserts that each is where its name says)
BRANCH_SHAPES = {
    "one_resident_wave": (300, 200_000, 64),
    "one_resident_wave_cut_by_the_floor": (300, 5000, 64),
    "many_row_blocks_320_tiles": (100_000, 100_000, 64),
    "many_row_blocks_three_rounds": (70_000, 20_000, 64),
    "floor_16_tiles_per_split": (300, 511, 64),
    "halving_by_row_blocks": (196_608, 20_000, 32),
    "below_halving_by_row_blocks": (196_608 - 128, 20_000, 32),
    "halving_by_partial_bytes": (100_000, 1_000_000, 64),
    "eight_waves_lse": (2048 + 300, 600_011, 64),
    "eight_waves_lse_256_tiles": (2048 + 300, 416_161, 64),
    "eight_waves_lse_255_tiles": (2048 + 300, 416_160, 64),
    "eight_waves_lse_511_anchors": (511, 2_100_000, 64),
    "eight_waves_lse_512_anchors": (512, 2_100_000, 64),
    "eight_waves_flash": (2000, 300_000, 64),
    "eight_waves_flash_256_tiles": (2000, 261_121, 64),
    "eight_waves_flash_255_tiles": (2000, 261_120, 64),
}


def padded(d):
    """functional._pad_dim: the width a problem reaches the library with"""
    return next((w for w in WIDTHS if d <= w), d)


def table_shapes():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import test_bce_gpu
    import test_infonce_gpu
    shapes = set()
    for mod in (test_infonce_gpu, test_bce_gpu):
        for fn in vars(mod).values():
            combos = [{}]
            for mark in getattr(fn, "pytestmark", []) if callable(fn) else []:
                if mark.name != "parametrize":
                    continue
                names = [s.strip() for s in mark.args[0].split(",")]
                if not set(names) & {"m", "n", "d"}:
                    continue
                rows = [v if len(names) > 1 else (v,) for v in mark.args[1]]
                combos = [dict(c, **dict(zip(names, row))) for c in combos for row in rows]
            for c in combos:
                if "m" not in c and "n" not in c:
                    continue
                m = c.get("m", c.get("n"))
                n = c.get("n", m)
                for d in ([c["d"]] if "d" in c else WIDTHS):
                    shapes |= {(m, n, d), (m, n, padded(d))}
    return shapes


def body_shapes():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import test_infonce_gpu
    marks = test_infonce_gpu.test_every_tile_count_parity_forward_and_backward.pytestmark
    ns = next(mk.args[1] for mk in marks if mk.name == "parametrize" and mk.args[0] == "n")
    shapes = BODY_SHAPES + [(TILE_COUNT_M, n, 64) for n in ns]
    return {(m, n, d) for m, n, d in shapes} | {(n, m, d) for m, n, d in shapes}


def cases():
    shapes = table_shapes() | body_shapes() | set(BRANCH_SHAPES.values())
    for d in WIDTHS + (UNSUPPORTED,):
        shapes |= {(0, 100, d), (100, 0, d), (0, 0, d), (1, 1, d), (257, 1000, d), (1000, 257, d)}
    return sorted(shapes)


def record(lib):
    return {
        "exports": list(SIZE_EXPORTS),
        "fwd_o_supported": [[d, f, int(lib.gcr_infonce_fwd_o_supported(d, f))] for d in WIDTHS + (UNSUPPORTED,) for f in FLAGS],
        "sizes": [[m, n, d] + [int(getattr(lib, name)(m, n, d)) for name in SIZE_EXPORTS] for m, n, d in cases()],
    }


def main():
    sys.path.insert(0, ROOT)
    from recommendation_amd import _build, _lib
    _build.build()
    got = record(_lib.lib())
    if "--check" in sys.argv:
        with open(GOLDEN) as f:
            want = json.load(f)
        sys.exit(0 if got == want else "differs from " + GOLDEN)
    with open(GOLDEN, "w") as f:
        f.write("{\n")
        f.write(' "exports": ' + json.dumps(got["exports"]) + ",\n")
        f.write(' "fwd_o_supported": ' + json.dumps(got["fwd_o_supported"]) + ",\n")
        f.write(' "sizes": [\n' + ",\n".join("  " + json.dumps(row) for row in got["sizes"]) + "\n ]\n}\n")
    print(GOLDEN, len(got["sizes"]), "shapes")


if __name__ == "__main__":
    main()
