#!/usr/bin/env python3
"""Writes tests/golden/launch_workspace.json: what the host-only size queries of the loss, dense and BPR units return for
the shapes of `cases()`.  Only exports are called, so the script runs against any build of the library; the committed file
was recorded from the commit BEFORE the units' layouts moved onto the shared workspace carver (csrc/gcr_host.h), and
tests/test_launch_workspace_cpu.py holds every later build to it.

    python scripts/gen_launch_workspace_golden.py [--check]

Per query: every row count of ROWS (and 2^24 - 1, 2^24 where the entry bounds the batch) at the widths of its launch ladder,
every supported width at a few row counts, one unsupported width (the query returns 0 there), and every shape that the bodies
of tests/test_{buir,directau,bt,tri,mim,mhcn,bpr_paths}_gpu.py build (read from those modules' tables where they have one)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_workspace.json")

ROWS = (0, 1, 2, 7, 8, 31, 32, 33, 255, 256, 257, 4095, 4096, 262_144, 1_100_000)
BATCH_BOUND = ((1 << 24) - 1, 1 << 24)                      # gcr_buir_* / gcr_directau_*: batch < 2^24
FEW_ROWS = (1, 257, 4096)                                   # the row counts at which EVERY supported width is recorded

# query -> (arity, widths recorded at every row count, every supported width, one unsupported width, batch-bounded)
ONE_TO_256 = tuple(range(1, 257))
QUERIES = {
    "gcr_buir_workspace_bytes": (2, (16, 32, 48, 64, 128, 256, 512), tuple(range(16, 513, 16)), 40, True),
    "gcr_directau_workspace_bytes": (2, (2, 32, 64, 100, 128, 256, 512), tuple(range(2, 513, 2)), 0, True),
    "gcr_weighted_colsum_workspace_bytes": (2, (1, 3, 32, 64, 100, 128, 256), ONE_TO_256, 257, False),
    "gcr_gate_bwd_workspace_bytes": (2, (1, 3, 32, 64, 100, 128, 256), ONE_TO_256, 257, False),
    "gcr_channel_mix_bwd_workspace_bytes": (2, (32, 64, 128, 256), (32, 64, 128, 256), 96, False),
    "gcr_mim_workspace_bytes": (2, (32, 64, 128, 256), (32, 64, 128, 256), 96, False),
    "gcr_bt_workspace_bytes": (2, (32, 64, 96, 128, 256), (32, 64, 96, 128, 256), 48, False),
    "gcr_col_stats_workspace_bytes": (2, (4, 32, 48, 64, 256, 1024), tuple(range(4, 1025, 4)), 50, False),
    "gcr_sort_index_workspace_bytes": (1, (), (), None, False),
    "gcr_sort_pairs_u64_workspace_bytes": (1, (), (), None, False),
    "gcr_tri_member_words": (1, (), (), None, False),
}
# these two add rocPRIM's temporary storage size, which rocPRIM derives from the device it sees: record (and --check) them
# with no device visible, as the committed file was
ROCPRIM_BACKED = ("gcr_sort_index_workspace_bytes", "gcr_sort_pairs_u64_workspace_bytes")
GRAM_DIMS, GRAM_UNSUPPORTED = (32, 64, 96, 128), 48         # gcr_gram_tn_workspace_bytes(n, dx, dg)
TRI_WIDTHS, TRI_KS, TRI_UNSUPPORTED = (32, 64, 128), (1, 5, 20, 32), (256, 33)   # gcr_tri_workspace_bytes(m, d, k)

# shapes built inside test bodies that no table of the module names.  tests/test_buir_gpu.py: the launch-shape table, the
# single-user and three-row cases, the bitwise pair, the empty batch; tests/test_directau_gpu.py: the single row, the 77 x 48
# pair, the 200-sample step and the reproducibility table (its fixture's cases and configs are read below);
# tests/test_mim_gpu.py: the two reproducibility shapes; tests/test_bt_gpu.py: the column statistics at d = 48 and 1024 and
# the unsupported widths
BUIR_BODY = [(1, 64), (63, 64), (64, 64), (65, 64), (130, 64), (257, 64), (65, 16), (65, 32), (65, 128), (65, 256), (65, 512),
             (257, 48), (0, 64)]
DIRECTAU_BODY = [(1, 64), (77, 48), (200, 64), (2048, 64), (300, 512), (127, 32)]
MIM_BODY = [(775, 64), (20011, 32)]
BT_BODY = [(513, 48), (513, 512), (513, 1024)]


def _test_modules():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import test_bpr_paths_gpu as bpr
    import test_bt_gpu as bt
    import test_directau_gpu as au
    import test_mim_gpu as mim
    import test_tri_gpu as tri
    return bpr, bt, au, mim, tri


def mhcn_shapes():
    """(users, d) of the two MHCN fixtures: gram_tn, weighted_colsum, gate, channel_mix and the MIM loss run at them"""
    out = []
    for name in ("mhcn.npz", "mhcn_wide.npz"):
        with np.load(os.path.join(ROOT, "tests", "golden", name)) as z:
            out.append(tuple(int(v) for v in z["user_emb"].shape))
    return out


def body_shapes():
    """query -> set of argument tuples the GPU test bodies reach"""
    bpr, bt, au, mim, tri = _test_modules()
    mhcn = mhcn_shapes()
    batches = sorted({bpr.WIDTH_BATCH, bpr.PATTERN_BATCH} | {c[1] for c in bpr.BATCH_EDGES} | {t[0] for t in bpr.TRIPS})
    sort_n = {(b * n_neg,) for b in batches for n_neg in (1, 2, 3)} | {(b,) for b, _ in BUIR_BODY}
    tri_shapes = {(m, d, k) for m, d, k, _ in tri.SPLIT_CASES}
    tri_shapes |= {(m, d, k) for d in tri.WIDTHS for k in tri.KS + (tri.MAX_K,) for m in tri.rows_for(k)}
    au_shapes = set(DIRECTAU_BODY) | {(c.batch, c.d) for c in au.CASES}
    mim_shapes = {(n, d) for n in mim.ROWS for d in mim.WIDTHS} | {(n, d) for n, d, _, _ in mim.FOLD_CASES}
    mim_shapes |= set(MIM_BODY) | set(mhcn)
    return {
        "gcr_buir_workspace_bytes": set(BUIR_BODY),
        "gcr_directau_workspace_bytes": au_shapes,
        "gcr_weighted_colsum_workspace_bytes": set(mhcn),
        "gcr_gate_bwd_workspace_bytes": set(mhcn),
        "gcr_channel_mix_bwd_workspace_bytes": set(mhcn),
        "gcr_mim_workspace_bytes": mim_shapes,
        "gcr_bt_workspace_bytes": set(bt.ALL_SHAPES) | set(BT_BODY),
        "gcr_col_stats_workspace_bytes": set(bt.ALL_SHAPES) | set(BT_BODY),
        "gcr_sort_index_workspace_bytes": sort_n,
        "gcr_sort_pairs_u64_workspace_bytes": sort_n,
        "gcr_tri_member_words": {(m,) for m, _, _ in tri_shapes},
        "gcr_gram_tn_workspace_bytes": {(n, d, d) for n, d in mhcn},
        "gcr_tri_workspace_bytes": tri_shapes,
    }


def cases():
    """query -> sorted list of argument tuples"""
    out = {name: set(shapes) for name, shapes in body_shapes().items()}
    for name, (arity, ladder, supported, unsupported, bounded) in QUERIES.items():
        rows = ROWS + (BATCH_BOUND if bounded else ())
        if arity == 1:
            out[name] |= {(n,) for n in ROWS + BATCH_BOUND}
            continue
        out[name] |= {(n, d) for n in rows for d in ladder + (unsupported,)}
        out[name] |= {(n, d) for n in FEW_ROWS for d in supported}
    out["gcr_gram_tn_workspace_bytes"] |= {(n, dx, dg) for n in ROWS for dx in GRAM_DIMS + (GRAM_UNSUPPORTED,)
                                           for dg in GRAM_DIMS + (GRAM_UNSUPPORTED,)}
    out["gcr_tri_workspace_bytes"] |= {(m, d, k) for m in ROWS for d in TRI_WIDTHS for k in TRI_KS}
    out["gcr_tri_workspace_bytes"] |= {(m, TRI_UNSUPPORTED[0], 5) for m in ROWS} | {(m, 64, TRI_UNSUPPORTED[1]) for m in ROWS}
    return {name: sorted(shapes) for name, shapes in sorted(out.items())}


def record(lib):
    return {name: [list(args) + [int(getattr(lib, name)(*args))] for args in shapes] for name, shapes in cases().items()}


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
        f.write("{\n" + ",\n".join(' "%s": %s' % (name, json.dumps(rows, separators=(",", ":"))) for name, rows in got.items())
                + "\n}\n")
    print(GOLDEN, sum(len(rows) for rows in got.values()), "entries")


if __name__ == "__main__":
    main()
