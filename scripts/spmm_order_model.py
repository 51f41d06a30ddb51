"""A CPU model of the user half of a LightGCN layer's gathers: bytes that miss in L2 per non-zero, by order of the rows.

Prices a row order (graph.RowOrder) without a GPU.  numpy only.

    python scripts/spmm_order_model.py                       # cfg2 sizes, about a minute
    python scripts/spmm_order_model.py --users 10000000 --items 1000000 --edges 100000000     # cfg4 sizes, several minutes
    python scripts/spmm_order_model.py --in-flight 128 --lru-rows 12288

The model:
  * the graph of bench.py's generator: users uniform, items Zipf(1) with no item above 0.5 % of the draws, unique pairs;
  * the user rows are cut into partitions of at most --part non-zeros in whole rows (at most 64 rows), as the planner cuts
    them, and dealt round-robin over 8 XCDs, as the hardware deals workgroups;
  * one XCD is one LRU over --lru-rows 256-B rows of the item table (16 384 rows = 4 MiB); the streams (CSR words, acc_in,
    the outputs) do not allocate.  A gather of a row that is not among the --lru-rows most recently used rows of its XCD
    is a miss and costs 256 B;
  * --in-flight G: G partitions of an XCD run side by side and take turns after every 16 gathers (the kernel's batch);
    G = 1 walks one partition after the other.
Recency is kept per block of 512 consecutive gathers of an XCD's stream, not per gather: a row is resident when fewer than
--lru-rows distinct rows were touched in the blocks after the one that touched it last, and a row met twice inside one
block misses once at most.  That is exact LRU up to one block (3 % of the default capacity).

Orders: `stored` (user id), `coldest` (graph.coldest_column_order's key: the degree, then the id, of the row's
least-referenced column; stable), `coldest2` (the second-coldest column as a second key), `random`.
Measured beside it on MI355X (EXPERIMENTS.md "SpMM: user rows in order of their coldest column"): cfg2, stored order 77
B per non-zero, coldest-column order 54."""
import argparse
import json
import time

import numpy as np

XCDS = 8
ROW_BYTES = 256
BLOCK = 512


def synth(n_users, n_items, n_edges, seed):
    """(user, item) int64 arrays, unique pairs, sorted by (user, item)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_items + 1, dtype=np.float64)
    p /= p.sum()
    for _ in range(50):
        over = p > 0.005
        if not over.any():
            break
        excess = (p[over] - 0.005).sum()
        p[over] = 0.005
        p[~over] += excess * p[~over] / p[~over].sum()
    item = rng.permutation(n_items)[np.searchsorted(np.cumsum(p), rng.random(n_edges)).clip(0, n_items - 1)]
    user = rng.integers(0, n_users, n_edges)
    key = np.unique(user * n_items + item)
    return key // n_items, key % n_items


def row_keys(rowptr, col, n_items):
    """(coldest, second coldest) key per row: degree * n_items + id of the column; rows without one get the largest key."""
    cnt = np.bincount(col, minlength=n_items)
    k = cnt[col] * n_items + col
    big = np.iinfo(np.int64).max
    deg = np.diff(rowptr)
    first = np.full(deg.size, big, dtype=np.int64)
    has = deg > 0
    first[has] = np.minimum.reduceat(k, rowptr[:-1][has])
    rows = np.repeat(np.arange(deg.size), deg)
    k2 = np.where(k == first[rows], big, k)
    second = np.full(deg.size, big, dtype=np.int64)
    second[has] = np.minimum.reduceat(k2, rowptr[:-1][has])
    return first, second


def partitions(deg, part):
    """Partition id of every row in walk order: at most `part` non-zeros and 64 rows each (a longer row is its own)."""
    pid = np.empty(deg.size, dtype=np.int64)
    cur, nnz, rows = 0, 0, 0
    for r, d in enumerate(deg.tolist()):
        if rows and (rows == 64 or nnz + d > part):
            cur, nnz, rows = cur + 1, 0, 0
        pid[r] = cur
        nnz += d
        rows += 1
    return pid


def xcd_stream(cols, pid_of_nnz, xcd, in_flight):
    """The gathers of one XCD in the order they are issued."""
    mine = pid_of_nnz % XCDS == xcd
    c, p = cols[mine], pid_of_nnz[mine] // XCDS
    if in_flight <= 1:
        return c
    start = np.flatnonzero(np.r_[True, p[1:] != p[:-1]])
    pos = np.arange(c.size) - np.repeat(start, np.diff(np.r_[start, c.size]))         # position inside the partition
    order = np.lexsort((p % in_flight, pos // 16, p // in_flight))                     # group, then turn, then partition
    return c[order]


def lru_misses(stream, n_items, capacity):
    """Misses of an LRU of `capacity` rows over `stream`, recency kept per block of BLOCK gathers."""
    n_blocks = -(-stream.size // BLOCK)
    last = np.full(n_items, -1, dtype=np.int64)                   # block that touched a row last
    count = np.zeros(n_blocks + 1, dtype=np.int64)                # rows whose last touch is that block
    misses = 0
    for b in range(n_blocks):
        rows = np.unique(stream[b * BLOCK:(b + 1) * BLOCK])
        # A row touched last in block t is resident when the rows touched last in blocks t + 1 .. b - 1 number fewer than the
        # capacity.  back[j] counts those of blocks b - 1 - j .. b - 1, so with m entries of `back` below the capacity the
        # resident rows are those with t >= b - 1 - m (a window of 8 192 blocks back holds any capacity asked for here)
        back = np.cumsum(count[max(0, b - 8192):b][::-1])
        m = int(np.searchsorted(back, capacity, side="left"))
        was = last[rows]
        misses += int(((was < 0) | (was < b - 1 - m)).sum())     # never touched, or pushed out since
        np.subtract.at(count, was[was >= 0], 1)
        last[rows] = b
        count[b] = rows.size
    return misses


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--seed", type=int, default=20250919)
    ap.add_argument("--part", type=int, default=512)
    ap.add_argument("--lru-rows", type=int, default=16384)
    ap.add_argument("--in-flight", type=int, default=1)
    ap.add_argument("--order", action="append", choices=["stored", "coldest", "coldest2", "random"])
    a = ap.parse_args()
    t0 = time.time()
    user, item = synth(a.users, a.items, a.edges, a.seed)
    deg = np.bincount(user, minlength=a.users)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    first, second = row_keys(rowptr, item, a.items)
    out = {"users": a.users, "items": a.items, "nnz": int(item.size), "part": a.part, "lru_rows": a.lru_rows,
           "in_flight": a.in_flight, "bytes_per_nnz": {}}
    for name in a.order or ["stored", "coldest"]:
        if name == "stored":
            order = np.arange(a.users)
        elif name == "coldest":
            order = np.argsort(first, kind="stable")
        elif name == "coldest2":
            order = np.lexsort((second, first))
        else:
            order = np.random.default_rng(1).permutation(a.users)
        d = deg[order]
        src = np.repeat(rowptr[:-1][order], d) + (np.arange(item.size) - np.repeat(np.cumsum(d) - d, d))
        cols = item[src]
        pid_of_nnz = np.repeat(partitions(d, a.part), d)
        misses = sum(lru_misses(xcd_stream(cols, pid_of_nnz, x, a.in_flight), a.items, a.lru_rows) for x in range(XCDS))
        out["bytes_per_nnz"][name] = round(misses * ROW_BYTES / item.size, 2)
        print(f"{name}: {out['bytes_per_nnz'][name]} B per non-zero ({misses} misses, {time.time() - t0:.0f} s)", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
