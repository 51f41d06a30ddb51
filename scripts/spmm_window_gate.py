"""Gate for summing the heaviest rows by column window: does a windowed launch fetch fewer bytes per gathered non-zero?

No kernel is changed.  The workload graph (bench.py's generator and seed) is built once; its hub rows (degree >
max(nnz_per_part, 8 W), W = ceil(n_cols / window_rows) column windows) are copied window-major into a companion CSR `H` with
W x n_hub rows — row w * n_hub + h holds the non-zeros of hub row h whose column lies in window w, in stored order — and
`Fn.spmm_into(H, x, y=partials)` runs on it with a small `nnz_per_part` and the descriptors in XCD-grouped order by window
(reorder.xcd_grouped_order), so that the waves resident on one XCD gather from a few windows of the table at a time.
Set against it: the same launch on the item-side rows of the graph and on the hub rows alone, both with the library's
default plan (512 non-zeros per partition, row order).

    python scripts/spmm_window_gate.py --workload cfg2                    # ms per launch (HIP events), no counters
    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d <dir> -- \
        python scripts/spmm_window_gate.py --workload cfg2 --counters     # two launches per case, counters in a run of their own
    python scripts/spmm_window_gate.py --summarize <dir>                  # FETCH_SIZE per gathered non-zero, no GPU

The run writes <out>/window_gate_<workload>[_counters].json (--out, default bench_out/): the cases in dispatch order, which --summarize pairs
with the `spmm_parts` rows of rocprofv3's counter_collection.csv.  FETCH_SIZE counts 32-B units x 2 on gfx950 short of the
fabric bytes (calibration 0.502), so the figures below are FETCH_SIZE x 2 in bytes."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW_ROWS = (2048, 4096, 8192)
NNZ_PER_PART = (32, 64, 128)


def walk_host(rowptr, npp):
    """gcr_plan.cpp's walk() in Python, for partition sizes below the library's lower bound of 64: (desc [n_parts, 4],
    long_row, long_slot0).  Equal to the library's plan at npp >= 64 (checked by --selftest)."""
    desc, long_row, long_slot0 = [], [], []
    slots = 0
    n_rows = rowptr.size - 1
    cur_row0, cur_nnz0, cur_rows = 0, int(rowptr[0]), 0
    rp = rowptr.tolist()
    for r in range(n_rows):
        deg = rp[r + 1] - rp[r]
        if deg > npp:
            if cur_rows:
                desc.append((cur_nnz0, rp[r], cur_row0 | (cur_rows << 32), -1))
                cur_rows = 0
            chunks = (deg + npp - 1) // npp
            long_row.append(r)
            long_slot0.append(slots)
            for c in range(chunks):
                desc.append((rp[r] + deg * c // chunks, rp[r] + deg * (c + 1) // chunks, r | (1 << 32), slots))
                slots += 1
            cur_row0, cur_nnz0 = r + 1, rp[r + 1]
            continue
        if cur_rows == 0:
            cur_row0, cur_nnz0 = r, rp[r]
        elif cur_rows == 64 or rp[r + 1] - cur_nnz0 > npp:
            desc.append((cur_nnz0, rp[r], cur_row0 | (cur_rows << 32), -1))
            cur_row0, cur_nnz0, cur_rows = r, rp[r], 0
        cur_rows += 1
    if cur_rows:
        desc.append((cur_nnz0, rp[n_rows], cur_row0 | (cur_rows << 32), -1))
    long_slot0.append(slots)
    return (np.asarray(desc, dtype=np.int64).reshape(-1, 4), np.asarray(long_row, dtype=np.int32),
            np.asarray(long_slot0, dtype=np.int32), slots)


def small_part_plan(graph, npp, row_group):
    """Replace `graph.plan` (built by the library at >= 64) by the Python walk at `npp`, XCD-grouped by `row_group`."""
    import torch
    from recommendation_amd.reorder import xcd_grouped_order
    desc, long_row, long_slot0, slots = walk_host(graph.rowptr_host, npp)
    p = graph.plan
    order = xcd_grouped_order(desc, row_group)
    pad = np.array([0, 0, 0, -1], dtype=np.int64)
    desc = np.where((order >= 0)[:, None], desc[np.maximum(order, 0)], pad[None, :])
    p.n_parts, p.n_long, p.n_slots, p.nnz_per_part, p.grouped = int(order.size), int(long_row.size), int(slots), npp, True
    p.desc_host = desc
    p.desc = torch.from_numpy(np.ascontiguousarray(desc)).to(graph.device)
    p.long_row = torch.from_numpy(long_row if long_row.size else np.zeros(1, np.int32)).to(graph.device)
    p.long_slot0 = torch.from_numpy(long_slot0).to(graph.device)
    graph._workspaces = {}


def windowed_companion(graph, window_rows, npp, hub_min_degree=None):
    """(H, n_hub, W, hub_nnz): the companion CSR of the hub rows of `graph`, built with torch on the graph's device."""
    import torch
    import recommendation_amd as ra
    dev = graph.device
    W = -(-graph.n_cols // window_rows)
    thr = max(npp, 8 * W) if hub_min_degree is None else hub_min_degree
    deg = graph.rowptr[1:] - graph.rowptr[:-1]
    hub = torch.nonzero(deg > thr).flatten()
    n_hub = int(hub.numel())
    if n_hub == 0:
        return None, 0, W, 0
    hub_index = torch.full((graph.n_rows,), -1, dtype=torch.int64, device=dev)
    hub_index[hub] = torch.arange(n_hub, device=dev)
    rows = torch.repeat_interleave(torch.arange(graph.n_rows, device=dev), deg)
    e = torch.nonzero(hub_index[rows] >= 0).flatten()
    h = hub_index[rows[e]]
    del rows
    c = graph.col[e].to(torch.int64)
    sorted_rows = bool((((c[1:] >= c[:-1]) | (h[1:] != h[:-1]))).all())
    if not sorted_rows:
        raise ValueError("a hub row's columns are not sorted: the graph is not eligible")
    key = (c // window_rows) * n_hub + h
    order = torch.argsort(key, stable=True)                       # window-major, stored order inside a segment
    rp = torch.zeros(W * n_hub + 1, dtype=torch.int64, device=dev)
    rp[1:] = torch.cumsum(torch.bincount(key, minlength=W * n_hub), 0)
    e = e[order]
    val = None if graph.val is None else graph.val[e]
    group = np.repeat(np.arange(W, dtype=np.int64), n_hub)        # window id of every row of H
    H = ra.CsrGraph(rp, graph.col[e], val, W * n_hub, graph.n_cols, dev, nnz_per_part=max(npp, 64), row_group=group,
                    hub_window_rows=0)
    if npp < 64:
        small_part_plan(H, npp, group)
    return H, n_hub, W, int(e.numel())


def row_subset(graph, row_mask):
    """The rows of `graph` selected by the boolean `row_mask` as a CSR of their own (library's default plan)."""
    import torch
    import recommendation_amd as ra
    deg = graph.rowptr[1:] - graph.rowptr[:-1]
    rows = torch.repeat_interleave(row_mask, deg)
    e = torch.nonzero(rows).flatten()
    d = deg[row_mask]
    rp = torch.zeros(d.numel() + 1, dtype=torch.int64, device=graph.device)
    rp[1:] = torch.cumsum(d, 0)
    return ra.CsrGraph(rp, graph.col[e], None if graph.val is None else graph.val[e], int(d.numel()), graph.n_cols,
                       graph.device, hub_window_rows=0)


def out_dir(args):
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    return out


def run(args):
    import torch
    import bench
    import recommendation_amd as ra
    from recommendation_amd import functional as Fn

    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[args.workload]
    n_u, n_i = wl["users"], wl["items"]
    users, items = bench.synth_interactions_device(n_u, n_i, wl["edges"], bench.SEED, dev)
    graph = ra.CsrGraph.bipartite_sym_norm(users, items, n_u, n_i, dev, hub_window_rows=0)     # every case states its own plan
    del users, items
    n, d = n_u + n_i, args.d
    x = torch.empty(n, d, device=dev)
    torch.nn.init.xavier_uniform_(x, generator=torch.Generator(device=dev).manual_seed(0))
    launches = 2 if args.counters else args.launches
    cases = []

    def measure(label, g, extra):
        y = torch.empty(g.n_rows, d, device=dev)
        Fn.spmm_into(g, x, y=y)                                  # warm-up: the first dispatch of every case
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches - 1):
            Fn.spmm_into(g, x, y=y)
        e1.record()
        torch.cuda.synchronize()
        ent = {"case": label, "nnz": g.nnz, "rows": g.n_rows, "n_parts": g.plan.n_parts, "n_long": g.plan.n_long,
               "n_slots": g.plan.n_slots, "nnz_per_part": g.plan.nnz_per_part, "dispatches": launches,
               "ms_per_launch": None if args.counters else round(e0.elapsed_time(e1) / (launches - 1), 5)}
        ent.update(extra)
        cases.append(ent)
        print(json.dumps(ent), flush=True)
        return y

    deg = graph.rowptr[1:] - graph.rowptr[:-1]
    is_item = torch.arange(n, device=dev) >= n_u
    measure("whole graph, classic plan", graph, {})
    measure("item-side rows, classic plan", row_subset(graph, is_item), {})
    ref = {}
    for window_rows in args.window_rows or WINDOW_ROWS:
        W = -(-graph.n_cols // window_rows)
        for npp in args.nnz_per_part or NNZ_PER_PART:
            thr = max(npp, 8 * W)
            if thr not in ref:                                   # the same hub rows under the classic plan
                g_hub = row_subset(graph, deg > thr)
                ref[thr] = measure("hub rows, classic plan", g_hub, {"hub_min_degree": thr})
                del g_hub
            H, n_hub, W, hub_nnz = windowed_companion(graph, window_rows, npp)
            part = measure("hub rows, windowed", H, {"window_rows": window_rows, "windows": W, "n_hub": n_hub,
                                                     "hub_min_degree": thr})
            if not args.counters:                                # the window partials add up to the classic hub rows
                got = part.view(W, n_hub, d).sum(0)
                err = float((got - ref[thr]).abs().max() / ref[thr].abs().max())
                cases[-1]["max_rel_diff_to_classic"] = err
                print("  window sums against the classic hub rows: max diff / max = %.2e" % err, flush=True)
            del H, part
    out = out_dir(args)
    name = "window_gate_%s%s.json" % (args.workload, "_counters" if args.counters else "")
    with open(os.path.join(out, name), "w") as f:
        json.dump({"workload": args.workload, "d": d, "nnz": graph.nnz, "n": n, "cases": cases}, f, indent=1)
    print("wrote " + os.path.join(out, name))


def summarize(args):
    found = glob.glob(os.path.join(args.summarize, "**", "*_counter_collection.csv"), recursive=True)
    if len(found) != 1:
        sys.exit("expected one counter_collection.csv under %s, found %d" % (args.summarize, len(found)))
    by_dispatch = {}
    for r in csv.DictReader(open(found[0])):
        if "spmm_parts" in r["Kernel_Name"]:
            by_dispatch.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = float(r["Counter_Value"])
    rows = [by_dispatch[k] for k in sorted(by_dispatch)]
    info = json.load(open(os.path.join(out_dir(args), "window_gate_%s_counters.json" % args.workload)))
    if sum(c["dispatches"] for c in info["cases"]) != len(rows):
        sys.exit("%d spmm_parts dispatches in the trace, the run lists %d" % (len(rows), sum(c["dispatches"] for c in info["cases"])))
    k = 0
    for c in info["cases"]:
        k += c["dispatches"]
        c["counters"] = rows[k - 1]                                                      # the last (warm) dispatch
    if "FETCH_SIZE" not in rows[0]:                     # any other counter set: listed per case, e.g. TCC_HIT_sum TCC_MISS_sum
        for c in info["cases"]:
            print("%-30s %7s %5d %9d  %s" % (c["case"], c.get("window_rows", "-"), c["nnz_per_part"], c["nnz"],
                                             "  ".join("%s=%.6g" % kv for kv in sorted(c["counters"].items()))))
        with open(os.path.join(out_dir(args), "window_gate_%s_%s.json" % (args.workload, "_".join(sorted(rows[0])))), "w") as f:
            json.dump(info, f, indent=1)
        return
    for c in info["cases"]:
        c["fabric_read_bytes_per_nnz"] = round(2.0 * c["counters"]["FETCH_SIZE"] * 1024 / c["nnz"], 2)
    item = next(c for c in info["cases"] if c["case"].startswith("item-side"))["fabric_read_bytes_per_nnz"]
    hub = {c["hub_min_degree"]: c["fabric_read_bytes_per_nnz"] for c in info["cases"] if c["case"] == "hub rows, classic plan"}
    print("%-30s %7s %5s %6s %9s %8s %10s %9s %9s" % ("case", "window", "npp", "n_hub", "nnz", "parts", "B per nnz", "vs item", "vs hub"))
    for c in info["cases"]:
        b = c["fabric_read_bytes_per_nnz"]
        c["item_side_over_this"] = round(item / b, 3)
        vs_hub = hub.get(c.get("hub_min_degree"))
        print("%-30s %7s %5d %6s %9d %8d %10.1f %8.2fx %9s" % (c["case"], c.get("window_rows", "-"), c["nnz_per_part"],
              c.get("n_hub", "-"), c["nnz"], c["n_parts"], b, item / b, "%.2fx" % (vs_hub / b) if vs_hub else "-"))
    with open(os.path.join(out_dir(args), "window_gate_%s_fetch.json" % args.workload), "w") as f:
        json.dump(info, f, indent=1)


def selftest():
    """The Python walk equals the library's at 64 and 128 on a random degree sequence (no GPU)."""
    import ctypes
    from recommendation_amd import _lib
    rng = np.random.default_rng(0)
    deg = np.concatenate([rng.integers(0, 40, 500), rng.integers(60, 700, 40), [0, 1, 64, 65, 128, 129]])
    rng.shuffle(deg)
    rp = np.zeros(deg.size + 1, dtype=np.int64)
    np.cumsum(deg, out=rp[1:])
    L = _lib.lib()
    for npp in (64, 128):
        desc, long_row, long_slot0, slots = walk_host(rp, npp)
        sizes = (ctypes.c_int64 * 3)()
        p = ctypes.addressof(sizes)
        _lib.check(L.gcr_spmm_plan_size_host(rp.ctypes.data, deg.size, npp, p, p + 8, p + 16), "size")
        ref = np.empty((sizes[0], 4), dtype=np.int64)
        lr, ls = np.zeros(max(sizes[1], 1), dtype=np.int32), np.zeros(sizes[1] + 1, dtype=np.int32)
        _lib.check(L.gcr_spmm_plan_fill_host(rp.ctypes.data, deg.size, npp, ref.ctypes.data, lr.ctypes.data, ls.ctypes.data), "fill")
        assert (sizes[0], sizes[1], sizes[2]) == (desc.shape[0], long_row.size, slots)
        assert np.array_equal(ref, desc) and np.array_equal(lr[: sizes[1]], long_row) and np.array_equal(ls, long_slot0)
    print("selftest ok")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cfg2", choices=["cfg1", "cfg2", "cfg4"])
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--window-rows", type=int, action="append", help="window sizes to sweep (default 2048 4096 8192)")
    ap.add_argument("--nnz-per-part", type=int, action="append", help="partition sizes to sweep (default 32 64 128)")
    ap.add_argument("--launches", type=int, default=11, help="dispatches per case, the first a warm-up")
    ap.add_argument("--counters", action="store_true", help="two dispatches per case, no timing: for a rocprofv3 --pmc run")
    ap.add_argument("--summarize", metavar="DIR", help="pair the counter run's trace under DIR with its case list")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"), help="directory of the case lists and summaries")
    ap.add_argument("--selftest", action="store_true")
    a = ap.parse_args()
    if a.selftest:
        selftest()
    elif a.summarize:
        summarize(a)
    else:
        run(a)
