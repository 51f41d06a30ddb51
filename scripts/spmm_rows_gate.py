"""Gate for the plain SpMM launch: where does the main launch of a cfg2 layer spend its time, user rows or item rows?

No kernel is changed.  The workload graph (bench.py's generator and seed, hub plan on) is built once.  The descriptor array
of the main plan (graph.hub.main, or graph.plan without a hub plan) is in row order, so a prefix or a suffix of it is a
valid launch: rows not covered are simply not written.  The Horner layer's launch (acc_in = x0, one acc_out, no y) runs on
    (a) the partitions of the user rows            (they gather from the item table, n_items x d x 4 bytes)
    (b) the partitions of the non-hub item rows    (they gather from the user table)
    (c) all of them, with the split rows' reduction
through --entry parts (gcr_spmm_csr_acc2_f32, `spmm_parts`) and / or --entry rows (gcr_spmm_rows_f32, `spmm_rows`).
Beside them the gather probe (gcr_probe_gather_rows_f32: 256-B rows, 16 loads in flight per wave) reads as many random rows
as (a) gathers from the item table alone, and as many as (c) from the whole table.

    python scripts/spmm_rows_gate.py                                   # ms per launch: 10 x 20 launches by HIP events
    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d <dir> -- \\
        python scripts/spmm_rows_gate.py --counters                    # two launches per case; one counter set per run:
                                                                       # FETCH_SIZE | WRITE_SIZE | TCC_HIT_sum TCC_MISS_sum |
                                                                       # SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY
                                                                       # (FETCH_SIZE and WRITE_SIZE do not fit one pass)
    python scripts/spmm_rows_gate.py --summarize <dir> [<dir> ...]     # pairs the traces with the case list, no GPU

The run writes <out>/rows_gate_<workload>[_counters].json.  FETCH_SIZE counts 32-B units x 2 short of the fabric bytes on
gfx950 (calibration 0.502), so --summarize prints FETCH_SIZE x 2 + WRITE_SIZE in bytes."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("spmm_parts", "spmm_rows", "probe_gather")
LONG_ROWS = "spmm_long_rows"          # the split rows' reduction of case (c): its counters are added to the launch it follows


def out_dir(args):
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    return out


def run(args):
    import torch
    import bench
    import recommendation_amd as ra
    import copy
    from recommendation_amd import _lib
    from recommendation_amd import spmm_launch as L

    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS[args.workload]
    n_u, n_i = wl["users"], wl["items"]
    users, items = bench.synth_interactions_device(n_u, n_i, wl["edges"], bench.SEED, dev)
    graph = ra.CsrGraph.bipartite_sym_norm(users, items, n_u, n_i, dev, row_order=False if args.row_order == "off" else None)
    del users, items
    n, d = n_u + n_i, args.d
    x0 = torch.empty(n, d, device=dev)
    torch.nn.init.xavier_uniform_(x0, generator=torch.Generator(device=dev).manual_seed(0))
    x = x0 * 0.5 + 0.01
    out = torch.empty_like(x0)
    hub = graph.hub if graph.hub is not None and graph.hub.eligible(d) else None
    p = graph.plan if hub is None else hub.main
    # the graph's row order (graph.RowOrder), when it has one: its plan stands in for `p` and only --entry rows can walk it.
    # P keeps the user rows in front of the item rows, so the segments below are cut in the same way
    rp = graph.rows_p if graph.rows_p is not None and graph.rows_p.eligible(d) and (hub is not None or graph.hub is None) else None
    if rp is not None:
        p = rp.plan
        args.entry = [e for e in args.entry if e == "rows"] or sys.exit("a row-ordered plan runs through --entry rows only")
    ws = graph.workspace(d)
    stream = _lib.cur_stream(dev)
    desc_host = p.desc_host
    row0 = desc_host[:, 2] & 0xFFFFFFFF
    split = int((row0 < n_u).sum())                       # partitions are in row order: [0, split) start at a user row
    assert bool((row0[:split] < n_u).all()) and bool((row0[split:] >= n_u).all())
    deg = (graph.rowptr[1:] - graph.rowptr[:-1]).cpu().numpy()
    nnz_of = lambda a, b: int((desc_host[a:b, 1] - desc_host[a:b, 0]).sum())
    segments = [("user rows", 0, split, 0), ("item rows (non-hub)", split, p.n_parts, 0), ("all", 0, p.n_parts, p.n_long)]
    repeats, launches = (1, 2) if args.counters else (args.repeats, args.launches)
    cases = []

    def timed(label, fn, extra):
        fn()                                              # warm-up: the first dispatch of every case
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches - (1 if args.counters else 0)):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / max(launches - (1 if args.counters else 0), 1))
        ent = {"case": label, "dispatches": launches if args.counters else 1 + repeats * launches}
        if not args.counters:
            ent.update({"ms_per_launch": round(sum(ms) / len(ms), 5), "spread_ms": round(max(ms) - min(ms), 5),
                        "ms_min": round(min(ms), 5)})
        ent.update(extra)
        cases.append(ent)
        print(json.dumps(ent), flush=True)

    for entry in args.entry:
        if entry == "rows" and not hasattr(_lib.lib(), "gcr_spmm_rows_f32"):
            sys.exit("this library has no gcr_spmm_rows_f32")
        for label, a, b, n_long in segments:
            part = copy.copy(p)                           # a run of the plan's partitions, with or without its split rows
            part.desc, part.n_parts, part.n_long = p.desc[a:b], b - a, n_long
            layer = dict(x=x, d=d, acc_in=x0, acc_out=out, partials=ws, on=stream)
            if entry == "rows" and rp is not None:
                fn = lambda part=part, layer=layer: L.rows_mapped(rp, part, **layer)
            elif entry == "rows":
                fn = lambda part=part, layer=layer: L.rows(graph, part, **layer)
            else:
                fn = lambda part=part, layer=layer: L.csr_acc2(graph, part, acc_in2_scale=0.0, **layer)
            rows_written = int((desc_host[a:b, 2][desc_host[a:b, 3] < 0] >> 32).sum())
            timed(f"{label}, {entry}", fn, {"entry": entry, "n_parts": b - a, "nnz": nnz_of(a, b), "rows_written": rows_written,
                                            "kernel": "spmm_" + entry})

    # the gather probe: as many random 256-B rows as the segment gathers, from the table the segment gathers from
    if d == 64:
        g = torch.Generator(device=dev).manual_seed(7)
        for label, table, n_idx in (("probe, item table", x[n_u:], nnz_of(0, split)), ("probe, whole table", x, nnz_of(0, p.n_parts))):
            n_idx = max(64, n_idx // 64 * 64)
            idx = torch.randint(0, table.shape[0], (n_idx,), device=dev, dtype=torch.int32, generator=g)
            sink = torch.empty(n_idx // 64, 64, device=dev)
            fn = lambda table=table, idx=idx, sink=sink: _lib.call("gcr_probe_gather_rows_f32", table, table.shape[0], idx,
                                                                   idx.numel(), sink, on=stream)
            timed(label, fn, {"entry": "probe", "nnz": n_idx, "table_bytes": int(table.shape[0]) * d * 4, "kernel": "probe_gather"})
            if not args.counters:
                cases[-1]["gathered_TB_per_s"] = round(n_idx * 256 / cases[-1]["ms_per_launch"] / 1e9, 3)
    info = {"row_order": rp is not None, "workload": args.workload, "d": d, "nnz": graph.nnz, "n": n, "n_users": n_u, "hub_plan": hub is not None,
            "hub_nnz": None if hub is None else hub.hub_nnz, "mean_degree_users": float(deg[:n_u].mean()), "cases": cases}
    name = "rows_gate_%s%s.json" % (args.workload, "_counters" if args.counters else "")
    with open(os.path.join(out_dir(args), name), "w") as f:
        json.dump(info, f, indent=1)
    print("wrote " + os.path.join(out_dir(args), name))


def trace_rows(path):
    """Counters of one --pmc pass, one entry per launch of the gate, in dispatch order."""
    found = glob.glob(os.path.join(path, "**", "*_counter_collection.csv"), recursive=True)
    if len(found) != 1:
        sys.exit("expected one counter_collection.csv under %s, found %d" % (path, len(found)))
    by_dispatch = {}
    for r in csv.DictReader(open(found[0])):
        kern = next((k for k in KERNELS + (LONG_ROWS,) if k in r["Kernel_Name"]), None)
        if kern is not None:
            ent = by_dispatch.setdefault(int(r["Dispatch_Id"]), {"kernel": kern})
            ent[r["Counter_Name"]] = ent.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    rows = []
    for k in sorted(by_dispatch):
        ent = by_dispatch[k]
        if ent["kernel"] != LONG_ROWS:
            rows.append(ent)
        elif rows:                                        # one launch = the partitions' kernel + the split rows' reduction
            for nm, v in ent.items():
                if nm != "kernel":
                    rows[-1][nm] = rows[-1].get(nm, 0.0) + v
            rows[-1]["with_long_rows"] = True
    return rows


def summarize(args):
    info = json.load(open(os.path.join(out_dir(args), "rows_gate_%s_counters.json" % args.workload)))
    for path in args.summarize:                           # one directory per counter set: the passes are merged
        rows = trace_rows(path)
        if sum(c["dispatches"] for c in info["cases"]) != len(rows):
            sys.exit("%s: %d dispatches in the trace, the run lists %d" % (path, len(rows), sum(c["dispatches"] for c in info["cases"])))
        k = 0
        for c in info["cases"]:
            k += c["dispatches"]
            got = dict(rows[k - 1])                                                       # the last (warm) dispatch
            if got.pop("kernel") != c["kernel"]:
                sys.exit("%s: dispatch %d is not a %s" % (path, k - 1, c["kernel"]))
            if got.pop("with_long_rows", False):
                c["counters_include"] = LONG_ROWS
            c.setdefault("counters", {}).update(got)
    for c in info["cases"]:
        got = c["counters"]
        if "FETCH_SIZE" in got and "WRITE_SIZE" in got:
            c["fabric_bytes"] = int((2.0 * got["FETCH_SIZE"] + got["WRITE_SIZE"]) * 1024)
            c["fabric_bytes_per_nnz"] = round(c["fabric_bytes"] / max(c["nnz"], 1), 2)
        if "TCC_HIT_sum" in got and "TCC_MISS_sum" in got:
            c["tcc_hit_rate"] = round(got["TCC_HIT_sum"] / max(got["TCC_HIT_sum"] + got["TCC_MISS_sum"], 1.0), 4)
        if "SQ_WAVE_CYCLES" in got:
            for nm in ("SQ_ACTIVE_INST_ANY", "SQ_WAIT_INST_ANY", "SQ_WAIT_ANY"):
                if nm in got:
                    c[nm.lower() + "_over_wave_cycles"] = round(got[nm] / max(got["SQ_WAVE_CYCLES"], 1.0), 4)
        print("%-28s %s" % (c["case"], "  ".join("%s=%s" % kv for kv in sorted(c.items()) if kv[0] not in ("case", "counters", "kernel", "entry"))))
    with open(os.path.join(out_dir(args), "rows_gate_%s_%s.json" % (args.workload, args.tag or "counters_summary")), "w") as f:
        json.dump(info, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cfg2", choices=["cfg1", "cfg2", "cfg4"])
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--entry", action="append", choices=["parts", "rows"], help="default: both")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--row-order", default="on", choices=["on", "off"], help="off: build the graph with row_order=False")
    ap.add_argument("--counters", action="store_true", help="two dispatches per case, no timing: for a rocprofv3 --pmc run")
    ap.add_argument("--summarize", metavar="DIR", nargs="+", help="pair the counter runs' traces under each DIR with the case list")
    ap.add_argument("--tag", help="name of the summary written by --summarize")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"), help="directory of the case lists and summaries")
    a = ap.parse_args()
    a.entry = a.entry or ["parts", "rows"]
    if a.summarize:
        summarize(a)
    else:
        run(a)
