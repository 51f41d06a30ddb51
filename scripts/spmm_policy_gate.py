"""Gate for cache-policy hints in the SpMM: does an `nt` load or store on gfx950 change what an XCD's L2 keeps?

No SpMM kernel is involved.  gcr_probe_policy_rows_f32 runs the gather probe's loop over two tables in one launch, shaped
like the user rows of a cfg2 layer (case (a) of scripts/spmm_rows_gate.py):
    * a hot table of 2 MiB (8 192 rows of 256 B), gathered uniformly, always with plain loads: it fits an L2 twice over;
    * a cold table of 256 MiB, gathered uniformly: practically every cold gather misses and, allocated, pushes hot rows out;
    * the two interleaved 1 : 1 inside every batch of 16 gathers in flight;
    * a sequential stream read of 64 B per gather and one 256-B row store per 16 gathers.
Under LRU a hot row's reuse distance in its L2 is 8 192 hot gathers, between which 2 MiB of hot rows, 2 MiB of cold rows
and 1.25 MiB of stream and store lines are inserted: 5.25 MiB against 4 MiB, so plain launches miss on most hot gathers.
A class of access (cold gathers, stream loads, row stores) whose `nt` form does not allocate, or allocates at a lower
priority, takes its share out of that distance and the hot table's hits go up: fewer fetched bytes per gather at the same
gather count.  The cells are plain (twice: its run-to-run spread is the yardstick), each class alone, the two streams
together, and all three.

    python scripts/spmm_policy_gate.py                                  # ms per launch by HIP events, cells interleaved
    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d <dir> -- \\
        python scripts/spmm_policy_gate.py --counters                   # three launches per cell; one counter set per run:
                                                                        # FETCH_SIZE | WRITE_SIZE | TCC_HIT_sum TCC_MISS_sum
    python scripts/spmm_policy_gate.py --summarize <dir> [<dir> ...]    # pairs the traces with the cell list, no GPU

The run writes <out>/policy_gate[_counters].json.  FETCH_SIZE and WRITE_SIZE are in KiB, and FETCH_SIZE counts half of the
fabric bytes on gfx950 (calibration 0.502), so --summarize prints FETCH_SIZE x 2 in bytes per gather."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL = "probe_policy_kernel"
NT_COLD, NT_STREAM, NT_STORE = 1, 2, 4
CELLS = [("plain", 0), ("plain (repeat)", 0), ("cold gathers nt", NT_COLD), ("stream loads nt", NT_STREAM),
         ("row stores nt", NT_STORE), ("stream loads + row stores nt", NT_STREAM | NT_STORE),
         ("all three nt", NT_COLD | NT_STREAM | NT_STORE)]
COUNTER_LAUNCHES = 3                                      # per cell in a --counters run; the first is not used


def out_dir(args):
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    return out


def run(args):
    import torch
    from recommendation_amd import _lib

    dev = torch.device("cuda", 0)
    n_hot, n_cold = args.hot_rows, args.cold_mib * 4096   # 256-B rows
    n_idx = args.gathers // 64 * 64
    g = torch.Generator(device=dev).manual_seed(7)
    hot = torch.rand(n_hot, 64, device=dev, generator=g)
    cold = torch.rand(n_cold, 64, device=dev, generator=g)
    idx = torch.empty(n_idx, device=dev, dtype=torch.int32)
    idx[0::2] = torch.randint(0, n_hot, (n_idx // 2,), device=dev, dtype=torch.int32, generator=g)
    idx[1::2] = torch.randint(0, n_cold, (n_idx // 2,), device=dev, dtype=torch.int32, generator=g)
    stream_in = torch.rand(n_idx // 16, 64, 4, device=dev, generator=g)
    outs = {flags: torch.full((n_idx // 16, 64), float("nan"), device=dev) for flags in sorted({f for _, f in CELLS})}
    stream = _lib.cur_stream(dev)

    def launch(flags):
        _lib.call("gcr_probe_policy_rows_f32", hot, n_hot, cold, n_cold, idx, n_idx, stream_in, outs[flags], flags, on=stream)

    cells = [{"cell": label, "nt_flags": flags} for label, flags in CELLS]
    if args.counters:
        for c in cells:
            for _ in range(COUNTER_LAUNCHES):
                launch(c["nt_flags"])
            c["dispatches"] = COUNTER_LAUNCHES
        torch.cuda.synchronize()
    else:
        for flags in outs:                                # warm-up, and every cell's words against the plain cell's
            launch(flags)
        torch.cuda.synchronize()
        k = min(n_idx // 16, 4096)                        # and the first batches against torch
        ids = idx[:16 * k].long().view(k, 8, 2)
        want = hot[ids[:, :, 0]].sum(1) + cold[ids[:, :, 1]].sum(1) + stream_in[:k].sum(2)
        assert torch.allclose(outs[0][:k], want, rtol=1e-5, atol=1e-5), "the probe does not sum what it says"
        assert all(torch.equal(outs[0], o) for o in outs.values()), "the cells differ in what they compute"
        ms = [[] for _ in cells]
        for _ in range(args.repeats):                     # the cells take turns: drift hits all of them alike
            for c, acc in zip(cells, ms):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    launch(c["nt_flags"])
                e1.record()
                torch.cuda.synchronize()
                acc.append(e0.elapsed_time(e1) / args.launches)
        for c, acc in zip(cells, ms):
            c.update({"ms_per_launch": round(sum(acc) / len(acc), 5), "ms_min": round(min(acc), 5),
                      "spread_ms": round(max(acc) - min(acc), 5),
                      "gathered_TB_per_s": round(n_idx * 256 / (sum(acc) / len(acc)) / 1e9, 3)})
    for c in cells:
        print(json.dumps(c), flush=True)
    info = {"gathers": n_idx, "hot_rows": n_hot, "hot_bytes": n_hot * 256, "cold_rows": n_cold, "cold_bytes": n_cold * 256,
            "stream_bytes_per_gather": 64, "store_bytes_per_gather": 16, "cells": cells}
    name = "policy_gate%s.json" % ("_counters" if args.counters else "")
    with open(os.path.join(out_dir(args), name), "w") as f:
        json.dump(info, f, indent=1)
    print("wrote " + os.path.join(out_dir(args), name))


def trace_rows(path):
    """Counters of one --pmc pass, one entry per launch of the probe, in dispatch order."""
    found = glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True)
    if len(found) != 1:
        sys.exit("expected one counter_collection.csv under %s, found %d" % (path, len(found)))
    by_dispatch = {}
    for r in csv.DictReader(open(found[0])):
        if KERNEL in r["Kernel_Name"]:
            ent = by_dispatch.setdefault(int(r["Dispatch_Id"]), {})
            ent[r["Counter_Name"]] = ent.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    return [by_dispatch[k] for k in sorted(by_dispatch)]


def summarize(args):
    info = json.load(open(os.path.join(out_dir(args), "policy_gate_counters.json")))
    n = info["gathers"]
    for path in args.summarize:                           # one directory per counter set: the passes are merged
        rows = trace_rows(path)
        if sum(c["dispatches"] for c in info["cells"]) != len(rows):
            sys.exit("%s: %d launches in the trace, the run lists %d" % (path, len(rows), sum(c["dispatches"] for c in info["cells"])))
        k = 0
        for c in info["cells"]:
            for got in rows[k + 1:k + c["dispatches"]]:   # every launch of the cell but its first
                for nm, v in got.items():
                    c.setdefault("counters", {}).setdefault(nm, []).append(v)
            k += c["dispatches"]
    for c in info["cells"]:
        got = c.get("counters", {})
        if "FETCH_SIZE" in got:
            c["fetched_bytes_per_gather"] = [round(2.0 * v * 1024 / n, 2) for v in got["FETCH_SIZE"]]
        if "WRITE_SIZE" in got:
            c["written_bytes_per_gather"] = [round(v * 1024 / n, 2) for v in got["WRITE_SIZE"]]
        if "TCC_HIT_sum" in got and "TCC_MISS_sum" in got:
            c["tcc_hit_rate"] = [round(h / max(h + m, 1.0), 4) for h, m in zip(got["TCC_HIT_sum"], got["TCC_MISS_sum"])]
            c["tcc_requests"] = [int(h + m) for h, m in zip(got["TCC_HIT_sum"], got["TCC_MISS_sum"])]
        print("%-28s %s" % (c["cell"], "  ".join("%s=%s" % kv for kv in sorted(c.items()) if kv[0] not in ("cell", "counters", "dispatches"))))
    plain = [c for c in info["cells"] if c["nt_flags"] == 0]
    for key in ("fetched_bytes_per_gather", "tcc_hit_rate"):
        vals = [v for c in plain for v in c.get(key, [])]
        if vals:
            info["plain_spread_" + key] = round(max(vals) - min(vals), 4)
            print("plain cells, %s: %d launches, spread %s" % (key, len(vals), info["plain_spread_" + key]))
    with open(os.path.join(out_dir(args), "policy_gate_%s.json" % (args.tag or "counters_summary")), "w") as f:
        json.dump(info, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gathers", type=int, default=10_000_000, help="as many as case (a) of spmm_rows_gate.py on cfg2")
    ap.add_argument("--hot-rows", type=int, default=8192, help="256-B rows of the hot table (2 MiB)")
    ap.add_argument("--cold-mib", type=int, default=256, help="size of the cold table")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--counters", action="store_true", help="three launches per cell, no timing: for a rocprofv3 --pmc run")
    ap.add_argument("--summarize", metavar="DIR", nargs="+", help="pair the counter runs' traces under each DIR with the cell list")
    ap.add_argument("--tag", help="name of the summary written by --summarize")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"), help="directory of the cell lists and summaries")
    a = ap.parse_args()
    if a.summarize:
        summarize(a)
    else:
        run(a)
