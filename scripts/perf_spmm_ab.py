"""Interleaved A/B of the SpMM layer between builds of libgcr, in ONE process on one GPU.

    scripts/build_ab.sh <parent-rev> libgcr_base          # the parent's library -> build/libgcr_base.so
    python scripts/perf_spmm_ab.py --lib build/libgcr_base.so --lib recommendation_amd/libgcr.so --workload cfg2

Every --lib is opened with ctypes next to the others (the first one is the base).  The workload graph (bench.py's
generator and seed) is built once through the package; then `gcr_spmm_csr_acc2_f32` of each library is timed in turn with
the arguments of the Horner layer of functional.lightgcn_propagate (x = the previous layer's output, acc_in = x0, one
acc_out, no y; --acc2 adds the second addend of the Horner backward): warm-up first, then --alternations rounds of
--launches launches per library between two HIP events.
Prints ms per layer for every alternation, the mean and the spread (max - min) per library, and whether each library's
output is torch.equal to the base's.  A build "beats" the base when its mean is lower by more than three times the
larger of the two spreads.

A library that exports gcr_spmm_hub_reduce_f32 runs the layer as functional.spmm_into does on this graph: the windowed
companion of the hub rows, their reduction, then the main plan (graph.HubPlan) -- three launches between the same two events.
Its hub rows are summed in another order than the base's, so `equal_to_base` is false there and the largest difference
relative to the largest output is printed beside it.  --hub-config WINDOW_ROWS:NNZ_PER_PART[:MIN_DEGREE] (repeatable) times
that library once per companion layout instead of the graph's own.  A library that also exports gcr_spmm_hub_parts_f32
runs the companion (d <= 64) through it, as functional.spmm_into does.  A library that exports gcr_spmm_rows_f32 runs the
main launch (d <= 64, not --acc2) through it, again as functional.spmm_into does; its words are the generic launch's, so
`equal_to_base` must hold against a base with the same plan.  A library that exports gcr_spmm_windowed_f32 runs the whole
windowed layer (d <= 64, not --acc2) through it, three launches, again as functional.spmm_into does.  --order CELL
(repeatable; hub_first or main_first, optionally followed by :long_rows_first) times such a library once per cell instead
of the graph's own order: which range of blocks leads the one grid, and whether the main plan's descriptors keep plan
order or graph.long_rows_first_order's; two_walks launches the two ranges one after the other (the merged split-row launch
without the one grid).  A library that exports gcr_spmm_windowed_mapped_f32 runs the graph's own windowed layer with
the graph's row order (graph.RowOrder) when it has one, once more as functional.spmm_into does; --no-row-order keeps every
library on the stored order.  --five-launch keeps such a library on the three older entries.  --shared-output makes every
library write the same output array: with an array of its own per library, a library's place in the list moved its time by
1-4 % (other addresses), more than most differences this script is asked about; give a library twice to see what is left.

The measurement runs in a child process under a time limit of its own (--timeout seconds); the parent never touches the
GPU and stops at the first failure."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import torch
    import bench
    import recommendation_amd as ra
    from recommendation_amd import _lib

    dev = "cuda:0"
    wl = bench.WORKLOADS[args.workload]
    n_u, n_i = wl["users"], wl["items"]
    users, items = bench.synth_interactions_device(n_u, n_i, wl["edges"], bench.SEED, dev)
    graph = ra.CsrGraph.bipartite_sym_norm(users, items, n_u, n_i, dev)
    del users, items
    n, d = n_u + n_i, args.d
    x0 = torch.empty(n, d, device=dev)
    torch.nn.init.xavier_uniform_(x0, generator=torch.Generator(device=dev).manual_seed(0))
    p, ws = graph.plan, graph.workspace(d)
    from recommendation_amd import spmm_launch as L
    from recommendation_amd.graph import HubPlan, long_rows_first_order
    libs, plans, orders = [], {}, {}
    for path in args.lib:
        call = _lib.call_on(ctypes.CDLL(os.path.abspath(path)))             # the exports this library has, and no others
        rows = d <= 64 and not args.acc2 and call.has("gcr_spmm_rows_f32")
        if not call.has("gcr_spmm_hub_reduce_f32") or args.acc2:           # the second-addend form never takes the windowed plan
            libs.append((path, call, None, False, rows, None))
            continue
        own = d <= 64 and call.has("gcr_spmm_hub_parts_f32")
        fused = d <= 64 and not args.five_launch and call.has("gcr_spmm_windowed_f32")

        def add(name, hub):
            if not fused or hub is None or not args.order:
                cell = None if not fused or hub is None else (int(hub.main_first), hub.main, None)
                rp = graph.rows_p
                if (cell is not None and hub is graph.hub and rp is not None and rp.eligible(d) and not args.no_row_order
                        and call.has("gcr_spmm_windowed_mapped_f32")):
                    cell = (int(hub.main_first), rp.plan, rp)
                libs.append((name, call, hub, own, rows, cell))
                return
            for c in args.order:                           # one entry per order of the work, the same plans
                first, _, desc_order = c.partition(":")
                if (first, desc_order) not in orders:
                    orders[first, desc_order] = (["hub_first", "main_first", "two_walks"].index(first), hub.main if not desc_order else
                                                 hub.main.permuted(long_rows_first_order(hub.main.desc_host)), None)
                libs.append((f"{name} [{c}]", call, hub, own, rows, orders[first, desc_order]))

        if not args.hub_config:
            add(path, graph.hub if graph.hub is not None and graph.hub.eligible(d) else None)
        for cfg in args.hub_config or []:
            wr, npp, *mind = (int(v) for v in cfg.split(":"))
            if cfg not in plans:                           # one companion per layout, shared by the libraries
                plans[cfg] = HubPlan.build(graph, wr, min_degree=mind[0] if mind else None, nnz_per_part=npp, forced=True)
            orders = {}
            add(f"{path} [hub {cfg}]", plans[cfg])
    stream = _lib.cur_stream(torch.device(dev))

    # --acc2: the Horner backward's form, a second addend with its own scale (the ACC2 instantiation of the kernel)
    in2 = torch.randn(n, d, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) if args.acc2 else None
    in2_scale = 0.25 if args.acc2 else 0.0

    def launch(lib, x, out):
        _, call, hub, own, rows, cell = lib
        layer = dict(x=x, d=d, acc_in=x0, acc_out=out, on=stream, call=call)         # the Horner layer: one acc_out, no y
        q = p
        if cell is not None:
            main_first, q, rp = cell
            H = hub.H
            win = dict(hub_split=H.workspace(d), partials=ws, hub_partials=hub.partials(d), main_first=main_first, **layer)
            if rp is not None:
                L.windowed_mapped(H, H.plan, rp, q, hub, **win)
            else:
                L.windowed(H, H.plan, graph, q, hub, **win)
            return
        if hub is not None:
            H, part = hub.H, hub.partials(d)
            if own:
                L.hub_parts(H, H.plan, x=x, d=d, y=part, partials=H.workspace(d), on=stream, call=call)
            else:
                L.csr_acc2(H, H.plan, x=x, d=d, y=part, acc_in2_scale=0.0, partials=H.workspace(d), on=stream, call=call)
            L.hub_reduce(hub, partials=part, d=d, n_rows=graph.n_rows, acc_in=x0, acc_out=out, on=stream, call=call)
            q = hub.main
        if rows:
            L.rows(graph, q, partials=ws, **layer)
            return
        L.csr_acc2(graph, q, partials=ws, acc_in2=in2, acc_in2_scale=in2_scale, **layer)

    z = torch.empty_like(x0)
    launch(libs[0], x0, z)                         # layer 1 of the base: the input of the timed (second) layer
    # --shared-output: every library writes the same array, so no cell is timed on other addresses than the base (an output
    # array of its own per library moved a cell by 1-4 % with its position in the list); the words are compared on copies
    shared = torch.empty_like(x0) if args.shared_output else None
    outs = [shared if args.shared_output else torch.empty_like(x0) for _ in libs]
    snaps = []
    for lib, out in zip(libs, outs):
        for _ in range(args.warmup):
            launch(lib, z, out)
        if args.shared_output:
            torch.cuda.synchronize()
            snaps.append(out.clone())
    torch.cuda.synchronize()
    ms = [[] for _ in libs]
    for _ in range(args.alternations):
        for k, (lib, out) in enumerate(zip(libs, outs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                launch(lib, z, out)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.launches)
    if args.shared_output:
        outs = snaps
    report = {"workload": args.workload, "acc2": bool(args.acc2), "d": d, "nnz": graph.nnz, "n_parts": p.n_parts, "n_long": p.n_long,
              "alternations": args.alternations, "launches": args.launches, "libs": []}
    for k, (path, _, hub, _, rows, cell) in enumerate(libs):
        m = sum(ms[k]) / len(ms[k])
        ent = {"lib": path, "ms_per_layer": [round(v, 5) for v in ms[k]], "mean": round(m, 5),
               "spread": round(max(ms[k]) - min(ms[k]), 5), "equal_to_base": bool(torch.equal(outs[k], outs[0])),
               "max_diff_over_max": float((outs[k] - outs[0]).abs().max() / outs[0].abs().max()),
               "main_entry": "gcr_spmm_windowed_mapped_f32" if cell is not None and cell[2] is not None else
                             "gcr_spmm_windowed_f32" if cell is not None else
                             "gcr_spmm_csr_acc2_f32" if not rows else "gcr_spmm_rows_f32",
               "windowed": None if hub is None else {"window_rows": hub.window_rows, "windows": hub.n_windows,
                                                      "n_hub": hub.n_hub, "hub_nnz": hub.hub_nnz,
                                                      "nnz_per_part": hub.H.plan.nnz_per_part}}
        if hub is not None:
            others = torch.ones(n, dtype=torch.bool, device=dev)
            others[hub.hub_row.long()] = False
            ent["other_rows_equal_to_base"] = bool(torch.equal(outs[k][others], outs[0][others]))
        if k:
            base = report["libs"][0]
            margin = 3 * max(base["spread"], ent["spread"])
            ent["gain_ms"] = round(base["mean"] - m, 5)
            ent["gain_pct"] = round(100 * (base["mean"] - m) / base["mean"], 2)
            ent["beats_base"] = bool(base["mean"] - m > margin)
        report["libs"].append(ent)
        print(f"{path}: " + " ".join(f"{v:.4f}" for v in ms[k]) + f" | mean {m:.4f} ms spread {ent['spread']:.4f}"
              + (f" | {ent['gain_pct']:+.2f} % vs base, beats base: {ent['beats_base']}, equal: {ent['equal_to_base']}, "
                 f"max diff / max {ent['max_diff_over_max']:.1e}" if k else ""))
    print(json.dumps(report))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", action="append", required=True, help="library path; give it at least twice, the base first")
    ap.add_argument("--workload", action="append", choices=["cfg1", "cfg2", "cfg4"], help="default: cfg2")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--acc2", action="store_true", help="time the second-addend form (acc_in2 given) instead")
    ap.add_argument("--hub-config", action="append", metavar="WINDOW_ROWS:NNZ_PER_PART[:MIN_DEGREE]",
                    help="time a library with the windowed plan once per companion layout (default: the graph's own)")
    ap.add_argument("--order", action="append", metavar="CELL",
                    choices=["hub_first", "main_first", "hub_first:long_rows_first", "main_first:long_rows_first", "two_walks"],
                    help="time a library with gcr_spmm_windowed_f32 once per order of the work (default: the graph's own)")
    ap.add_argument("--shared-output", action="store_true", help="every library writes the same output array")
    ap.add_argument("--no-row-order", action="store_true", help="keep every library on the stored order of the rows")
    ap.add_argument("--five-launch", action="store_true", help="keep every library on the three older windowed entries")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per workload (child process)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if len(args.lib) < 2:
        ap.error("need at least two --lib")
    if args.alternations < 5 or args.launches < 20:
        ap.error("at least 5 alternations of at least 20 launches")
    for path in args.lib:
        if not os.path.exists(path):
            ap.error(f"{path} does not exist")
    if args.child:
        args.workload = args.workload[0]
        return child(args)
    for wl in args.workload or ["cfg2"]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", wl, "--d", str(args.d),
               "--alternations", str(args.alternations), "--launches", str(args.launches), "--warmup", str(args.warmup)]
        for path in args.lib:
            cmd += ["--lib", path]
        if args.acc2:
            cmd.append("--acc2")
        for cfg in args.hub_config or []:
            cmd += ["--hub-config", cfg]
        for c in args.order or []:
            cmd += ["--order", c]
        if args.five_launch:
            cmd.append("--five-launch")
        if args.no_row_order:
            cmd.append("--no-row-order")
        if args.shared_output:
            cmd.append("--shared-output")
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"{wl}: no result within {args.timeout} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"{wl}: child exited with {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
