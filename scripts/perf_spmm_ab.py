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
`equal_to_base` must hold against a base with the same plan.

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
    res, argt = _lib.SIGNATURES["gcr_spmm_csr_acc2_f32"]
    from recommendation_amd.graph import HubPlan
    libs, plans = [], {}
    for path in args.lib:
        h = ctypes.CDLL(os.path.abspath(path))
        fn = h.gcr_spmm_csr_acc2_f32
        fn.restype, fn.argtypes = res, argt
        rows = getattr(h, "gcr_spmm_rows_f32", None) if d <= 64 and not args.acc2 else None
        if rows is not None:
            rows.restype, rows.argtypes = _lib.SIGNATURES["gcr_spmm_rows_f32"]
        red = getattr(h, "gcr_spmm_hub_reduce_f32", None)
        if red is None or args.acc2:                       # the second-addend form never takes the windowed plan
            libs.append((path, fn, None, None, None, rows))
            continue
        red.restype, red.argtypes = _lib.SIGNATURES["gcr_spmm_hub_reduce_f32"]
        own = getattr(h, "gcr_spmm_hub_parts_f32", None) if d <= 64 else None
        if own is not None:
            own.restype, own.argtypes = _lib.SIGNATURES["gcr_spmm_hub_parts_f32"]
        if not args.hub_config:
            hub = graph.hub if graph.hub is not None and graph.hub.eligible(d) else None
            libs.append((path, fn, red, hub, own, rows))
        for cfg in args.hub_config or []:
            wr, npp, *mind = (int(v) for v in cfg.split(":"))
            if cfg not in plans:                           # one companion per layout, shared by the libraries
                plans[cfg] = HubPlan.build(graph, wr, min_degree=mind[0] if mind else None, nnz_per_part=npp, forced=True)
            libs.append((f"{path} [hub {cfg}]", fn, red, plans[cfg], own, rows))
    stream = _lib.cur_stream(torch.device(dev))

    # --acc2: the Horner backward's form, a second addend with its own scale (the ACC2 instantiation of the kernel)
    in2 = torch.randn(n, d, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) if args.acc2 else None
    in2_scale = 0.25 if args.acc2 else 0.0

    def launch(lib, x, out):
        _, fn, red, hub, own, rows = lib
        q = p
        if hub is not None:
            H, hp, part = hub.H, hub.H.plan, hub.partials(d)
            if own is not None:
                _lib.check(own(_lib.dptr(hp.desc), hp.n_parts, _lib.dptr(hp.long_row), _lib.dptr(hp.long_slot0), hp.n_long,
                               _lib.dptr(H.rowptr), _lib.dptr(H.col), _lib.dptr(H.val), _lib.dptr(x), d, _lib.dptr(part),
                               _lib.dptr(H.workspace(d)), H.n_rows, H.n_cols, stream), "gcr_spmm_hub_parts_f32")
            else:
                _lib.check(fn(_lib.dptr(hp.desc), hp.n_parts, _lib.dptr(hp.long_row), _lib.dptr(hp.long_slot0), hp.n_long,
                              _lib.dptr(H.rowptr), _lib.dptr(H.col), _lib.dptr(H.val), None, 1.0, _lib.dptr(x), d,
                              _lib.dptr(part), None, None, 0.0, None, 1.0, 0, None, _lib.dptr(H.workspace(d)), H.n_rows,
                              H.n_cols, None, stream), "gcr_spmm_csr_acc2_f32")
            _lib.check(red(_lib.dptr(hub.hub_row), hub.n_hub, hub.n_windows, _lib.dptr(part), d, 1.0, None, _lib.dptr(x0),
                           _lib.dptr(out), 1.0, graph.n_rows, stream), "gcr_spmm_hub_reduce_f32")
            q = hub.main
        if rows is not None:
            _lib.check(rows(_lib.dptr(q.desc), q.n_parts, _lib.dptr(q.long_row), _lib.dptr(q.long_slot0), q.n_long,
                            _lib.dptr(graph.rowptr), _lib.dptr(graph.col), _lib.dptr(graph.val), 1.0, _lib.dptr(x), d, None,
                            _lib.dptr(x0), _lib.dptr(out), 1.0, _lib.dptr(ws), graph.n_rows, graph.n_cols, stream),
                       "gcr_spmm_rows_f32")
            return
        _lib.check(fn(_lib.dptr(q.desc), q.n_parts, _lib.dptr(q.long_row), _lib.dptr(q.long_slot0), q.n_long,
                      _lib.dptr(graph.rowptr), _lib.dptr(graph.col), _lib.dptr(graph.val), None, 1.0, _lib.dptr(x), d, None,
                      _lib.dptr(x0), _lib.dptr(in2), in2_scale, _lib.dptr(out), 1.0, 0, None, _lib.dptr(ws), graph.n_rows,
                      graph.n_cols, None, stream), "gcr_spmm_csr_acc2_f32")

    z = torch.empty_like(x0)
    launch(libs[0], x0, z)                         # layer 1 of the base: the input of the timed (second) layer
    outs = [torch.empty_like(x0) for _ in libs]
    for lib, out in zip(libs, outs):
        for _ in range(args.warmup):
            launch(lib, z, out)
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
    report = {"workload": args.workload, "acc2": bool(args.acc2), "d": d, "nnz": graph.nnz, "n_parts": p.n_parts, "n_long": p.n_long,
              "alternations": args.alternations, "launches": args.launches, "libs": []}
    for k, (path, _, _, hub, _, rows) in enumerate(libs):
        m = sum(ms[k]) / len(ms[k])
        ent = {"lib": path, "ms_per_layer": [round(v, 5) for v in ms[k]], "mean": round(m, 5),
               "spread": round(max(ms[k]) - min(ms[k]), 5), "equal_to_base": bool(torch.equal(outs[k], outs[0])),
               "max_diff_over_max": float((outs[k] - outs[0]).abs().max() / outs[0].abs().max()),
               "main_entry": "gcr_spmm_csr_acc2_f32" if rows is None else "gcr_spmm_rows_f32",
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
