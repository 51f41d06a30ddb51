"""What scripts/perf_{buir,directau,mhcn,sept}_step.py share: per-call device-event timing, the round-by-round alternation
of the variants, the quantile / `spread` record, the pairwise verdict, the launch count of one call and the parent / child
`main` pieces.  torch is imported inside the functions: the parent process never touches the GPU."""
import argparse
import json
import os
import subprocess
import sys


def timed(fn, data):
    """ms of every fn(item), each between its own pair of device events; one synchronize at the end."""
    import torch
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in data]
    for (e0, e1), item in zip(evs, data):
        e0.record()
        fn(item)
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in evs]


def measure(fns, variants, batches, args, **only_fields):
    """{variant: per-call ms} over args.rounds x args.steps calls after args.warmup.  `--only`: that variant alone, one
    JSON line ({"only", only_fields.., "steps"}), returns None."""
    if args.only:
        timed(fns[args.only], batches(args.steps))
        print(json.dumps({"only": args.only, **only_fields, "steps": args.steps}))
        return None
    for k in variants:
        timed(fns[k], batches(args.warmup))
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):                          # alternate: drift of the clocks hits all variants alike
        data = batches(args.steps)
        for k in variants:
            ms[k] += timed(fns[k], data)
    return ms


def add_records(case, ms, variants):
    """case[variant + "_ms"] = median, min, max, p10, p90 and spread = p90 - p10 of the per-call times."""
    import numpy as np
    for k in variants:
        q = np.quantile(ms[k], [0.1, 0.5, 0.9])
        case[k + "_ms"] = {"median": round(float(q[1]), 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4),
                           "p10": round(float(q[0]), 4), "p90": round(float(q[2]), 4), "spread": round(float(q[2] - q[0]), 4)}


def add_verdict(case, fast, slow, diff_key=None, verdict_key=None):
    """The medians' difference slow - fast and whether it exceeds the larger of the two spreads."""
    f, s = case[fast + "_ms"], case[slow + "_ms"]
    case[diff_key or f"{slow}_minus_{fast}_ms"] = round(s["median"] - f["median"], 4)
    case[verdict_key or f"{fast}_faster_by_more_than_spread"] = bool(s["median"] - f["median"] > max(f["spread"], s["spread"]))


def add_launches(case, key, fn, item):
    """case[key + "_launches"]: the device kernels (and memsets / copies) of one fn(item), by torch.profiler."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(item)
            torch.cuda.synchronize()
        case[key + "_launches"] = int(sum(e.count for e in prof.key_averages() if getattr(e, "device_time_total", 0) > 0
                                          or getattr(e, "cuda_time_total", 0) > 0))
    except Exception as exc:                              # a profiler that cannot attach is not a failed measurement
        case[key + "_launches"] = None
        case[key + "_launches_error"] = repr(exc)[:200]


def parse_args(variants, steps, warmup, rounds, what="calls", batch=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--rounds", type=int, default=rounds)
    if batch:
        ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--only", choices=variants)
    ap.add_argument("--leg", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.rounds * args.steps < 20 and not args.only:
        raise SystemExit(f"at least 20 measured {what} per variant (rounds x steps)")
    return args


def run_child(script, args, timeout_s, extra=(), label=""):
    """The last stdout line of `script --leg` in a fresh child process under its own time limit."""
    cmd = [sys.executable, os.path.abspath(script), "--leg", *extra, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--rounds", str(args.rounds)]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"{label}no result within {timeout_s} s; stopping")
    if res.returncode != 0:
        raise SystemExit(f"{label}the measurement failed with status {res.returncode}; stopping")
    return res.stdout.strip().splitlines()[-1]
