#!/usr/bin/env python3
"""Times SEPT's tri-training block and SEPTModel.train_step on the HIP path:

    tri_fused       functional.tri_training_loss (gcr_tri_fwd_f32 / gcr_tri_bwd_f32), forward + backward, on four given
                    tables at M = 2048 distinct users, d = 64, k = 10
    tri_composed    the same through functional.tri_training_loss_composed: torch's label_prediction and topk +
                    losses.neighbor_discrimination (what the library could run before the kernel)
    step_fused      a whole tri-training train_step on a synthetic graph: 100 000 users x 40 000 items, 10 interactions per
                    user, social / sharing views with 12 / 8 non-zeros per row; d = 64, 2 layers, B = 2048, Adam
    step_composed   the same step of a second model held on the composition

One child process under its own time limit (the parent never touches the GPU); inside it the variants alternate round by
round, every call between its own pair of device events after warm-up.  Prints ONE JSON line: per variant the median, min,
max and the 10 % / 90 % quantiles of the per-call times — `spread` = p90 - p10 — over rounds x steps >= 20 calls.  Needs a GPU.

    python scripts/perf_sept_step.py [--steps 5] [--warmup 3] [--rounds 4]
    python scripts/perf_sept_step.py --only tri_fused --steps 30      (one variant in this process, for a kernel trace)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

EMB, BATCH, K, M_TRI = 64, 2048, 10, 2048
USERS, ITEMS, DEG_R, DEG_SOCIAL, DEG_SHARING, SEED = 100_000, 40_000, 10, 12, 8, 20261019
VARIANTS = ("tri_fused", "tri_composed", "step_fused", "step_composed")
LEG_TIMEOUT_S = 420


def leg(args):
    import numpy as np
    import torch
    import recommendation_amd as ra
    from recommendation_amd import functional as Fn
    from recommendation_amd.sept import SEPTModel

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    rows = torch.arange(USERS, device=dev)

    def view(deg):                                        # a normalised [U, U] operator with `deg` entries per row
        col = torch.randint(0, USERS, (USERS * deg,), device=dev, generator=gen)
        return ra.CsrGraph.row_normalised(rows.repeat_interleave(deg), col, None, USERS, USERS, dev)

    u = rows.repeat_interleave(DEG_R)
    i = torch.randint(0, ITEMS, (USERS * DEG_R,), device=dev, generator=gen)
    keys = torch.unique(u * ITEMS + i)
    pu, pi = keys // ITEMS, keys % ITEMS
    rowptr = torch.zeros(USERS + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(pu, minlength=USERS), 0)
    norm_adj = ra.CsrGraph.bipartite_raw(u, i, USERS, ITEMS, dev)
    social, sharing = view(DEG_SOCIAL), view(DEG_SHARING)
    conf = {"emb_size": EMB, "batch_size": BATCH, "lr": 1e-3, "reg_lambda": 1e-4, "max.epoch": 6,
            "SEPT": {"n_layer": 2, "ss_rate": 0.005, "drop_rate": 0.3, "ins_cnt": K}}
    models = {k: SEPTModel.from_graphs(conf, norm_adj, social, sharing, rowptr, pi.to(torch.int32).contiguous(), seed=0)
              for k in ("step_fused", "step_composed")}
    models["step_composed"].tri_loss = Fn.tri_training_loss_composed
    aug = models["step_fused"].augmented_graph(3)
    tabs = [torch.randn(3 * M_TRI, EMB, device=dev, generator=gen).requires_grad_(True) for _ in range(4)]
    uniq = torch.arange(M_TRI, device=dev) * 3 + 1
    assert Fn.tri_training_supported(EMB, K)

    def batches(count):
        return [(torch.randint(0, USERS, (BATCH,), device=dev, generator=gen), torch.randint(0, ITEMS, (BATCH,), device=dev, generator=gen),
                 torch.randint(0, ITEMS, (BATCH,), device=dev, generator=gen)) for _ in range(count)]

    def tri(fn):
        def run(_):
            for t in tabs:
                t.grad = None
            fn(*tabs, uniq, K, 0.1)[0].sum().backward()
        return run

    fns = {"tri_fused": tri(Fn.tri_training_loss), "tri_composed": tri(Fn.tri_training_loss_composed),
           "step_fused": lambda b: models["step_fused"].train_step(b, True, aug),
           "step_composed": lambda b: models["step_composed"].train_step(b, True, aug)}

    def timed(fn, data):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in data]
        for (e0, e1), b in zip(evs, data):
            e0.record()
            fn(b)
            e1.record()
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in evs]

    if args.only:
        timed(fns[args.only], batches(args.steps))
        print(json.dumps({"only": args.only, "steps": args.steps}))
        return
    for k in VARIANTS:
        timed(fns[k], batches(args.warmup))
    ms = {k: [] for k in VARIANTS}
    for _ in range(args.rounds):                          # alternate: drift of the clocks hits all variants alike
        data = batches(args.steps)
        for k in VARIANTS:
            ms[k] += timed(fns[k], data)
    case = {"users": USERS, "items": ITEMS, "emb": EMB, "batch": BATCH, "k": K, "m_tri": M_TRI,
            "calls_per_variant": args.rounds * args.steps, "device": torch.cuda.get_device_name(0)}
    for k in VARIANTS:
        q = np.quantile(ms[k], [0.1, 0.5, 0.9])
        case[k + "_ms"] = {"median": round(float(q[1]), 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4),
                           "p10": round(float(q[0]), 4), "p90": round(float(q[2]), 4), "spread": round(float(q[2] - q[0]), 4)}
    for a, b in (("tri_fused", "tri_composed"), ("step_fused", "step_composed")):
        f, c = case[a + "_ms"], case[b + "_ms"]
        case[f"{b}_minus_{a}_ms"] = round(c["median"] - f["median"], 4)
        case[f"{a}_faster_by_more_than_spread"] = bool(c["median"] - f["median"] > max(f["spread"], c["spread"]))
    print(json.dumps(case))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--leg", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.rounds * args.steps < 20 and not args.only:
        raise SystemExit("at least 20 measured calls per variant (rounds x steps)")
    if args.leg or args.only:
        return leg(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--rounds", str(args.rounds)]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LEG_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"no result within {LEG_TIMEOUT_S} s; stopping")
    if res.returncode != 0:
        raise SystemExit(f"the measurement failed with status {res.returncode}; stopping")
    print(res.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    main()
