#!/usr/bin/env python3
"""Times DirectAUModel.train_step on the 1M x 100K / 10M-interaction graph (bench.py's cfg2; d = 64, 3 layers, B = 512
and 2048, Adam) and, from the final tables alone, the loss side (forward + backward of directau.py:222-226): the fused
path (`losses.directau_loss`: gcr_directau_fwd_f32 / _bwd_f32) against the same loss composed only from what the
library had before it — `gather_rows` x 3, F.normalize, torch.pdist, torch element-wise ops — on the same encoder.

Every batch size is measured in a child process of its own under its own time limit (the parent never touches the GPU
and stops at the first child that fails); inside a child the variants alternate round by round, every step between its
own pair of device events after warm-up.  Prints ONE JSON line: per variant the median, min, max and the 10 % / 90 %
quantiles of the per-step times — `spread` = p90 - p10 — over rounds x steps >= 20 steps.  Needs a GPU.

    python scripts/perf_directau_step.py [--steps 10] [--warmup 5] [--rounds 4]
    python scripts/perf_directau_step.py --only fused_loss --batch 2048 --steps 30     (one variant in this process, for a
        kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/perf_directau_step.py --only ...; two step
        counts give the launches per step by difference)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

EMB, LAYERS, GAMMA, REG = 64, 3, 1.0, 1e-4
VARIANTS = ("fused_step", "composed_step", "fused_loss", "composed_loss", "composed_once_loss")
LEG_TIMEOUT_S = 280


def composed_loss(user_emb, item_emb, u, i, j, gamma, reg, batch_size, once=False):
    """directau.py:222-226 from the ops of the parent commit.  once: uniformity(u_emb), which the reference evaluates for
    pos_loss and again for neg_loss, is evaluated once as the fused path does (three pdist calls instead of four), so
    that the comparison does not credit the kernel with work a user could have saved in torch."""
    import torch
    import torch.nn.functional as F
    from recommendation_amd import functional as Fn
    from recommendation_amd import losses as Ls

    def alignment(x, y):
        diff = F.normalize(x, dim=1) - F.normalize(y, dim=1)
        return torch.mean(torch.sum(diff * diff, dim=1))

    def uniformity(x, t=2.0):
        dist = torch.pdist(F.normalize(x, dim=1))
        return torch.log(torch.mean(torch.exp(-t * dist * dist)) + 1e-8)

    def calculate_loss(a, b):
        return alignment(a, b) + gamma * (uniformity(a) + uniformity(b)) / 2

    ue, pe, ne = Fn.gather_rows(user_emb, u), Fn.gather_rows(item_emb, i), Fn.gather_rows(item_emb, j)
    if once:
        uu = uniformity(ue)
        pos = alignment(ue, pe) + gamma * (uu + uniformity(pe)) / 2
        neg = alignment(ue, ne) + gamma * (uu + uniformity(ne)) / 2
        return pos - neg + Ls.l2_reg_loss(reg, ue, pe, ne) / batch_size
    return calculate_loss(ue, pe) - calculate_loss(ue, ne) + Ls.l2_reg_loss(reg, ue, pe, ne) / batch_size


def leg(args):
    """One batch size (or one `--only` variant) in this process."""
    import numpy as np
    import torch
    import bench
    import recommendation_amd as ra
    from recommendation_amd import losses as Ls
    from recommendation_amd.directau import DirectAUModel

    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["cfg2"]
    n_u, n_i = wl["users"], wl["items"]
    users, items = bench.synth_interactions_device(n_u, n_i, wl["edges"], bench.SEED, dev)
    graph = ra.CsrGraph.bipartite_raw(users, items, n_u, n_i, dev)            # directau.py:132-141: the raw 0/1 adjacency
    conf = {"embedding.size": EMB, "batch.size": args.batch, "learning.rate": 1e-3, "reg.lambda": REG, "optimizer": "adam",
            "DirectAU": {"gamma": GAMMA, "n_layers": LAYERS}}
    models = {k: DirectAUModel.from_graph(conf, graph, n_u, n_i, seed=0) for k in ("fused_step", "composed_step")}
    with torch.no_grad():
        tabs = [t.clone().requires_grad_(True) for t in models["fused_step"].embeddings()]
    gen = torch.Generator(device=dev).manual_seed(1)

    def batches(count):
        return [(torch.randint(0, n_u, (args.batch,), device=dev, generator=gen),
                 torch.randint(0, n_i, (args.batch,), device=dev, generator=gen),
                 torch.randint(0, n_i, (args.batch,), device=dev, generator=gen)) for _ in range(count)]

    def composed_step(m, b):
        m.optimizer.zero_grad(set_to_none=True)
        user_emb, item_emb = m.encode()
        composed_loss(user_emb, item_emb, *b, m.gamma, m.reg, m.batch_size).backward()
        m.optimizer.step()

    def loss_side(fn):
        def run(b):
            tabs[0].grad = tabs[1].grad = None
            fn(b).backward()
        return run

    fns = {"fused_step": lambda b: models["fused_step"].train_step(b),
           "composed_step": lambda b: composed_step(models["composed_step"], b),
           "fused_loss": loss_side(lambda b: Ls.directau_loss(tabs[0], tabs[1], *b, GAMMA, REG, args.batch)[3]),
           "composed_loss": loss_side(lambda b: composed_loss(tabs[0], tabs[1], *b, GAMMA, REG, args.batch)),
           "composed_once_loss": loss_side(lambda b: composed_loss(tabs[0], tabs[1], *b, GAMMA, REG, args.batch, once=True))}

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
        print(json.dumps({"only": args.only, "batch": args.batch, "steps": args.steps}))
        return
    for k in VARIANTS:
        timed(fns[k], batches(args.warmup))
    ms = {k: [] for k in VARIANTS}
    for _ in range(args.rounds):                          # alternate: drift of the clocks hits all variants alike
        data = batches(args.steps)
        for k in VARIANTS:
            ms[k] += timed(fns[k], data)
    case = {"batch": args.batch, "steps_per_variant": args.rounds * args.steps, "device": torch.cuda.get_device_name(0)}
    for k in VARIANTS:
        q = np.quantile(ms[k], [0.1, 0.5, 0.9])
        case[k + "_ms"] = {"median": round(float(q[1]), 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4),
                           "p10": round(float(q[0]), 4), "p90": round(float(q[2]), 4), "spread": round(float(q[2] - q[0]), 4)}
    for side in ("loss", "step", "once_loss"):
        f, c = case["fused_loss_ms" if side == "once_loss" else f"fused_{side}_ms"], case[f"composed_{side}_ms"]
        case[f"{side}_composed_minus_fused_ms"] = round(c["median"] - f["median"], 4)
        case[f"{side}_faster_by_more_than_spread"] = bool(c["median"] - f["median"] > max(f["spread"], c["spread"]))
    print(json.dumps(case))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--leg", action="store_true", help="(internal) measure --batch in this process")
    args = ap.parse_args()
    if args.rounds * args.steps < 20 and not args.only:
        raise SystemExit("at least 20 measured steps per variant (rounds x steps)")
    if args.leg or args.only:
        args.batch = args.batch or 2048
        return leg(args)
    out = {"graph": "cfg2 (1M x 100K, 10M interactions, raw adjacency)", "emb": EMB, "n_layers": LAYERS, "cases": []}
    for batch in ((args.batch,) if args.batch else (512, 2048)):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--batch", str(batch), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LEG_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"B = {batch}: no result within {LEG_TIMEOUT_S} s; stopping")
        if res.returncode != 0:
            raise SystemExit(f"B = {batch}: the measurement failed with status {res.returncode}; stopping")
        out["cases"].append(json.loads(res.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
