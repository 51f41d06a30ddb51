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
import json
import os
import sys

import perf_step_common as pc

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

    ms = pc.measure(fns, VARIANTS, batches, args, batch=args.batch)
    if ms is None:
        return
    case = {"batch": args.batch, "steps_per_variant": args.rounds * args.steps, "device": torch.cuda.get_device_name(0)}
    pc.add_records(case, ms, VARIANTS)
    for side in ("loss", "step", "once_loss"):
        pc.add_verdict(case, "fused_loss" if side == "once_loss" else f"fused_{side}", f"composed_{side}",
                       f"{side}_composed_minus_fused_ms", f"{side}_faster_by_more_than_spread")
    print(json.dumps(case))


def main():
    args = pc.parse_args(VARIANTS, steps=10, warmup=5, rounds=4, what="steps", batch=True)
    if args.leg or args.only:
        args.batch = args.batch or 2048
        return leg(args)
    out = {"graph": "cfg2 (1M x 100K, 10M interactions, raw adjacency)", "emb": EMB, "n_layers": LAYERS, "cases": []}
    for batch in ((args.batch,) if args.batch else (512, 2048)):
        out["cases"].append(json.loads(pc.run_child(__file__, args, LEG_TIMEOUT_S, ("--batch", str(batch)), f"B = {batch}: ")))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
