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
import json
import os
import sys

import perf_step_common as pc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

EMB, BATCH, K, M_TRI = 64, 2048, 10, 2048
USERS, ITEMS, DEG_R, DEG_SOCIAL, DEG_SHARING, SEED = 100_000, 40_000, 10, 12, 8, 20261019
VARIANTS = ("tri_fused", "tri_composed", "step_fused", "step_composed")
LEG_TIMEOUT_S = 420


def leg(args):
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

    ms = pc.measure(fns, VARIANTS, batches, args)
    if ms is None:
        return
    case = {"users": USERS, "items": ITEMS, "emb": EMB, "batch": BATCH, "k": K, "m_tri": M_TRI,
            "calls_per_variant": args.rounds * args.steps, "device": torch.cuda.get_device_name(0)}
    pc.add_records(case, ms, VARIANTS)
    for a, b in (("tri_fused", "tri_composed"), ("step_fused", "step_composed")):
        pc.add_verdict(case, a, b)
    print(json.dumps(case))


def main():
    args = pc.parse_args(VARIANTS, steps=5, warmup=3, rounds=4)
    if args.leg or args.only:
        return leg(args)
    print(pc.run_child(__file__, args, LEG_TIMEOUT_S))


if __name__ == "__main__":
    main()
