#!/usr/bin/env python3
"""Times SSL4RecModel.train_step at the sizes a user runs (U = 1M, I = 100K, emb 64; B = 2048 / 4096; n.layers 1 / 2)
against the same step composed from the ops the library had before the fused gather + dropout-views kernel
(`gather_rows` + `F.dropout` x 2 + three item-tower calls).  The two alternate in one process, device events after
warm-up; prints ONE JSON line.  Needs a GPU.

    python scripts/perf_ssl4rec_step.py [--steps 20] [--warmup 5] [--rounds 5]
    python scripts/perf_ssl4rec_step.py --only fused --batch 4096 --layers 2 --steps 30     (one variant, for a kernel trace:
        rocprofv3 --kernel-trace --stats -- python scripts/perf_ssl4rec_step.py --only ...; two step counts give the
        launches per step by difference, `--only` prints the step count it ran)
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from recommendation_amd import functional as Fn  # noqa: E402
from recommendation_amd import losses as Ls  # noqa: E402
from recommendation_amd.ssl4rec import SSL4RecModel  # noqa: E402

N_USERS, N_ITEMS, EMB = 1_000_000, 100_000, 64


def build(n_layers, batch, seed=0):
    conf = {"embedding.size": EMB, "batch.size": batch, "learning.rate": 1e-3, "reg.lambda": 1e-4, "n.layers": n_layers,
            "SSL4Rec": {"alpha": 0.1, "tau": 0.2, "drop": 0.1}}
    data = types.SimpleNamespace(user_num=N_USERS, item_num=N_ITEMS, device=torch.device("cuda"))
    return SSL4RecModel(conf, data, None, device="cuda", seed=seed)


def composed_step(m, u, i):
    """ssl4rec.py:218-225 from the ops of the parent commit: three gathers, two torch dropouts, three item-tower calls."""
    enc = m.model
    m.optimizer.zero_grad(set_to_none=True)
    u_emb = enc.user_net(Fn.gather_rows(enc.initial_user, u))
    i_emb = enc.item_net(Fn.gather_rows(enc.initial_item, i))
    emb = Fn.gather_rows(enc.initial_item, i)
    v1, v2 = enc.item_net(F.dropout(emb, m.drop)), enc.item_net(F.dropout(emb, m.drop))
    rec_loss = Ls.batch_softmax_loss(u_emb, i_emb, m.tau)
    cl_loss = m.cl_rate * Ls.InfoNCE(v1, v2, m.tau)
    batch_loss = rec_loss + cl_loss + Ls.l2_reg_loss(m.reg_weight, u_emb, i_emb)
    batch_loss.backward()
    m.optimizer.step()
    return rec_loss.detach(), cl_loss.detach(), batch_loss.detach()


def batches(batch, count, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [(torch.randint(0, N_USERS, (batch,), device="cuda", generator=g),
             torch.randint(0, N_ITEMS, (batch,), device="cuda", generator=g)) for _ in range(count)]


def timed(fn, model, data):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for u, i in data:
        fn(model, u, i)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / len(data)


def fused_step(m, u, i):
    return m.train_step(u, i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("fused", "composed"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_ssl4rec_step.py needs a GPU")
    if args.only:
        model = build(args.layers, args.batch)
        fn = fused_step if args.only == "fused" else composed_step
        ms = timed(fn, model, batches(args.batch, args.steps, 1))
        print(json.dumps({"only": args.only, "batch": args.batch, "n_layers": args.layers, "steps": args.steps,
                          "ms_per_step_first_steps_included": round(ms, 4)}))
        return
    out = {"users": N_USERS, "items": N_ITEMS, "emb": EMB, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "cases": []}
    for n_layers in (1, 2):
        for batch in (2048, 4096):
            # one model per variant (own Adam state), same seed, same batches
            models = {"fused": build(n_layers, batch), "composed": build(n_layers, batch)}
            fns = {"fused": fused_step, "composed": composed_step}
            warm = batches(batch, args.warmup, 1)
            for k in fns:
                timed(fns[k], models[k], warm)
            ms = {k: [] for k in fns}
            for r in range(args.rounds):                     # alternate: drift of the clocks hits both alike
                data = batches(batch, args.steps, 100 + r)
                for k in fns:
                    ms[k].append(timed(fns[k], models[k], data))
            case = {"n_layers": n_layers, "batch": batch}
            for k in fns:
                case[k + "_ms"] = {"median": round(float(np.median(ms[k])), 4), "min": round(min(ms[k]), 4),
                                   "max": round(max(ms[k]), 4)}
            case["fused_over_composed"] = round(case["fused_ms"]["median"] / case["composed_ms"]["median"], 4)
            out["cases"].append(case)
            del models
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
