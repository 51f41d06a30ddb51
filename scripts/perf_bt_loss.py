#!/usr/bin/env python3
"""Times the Barlow Twins loss, forward + backward, on two full-batch views of N = 1,100,000 nodes (the cfg2 node count) at
d = 64, 128 and 256:

    fused      functional.bt_loss (gcr_bt_fwd_f32 / gcr_bt_bwd_f32): one evaluation serves both directions
    composed   functional.bt_loss_composed run as (l(h1, h2) + l(h2, h1)) * 0.5, the way the reference's
               WithinEmbedContrast calls it (gbt.py:392-395), through torch's autograd

One child process under its own time limit (the parent never touches the GPU); inside it, per width, the two variants
alternate round by round, every call between its own pair of device events after warm-up.  Prints ONE JSON line: per width
and variant the median, min, max and the 10 % / 90 % quantiles of the per-call times, the device launches of one call
(torch.profiler), the ratio of the medians, and what the fused time is held against:
    memory floor    8 N d 4 B (three reads of each view and two gradient writes of the two-pass form) at the HBM peak
    compute floor   3 x 2 N d^2 flop (the product and the two gradient products) at the f32 MFMA peak
`fraction_of_floor` = the higher floor over the fused median.  Before timing, the gradients of either variant are compared
with the composition run in float64 on the same views (`grad_max_rel_err_vs_float64`).  Needs a GPU.

    python scripts/perf_bt_loss.py [--steps 5] [--warmup 2] [--rounds 4]
"""
import json
import os
import sys

import perf_step_common as pc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

NODES, WIDTHS, SEED = 1_100_000, (64, 128, 256), 20261020
HBM_BYTES_PER_S, MFMA_F32_FLOP_PER_S = 8.0e12, 157.3e12     # MI355X peaks
VARIANTS = ("fused", "composed")
LEG_TIMEOUT_S = 540


def leg(args):
    import torch
    from recommendation_amd import functional as Fn

    dev = torch.device("cuda", 0)
    out = {"nodes": NODES, "calls_per_variant": args.rounds * args.steps, "device": torch.cuda.get_device_name(0)}
    for d in WIDTHS:
        gen = torch.Generator(device=dev).manual_seed(SEED + d)
        mix = torch.randn(d, d, device=dev, generator=gen) / d ** 0.5
        h1 = (torch.randn(NODES, d, device=dev, generator=gen) @ mix + torch.randn(d, device=dev, generator=gen))
        h2 = 0.7 * h1 + 0.3 * torch.randn(NODES, d, device=dev, generator=gen) @ mix
        h1.requires_grad_(True)
        h2.requires_grad_(True)
        assert Fn.bt_supported(d)

        def fused(_):
            h1.grad = h2.grad = None
            Fn.bt_loss(h1, h2).backward()

        def composed(_):
            h1.grad = h2.grad = None
            ((Fn.bt_loss_composed(h1, h2) + Fn.bt_loss_composed(h2, h1)) * 0.5).backward()

        fns = {"fused": fused, "composed": composed}
        fused(None)
        grads = [h1.grad.clone(), h2.grad.clone()]
        loss_f = float(Fn.bt_loss(h1, h2))
        composed(None)
        loss_c = float((Fn.bt_loss_composed(h1, h2) + Fn.bt_loss_composed(h2, h1)) * 0.5)
        grads_c = [h1.grad.clone(), h2.grad.clone()]
        # faster and different is not faster: both variants against the composition in float64 at the timed size
        # (on the CPU, where the tests' float64 references are computed too)
        a64, b64 = (t.detach().cpu().double().requires_grad_(True) for t in (h1, h2))
        loss64 = Fn.bt_loss_composed(a64, b64)
        loss64.backward()
        rel = lambda got: max(float((g.cpu().double() - r.grad).abs().max() / r.grad.abs().max())
                              for g, r in zip(got, (a64, b64)))
        case = {"loss_fused": loss_f, "loss_composed": loss_c, "loss_float64": float(loss64),
                "grad_max_rel_err_vs_float64": {"fused": rel(grads), "composed": rel(grads_c)}}
        a64 = b64 = loss64 = grads_c = None
        ms = pc.measure(fns, VARIANTS, lambda count: [None] * count, args, d=d)
        if ms is None:
            continue
        pc.add_records(case, ms, VARIANTS)
        pc.add_verdict(case, "fused", "composed")
        case["composed_over_fused"] = round(case["composed_ms"]["median"] / case["fused_ms"]["median"], 3)
        mem_ms = 8 * NODES * d * 4 / HBM_BYTES_PER_S * 1e3
        flop_ms = 3 * 2 * NODES * d * d / MFMA_F32_FLOP_PER_S * 1e3
        case["memory_floor_ms"], case["compute_floor_ms"] = round(mem_ms, 4), round(flop_ms, 4)
        case["bound_by"] = "memory" if mem_ms >= flop_ms else "compute"
        case["fraction_of_floor"] = round(max(mem_ms, flop_ms) / case["fused_ms"]["median"], 4)
        for k in VARIANTS:
            pc.add_launches(case, k, fns[k], None)
        out[f"d{d}"] = case
        h1 = h2 = grads = None
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    args = pc.parse_args(VARIANTS, steps=5, warmup=2, rounds=4)
    if args.leg or args.only:
        return leg(args)
    print(pc.run_child(__file__, args, LEG_TIMEOUT_S))


if __name__ == "__main__":
    main()
