#!/usr/bin/env python3
"""Times DiffNet's social-diffusion layer and DiffNetModel.train_step on the HIP path, on two social graphs over the 1M
users of the cfg2-size synthetic data (1M users x 100K items, 10M interactions), d = 64, 2 layers, B = 2048:

    uniform     ten followees per user (10M entries)
    powerlaw    Pareto degrees (mean about ten) with one row of 20 000 entries

Per graph G:
    layer_gather_G    one layer forward + backward through functional.diffuse_layer(gather=True): S x summed inside
                      gcr_diffuse_fwd_f32 / gcr_diffuse_bwd_f32, then the SpMM on S^T for dx
    layer_spmm_G      the same with gather=False: the tuned SpMM into a scratch z before either kernel
    layer_composed_G  functional.diffuse_layer_composed: spmm, cat, matmul, relu and their autograd
    step_fused_G      a whole train_step (two layers, the A items addend, the BPR sums, Adam), `gather` by the library's rule
    step_composed_G   the same step of a second model held on the composition

One child process under its own time limit (the parent never touches the GPU); inside it the variants alternate round by
round, every call between its own pair of device events after warm-up.  Prints ONE JSON line: per variant the median, min,
max and the 10 % / 90 % quantiles of the per-call times — `spread` = p90 - p10 — over rounds x steps >= 20 calls, the pairwise
verdicts, the device kernels one call of each layer variant launches (torch.profiler), and the forward's byte floor
2 U d 4 B at the probe-measured copy bandwidth of the same run.  Needs a GPU.

    python scripts/perf_diffnet_step.py [--steps 5] [--warmup 3] [--rounds 4]
    python scripts/perf_diffnet_step.py --only layer_gather_uniform --steps 30      (one variant, for a kernel trace)
"""
import json
import os
import sys

import perf_step_common as pc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

EMB, BATCH, LAYERS = 64, 2048, 2
USERS, ITEMS, EDGES, SEED = 1_000_000, 100_000, 10_000_000, 20261020
HUB_DEGREE = 20_000
GRAPHS = ("uniform", "powerlaw")
KINDS = ("layer_gather", "layer_spmm", "layer_composed", "step_fused", "step_composed")
VARIANTS = tuple(f"{k}_{g}" for g in GRAPHS for k in KINDS)
LEG_TIMEOUT_S = 540


def social_graph(kind, dev, gen):
    """S [U, U] with values 1 / degree (every followee distinct up to chance), entries in random column order."""
    import torch
    import recommendation_amd as ra
    if kind == "uniform":
        deg = torch.full((USERS,), 10, dtype=torch.int64, device=dev)
    else:
        r = torch.rand(USERS, device=dev, generator=gen).clamp_min(1e-6)
        deg = (3.0 * r.pow(-1.0 / 1.5)).to(torch.int64).clamp_(1, 5000)          # Pareto(1.5) from 3: mean about 9
        deg[12345] = HUB_DEGREE
    row = torch.repeat_interleave(torch.arange(USERS, device=dev), deg)
    col = torch.randint(0, USERS, (row.numel(),), device=dev, generator=gen)
    val = (1.0 / deg.to(torch.float32))[row]
    return ra.CsrGraph.from_coo(row, col, val, USERS, USERS, dev), int(deg.max()), int(row.numel())


def leg(args):
    import torch
    import recommendation_amd as ra
    from recommendation_amd import _lib, functional as Fn
    from recommendation_amd.diffnet import DiffNetModel

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    u = torch.randint(0, USERS, (EDGES,), device=dev, generator=gen)
    i = torch.randint(0, ITEMS, (EDGES,), device=dev, generator=gen)
    distinct = torch.bincount(torch.unique(u * ITEMS + i) // ITEMS, minlength=USERS).clamp_min(1)
    a = ra.CsrGraph.from_coo(u, i, (1.0 / distinct.to(torch.float32))[u], USERS, ITEMS, dev)
    conf = {"n_layer": LAYERS, "emb_size": EMB, "batch_size": BATCH, "lr": 1e-3, "reg_lambda": 1e-4, "regU": 1}
    assert Fn.diffuse_supported(EMB)
    x = (0.1 * torch.randn(USERS, EMB, device=dev, generator=gen)).requires_grad_(True)
    w = torch.nn.init.xavier_uniform_(torch.empty(2 * EMB, EMB, device=dev), generator=gen).requires_grad_(True)
    g_out = torch.randn(USERS, EMB, device=dev, generator=gen)

    def batches(count):
        sel = [torch.randint(0, EDGES, (BATCH,), device=dev, generator=gen) for _ in range(count)]
        return [(u[s].contiguous(), i[s].contiguous(), torch.randint(0, ITEMS, (BATCH,), device=dev, generator=gen)) for s in sel]

    def layer(fn):
        def run(_batch):
            x.grad = w.grad = None
            fn(x, w).backward(g_out)
        return run

    fns, info = {}, {}
    for name in GRAPHS:
        s, max_deg, nnz = social_graph(name, dev, gen)
        s.t                                                   # the transposed operator is built once, outside the timing
        info[name] = {"max_degree": max_deg, "nnz": nnz, "gather_by_rule": max_deg <= Fn.DIFFUSE_GATHER_MAX_DEGREE}
        fused = DiffNetModel.from_graphs(conf, s, a, seed=0)
        composed = DiffNetModel.from_graphs(conf, s, a, seed=0, fused=False)
        fns[f"layer_gather_{name}"] = layer(lambda xx, ww, s=s: Fn.diffuse_layer(s, xx, ww, gather=True))
        fns[f"layer_spmm_{name}"] = layer(lambda xx, ww, s=s: Fn.diffuse_layer(s, xx, ww, gather=False))
        fns[f"layer_composed_{name}"] = layer(lambda xx, ww, s=s: Fn.diffuse_layer_composed(s, xx, ww))
        fns[f"step_fused_{name}"] = fused.train_step
        fns[f"step_composed_{name}"] = composed.train_step

    ms = pc.measure(fns, VARIANTS, batches, args)
    if ms is None:
        return
    case = {"users": USERS, "items": ITEMS, "edges": EDGES, "emb": EMB, "batch": BATCH, "layers": LAYERS, "graphs": info,
            "gather_max_degree": Fn.DIFFUSE_GATHER_MAX_DEGREE, "calls_per_variant": args.rounds * args.steps,
            "device": torch.cuda.get_device_name(0)}
    pc.add_records(case, ms, VARIANTS)
    for name in GRAPHS:
        for fast, slow in (("layer_gather", "layer_spmm"), ("layer_spmm", "layer_gather"), ("layer_gather", "layer_composed"),
                           ("layer_spmm", "layer_composed"), ("step_fused", "step_composed")):
            pc.add_verdict(case, f"{fast}_{name}", f"{slow}_{name}",
                           verdict_key=f"{fast}_{name}_faster_than_{slow}_by_more_than_spread")
    # the forward's floor: one read of x and one write of h, at the copy bandwidth this run measures
    src, dst = torch.empty(USERS * EMB, device=dev), torch.empty(USERS * EMB, device=dev)
    copy = lambda _: _lib.call("gcr_probe_copy_f32", src, dst, src.numel(), on=src)          # noqa: E731
    pc.timed(copy, range(3))
    copy_ms = sorted(pc.timed(copy, range(9)))[4]
    case["copy_2Ud4_bytes_ms"] = round(copy_ms, 4)
    case["mfma_floor_ms"] = round(USERS * 2 * EMB * EMB * 2 / 157.3e12 * 1e3, 4)
    one = batches(1)[0]
    for k in VARIANTS:
        if k.startswith("layer_"):
            pc.add_launches(case, k, fns[k], one)
    print(json.dumps(case))


def main():
    args = pc.parse_args(VARIANTS, steps=5, warmup=3, rounds=4)
    if args.leg or args.only:
        return leg(args)
    print(pc.run_child(__file__, args, LEG_TIMEOUT_S))


if __name__ == "__main__":
    main()
