#!/usr/bin/env python3
"""Times the graph-attention aggregation and a whole GATRec step on the HIP path against the composition, on the cfg2-size
bipartite graph (1M users x 100K items, 10M interactions with a skewed item popularity: edge_index of gat.py:51-52 has
20M directed edges over 1.1M nodes, the heaviest item row a few ten thousand entries).

Per (heads, c) in {(1, 64), (2, 64), (4, 64)} and attention dropout pe in {0, 0.2}:
    layer_fused_HxC_peP      functional.gat_aggregate forward + backward (gcr_gat_fwd_f32 / gcr_gat_bwd_f32)
    layer_composed_HxC_peP   functional.gat_aggregate_composed and its autograd: alpha [E, H], messages [E, H, C]
and for gat.py's default configuration (in = hidden = out = 64, 2 heads, both dropouts 0.2):
    step_fused, step_composed    GATRec.loss + backward + FusedAdam step, full batch (10M pairs), the two GATConv layers
                                 through the fused node resp. the composition

One child process under its own time limit (the parent never touches the GPU); inside it the variants alternate round by
round, every call between its own pair of device events after warm-up.  Prints ONE JSON line: per variant the median, min,
max, p10, p90 and spread of the per-call times over rounds x steps >= 20 calls, the peak device memory of one call above
what is allocated before it, the pairwise verdicts, and for every fused layer the fraction of a byte estimate at the
probe-measured copy bandwidth of the same run:
    forward   nnz H C 4 gathered + 2 n H C 4 streamed;   backward   two such gathers + three streams.
Needs a GPU.

    python scripts/perf_gat_layer.py [--steps 5] [--warmup 2] [--rounds 4]
    python scripts/perf_gat_layer.py --only layer_fused_2x64_pe0 --steps 30      (one variant, for a kernel trace)
"""
import json
import os
import sys

import perf_step_common as pc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

USERS, ITEMS, EDGES, SEED = 1_000_000, 100_000, 10_000_000, 20261021
SHAPES = ((1, 64), (2, 64), (4, 64))
PES = (0.0, 0.2)
LAYERS = tuple(f"layer_{kind}_{h}x{c}_pe{int(pe * 100)}" for h, c in SHAPES for pe in PES for kind in ("fused", "composed"))
VARIANTS = LAYERS + ("step_fused", "step_composed")
LEG_TIMEOUT_S = 900


def leg(args):
    import torch
    from recommendation_amd import _lib, functional as Fn
    from recommendation_amd.gat import GATRec, bipartite_edge_index, gat_graph
    from recommendation_amd.optim import FusedAdam

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    u = torch.randint(0, USERS, (EDGES,), device=dev, generator=gen)
    i = (ITEMS * torch.rand(EDGES, device=dev, generator=gen).square()).to(torch.int64).clamp_(0, ITEMS - 1)
    edge_index = bipartite_edge_index(u.cpu(), i.cpu(), USERS).to(dev)
    n = USERS + ITEMS
    graph = gat_graph(edge_index, n, dev)
    graph.t                                                   # the transposed operator is built once, outside the timing
    nnz = graph.nnz
    max_row = int((graph.rowptr[1:] - graph.rowptr[:-1]).max())

    fns, keep_alive = {}, []
    for heads, c in SHAPES:
        assert Fn.gat_supported(heads, c)
        h = (0.3 * torch.randn(n, heads * c, device=dev, generator=gen)).requires_grad_(True)
        a_src = torch.randn(n, heads, device=dev, generator=gen).requires_grad_(True)
        a_dst = torch.randn(n, heads, device=dev, generator=gen).requires_grad_(True)
        g_out = torch.randn(n, heads * c, device=dev, generator=gen)
        keep_alive.append((h, a_src, a_dst, g_out))
        for pe in PES:
            bits = Fn.edge_mask_bits((nnz + n) * heads, pe, 7, dev) if pe else None
            for kind, fn in (("fused", Fn.gat_aggregate), ("composed", Fn.gat_aggregate_composed)):
                def run(_item, fn=fn, h=h, a_src=a_src, a_dst=a_dst, g_out=g_out, heads=heads, bits=bits, pe=pe):
                    h.grad = a_src.grad = a_dst.grad = None
                    fn(graph, h, a_src, a_dst, heads, 0.2, bits, pe).backward(g_out)
                fns[f"layer_{kind}_{heads}x{c}_pe{int(pe * 100)}"] = run

    def step_of(fused):
        torch.manual_seed(0)
        model = GATRec(USERS, ITEMS, 64, 64, 64, 2, 0.2, 0.2, 0.2).to(dev).train()
        model.gat1.fused = model.gat2.fused = fused
        model._graph_key, model._graph = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version), graph
        opt = FusedAdam(list(model.parameters()), lr=0.005)

        def run(neg):
            opt.zero_grad(set_to_none=True)
            model.loss(edge_index, neg).backward()
            opt.step()
        return run

    fns["step_fused"], fns["step_composed"] = step_of(True), step_of(False)

    def batches(count):
        return [torch.randint(0, ITEMS, (EDGES,), device=dev, generator=gen) for _ in range(count)]

    ms = pc.measure(fns, VARIANTS, batches, args)
    if ms is None:
        return
    case = {"users": USERS, "items": ITEMS, "interactions": EDGES, "n": n, "nnz": nnz, "max_row": max_row,
            "calls_per_variant": args.rounds * args.steps, "device": torch.cuda.get_device_name(0)}
    pc.add_records(case, ms, VARIANTS)
    one = batches(1)[0]
    for k in VARIANTS:                                        # peak memory of one call above what the inputs hold
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fns[k](one)
        torch.cuda.synchronize()
        case[k + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    for k in LAYERS[::2]:
        pc.add_verdict(case, k, k.replace("fused", "composed"))
        fk, ck = case[k + "_ms"], case[k.replace("fused", "composed") + "_ms"]
        case[k + "_bands_disjoint"] = bool(fk["p90"] < ck["p10"])
    pc.add_verdict(case, "step_fused", "step_composed")
    # the byte estimate at the copy bandwidth this run measures
    src, dst = torch.empty(1 << 28, device=dev), torch.empty(1 << 28, device=dev)
    copy = lambda _: _lib.call("gcr_probe_copy_f32", src, dst, src.numel(), on=src)          # noqa: E731
    pc.timed(copy, range(3))
    copy_ms = sorted(pc.timed(copy, range(9)))[4]
    bw = 2 * src.numel() * 4 / (copy_ms * 1e-3)
    case["copy_bandwidth_gbs"] = round(bw / 1e9, 1)
    for heads, c in SHAPES:
        gather, stream = nnz * heads * c * 4, n * heads * c * 4
        est_ms = (3 * gather + 5 * stream) / bw * 1e3
        for pe in PES:
            k = f"layer_fused_{heads}x{c}_pe{int(pe * 100)}"
            case[k + "_estimate_ms"] = round(est_ms, 3)
            case[k + "_fraction_of_estimate"] = round(est_ms / case[k + "_ms"]["median"], 3)
    print(json.dumps(case))


def main():
    args = pc.parse_args(VARIANTS, steps=5, warmup=2, rounds=4)
    if args.leg or args.only:
        return leg(args)
    print(pc.run_child(__file__, args, LEG_TIMEOUT_S))


if __name__ == "__main__":
    main()
