#!/usr/bin/env python3
"""Times one GraphSAGE hidden layer and a whole GraphSAGE step on the HIP path against the composition, on the cfg2-size
bipartite graph (1M users x 100K items, 10M interactions with a skewed item popularity: edge_index of graphsage.py:43-44
has 20M directed edges over 1.1M nodes).

Per (din, dout, activation, p) in {(64, 64, relu, 0.2), (64, 128, gelu, 0), (128, 64, none, 0)} and, with relu and p = 0.2,
the other six width pairs:
    layer_fused_DINxDOUT_ACT      functional.sage_layer's node forward + backward (the SpMM for z, gcr_sage_fwd_f32; the SpMM
                                  again, gcr_sage_bwd_f32, the SpMM on A^T with its addend)
    layer_composed_DINxDOUT_ACT   functional.sage_layer_composed and its autograd (the SpMM each way, two GEMMs each way,
                                  the add, bias and activation as torch ops) followed by F.dropout, as the reference draws it
and for graphsage.py's default configuration (in = hidden = out = 64, two layers, relu, dropout 0.2, Adam, bpr):
    step_fused, step_composed     GraphSAGEModel's loss + backward + FusedAdam step, full batch (10M pairs), the two
                                  SAGEConv layers through the fused node resp. the composition

One child process under its own time limit (the parent never touches the GPU); inside it the variants alternate round by
round, every call between its own pair of device events after warm-up.  Prints ONE JSON line: per variant the median, min,
max, p10, p90 and spread of the per-call times over rounds x steps >= 20 calls, the peak device memory of one call above
what is allocated before it, per layer whether the p10 - p90 bands are disjoint in the fused path's favour (the condition
under which `functional.sage_layer` keeps a pair on the fused path: functional.SAGE_COMPOSED_PAIRS), and for every fused
layer the fraction of a byte estimate at the probe-measured copy bandwidth of the same run:
    gathers   3 nnz din 4  (the SpMM forward, again in the backward, and the transposed one)
    streams   n 4 (10 din + 3 dout)  (z written twice and read twice, x read twice, h written, h or pre and g read, p and
              q written, q read and dx written), + n 4 dout under gelu (pre written).
Needs a GPU.

    python scripts/perf_sage_layer.py [--steps 5] [--warmup 2] [--rounds 4]
    python scripts/perf_sage_layer.py --only layer_fused_64x64_relu --steps 30      (one variant, for a kernel trace)
"""
import json
import os
import sys

import perf_step_common as pc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

USERS, ITEMS, EDGES, SEED = 1_000_000, 100_000, 10_000_000, 20261021
# the three configurations the layer was specified with, then the other six width pairs (SAGE_COMPOSED_PAIRS is per pair)
SHAPES = ((64, 64, "relu", 0.2), (64, 128, "gelu", 0.0), (128, 64, "none", 0.0),
          (32, 32, "relu", 0.2), (32, 64, "relu", 0.2), (32, 128, "relu", 0.2), (64, 32, "relu", 0.2), (128, 32, "relu", 0.2),
          (128, 128, "relu", 0.2))
LAYERS = tuple(f"layer_{kind}_{a}x{b}_{act}" for a, b, act, _ in SHAPES for kind in ("fused", "composed"))
VARIANTS = LAYERS + ("step_fused", "step_composed")
LEG_TIMEOUT_S = 900


def leg(args):
    import torch
    from recommendation_amd import _lib, functional as Fn
    from recommendation_amd.graphsage import GraphSAGEModel
    from recommendation_amd.model_base import prepared_data

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    u = torch.randint(0, USERS, (EDGES,), device=dev, generator=gen)
    i = (ITEMS * torch.rand(EDGES, device=dev, generator=gen).square()).to(torch.int64).clamp_(0, ITEMS - 1)
    n = USERS + ITEMS
    data = prepared_data(USERS, ITEMS, dev, uid=u.cpu().numpy(), iid=i.cpu().numpy())

    def model_of(fused):
        m = GraphSAGEModel({}, data, None, device=dev, seed=0)
        for conv in m.model.layers:
            conv.fused = fused
        return m

    models = {True: model_of(True), False: model_of(False)}
    graph = models[True].model.prepare(models[True].edge_index, n)          # the operator and its transpose, outside the timing
    models[False].model._graph_key, models[False].model._graph = \
        (models[False].edge_index.data_ptr(), tuple(models[False].edge_index.shape), models[False].edge_index._version, n), graph
    nnz = graph.nnz
    max_row = int((graph.rowptr[1:] - graph.rowptr[:-1]).max())

    fns, keep_alive = {}, []
    for din, dout, act, p in SHAPES:
        assert Fn.sage_supported(din, dout)
        b = din ** -0.5
        x = torch.randn(n, din, device=dev, generator=gen).requires_grad_(True)
        wl, wr = (torch.empty(dout, din, device=dev).uniform_(-b, b, generator=gen).requires_grad_(True) for _ in range(2))
        bias = torch.empty(dout, device=dev).uniform_(-b, b, generator=gen).requires_grad_(True)
        g_out = torch.randn(n, dout, device=dev, generator=gen)
        bits = Fn.edge_mask_bits(n * dout, p, 7, dev) if p else None
        keep_alive.append((x, wl, wr, bias, g_out, bits))
        for kind in ("fused", "composed"):
            if kind == "fused":         # the node itself: the measurement must not follow SAGE_COMPOSED_PAIRS' routing
                def run(_item, x=x, wl=wl, wr=wr, bias=bias, g_out=g_out, act=act, bits=bits, p=p):
                    x.grad = wl.grad = wr.grad = bias.grad = None
                    Fn._SageLayer.apply(x, wl, wr, bias, graph, Fn.SAGE_ACTS[act], bits, 1.0 / (1.0 - p)).backward(g_out)
            else:                       # the dropout as the reference draws it (F.dropout), not a replayed bitmap
                def run(_item, x=x, wl=wl, wr=wr, bias=bias, g_out=g_out, act=act, p=p):
                    x.grad = wl.grad = wr.grad = bias.grad = None
                    torch.nn.functional.dropout(Fn.sage_layer_composed(graph, x, wl, wr, bias, act), p, True).backward(g_out)
            fns[f"layer_{kind}_{din}x{dout}_{act}"] = run

    fns["step_fused"], fns["step_composed"] = models[True].train_step, models[False].train_step

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
    for k in LAYERS[::2] + ("step_fused",):
        other = k.replace("fused", "composed")
        pc.add_verdict(case, k, other)
        case[k + "_bands_disjoint"] = bool(case[k + "_ms"]["p90"] < case[other + "_ms"]["p10"])
    # the byte estimate at the copy bandwidth this run measures
    src, dst = torch.empty(1 << 28, device=dev), torch.empty(1 << 28, device=dev)
    copy = lambda _: _lib.call("gcr_probe_copy_f32", src, dst, src.numel(), on=src)          # noqa: E731
    pc.timed(copy, range(3))
    copy_ms = sorted(pc.timed(copy, range(9)))[4]
    bw = 2 * src.numel() * 4 / (copy_ms * 1e-3)
    case["copy_bandwidth_gbs"] = round(bw / 1e9, 1)
    for din, dout, act, _ in SHAPES:
        k = f"layer_fused_{din}x{dout}_{act}"
        nbytes = 3 * nnz * din * 4 + n * 4 * (10 * din + (4 if act == "gelu" else 3) * dout)
        case[k + "_estimate_mb"] = round(nbytes / 1e6, 1)
        case[k + "_estimate_ms"] = round(nbytes / bw * 1e3, 3)
        case[k + "_fraction_of_estimate"] = round(nbytes / bw * 1e3 / case[k + "_ms"]["median"], 3)
        case[k + "_effective_gbs"] = round(nbytes / (case[k + "_ms"]["median"] * 1e-3) / 1e9, 1)
    print(json.dumps(case))


def main():
    args = pc.parse_args(VARIANTS, steps=5, warmup=2, rounds=4)
    if args.leg or args.only:
        return leg(args)
    print(pc.run_child(__file__, args, LEG_TIMEOUT_S))


if __name__ == "__main__":
    main()
