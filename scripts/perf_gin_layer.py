#!/usr/bin/env python3
"""Times one GIN layer of BGRL's encoder and a whole BGRL step on the HIP path against the composition, on the cfg2-size
bipartite graph (1M users x 100K items, 10M interactions with a skewed item popularity: the edge_index of
bgrl_g2l.py:106-123 has 20M directed edges over 1.1M nodes).

Per width pair (din, dout) in {32, 64, 128}^2, with dropout 0.2 and no edge mask:
    layer_fused_DINxDOUT      functional.gin_layer's node forward + backward (the SpMM for s = x + A x, gcr_gin_fwd_f32;
                              gcr_gin_bwd_f32, the SpMM on A^T with its addend)
    layer_composed_DINxDOUT   functional.gin_layer_composed and its autograd (the SpMM each way, the add, two GEMMs each way,
                              the biases and both ReLUs as torch ops) followed by F.dropout, as the reference draws it
and for bgrl_g2l.py's default configuration (hidden 32, two layers, dropout 0.2, edge_p 0.2, feat_p 0.1, Adam):
    step_fused, step_composed BGRLModel.train_step: two views through the online and the target encoder, the loss, the
                              backward, FusedAdam and the target's update, the GIN layers through the fused node resp. the
                              composition

One child process under its own time limit (the parent never touches the GPU); inside it the variants alternate round by
round, every call between its own pair of device events after warm-up.  Prints ONE JSON line: per variant the median, min,
max, p10, p90 and spread of the per-call times over rounds x steps >= 20 calls, the peak device memory of one call above
what is allocated before it, per layer whether the p10 - p90 bands are disjoint in the fused path's favour (the condition
under which `functional.gin_layer` keeps a pair on the fused path: functional.GIN_COMPOSED_PAIRS), and for every fused
layer the fraction of a byte estimate at the probe-measured copy bandwidth of the same run:
    gathers   2 nnz din 4  (the SpMM forward and the transposed one; s is saved, not recomputed)
    streams   n 4 (7 din + 3 dout)  (x read and s written; s read and h written; s, h and g read and ds written; ds read
              and dx written).
Needs a GPU.

    python scripts/perf_gin_layer.py [--steps 5] [--warmup 2] [--rounds 4]
    python scripts/perf_gin_layer.py --only layer_fused_64x64 --steps 30      (one variant, for a kernel trace)
"""
import json
import os
import sys

import perf_step_common as pc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

USERS, ITEMS, EDGES, SEED = 1_000_000, 100_000, 10_000_000, 20261021
P = 0.2
SHAPES = tuple((a, b) for a in (32, 64, 128) for b in (32, 64, 128))
LAYERS = tuple(f"layer_{kind}_{a}x{b}" for a, b in SHAPES for kind in ("fused", "composed"))
VARIANTS = LAYERS + ("step_fused", "step_composed")
LEG_TIMEOUT_S = 900


def leg(args):
    import torch
    from recommendation_amd import _lib, functional as Fn
    from recommendation_amd.bgrl import BGRLModel
    from recommendation_amd.model_base import prepared_data

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    u = torch.randint(0, USERS, (EDGES,), device=dev, generator=gen)
    i = (ITEMS * torch.rand(EDGES, device=dev, generator=gen).square()).to(torch.int64).clamp_(0, ITEMS - 1)
    n = USERS + ITEMS
    data = prepared_data(USERS, ITEMS, dev, uid=u.cpu().numpy(), iid=i.cpu().numpy())

    def model_of(fused):
        m = BGRLModel({}, data, None, device=dev, seed=0)
        for conv in m.encoder.online_encoder.layers:
            conv.fused = fused                      # the target encoder is a deep copy: it inherits the flag
        return m

    models = {True: model_of(True), False: model_of(False)}
    enc = {k: m.encoder.online_encoder for k, m in models.items()}
    graph = enc[True].prepare(models[True].edge_index, n)                   # the operator and its transpose, outside the timing
    ei = models[False].edge_index
    enc[False]._graph_key, enc[False]._graph, enc[False]._graph_src = (ei.data_ptr(), tuple(ei.shape), ei._version, n), graph, ei
    nnz = graph.nnz
    max_row = int((graph.rowptr[1:] - graph.rowptr[:-1]).max())

    fns, keep_alive = {}, []
    for din, dout in SHAPES:
        assert Fn.gin_supported(din, dout)
        a, b = din ** -0.5, dout ** -0.5
        x = torch.randn(n, din, device=dev, generator=gen).requires_grad_(True)
        w1 = torch.empty(dout, din, device=dev).uniform_(-a, a, generator=gen).requires_grad_(True)
        b1 = torch.empty(dout, device=dev).uniform_(-a, a, generator=gen).requires_grad_(True)
        w2 = torch.empty(dout, dout, device=dev).uniform_(-b, b, generator=gen).requires_grad_(True)
        b2 = torch.empty(dout, device=dev).uniform_(-b, b, generator=gen).requires_grad_(True)
        g_out = torch.randn(n, dout, device=dev, generator=gen)
        bits = Fn.edge_mask_bits(n * dout, P, 7, dev)
        t = (x, w1, b1, w2, b2)
        keep_alive.append(t + (g_out, bits))

        def fused(_item, t=t, g_out=g_out, bits=bits):      # the node itself: the measurement must not follow GIN_COMPOSED_PAIRS
            for v in t:
                v.grad = None
            Fn._GinLayer.apply(*t, graph, 0.0, bits, 1.0 / (1.0 - P), None, None).backward(g_out)

        def composed(_item, t=t, g_out=g_out):              # the dropout as the reference draws it, not a replayed bitmap
            for v in t:
                v.grad = None
            torch.nn.functional.dropout(Fn.gin_layer_composed(graph, *t), P, True).backward(g_out)

        fns[f"layer_fused_{din}x{dout}"], fns[f"layer_composed_{din}x{dout}"] = fused, composed

    fns["step_fused"] = lambda _item: models[True].train_step()
    fns["step_composed"] = lambda _item: models[False].train_step()

    ms = pc.measure(fns, VARIANTS, lambda count: [None] * count, args)
    if ms is None:
        return
    case = {"users": USERS, "items": ITEMS, "interactions": EDGES, "n": n, "nnz": nnz, "max_row": max_row,
            "calls_per_variant": args.rounds * args.steps, "device": torch.cuda.get_device_name(0)}
    pc.add_records(case, ms, VARIANTS)
    for k in VARIANTS:                                        # peak memory of one call above what the inputs hold
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fns[k](None)
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
    for din, dout in SHAPES:
        k = f"layer_fused_{din}x{dout}"
        nbytes = 2 * nnz * din * 4 + n * 4 * (7 * din + 3 * dout)
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
