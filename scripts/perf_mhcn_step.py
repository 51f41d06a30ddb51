#!/usr/bin/env python3
"""Times MHCNModel.train_step at bench.py's cfg5 size (250 000 users x 50 000 items, H_s / H_j / H_p with 24 / 16 / 8
non-zeros per row, R with 10; d = 64, 2 layers, B = 2048, Adam) and, from a fixed final user table, the self-supervision
side alone (mhcn.py:470-473: three gates, three SpMMs, three hierarchical losses, forward + backward):

    ss_kernel       the three losses through functional.mim_loss (gcr_mim_fwd_f32 / gcr_mim_bwd_f32)
    ss_composed     the same through the torch composition (MHCNEncoder.hierarchical_self_supervision_composed: what the
                    library ran before the kernel)
    step_kernel     the whole train_step
    step_composed   the whole train_step of a second model whose encoder is held on the composition
    mim_only / composed_only   one loss, forward + backward, on given em and edge (no gate, no SpMM): the kernel family's
                    own bytes over its time against the HBM rate

One child process under its own time limit (the parent never touches the GPU); inside it the variants alternate round by
round, every call between its own pair of device events after warm-up.  Prints ONE JSON line: per variant the median,
min, max and the 10 % / 90 % quantiles of the per-call times — `spread` = p90 - p10 — over rounds x steps >= 20 calls.
Needs a GPU.

    python scripts/perf_mhcn_step.py [--steps 5] [--warmup 3] [--rounds 4]
    python scripts/perf_mhcn_step.py --only mim_only --steps 30      (one variant in this process, for a kernel trace:
        rocprofv3 --kernel-trace --stats -- python scripts/perf_mhcn_step.py --only ...)
"""
import json
import os
import sys

import perf_step_common as pc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

EMB, BATCH = 64, 2048
VARIANTS = ("ss_kernel", "ss_composed", "step_kernel", "step_composed", "mim_only", "composed_only")
LEG_TIMEOUT_S = 420
HBM_COPY_TBS, HBM_SPEC_TBS = 6.3, 8.0          # MI355X: measured float4 copy rate, data-sheet rate


def mim_bytes(n, d):
    """Bytes gcr_mim_fwd_f32 + gcr_mim_bwd_f32 move when nothing hits a cache: forward 1 (column sums) + 5 row operands,
    backward 6 row operands + 2 row results, of n * d * 4 bytes each; the permutations, their inverses (set, written,
    read) and the [3, n] coefficients (written once, read about six times)."""
    return 14 * n * d * 4 + n * (3 * 8 + 3 * 4) + n * (3 * 8 * 4 + 2 * 8 + 6 * 4)


def leg(args):
    import torch
    import bench
    import recommendation_amd as ra
    from recommendation_amd import functional as Fn
    from recommendation_amd.mhcn import MHCNEncoder, MHCNModel

    dev = torch.device("cuda", 0)
    cfg = bench.CFG5
    n_u, n_i = cfg["users"], cfg["items"]
    gen = torch.Generator(device=dev).manual_seed(bench.SEED)
    rows = torch.arange(n_u, device=dev)

    def rand_block(n_cols, deg):                          # bench.cfg5_measure's synthetic operators
        return ra.CsrGraph.row_normalised(rows.repeat_interleave(deg), torch.randint(0, n_cols, (n_u * deg,), device=dev,
                                                                                      generator=gen), None, n_u, n_cols, dev)

    graphs = [rand_block(n_u, k) for k in cfg["deg"]] + [rand_block(n_i, cfg["deg_r"])]
    conf = {"emb_size": EMB, "batch_size": BATCH, "lr": 1e-3, "reg_lambda": 1e-4, "max.epoch": 1,
            "MHCN": {"n_layer": cfg["layers"], "ss_rate": 0.01}}
    models = {k: MHCNModel.from_graphs(conf, *graphs, seed=0) for k in ("step_kernel", "step_composed")}
    composed = MHCNEncoder.hierarchical_self_supervision_composed
    models["step_composed"].model.hierarchical_self_supervision = composed
    enc = models["step_kernel"].model
    with torch.no_grad():
        final_user = enc.propagate()[0].clone().requires_grad_(True)
        em = enc.self_supervised_gating(final_user, 1).clone().requires_grad_(True)
        edge = Fn.spmm(enc.H_s, em).clone().requires_grad_(True)
    assert Fn.mim_supported(em)

    def batches(count):
        return [(torch.randint(0, n_u, (BATCH,), device=dev, generator=gen), torch.randint(0, n_i, (BATCH,), device=dev, generator=gen),
                 torch.randint(0, n_i, (BATCH,), device=dev, generator=gen)) for _ in range(count)]

    def ss_side(one):
        def run(_):
            final_user.grad = None
            enc.zero_grad(set_to_none=True)
            ss = 0
            for c, adj in enumerate((enc.H_s, enc.H_j, enc.H_p)):
                ss = ss + one(enc.self_supervised_gating(final_user, c + 1), adj)
            (enc.ss_rate * ss).backward()
        return run

    def composed_only(_):
        em.grad = edge.grad = None
        p = [torch.randperm(n_u, device=dev) for _ in range(3)]
        pos, neg1, neg2 = (em * edge).sum(1), (em[p[0]] * edge).sum(1), (edge[p[1]] * em).sum(1)
        local = (-torch.log(torch.sigmoid(pos - neg1)) - torch.log(torch.sigmoid(neg1 - neg2))).sum()
        graph = edge.mean(0, keepdim=True)
        ((-torch.log(torch.sigmoid((edge * graph).sum(1) - (edge[p[2]] * graph).sum(1)))).sum() + local).backward()

    def mim_only(_):
        em.grad = edge.grad = None
        Fn.mim_loss(em, edge).backward()

    fns = {"ss_kernel": ss_side(enc.hierarchical_self_supervision), "ss_composed": ss_side(composed),
           "step_kernel": lambda b: models["step_kernel"].train_step(b),
           "step_composed": lambda b: models["step_composed"].train_step(b),
           "mim_only": mim_only, "composed_only": composed_only}

    ms = pc.measure(fns, VARIANTS, batches, args)
    if ms is None:
        return
    case = {"users": n_u, "items": n_i, "emb": EMB, "batch": BATCH, "calls_per_variant": args.rounds * args.steps,
            "device": torch.cuda.get_device_name(0)}
    pc.add_records(case, ms, VARIANTS)
    for a, b in (("ss_kernel", "ss_composed"), ("step_kernel", "step_composed"), ("mim_only", "composed_only")):
        pc.add_verdict(case, a, b)
    case["ss_share_of_step"] = round(case["ss_kernel_ms"]["median"] / case["step_kernel_ms"]["median"], 4)
    case["ss_composed_share_of_step"] = round(case["ss_composed_ms"]["median"] / case["step_composed_ms"]["median"], 4)
    tbs = mim_bytes(n_u, EMB) / (case["mim_only_ms"]["median"] * 1e-3) / 1e12       # includes the three randperm draws
    case["mim_only_bytes"] = mim_bytes(n_u, EMB)
    case["mim_only_tb_per_s"] = round(tbs, 3)
    case["mim_only_of_hbm_copy_rate"] = round(tbs / HBM_COPY_TBS, 3)
    case["mim_only_of_hbm_spec_rate"] = round(tbs / HBM_SPEC_TBS, 3)
    print(json.dumps(case))


def main():
    args = pc.parse_args(VARIANTS, steps=5, warmup=3, rounds=4)
    if args.leg or args.only:
        return leg(args)
    print(pc.run_child(__file__, args, LEG_TIMEOUT_S))


if __name__ == "__main__":
    main()
