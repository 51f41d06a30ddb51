#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/gat_steps.npz: the GAT aggregation's component cases, one whole GATConv
layer, and six full-batch training steps of gat.py run by the reference itself at three configurations.

Runs ONLY where the reference sources are (like oracle/gen_golden.py, whose `load_defs` / `load_stmts` it uses); the
fixture is plain data.  gat.py does not import (torch_geometric is absent), so its pieces are taken out of its AST and
executed unchanged:
  * `load_data` (gat.py:43-53) on the train / test pairs of tests/golden/lightgcn_steps.npz: 120 users x 72 items, 1200
    pairs with their duplicates, hubs and isolated ids;
  * the `GATRec` class (gat.py:14-40);
  * `train_model`'s construction of model and optimiser (gat.py:92-101) and the body of its epoch loop (gat.py:104-120:
    zero_grad, forward, `torch.randint` negatives, BPR, backward, Adam step), once per step.
The stand-ins:
  * `GATConv`, a few lines of torch below written from PyG's documented semantics with the defaults gat.py leaves in
    place; it computes in the dtype of x, so the float64 run is float64 throughout, and it draws its attention dropout
    through `F`.  GATConv parity with PyG itself STAYS UNPINNED (the library is absent and the reference holds no fixture);
  * `F`, whose `dropout` draws `rand(shape) >= p` in float32 whatever x's dtype (so both runs of a case draw the same
    masks), records the keep mask, and replays a preset one for the component cases; `elu` passes through.
`torch.randint` and the dropouts draw from the global generator, seeded identically before the loop of every run; the
negatives and masks of every step are read back and the float32 and float64 runs are asserted to have drawn the same.
One thread, so that scatter-adds sum in one order.

Initial parameters: `gat_rules.init_arrays`, a function of a seed, written over the reference's own draws.  LeakyReLU has
a kink at zero: every float64 z = a_src[j] + a_dst[i] of every layer, term and step must keep 8 x its float32 error from
zero (`gat_rules.has_margin`).  Among the first SEEDS_KEPT seeds that do, the one is kept whose smallest non-zero
|step-0 gradient + weight_decay x parameter| is largest: Adam's first update is lr g / (|g| + eps), so one element with
|g| near eps sets a whole parameter's float32 slack (scripts/gen_golden_lightgcn_steps.py); with 29 000 elements no seed
clears a fixed threshold (the best of twelve has 3e-9), so the scan takes the best it sees and stores the figure.
What the scan cannot remove is met on the other side: a parameter's float32 slack is the LARGEST |f32 final - f64 final|
over ORDERS float32 runs of the reference that differ only in the order of edge_index's columns (the same graph, the
same recorded masks edge for edge, the same negatives; index_add_ sums a target's messages in column order, which
neither PyG nor torch fixes, and a GPU's atomics do not even repeat).  With elements at |g| = 3e-9 one run's slack is one
draw of a lottery (between orders it varies by up to 8 x, printed below), and a fixture written from the
file order alone held this project's kernels to 1.86e-6 against 4 x 3.6e-7 on case B's item table while every other
parameter of the three cases sat at 0.02 - 0.6 of its bound.  The file order's own slack is stored beside it.

Contents (tests/gat_rules.py reads them):
  * component cases, every supported (heads, c), pe in {0, 0.5}, on an 8-node graph whose row degrees cycle through
    gat_rules.DEGREES: inputs = functions of a stored seed (checksum stored), the stand-in's float64 out, dh, da_src,
    da_dst, dbias STORED AS FLOAT32 (the file's size cap; it puts at most 2^-24 S on a measured error) and the float32
    run's drift per key;
  * one whole-GATConv case at (2, 64), 12 nodes, dropout 0.5: inputs, the keep mask, float64 out, dx, dW, datt_*, dbias
    (as float32) and drifts;
  * step cases A (defaults without dropout), B (4 heads of 32, slope 0.1, weight_decay 1e-4, no dropout), C (the defaults,
    both dropouts 0.2, masks recorded): per-step loss in both dtypes, step-0 gradients (float32 of float64) and their
    drift, float32(final - initial) of the float64 run, the float32 slack, per parameter."""
import os
import tempfile

import numpy as np
import pandas as pd
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from gen_golden_lightgcn_steps import load_class, save_npz  # noqa: E402
from oracle.gen_golden import REF, load_defs, load_stmts  # noqa: E402
import gat_rules as gr  # noqa: E402
import step_pins as sp  # noqa: E402

PATH = os.path.join(REF, "gat.py")
STEPS, NEG_SEED, SEEDS_KEPT, SEEDS_MAX, ORDERS = 6, 11, 12, 400, 8
DEFAULT = dict(in_channels=64, hidden_channels=64, out_channels=64, num_heads=2, dropout=0.2, edge_dropout=0.2,
               neg_slope=0.2, lr=0.005, weight_decay=0.0)                      # gat.py:130-141
CONFIGS = {"A": dict(DEFAULT, dropout=0.0, edge_dropout=0.0),
           "B": dict(DEFAULT, num_heads=4, hidden_channels=32, neg_slope=0.1, weight_decay=1e-4, dropout=0.0, edge_dropout=0.0),
           "C": dict(DEFAULT)}


class Functional:
    """Stands in for torch.nn.functional in the reference's namespace (module docstring)."""

    def __init__(self):
        self.masks, self.preset = [], []

    def dropout(self, x, p=0.5, training=True):
        if not training or p == 0.0:
            return x
        keep = torch.rand(x.shape, dtype=torch.float32) >= p          # drawn also beside a preset: the generator stays in step
        if self.preset:
            keep = self.preset.pop(0)
        self.masks.append(keep.numpy().copy())
        return x * keep.to(x.dtype) / (1.0 - p)

    def elu(self, x):
        return torch.nn.functional.elu(x)


F = Functional()
Z = []                  # every z the stand-in computed since the last clear, float64 arrays


def aggregate(h, a_src, a_dst, edge_index, heads, slope, p, training, bias):
    """The message passing of PyG's GATConv (concat=True, add_self_loops=True) in h's dtype: h [n, heads * c]."""
    n, c = h.shape[0], h.shape[1] // heads
    off = edge_index[0] != edge_index[1]                      # remove_self_loops, then add_self_loops
    loops = torch.arange(n)
    src, dst = torch.cat([edge_index[0][off], loops]), torch.cat([edge_index[1][off], loops])
    z = a_src[src] + a_dst[dst]
    Z.append(z.detach().double().numpy())
    e = torch.nn.functional.leaky_relu(z, slope)
    top = torch.zeros_like(a_dst).scatter_reduce(0, dst[:, None].expand(-1, heads), e.detach(), "amax", include_self=False)
    alpha = (e - top[dst]).exp()
    alpha = alpha / (torch.zeros_like(a_dst).index_add_(0, dst, alpha)[dst] + 1e-16)
    alpha = F.dropout(alpha, p=p, training=training)
    out = torch.zeros(n, heads, c, dtype=h.dtype).index_add_(0, dst, alpha.unsqueeze(-1) * h.view(n, heads, c)[src])
    return out.view(n, heads * c) + bias


class GATConv(torch.nn.Module):
    """Stand-in for torch_geometric.nn.GATConv (module docstring)."""

    def __init__(self, in_channels, out_channels, heads=1, dropout=0.0, negative_slope=0.2):
        super().__init__()
        self.heads, self.out_channels, self.dropout, self.negative_slope = heads, out_channels, dropout, negative_slope
        self.lin = torch.nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(heads * out_channels))
        for t in (self.lin.weight, self.att_src, self.att_dst):
            a = (6.0 / (t.size(-2) + t.size(-1))) ** 0.5
            torch.nn.init.uniform_(t, -a, a)

    def forward(self, x, edge_index):
        h = self.lin(x)
        hv = h.view(-1, self.heads, self.out_channels)
        return aggregate(h, (hv * self.att_src).sum(-1), (hv * self.att_dst).sum(-1), edge_index, self.heads,
                         self.negative_slope, self.dropout, self.training, self.bias)


def margin(z64, z32):
    return all(gr.has_margin(a, b) for a, b in zip(z64, z32))


class Reference:
    def __init__(self, train, test):
        self.ns = load_defs(PATH, {"load_data"})
        self.ns.update(pd=pd, GATConv=GATConv, F=F)
        load_class(PATH, "GATRec", self.ns)
        self.build = load_stmts(PATH, "train_model", 92, 101)
        self.body = load_stmts(PATH, "train_model", 104, 120)
        tmp = tempfile.mkdtemp()
        for name, arr in (("train.txt", train), ("test.txt", test)):
            with open(os.path.join(tmp, name), "w") as f:
                f.writelines(f"{u} {i} 1\n" for u, i in arr)
        self.data = self.ns["load_data"](os.path.join(tmp, "train.txt"), os.path.join(tmp, "test.txt"))

    def run(self, config, init, dtype, steps=STEPS, order=None, masks=None):
        """gat.py:92-101, the fixture's parameters, then gat.py:104-120 `steps` times -> dict of losses [steps], neg_i
        [steps, E], masks (per step, in call order), z (per call), grad0 and final (float64 arrays by parameter).
        order: a permutation of edge_index's columns (the same graph; index_add_ sums in another order), with `masks` = the
        recorded draws of the run in file order, replayed edge for edge."""
        edge_index, train_df, test_df, num_users, num_items = self.data
        if order is not None:
            edge_index = edge_index[:, torch.from_numpy(order)]
            assert not bool((edge_index[0] == edge_index[1]).any())      # no self loop: term e of a mask is column e
            terms = np.concatenate([order, edge_index.shape[1] + np.arange(num_users + num_items)])
            F.preset[:] = [torch.from_numpy(m[terms] if j % 2 else m) for step in masks for j, m in enumerate(step)]
        env = dict(self.ns, config=dict(config), edge_index=edge_index, train_df=train_df, test_df=test_df,
                   num_users=num_users, num_items=num_items)
        exec(self.build, env)
        model = env["model"].to(dtype)
        assert model.training and type(env["optimizer"]) is torch.optim.Adam
        params = dict(model.named_parameters())
        assert sorted(params) == sorted(gr.PARAMS)
        with torch.no_grad():
            for k in gr.PARAMS:
                params[k].copy_(torch.from_numpy(init[k]).to(dtype))
        torch.manual_seed(NEG_SEED)
        del Z[:], F.masks[:]
        losses, negs, masks, grad0 = [], [], [], None
        for _ in range(steps):
            exec(self.body, env)
            losses.append(float(env["loss"].item()))
            negs.append(env["neg_i"].numpy().copy())
            masks.append(list(F.masks))
            del F.masks[:]
            if grad0 is None:
                grad0 = {k: params[k].grad.detach().double().numpy().copy() for k in gr.PARAMS}
        final = {k: params[k].detach().double().numpy().copy() for k in gr.PARAMS}
        assert not F.preset
        return dict(loss=np.array(losses), neg=np.stack(negs), masks=masks, z=list(Z), grad0=grad0, final=final)


def first_grad(run, init, weight_decay):
    """Smallest non-zero |g| of what Adam's first step sees (an element no term reaches is exactly 0 and stays put)."""
    g = np.concatenate([(run["grad0"][k] + weight_decay * init[k].astype(np.float64)).reshape(-1) for k in gr.PARAMS])
    return float(np.abs(g[g != 0.0]).min())


def same_masks(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))


def component_cases(out):
    dst, src = gr.sweep_graph(gr.COMP_N)
    out["comp/dst"], out["comp/src"] = dst.astype(np.int16), src.astype(np.int16)
    ei = torch.from_numpy(np.stack([src, dst]))
    for heads, c in gr.PAIRS:
        for pe in gr.COMP_PE:
            pre = gr.comp_prefix(heads, c, pe)
            for seed in range(200):
                h, a_src, a_dst, g, bias = gr.inputs(gr.COMP_N, heads, c, seed)
                keep = gr.keep_mask(dst.size + gr.COMP_N, heads, pe, seed)
                res = {}
                for dtype in (torch.float64, torch.float32):
                    del Z[:]
                    F.preset[:] = [] if keep is None else [torch.from_numpy(keep)]
                    t = [torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (h, a_src, a_dst, bias)]
                    o = aggregate(t[0], t[1], t[2], ei, heads, gr.SLOPE, pe, True, t[3])
                    o.backward(torch.from_numpy(g).to(dtype))
                    res[dtype] = dict(zip(gr.KEYS + ("dbias",), [v.double().numpy() for v in
                                                                 (o.detach(), t[0].grad, t[1].grad, t[2].grad, t[3].grad)])), Z[0]
                del F.masks[:]
                if gr.has_margin(res[torch.float64][1], res[torch.float32][1]):
                    break
            else:
                raise AssertionError("no seed with a LeakyReLU margin")
            ref, f32 = res[torch.float64][0], res[torch.float32][0]
            out[pre + "seed"], out[pre + "checksum"] = seed, gr.checksum(h, a_src, a_dst, g, bias, keep)
            drift = gr.drift_of(f32, ref)
            for k, v in ref.items():
                out[pre + k], out[pre + "drift/" + k] = v.astype(np.float32), drift[k]
            print(f"component heads {heads} c {c} pe {pe}: seed {seed}, drift " + " ".join(f"{k} {v:.2g}" for k, v in drift.items()))


def conv_case(out):
    heads, c = gr.CONV_PAIR
    n, cin, pe = gr.CONV_N, gr.CONV_IN, gr.CONV_PE
    dst, src = gr.sweep_graph(n, seed=1)
    ei = torch.from_numpy(np.stack([src, dst]))
    names = ("x", "lin.weight", "att_src", "att_dst", "bias")
    for seed in range(200):
        rng = np.random.default_rng([n, cin, seed])
        x = rng.standard_normal((n, cin)).astype(np.float32)
        g = rng.standard_normal((n, heads * c)).astype(np.float32)
        bias = (0.1 * rng.standard_normal(heads * c)).astype(np.float32)
        keep = rng.random((dst.size + n, heads)) >= pe
        res = {}
        for dtype in (torch.float64, torch.float32):
            torch.manual_seed(seed)
            conv = GATConv(cin, c, heads=heads, dropout=pe, negative_slope=gr.SLOPE)
            with torch.no_grad():
                conv.bias.copy_(torch.from_numpy(bias))
            weights = {k: v.detach().numpy().copy() for k, v in conv.named_parameters()}
            conv = conv.to(dtype).train()
            del Z[:]
            F.preset[:] = [torch.from_numpy(keep)]
            xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
            o = conv(xt, ei)
            o.backward(torch.from_numpy(g).to(dtype))
            p = dict(conv.named_parameters())
            res[dtype] = dict(out=o.detach(), dx=xt.grad, dW=p["lin.weight"].grad, datt_src=p["att_src"].grad,
                              datt_dst=p["att_dst"].grad, dbias=p["bias"].grad), Z[0]
        del F.masks[:]
        if gr.has_margin(res[torch.float64][1], res[torch.float32][1]):
            break
    else:
        raise AssertionError("no seed with a LeakyReLU margin")
    ref, f32 = ({k: v.double().numpy() for k, v in res[d][0].items()} for d in (torch.float64, torch.float32))
    drift = gr.drift_of(f32, ref)
    out.update({"conv/dst": dst.astype(np.int16), "conv/src": src.astype(np.int16), "conv/x": x, "conv/g": g,
                "conv/keep": np.packbits(keep.reshape(-1)), "conv/seed": seed})
    out.update({f"conv/{k}": weights[k] for k in names[1:]})
    for k, v in ref.items():
        out[f"conv/{k}"], out[f"conv/drift/{k}"] = v.astype(np.float32), drift[k]
    print(f"GATConv case: seed {seed}, drift " + " ".join(f"{k} {v:.2g}" for k, v in drift.items()))


def step_case(ref, out, case, cfg):
    _, _, _, num_users, num_items = ref.data
    pre = f"{case}/"
    kept = []
    for seed in range(SEEDS_MAX):
        init = gr.init_arrays(cfg, num_users, num_items, seed)
        r64 = ref.run(cfg, init, torch.float64)
        r32 = ref.run(cfg, init, torch.float32)
        if margin(r64["z"], r32["z"]):
            kept.append((first_grad(r64, init, cfg["weight_decay"]), seed))
            if len(kept) == SEEDS_KEPT:
                break
    assert kept, "no seed with a LeakyReLU margin over all steps"
    first, seed = max(kept)
    init = gr.init_arrays(cfg, num_users, num_items, seed)
    r64, r32 = ref.run(cfg, init, torch.float64), ref.run(cfg, init, torch.float32)
    assert margin(r64["z"], r32["z"])
    assert np.array_equal(r64["neg"], r32["neg"]) and same_masks(r64["masks"], r32["masks"]), "the runs drew differently"
    assert np.isfinite(r64["loss"]).all() and r64["neg"].min() >= 0 and r64["neg"].max() < num_items
    # the float32 slack: the reference's own float32 error over ORDERS orders of edge_index's columns (module docstring)
    rng = np.random.default_rng([seed, ORDERS])
    finals32 = [r32["final"]]
    for _ in range(ORDERS - 1):
        r = ref.run(cfg, init, torch.float32, order=rng.permutation(ref.data[0].shape[1]), masks=r64["masks"])
        assert np.array_equal(r["neg"], r64["neg"]) and np.abs(r["loss"] - r64["loss"]).max() < 1e-5
        finals32.append(r["final"])
    print(f"case {case} {cfg}\n  init seed {seed} of {len(kept)} with a margin ({seed + 1} scanned to it at most), smallest "
          f"non-zero first-step |g| {first:.3g}\n  f64 loss {[f'{x:.9f}' for x in r64['loss']]}")
    out.update({pre + k: v for k, v in cfg.items()})
    out[pre + "init_seed"], out[pre + "init_checksum"], out[pre + "first_grad"] = seed, gr.checksum(*init.values()), first
    out[pre + "neg_i"], out[pre + "f64/loss"], out[pre + "f32/loss"] = r64["neg"].astype(np.uint8), r64["loss"], r32["loss"]
    if cfg["dropout"] or cfg["edge_dropout"]:
        assert all(len(m) == 4 for m in r64["masks"])                  # feature, attention, feature, attention
        for j, name in enumerate(("feat0", "att0", "feat1", "att1")):
            out[pre + name] = np.stack([np.packbits(m[j].reshape(-1)) for m in r64["masks"]])
    else:
        assert not any(r64["masks"])
    for k in gr.PARAMS:
        g64, g32 = r64["grad0"][k], r32["grad0"][k]
        out[f"{pre}f64/grad0/{k}"] = g64.astype(np.float32)
        drift = out[f"{pre}drift/{k}"] = float(np.abs(g32 - g64).max() / np.abs(g64).max())
        delta = (r64["final"][k] - init[k].astype(np.float64)).astype(np.float32)
        assert np.abs(init[k].astype(np.float64) + delta.astype(np.float64) - r64["final"][k]).max() < 4e-9
        out[f"{pre}f64/delta/{k}"] = delta
        slacks = [float(np.abs(f[k] - r64["final"][k]).max()) for f in finals32]
        slack = out[f"{pre}slack/{k}"] = max(slacks)
        out[f"{pre}slack_file_order/{k}"] = slacks[0]
        moved = float(np.abs(r64["final"][k] - init[k]).max())
        print(f"  {k:24s} slack {slack:.3g} (file order {slacks[0]:.3g}, smallest {min(slacks):.3g}) grad drift {drift:.3g} moved {moved:.3g}")
        assert sp.has_moved(moved, max(slack, sp.FLOOR)), (case, k, moved, slack)


def main(out_dir):
    torch.set_num_threads(1)
    lg = sp.load("lightgcn")
    train = np.stack([lg["train_user"], lg["train_item"]], 1).astype(np.int64)
    test = np.stack([lg["test_user"], lg["test_item"]], 1).astype(np.int64)
    ref = Reference(train, test)
    edge_index, train_df, _, num_users, num_items = ref.data
    assert (num_users, num_items, len(train_df), edge_index.shape[1]) == (120, 72, 1200, 2400)
    out = dict(train_user=train[:, 0].astype(np.int16), train_item=train[:, 1].astype(np.int16),
               test_user=test[:, 0].astype(np.int16), test_item=test[:, 1].astype(np.int16), num_users=num_users,
               num_items=num_items, steps=STEPS, neg_seed=NEG_SEED, cases=np.array(sorted(CONFIGS)))
    component_cases(out)
    conv_case(out)
    for case, cfg in CONFIGS.items():
        step_case(ref, out, case, cfg)
    sg.save(out_dir, "gat_steps", out, write=save_npz)


if __name__ == "__main__":
    main(sg.out_dir())
