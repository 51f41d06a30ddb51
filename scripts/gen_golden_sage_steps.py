#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/sage_steps.npz: three single-layer cases of the SAGE layer and six
full-batch training steps of graphsage.py run by the reference itself at three configurations.

Runs ONLY where the reference sources are (like scripts/gen_golden_gat_steps.py, which it follows); the fixture is plain
data.  graphsage.py does not import (torch_geometric is absent), so its pieces are taken out of its AST and executed
unchanged:
  * the `GraphSAGE` class (graphsage.py:15-32);
  * `train_model`'s construction of the model and the optimiser (graphsage.py:88-93, 96) and the body of its epoch loop
    (graphsage.py:99-126: train(), zero_grad, forward, `torch.randint` negatives, BPR or BCE, backward, step), once per
    step,
on the train pairs of tests/golden/lightgcn_steps.npz (120 users x 72 items, 1200 pairs with their duplicates, hubs and
isolated ids) as graphsage.py:41-44 stacks them.  The stand-ins:
  * `SAGEConv`, a few lines of torch below written from PyG's documented semantics with the defaults graphsage.py leaves
    in place (mean aggregation, root weight, bias on lin_l only); it computes in the dtype of x.  SAGEConv parity with
    PyG itself STAYS UNPINNED (the library is absent and the reference holds no fixture);
  * `F`, whose `dropout` draws `rand(shape) >= p` in float32 whatever x's dtype (so both runs of a case draw the same
    masks) and records the keep mask, whose `relu` records its argument (the pre-activations the margin is asked of) and
    whose other functions pass through.
`torch.randint` and the dropouts draw from the global generator, seeded identically before the loop of every run; the
negatives and masks of every step are read back and the float32 and float64 runs are asserted to have drawn the same.
One thread, so that index_add_ sums in one order.

Initial parameters and node features: `sage_rules.init_arrays`, a function of a seed, written over the reference's own
draws.  ReLU has a kink at zero: every float64 pre-activation of every relu layer and step must keep 8 x its float32
error from zero (`sage_rules.has_margin`); seeds are scanned until one does, and among the first SEEDS_KEPT that do the one
is kept whose smallest non-zero |step-0 gradient + weight_decay x parameter| is largest (Adam's first update is
lr g / (|g| + eps), so one element with |g| near eps sets a whole parameter's float32 slack: the GAT writer's reason).  The
margin found is stored.  A parameter's float32 slack is the LARGEST |f32 final - f64 final| over ORDERS float32 runs of
the reference that differ only in the order of edge_index's columns (the same graph, masks and negatives; index_add_ sums
a node's messages in column order, which neither PyG nor torch fixes): one order's slack is one draw of a lottery, as the
GAT writer found.  The file order's own slack is stored beside it.  Sensitivity, as tests/step_pins.py asks: the float64
run with ONE TERM DROPPED — the root term lin_r(x) of every layer — ends more than DROPPED x atol away in every parameter
(`delta_root`), and every parameter moves by more than MOVED x slack.

Contents (tests/sage_rules.py reads them):
  * layer cases sage_rules.COMP_CASES at p = 0.5 on a 12-node graph: inputs = functions of a stored seed (checksum
    stored), the stand-in's float64 h, dx, dwl, dwr, dbias STORED AS FLOAT32 (the file's size cap) and the float32 run's
    drift per key;
  * step cases A (the defaults without dropout), B (gelu, hidden 128, n_layers 3, dropout 0.5 with recorded masks, SGD at
    lr 0.05), C (hidden 32, bce, dropout 0.2, AdamW with weight decay 1e-3): per-step loss in both dtypes, step-0
    gradients (float32 of float64) and their drift, float32(final - initial) of the float64 run, the slacks, delta_root,
    per parameter."""
import os
import types

import numpy as np
import pandas as pd
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from gen_golden_lightgcn_steps import load_class, save_npz  # noqa: E402
from oracle.gen_golden import REF, load_stmts  # noqa: E402
import sage_rules as sr  # noqa: E402
import step_pins as sp  # noqa: E402

PATH = os.path.join(REF, "graphsage.py")
STEPS, NEG_SEED, SEEDS_KEPT, SEEDS_MAX, ORDERS = 6, 11, 6, 400, 6
DEFAULT = dict(hidden_channels=64, n_layers=2, dropout=0.2, activation="relu", lr=0.01, weight_decay=1e-4, optimizer="Adam",
               loss_type="bpr")                                                  # graphsage.py:138-147
CONFIGS = {"A": dict(DEFAULT, dropout=0.0),
           "B": dict(DEFAULT, activation="gelu", hidden_channels=128, n_layers=3, dropout=0.5, optimizer="SGD", lr=0.05),
           "C": dict(DEFAULT, hidden_channels=32, loss_type="bce", optimizer="AdamW", weight_decay=1e-3)}


class Functional:
    """Stands in for torch.nn.functional in the reference's namespace (module docstring)."""

    def __init__(self):
        self.masks, self.preset, self.pre = [], [], []

    def dropout(self, x, p=0.5, training=True):
        if not training or p == 0.0:
            return x
        keep = torch.rand(x.shape, dtype=torch.float32) >= p          # drawn also beside a preset: the generator stays in step
        if self.preset:
            keep = self.preset.pop(0)
        self.masks.append(keep.numpy().copy())
        return x * keep.to(x.dtype) / (1.0 - p)

    def relu(self, x):
        self.pre.append(x.detach().double().numpy().copy())
        return torch.nn.functional.relu(x)

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)


F = Functional()
DROP_ROOT = [False]         # True: the stand-in leaves lin_r(x) out (the sensitivity rerun)


class SAGEConv(torch.nn.Module):
    """Stand-in for torch_geometric.nn.SAGEConv (module docstring)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin_l = torch.nn.Linear(in_channels, out_channels, bias=True)
        self.lin_r = torch.nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x, edge_index):
        src, dst = edge_index[0], edge_index[1]
        n = x.shape[0]
        deg = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, torch.ones(dst.numel(), dtype=x.dtype))
        z = torch.zeros_like(x).index_add_(0, dst, x[src]) / deg.clamp(min=1.0)[:, None]
        out = self.lin_l(z)
        return out if DROP_ROOT[0] else out + self.lin_r(x)


class Reference:
    def __init__(self, train):
        self.ns = dict(torch=torch, nn=torch.nn, F=F, SAGEConv=SAGEConv, device=torch.device("cpu"))
        load_class(PATH, "GraphSAGE", self.ns)
        self.build_model = load_stmts(PATH, "train_model", 88, 93)
        self.build_optimizer = load_stmts(PATH, "train_model", 96, 96)
        self.body = load_stmts(PATH, "train_model", 99, 126)
        self.train_df = pd.DataFrame({"user": train[:, 0], "item": train[:, 1], "rating": 1})
        self.num_users, self.num_items = 120, 72
        u, i = torch.from_numpy(train[:, 0]), torch.from_numpy(train[:, 1])
        self.edge_index = torch.stack([torch.cat([u, i + self.num_users]), torch.cat([i + self.num_users, u])])   # :41-44

    def run(self, config, init, dtype, steps=STEPS, order=None, masks=None, drop_root=False):
        """graphsage.py:88-96, the fixture's parameters and features, then graphsage.py:99-126 `steps` times -> dict of
        losses [steps], neg_i [steps, E], masks and relu pre-activations (per step, in call order), grad0 and final
        (float64 arrays by parameter).  order: a permutation of edge_index's columns, with `masks` = the recorded draws
        replayed (they are per node, so no re-ordering)."""
        edge_index = self.edge_index if order is None else self.edge_index[:, torch.from_numpy(order)]
        F.preset[:] = [] if masks is None else [torch.from_numpy(m) for step in masks for m in step]
        DROP_ROOT[0] = drop_root
        data = types.SimpleNamespace(x=torch.from_numpy(init["x"]).to(dtype), edge_index=edge_index)
        env = dict(self.ns, config=dict(config), data=data, train_df=self.train_df, num_users=self.num_users,
                   num_items=self.num_items)
        exec(self.build_model, env)
        env["model"] = model = env["model"].to(dtype)
        exec(self.build_optimizer, env)
        assert type(env["optimizer"]) is getattr(torch.optim, config["optimizer"])
        params = dict(model.named_parameters())
        names = sr.params_of(config)
        assert sorted(params) == sorted(names)
        with torch.no_grad():
            for k in names:
                params[k].copy_(torch.from_numpy(init[k]).to(dtype))
        torch.manual_seed(NEG_SEED)
        del F.masks[:], F.pre[:]
        losses, negs, all_masks, pres, grad0 = [], [], [], [], None
        for _ in range(steps):
            exec(self.body, env)
            assert model.training
            losses.append(float(env["loss"].item()))
            negs.append(env["neg_i"].numpy().copy())
            all_masks.append(list(F.masks))
            pres.append(list(F.pre))
            del F.masks[:], F.pre[:]
            if grad0 is None:
                grad0 = {k: (torch.zeros_like(params[k]) if params[k].grad is None else params[k].grad).detach().double()
                         .numpy().copy() for k in names}             # no gradient: lin_r in the run without the root term
        final = {k: params[k].detach().double().numpy().copy() for k in names}
        assert not F.preset
        DROP_ROOT[0] = False
        return dict(loss=np.array(losses), neg=np.stack(negs), masks=all_masks, pre=pres, grad0=grad0, final=final)


def margin(r64, r32):
    """(every relu pre-activation of every step keeps the margin, the smallest ratio |pre64| / max |pre32 - pre64|)."""
    pairs = [(a, b) for s64, s32 in zip(r64["pre"], r32["pre"]) for a, b in zip(s64, s32)]
    return all(sr.has_margin(a, b) for a, b in pairs), min([sr.margin_of(a, b) for a, b in pairs], default=np.inf)


def first_grad(run, init, names, weight_decay):
    """Smallest non-zero |g| of what the optimiser's first step sees."""
    g = np.concatenate([(run["grad0"][k] + weight_decay * init[k].astype(np.float64)).reshape(-1) for k in names])
    return float(np.abs(g[g != 0.0]).min())


def same_masks(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))


def component_cases(out):
    src, dst = sr.sweep_graph(sr.COMP_N)
    out["comp/src"], out["comp/dst"] = src.astype(np.int16), dst.astype(np.int16)
    ei = torch.from_numpy(np.stack([src, dst]))
    for din, dout, act in sr.COMP_CASES:
        pre = sr.comp_prefix(din, dout, act)
        for seed in range(200):
            x, wl, wr, bias, g = sr.inputs(sr.COMP_N, din, dout, seed)
            keep = sr.keep_mask(sr.COMP_N, dout, sr.COMP_P, seed)
            res = {}
            for dtype in (torch.float64, torch.float32):
                del F.pre[:]
                F.preset[:] = [torch.from_numpy(keep)]
                conv = SAGEConv(din, dout).to(dtype)
                with torch.no_grad():
                    for p, v in ((conv.lin_l.weight, wl), (conv.lin_r.weight, wr), (conv.lin_l.bias, bias)):
                        p.copy_(torch.from_numpy(v))
                xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
                h = conv(xt, ei)
                h = F.dropout(getattr(F, act)(h) if act != "none" else h, p=sr.COMP_P, training=True)
                h.backward(torch.from_numpy(g).to(dtype))
                vals = (h.detach(), xt.grad, conv.lin_l.weight.grad, conv.lin_r.weight.grad, conv.lin_l.bias.grad)
                res[dtype] = dict(zip(sr.KEYS, [v.double().numpy() for v in vals])), list(F.pre)
            del F.masks[:], F.pre[:]
            if act != "relu" or sr.has_margin(res[torch.float64][1][0], res[torch.float32][1][0]):
                break
        else:
            raise AssertionError("no seed with a ReLU margin")
        ref, f32 = res[torch.float64][0], res[torch.float32][0]
        out[pre + "seed"], out[pre + "checksum"] = seed, sr.checksum(x, wl, wr, bias, g, keep)
        drift = sr.drift_of(f32, ref)
        for k, v in ref.items():
            out[pre + k], out[pre + "drift/" + k] = v.astype(np.float32), drift[k]
        print(f"layer ({din}, {dout}) {act}: seed {seed}, drift " + " ".join(f"{k} {v:.2g}" for k, v in drift.items()))


def step_case(ref, out, case, cfg):
    pre = f"{case}/"
    names = sr.params_of(cfg)
    n_nodes = ref.num_users + ref.num_items
    relu, adam = cfg["activation"] == "relu", cfg["optimizer"] != "SGD"
    kept = []
    for seed in range(SEEDS_MAX):
        init = sr.init_arrays(cfg, n_nodes, seed)
        r64, r32 = ref.run(cfg, init, torch.float64), ref.run(cfg, init, torch.float32)
        if not relu or margin(r64, r32)[0]:
            kept.append((first_grad(r64, init, names, cfg["weight_decay"]), seed))
            if len(kept) == (SEEDS_KEPT if adam else 1):
                break
    assert kept, "no seed with a ReLU margin over all steps"
    first, seed = max(kept)
    init = sr.init_arrays(cfg, n_nodes, seed)
    r64, r32 = ref.run(cfg, init, torch.float64), ref.run(cfg, init, torch.float32)
    ok, ratio = margin(r64, r32)
    assert ok or not relu
    assert np.array_equal(r64["neg"], r32["neg"]) and same_masks(r64["masks"], r32["masks"]), "the runs drew differently"
    assert np.isfinite(r64["loss"]).all() and r64["neg"].min() >= 0 and r64["neg"].max() < ref.num_items
    rng = np.random.default_rng([seed, ORDERS])
    finals32 = [r32["final"]]
    for _ in range(ORDERS - 1):
        r = ref.run(cfg, init, torch.float32, order=rng.permutation(ref.edge_index.shape[1]), masks=r64["masks"])
        assert np.array_equal(r["neg"], r64["neg"]) and np.abs(r["loss"] - r64["loss"]).max() < 1e-5
        finals32.append(r["final"])
    dropped = ref.run(cfg, init, torch.float64, masks=r64["masks"], drop_root=True)
    assert np.array_equal(dropped["neg"], r64["neg"])
    print(f"case {case} {cfg}\n  init seed {seed} of {len(kept)} kept, smallest non-zero first-step |g| {first:.3g}, relu "
          f"margin ratio {ratio:.3g}\n  f64 loss {[f'{x:.9f}' for x in r64['loss']]}")
    out.update({pre + k: v for k, v in cfg.items()})
    out[pre + "init_seed"], out[pre + "init_checksum"], out[pre + "first_grad"] = seed, sr.checksum(*init.values()), first
    out[pre + "relu_margin"] = ratio if relu else 0.0
    out[pre + "neg_i"], out[pre + "f64/loss"], out[pre + "f32/loss"] = r64["neg"].astype(np.uint8), r64["loss"], r32["loss"]
    hidden = sr.n_convs(cfg) - 1
    if cfg["dropout"]:
        assert all(len(m) == hidden for m in r64["masks"])
        for j in range(hidden):
            out[f"{pre}keep{j}"] = np.stack([np.packbits(m[j].reshape(-1)) for m in r64["masks"]])
    else:
        assert not any(r64["masks"])
    for k in names:
        g64, g32 = r64["grad0"][k], r32["grad0"][k]
        out[f"{pre}f64/grad0/{k}"] = g64.astype(np.float32)
        drift = out[f"{pre}drift/{k}"] = float(np.abs(g32 - g64).max() / np.abs(g64).max())
        delta = (r64["final"][k] - init[k].astype(np.float64)).astype(np.float32)
        assert np.abs(init[k].astype(np.float64) + delta.astype(np.float64) - r64["final"][k]).max() < 4e-9
        out[f"{pre}f64/delta/{k}"] = delta
        slacks = [float(np.abs(f[k] - r64["final"][k]).max()) for f in finals32]
        slack = out[f"{pre}slack/{k}"] = max(slacks)
        out[f"{pre}slack_file_order/{k}"] = slacks[0]
        d_root = out[f"{pre}delta_root/{k}"] = float(np.abs(dropped["final"][k] - r64["final"][k]).max())
        moved = float(np.abs(r64["final"][k] - init[k]).max())
        atol = sp.atol_floor_1(slack)
        print(f"  {k:24s} slack {slack:.3g} (file order {slacks[0]:.3g}, smallest {min(slacks):.3g}) grad drift {drift:.3g} "
              f"moved {moved:.3g} d_root {d_root:.3g} ({d_root / atol:.0f}x atol)")
        assert sp.has_moved(moved, max(slack, sp.FLOOR)), (case, k, moved, slack)
        assert sp.sees_dropped(d_root, atol), (case, k, d_root, atol)


def main(out_dir):
    torch.set_num_threads(1)
    lg = sp.load("lightgcn")
    train = np.stack([lg["train_user"], lg["train_item"]], 1).astype(np.int64)
    test = np.stack([lg["test_user"], lg["test_item"]], 1).astype(np.int64)
    ref = Reference(train)
    assert (len(ref.train_df), ref.edge_index.shape[1]) == (1200, 2400)
    assert max(train[:, 0].max(), test[:, 0].max()) + 1 == 120 and max(train[:, 1].max(), test[:, 1].max()) + 1 == 72   # :38-39
    out = dict(train_user=train[:, 0].astype(np.int16), train_item=train[:, 1].astype(np.int16),
               test_user=test[:, 0].astype(np.int16), test_item=test[:, 1].astype(np.int16), num_users=120, num_items=72,
               steps=STEPS, neg_seed=NEG_SEED, cases=np.array(sorted(CONFIGS)))
    component_cases(out)
    for case, cfg in CONFIGS.items():
        step_case(ref, out, case, cfg)
    sg.save(out_dir, "sage_steps", out, write=save_npz)


if __name__ == "__main__":
    main(sg.out_dir())
