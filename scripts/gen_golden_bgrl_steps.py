#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/bgrl_steps.npz: three single-layer cases of the GIN layer and up to
six full-batch training steps of univariate/bgrl_g2l.py run by the reference itself at three configurations.

Runs ONLY where the reference sources are (like scripts/gen_golden_sage_steps.py, which it follows); the fixture is plain
data.  bgrl_g2l.py does not import (torch_geometric, torch_scatter and sklearn are absent), so its pieces are taken out of
its AST and executed unchanged:
  * the classes `Interaction`, `Graph`, `Augmentor`, `Compose`, `FeatureMasking`, `EdgeRemoving`, `Loss`, `BootstrapLatent`,
    `Sampler`, `SameScaleSampler`, `CrossScaleSampler`, `BootstrapContrast`, `Normalize`, `GConv`, `Encoder` and the functions
    `drop_feature`, `make_gin_conv`, `get_sampler`, `add_extra_mask`;
  * main's construction of the augmentors, the encoder, the contrast model and the optimiser (bgrl_g2l.py:648-661), the
    body of `train` (bgrl_g2l.py:576-582), once per step, and `GraphRecommender.predict`'s statements (bgrl_g2l.py:157-163),
on the train pairs of tests/golden/lightgcn_steps.npz (119 users and 71 items occur, 1200 pairs with their duplicates and
hubs) as `Interaction._build_adj` and `build_movielens_graph` stack them (bgrl_g2l.py:106-123).  The stand-ins, a few lines
each, written from PyG's and torch's documented semantics:
  * `GINConv(nn)`: out = nn(sum_j x_j + (1 + eps) x_i), eps = 0, in the dtype of x; GINConv parity with PyG itself STAYS
    UNPINNED (the library is absent and the reference holds no fixture);
  * `global_add_pool(x, batch)`: the column sum of one graph;  `dropout_adj(edge_index, edge_attr, p)`: `rand(E) >= p` keeps;
  * `F`, whose `dropout` draws `rand(shape) >= p` in float32 whatever x's dtype (so both runs of a case draw the same
    masks) and records the keep mask; `torch.nn.Dropout` likewise (the lifted classes see `torch.nn` through a proxy);
    `torch.nn.ReLU` and `torch.nn.PReLU` record their arguments (the kinks the margin is asked of).
Every draw comes from the global generator, seeded identically before the loop of every run; the masks of every step are
read back and the float32 and float64 runs are asserted to have drawn the same.  One thread, so that index_add_ sums in one
order.

Initial parameters and the node table: `gin_rules.init_arrays`, a function of a seed, written over the reference's own
draws.  ReLU and PReLU have a kink at zero: every float64 argument of every one of them in every step must keep 8 x its
float32 error from zero (`gin_rules.has_margin`); seeds are scanned (SEEDS_MAX, the SAGE writer's limit).  Over six steps
no seed does, on this graph or on one of 26 nodes: a step has some 10^5 such arguments (four encoder passes and the
predictor's two), and from the third Adam step on the float32 and float64 parameters are 1e-5 apart, which the arguments
inherit (best ratio of 40 seeds on the full graph by number of steps, case A: 23, 11, 3.0, 1.1, 0.2, 0.1; case C: 3.3,
0.08, ...).  The margin is not loosened; a case is SHRUNK instead until a seed keeps it: first in steps (from STEPS = 6 down
to MIN_STEPS = 2), then in training pairs (the first 1200, 600, ... of the file's); a seed whose record does not meet the sensitivity
conditions below (one-element PReLU weights move by Adam's lr x sign in the first steps, almost whatever the gradient) is
passed over in the same way.  The steps and pairs a case ended with are
stored (`<case>/steps`, `<case>/n_pairs`).  Among the first SEEDS_KEPT seeds that keep the margin over that many steps the
one is kept whose smallest non-zero |step-0 gradient + weight_decay x parameter| is largest (the SAGE writer's reason).  A tensor's float32 slack is the LARGEST |f32 final - f64 final| over
ORDERS float32 runs that differ only in the order of edge_index's columns.  Sensitivity, as tests/step_pins.py asks: the
float64 run with ONE TERM DROPPED — the root term (1 + eps) x_i of every layer — ends more than DROPPED x atol away in every
tensor the loss reaches (`delta_root`), and every such tensor moves by more than MOVED x slack; gin_rules.UNREACHED names the
three per encoder that the loss does not reach and says why.

Contents (tests/gin_rules.py reads them):
  * layer cases gin_rules.COMP_CASES at p = 0.5 and edge_p = 0.3 on a 12-node graph: inputs = functions of a stored seed
    (checksum stored), the stand-in's float64 h, dx, dw1, db1, dw2, db2 STORED AS FLOAT32 (the file's size cap) and the
    float32 run's drift per key;
  * step cases A (the defaults with every configurable drop probability 0), B (hidden 64, 3 layers, dropout 0.5, edge_p 0.3,
    feat_p 0.3), C (hidden 128, 1 layer, the defaults otherwise), each with its recorded masks: per-step loss in both dtypes,
    float32(final - initial) of the float64 run for every parameter of the online encoder, the predictor and the target
    encoder and for both running buffers of the five BatchNorms, the slacks, delta_root, and the eval-mode scores of
    SCORE_USERS users after the last step with their float32 drift."""
import ast
import os
import types

import numpy as np
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from gen_golden_lightgcn_steps import save_npz  # noqa: E402
from oracle.gen_golden import REF, load_stmts  # noqa: E402
import gin_rules as gr  # noqa: E402
import step_pins as sp  # noqa: E402

PATH = os.path.join(REF, "univariate", "bgrl_g2l.py")
STEPS, MIN_STEPS, DRAW_SEED, SEEDS_KEPT, SEEDS_MAX, ORDERS, SCORE_USERS = 6, 2, 11, 6, 400, 6, 8
PAIR_COUNTS = (1200, 600, 300, 150, 75, 40, 24, 16, 12)
DEFAULT = dict(hidden_dim=32, num_layers=2, dropout=0.2, lr=1e-2, batch_size=128, edge_p=0.2, feat_p=0.1, momentum=0.99,
               weight_decay=1e-5, activation=torch.nn.ReLU)                      # bgrl_g2l.py:622-633
CONFIGS = {"A": dict(DEFAULT, dropout=0.0, edge_p=0.0, feat_p=0.0),
           "B": dict(DEFAULT, hidden_dim=64, num_layers=3, dropout=0.5, edge_p=0.3, feat_p=0.3),
           "C": dict(DEFAULT, hidden_dim=128, num_layers=1)}
LIFTED = ("Interaction", "Graph", "Augmentor", "Compose", "drop_feature", "FeatureMasking", "Loss", "BootstrapLatent",
          "EdgeRemoving", "Sampler", "SameScaleSampler", "CrossScaleSampler", "get_sampler", "add_extra_mask",
          "BootstrapContrast", "Normalize", "make_gin_conv", "GConv", "Encoder")


class Recorder:
    def __init__(self):
        self.node, self.edge, self.feat, self.kinks = [], [], [], []
        self.node_preset, self.edge_preset = [], []
        self.drop_root = False

    def clear(self):
        del self.node[:], self.edge[:], self.feat[:], self.kinks[:]

    def keep(self, shape, p, preset, record):
        keep = torch.rand(shape, dtype=torch.float32) >= p            # drawn also beside a preset: the generator stays in step
        if preset:
            keep = preset.pop(0)
        record.append(keep.numpy().copy())
        return keep


REC = Recorder()


class Functional:
    """Stands in for torch.nn.functional in the reference's namespace (module docstring)."""

    def dropout(self, x, p=0.5, training=True):
        if not training or p == 0.0:
            return x
        return x * REC.keep(x.shape, p, REC.node_preset, REC.node).to(x.dtype) / (1.0 - p)

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)


F = Functional()


class Dropout(torch.nn.Module):
    def __init__(self, p=0.5):
        super().__init__()
        self.p = p

    def forward(self, x):
        return F.dropout(x, self.p, self.training)


class ReLU(torch.nn.ReLU):
    def forward(self, x):
        REC.kinks.append(x.detach().double().numpy().copy())
        return super().forward(x)


class PReLU(torch.nn.PReLU):
    def forward(self, x):
        REC.kinks.append(x.detach().double().numpy().copy())
        return super().forward(x)


class Proxy:
    """`base` with some attributes replaced."""

    def __init__(self, base, **over):
        self.__dict__.update(_base=base, _over=over)

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(self._base, name)


NN = Proxy(torch.nn, Dropout=Dropout, ReLU=ReLU, PReLU=PReLU)
TORCH = Proxy(torch, nn=NN)


class GINConv(torch.nn.Module):
    """Stand-in for torch_geometric.nn.GINConv (module docstring)."""

    def __init__(self, nn, eps=0.0):
        super().__init__()
        self.nn, self.eps = nn, eps

    def forward(self, x, edge_index, size=None):
        out = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]])
        if not REC.drop_root:
            out = out + (1 + self.eps) * x
        return self.nn(out)


def global_add_pool(x, batch):
    return x.sum(dim=0, keepdim=True)


def dropout_adj(edge_index, edge_attr=None, p=0.5):
    if p == 0.0:
        return edge_index, edge_attr
    keep = REC.keep((edge_index.shape[1],), p, REC.edge_preset, REC.edge)
    return edge_index[:, keep], None


def lift(ns):
    """exec the LIFTED top-level classes and functions of bgrl_g2l.py, unchanged and in file order, in `ns`."""
    tree = ast.parse(open(PATH).read())
    nodes = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in LIFTED]
    assert sorted(n.name for n in nodes) == sorted(LIFTED)
    exec(compile(ast.Module(body=nodes, type_ignores=[]), PATH, "exec"), ns)


class Reference:
    def __init__(self, train, test):
        import abc
        import copy
        import typing
        self.ns = dict(torch=TORCH, nn=NN, F=F, np=np, copy=copy, ABC=abc.ABC, abstractmethod=abc.abstractmethod,
                       Optional=typing.Optional, Tuple=typing.Tuple, NamedTuple=typing.NamedTuple, List=typing.List,
                       GINConv=GINConv, global_add_pool=global_add_pool, dropout_adj=dropout_adj, Adam=torch.optim.Adam,
                       device=torch.device("cpu"))
        lift(self.ns)
        drop_feature = self.ns["drop_feature"]

        def recording_drop_feature(x, drop_prob):
            out = drop_feature(x, drop_prob)
            REC.feat.append(~((out == 0).all(dim=0) & ~(x == 0).all(dim=0)).numpy())
            return out

        self.ns["drop_feature"] = recording_drop_feature
        self.build = load_stmts(PATH, "main", 648, 661)
        self.body = load_stmts(PATH, "train", 576, 582)
        self.predict = load_stmts(PATH, "GraphRecommender.predict", 157, 163)
        triples = lambda a: [[int(u), int(i), 1.0] for u, i in a]                        # noqa: E731
        self.data = self.ns["Interaction"]({}, triples(train), triples(test))
        adj = self.data.norm_adj.tocoo()
        self.edge_index = torch.tensor(np.stack([adj.row, adj.col]), dtype=torch.long)   # bgrl_g2l.py:122-123
        self.n_nodes = self.data.user_num + self.data.item_num

    def run(self, config, init, dtype, steps=STEPS, order=None, masks=None, drop_root=False):
        """bgrl_g2l.py:648-661, the fixture's parameters and table, then bgrl_g2l.py:576-582 `steps` times -> dict of losses
        [steps], the recorded masks and kink arguments per step, grad0, final (float64 arrays by state_dict name) and the
        eval-mode scores of the first SCORE_USERS users.  order: a permutation of edge_index's columns, with `masks` = the
        recorded draws replayed (the edge masks re-ordered with it)."""
        edge_index = self.edge_index if order is None else self.edge_index[:, torch.from_numpy(order)]
        REC.node_preset[:] = [] if masks is None else [torch.from_numpy(m) for step in masks for m in step["node"]]
        REC.edge_preset[:] = [] if masks is None else \
            [torch.from_numpy(m if order is None else m[order]) for step in masks for m in step["edge"]]
        REC.drop_root = drop_root
        data = types.SimpleNamespace(x=torch.from_numpy(init["x"]).to(dtype), edge_index=edge_index)
        env = dict(self.ns, param_config=dict(config), data=data)
        exec(self.build, env)
        encoder = env["encoder"] = env["encoder"].to(dtype)
        assert type(env["optimizer"]) is torch.optim.Adam and encoder.target_encoder is None
        params = dict(encoder.named_parameters())
        names = [k for k in gr.tensor_shapes(config, buffers=False) if not k.startswith("target_encoder.")]
        assert sorted(params) == sorted(names), sorted(set(params) ^ set(names))
        with torch.no_grad():
            for k in names:
                if k in init:
                    params[k].copy_(torch.from_numpy(init[k]).to(dtype))
        env.update(encoder_model=encoder, contrast_model=env["contrast"], momentum=config["momentum"])
        torch.manual_seed(DRAW_SEED)
        REC.clear()
        losses, all_masks, kinks, grad0 = [], [], [], None
        for _ in range(steps):
            exec(self.body, env)
            assert encoder.training and encoder.target_encoder.training
            losses.append(float(env["loss"].item()))
            all_masks.append(dict(node=list(REC.node), edge=list(REC.edge), feat=list(REC.feat)))
            kinks.append(list(REC.kinks))
            REC.clear()
            if grad0 is None:
                grad0 = {k: params[k].grad.detach().double().numpy().copy() for k in names}
        state = encoder.state_dict()
        final = {k: state[k].detach().double().numpy().copy() for k in gr.tensor_shapes(config)}
        assert not REC.node_preset and not REC.edge_preset
        scores = []
        graph = types.SimpleNamespace(x=data.x, edge_index=self.edge_index)
        me = types.SimpleNamespace(encoder=encoder, graph=graph, data=self.data)
        for user in sorted(self.data.user)[:SCORE_USERS]:
            penv = dict(self.ns, self=me, user=user)
            exec(self.predict, penv)
            scores.append(penv["scores"].double().numpy().copy())
        REC.clear()
        REC.drop_root = False
        return dict(loss=np.array(losses), masks=all_masks, kinks=kinks, grad0=grad0, final=final, scores=np.stack(scores))


def margin(r64, r32, steps=None):
    """(every ReLU and PReLU argument of the first `steps` steps keeps the margin, the smallest ratio
    |arg64| / max |arg32 - arg64|)."""
    pairs = [(a, b) for s64, s32 in zip(r64["kinks"][:steps], r32["kinks"][:steps]) for a, b in zip(s64, s32)]
    return all(gr.has_margin(a, b) for a, b in pairs), min([gr.margin_of(a, b) for a, b in pairs], default=np.inf)


def margin_steps(r64, r32):
    """The number of leading steps over which the margin holds."""
    n = 0
    while n < len(r64["kinks"]) and margin(r64, r32, n + 1)[0]:
        n += 1
    return n


def scan(ref, cfg):
    """(steps, [(first_grad, seed)]) over SEEDS_MAX seeds: the largest number of leading steps any seed keeps the margin
    over, and the first SEEDS_KEPT seeds that keep it that long."""
    held = []
    for seed in range(SEEDS_MAX):
        init = gr.init_arrays(cfg, ref.n_nodes, seed)
        r64, r32 = ref.run(cfg, init, torch.float64, MIN_STEPS), ref.run(cfg, init, torch.float32, MIN_STEPS)
        if margin_steps(r64, r32) == MIN_STEPS:         # the same draws, so the longer runs begin with these steps
            r64, r32 = ref.run(cfg, init, torch.float64), ref.run(cfg, init, torch.float32)
        held.append((margin_steps(r64, r32), first_grad(r64, init, cfg["weight_decay"]), seed))
    steps = max(h[0] for h in held)
    return steps, [(fg, seed) for n, fg, seed in held if n >= steps][:SEEDS_KEPT]


def first_grad(run, init, weight_decay):
    """Smallest non-zero |g| of what the optimiser's first step sees, over the parameters the loss reaches."""
    g = np.concatenate([(v + weight_decay * init[k].astype(np.float64)).reshape(-1) if k in init else v.reshape(-1)
                        for k, v in run["grad0"].items() if not gr.is_unreached(k)])
    return float(np.abs(g[g != 0.0]).min())


def same_masks(a, b):
    return len(a) == len(b) and all(len(x[k]) == len(y[k]) and all(np.array_equal(p, q) for p, q in zip(x[k], y[k]))
                                    for x, y in zip(a, b) for k in ("node", "edge", "feat"))


def component_cases(out):
    src, dst = gr.sweep_graph(gr.COMP_N)
    out["comp/src"], out["comp/dst"] = src.astype(np.int16), dst.astype(np.int16)
    ns = dict(torch=TORCH, GINConv=GINConv)
    lift_one = [n for n in ast.parse(open(PATH).read()).body if isinstance(n, ast.FunctionDef) and n.name == "make_gin_conv"]
    exec(compile(ast.Module(body=lift_one, type_ignores=[]), PATH, "exec"), ns)
    for din, dout in gr.COMP_CASES:
        pre = gr.comp_prefix(din, dout)
        for seed in range(200):
            x, w1, b1, w2, b2, g = gr.inputs(gr.COMP_N, din, dout, seed)
            keep, ek = gr.keep_mask(gr.COMP_N, dout, gr.COMP_P, seed), gr.edge_mask(src.size, gr.COMP_EDGE_P, seed)
            ei = torch.from_numpy(np.stack([src, dst])[:, ek])
            res = {}
            for dtype in (torch.float64, torch.float32):
                REC.clear()
                REC.node_preset[:] = [torch.from_numpy(keep)]
                conv = ns["make_gin_conv"](din, dout).to(dtype)
                with torch.no_grad():
                    for p, v in ((conv.nn[0].weight, w1), (conv.nn[0].bias, b1), (conv.nn[2].weight, w2), (conv.nn[2].bias, b2)):
                        p.copy_(torch.from_numpy(v))
                xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
                h = F.dropout(ReLU()(conv(xt, ei)), p=gr.COMP_P, training=True)          # bgrl_g2l.py:527-529
                h.backward(torch.from_numpy(g).to(dtype))
                vals = (h.detach(), xt.grad, conv.nn[0].weight.grad, conv.nn[0].bias.grad, conv.nn[2].weight.grad, conv.nn[2].bias.grad)
                res[dtype] = dict(zip(gr.KEYS, [v.double().numpy() for v in vals])), list(REC.kinks)
            REC.clear()
            if all(gr.has_margin(a, b) for a, b in zip(res[torch.float64][1], res[torch.float32][1])):
                break
        else:
            raise AssertionError("no seed with a ReLU margin")
        ref, f32 = res[torch.float64][0], res[torch.float32][0]
        out[pre + "seed"], out[pre + "checksum"] = seed, gr.checksum(x, w1, b1, w2, b2, g, keep, ek)
        drift = gr.drift_of(f32, ref)
        for k, v in ref.items():
            out[pre + k], out[pre + "drift/" + k] = v.astype(np.float32), drift[k]
        print(f"layer ({din}, {dout}): seed {seed}, drift " + " ".join(f"{k} {v:.2g}" for k, v in drift.items()))


def step_case(train, test, out, case, cfg):
    """Shrinks the case (module docstring) until a seed keeps the margin over at least MIN_STEPS steps AND the record it
    gives meets the sensitivity conditions; the seeds of a size are tried in the order of their first-step gradients."""
    for n_pairs in PAIR_COUNTS:
        ref = Reference(train[:n_pairs], test)
        steps, kept = scan(ref, cfg)
        print(f"case {case}: {n_pairs} pairs ({ref.n_nodes} nodes): the margin holds over {steps} steps at best ({len(kept)} seeds)")
        if steps < MIN_STEPS:
            continue
        for first, seed in sorted(kept, reverse=True):
            entries, bad = record_case(ref, cfg, case, seed, steps, n_pairs, first, len(kept))
            if not bad:
                out.update(entries)
                return
            print(f"  seed {seed}: not sensitive enough: {bad}")
    raise AssertionError(f"case {case}: no seed with a margin over {MIN_STEPS} steps and a sensitive record at any size")


def record_case(ref, cfg, case, seed, steps, n_pairs, first, n_kept):
    pre, out = f"{case}/", {}
    init = gr.init_arrays(cfg, ref.n_nodes, seed)
    r64, r32 = ref.run(cfg, init, torch.float64, steps), ref.run(cfg, init, torch.float32, steps)
    ok, ratio = margin(r64, r32)
    assert ok and same_masks(r64["masks"], r32["masks"]), "the runs drew differently"
    assert np.isfinite(r64["loss"]).all()
    assert all(len(m["node"]) == gr.n_node_masks(cfg) for m in r64["masks"])
    out[pre + "steps"], out[pre + "n_pairs"] = steps, n_pairs
    out[pre + "num_users"], out[pre + "num_items"] = ref.data.user_num, ref.data.item_num
    out[pre + "score_users"] = np.array(sorted(ref.data.user)[:SCORE_USERS], dtype=np.int16)
    rng = np.random.default_rng([seed, ORDERS])
    finals32 = [r32["final"]]
    for _ in range(ORDERS - 1):
        r = ref.run(cfg, init, torch.float32, steps, order=rng.permutation(ref.edge_index.shape[1]), masks=r64["masks"])
        assert same_masks(r["masks"], r64["masks"]) or cfg["edge_p"] > 0
        assert np.abs(r["loss"] - r64["loss"]).max() < 1e-4, (r["loss"], r64["loss"])
        finals32.append(r["final"])
    dropped = ref.run(cfg, init, torch.float64, steps, masks=r64["masks"], drop_root=True)
    print(f"case {case} {({k: v for k, v in cfg.items() if k != 'activation'})}\n  init seed {seed} of {n_kept} kept, smallest "
          f"non-zero first-step |g| {first:.3g}, kink margin ratio {ratio:.3g}\n  f64 loss {[f'{x:.9f}' for x in r64['loss']]}")
    out.update({pre + k: cfg[k] for k in gr.CONFIG_INTS + gr.CONFIG_FLOATS})
    out[pre + "init_seed"], out[pre + "init_checksum"], out[pre + "first_grad"] = seed, gr.checksum(*init.values()), first
    out[pre + "kink_margin"] = ratio
    out[pre + "f64/loss"], out[pre + "f32/loss"] = r64["loss"], r32["loss"]
    out[pre + "node"] = np.stack([np.stack([np.packbits(m.reshape(-1)) for m in step["node"]]) for step in r64["masks"]])
    for k in ("edge", "feat"):
        if cfg[k + "_p"] > 0:
            out[pre + k] = np.stack([np.stack([np.packbits(m) for m in step[k]]) for step in r64["masks"]])
    out[pre + "f64/scores"] = r64["scores"].astype(np.float32)
    out[pre + "drift/scores"] = float(np.abs(r32["scores"] - r64["scores"]).max() / np.abs(r64["scores"]).max())
    first_t, bad = gr.initial_tensors(cfg, init), []
    for k in gr.tensor_shapes(cfg):
        delta = (r64["final"][k] - first_t[k]).astype(np.float32)
        # float32 of the difference: exact to 4e-9 for a parameter, to 2^-24 of its size for a running statistic
        assert np.abs(first_t[k] + delta.astype(np.float64) - r64["final"][k]).max() <= max(4e-9, 2.0 ** -24 * np.abs(delta).max())
        out[f"{pre}f64/delta/{k}"] = delta
        slacks = [float(np.abs(f[k] - r64["final"][k]).max()) for f in finals32]
        slack = out[f"{pre}slack/{k}"] = max(slacks)
        d_root = out[f"{pre}delta_root/{k}"] = float(np.abs(dropped["final"][k] - r64["final"][k]).max())
        moved = float(np.abs(r64["final"][k] - first_t[k]).max())
        atol = sp.atol_floor_1(slack)
        print(f"  {k:52s} slack {slack:.3g} (file order {slacks[0]:.3g}) moved {moved:.3g} d_root {d_root:.3g} "
              f"({d_root / atol:.0f}x atol)")
        if not gr.is_unreached(k) and not sp.has_moved(moved, max(slack, sp.FLOOR)):
            bad.append(("has_moved", case, k, moved, slack))
        if not gr.is_unreached(k) and not sp.sees_dropped(d_root, atol):
            bad.append(("sees_dropped", case, k, d_root, atol))
    return out, bad


def main(out_dir):
    torch.set_num_threads(1)
    lg = sp.load("lightgcn")
    train = np.stack([lg["train_user"], lg["train_item"]], 1).astype(np.int64)
    test = np.stack([lg["test_user"], lg["test_item"]], 1).astype(np.int64)
    out = dict(train_user=train[:, 0].astype(np.int16), train_item=train[:, 1].astype(np.int16), draw_seed=DRAW_SEED,
               cases=np.array(sorted(CONFIGS)))
    component_cases(out)
    for case, cfg in CONFIGS.items():
        step_case(train, test, out, case, cfg)
    sg.save(out_dir, "bgrl_steps", out, write=save_npz)


if __name__ == "__main__":
    main(sg.out_dir())
