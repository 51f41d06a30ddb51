#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/lightgcn_steps.npz: six full-batch training steps of lightgcn.py run by
the reference itself, at four configurations of its own `param_grid`.

Runs ONLY where the reference sources are (like oracle/gen_golden.py, whose `load_defs` / `load_stmts` it uses); the
fixture is plain data.  lightgcn.py does not import (torch_geometric is absent), so its pieces are taken out of its AST and
executed unchanged:
  * `load_data` (lightgcn.py:30-40) on a seeded synthetic train / test file pair;
  * the `LightGCN` class (lightgcn.py:12-27);
  * `train_model`'s construction of model and optimiser (lightgcn.py:79-80: `getattr(torch.optim, ...)(model.parameters(),
    lr, weight_decay)`) and the body of its epoch loop (lightgcn.py:84-120: zero_grad, forward, `torch.randint` negatives,
    BPR or BCE, the regulariser, backward, optimiser step), once per step.
`LGConv` is the ONE stand-in, a few lines of torch below written from PyG's documented semantics as
oracle/oracle_np.py `gcn_norm_weights` states them; it computes in the dtype of x, so the float64 run is float64 throughout.
LGConv parity with PyG itself STAYS UNPINNED (the library is absent and the reference holds no fixture).

The graph: 120 users x 72 items, 1200 training pairs in ITEM-major file order (sorted by item, then user: the file order
differs from the user-major order of the operator's rows, and both the user rows and the item rows of the operator keep
ascending columns, which the windowed companion of the hub rows needs), eight of them copies of other pairs (one pair
three times), seven items and one user with more than 40 pairs (hub rows at the test's forced threshold), and one user id
and one item id that occur only in the test split: isolated nodes, deg^-1/2 = inf -> 0.  The isolated USER never reaches
the loss.  The isolated ITEM does: `torch.randint(0, num_items)` draws it as a negative, and the BCE branch scores every
item, so its row has a gradient that comes through no edge.

`torch.randint` draws from the global generator, seeded identically before the loop of every run of a configuration;
`neg_i` of every step is read back from the exec namespace (also under BCE, where it is drawn and unused) and the
float32 and float64 runs are asserted to have drawn the same.  One thread, so that scatter-adds sum in one order and the
file is reproduced byte for byte.

Per configuration, from the same float32 xavier tables (one pair per width):
  * float64 run: per-step loss, the step-0 gradients of both tables, the final tables as float32(final - init) (exact to
    4e-9, asserted; final = float64(init) + float64(delta));
  * float32 run: per-step loss, and as plain numbers slack = max |f32 final - f64 final| and the step-0 gradients'
    drift = max |f32 - f64| / max |f64|, per table;
  * float64 reruns with reg_weight = 0 (and for B with weight_decay = 0): max |delta final| per table, what a dropped term
    would move.
Asserted here and stored: every table moved by more than 100 x max(slack, 1e-7); every sensitivity figure is above
DROPPED_CPU = 10 times the tests' tolerance (`atol_floor_4` of tests/step_pins.py).

The seed of a width's tables is scanned from 100 + d upward for the first at which, in every Adam configuration of that
width, no element of the gradient that Adam's first step sees (the float64 run's step-0 gradient plus weight_decay x the
table, as torch.optim.Adam adds it) outside the isolated user's row is smaller than 3.2e-7.  Adam's
first update is lr g / (|g| + eps); at |g| ~ eps a float32 rounding of the gradient moves the element by
lr eps / (|g| + eps)^2 per unit of error, and that ONE element sets the whole table's slack: at the first seeds the
reference's own float32 run had 2.9e-7 on A's item table at an element with |g| = 2.0e-7 and 9.2e-7 on C's user table at
one with |g| = 1.6e-7, against 3e-8 to 5e-8 where no such element decides (D, plain SGD, shows the level).  A slack that is
one draw of that lottery is no yardstick for another float32 implementation, in either direction
(scripts/gen_golden_sept_steps.py, which scans at 1e-7 for lr = 1e-3; the amplification grows with lr / |g|^2, so
lr = 1e-2 takes sqrt(10) x 1e-7).  About 4400 seeds are tried at d = 64 (a minute in all); the seeds kept and the smallest
|g| are stored."""
import ast
import os
import tempfile
import zipfile

import numpy as np
import pandas as pd
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from oracle.gen_golden import REF, load_defs, load_stmts  # noqa: E402
import step_pins as sp  # noqa: E402
from step_pins import LIGHTGCN_TABLES as TABLES  # noqa: E402

PATH = os.path.join(REF, "lightgcn.py")

N_USERS, N_ITEMS, N_TRAIN, N_DUP, STEPS = 120, 72, 1200, 8, 6
ISO_USER, ISO_ITEM = 57, 30
HEAVY_USER, HEAVY_USER_DEG, HUB_DEGREE = 7, 45, 40
NEG_SEED = 7
MIN_FIRST_GRAD = 3.2e-7     # see the module docstring
# every value is one of lightgcn.py:143-152's param_grid; A is its default_config
CONFIGS = {
    "A": dict(embedding_dim=64, num_layers=3, loss_type="bpr", n_neg=1, optimizer="Adam", lr=0.01, reg_weight=1e-4,
              weight_decay=0.0),
    "B": dict(embedding_dim=32, num_layers=2, loss_type="bpr", n_neg=3, optimizer="Adam", lr=0.01, reg_weight=1e-4,
              weight_decay=1e-4),
    "C": dict(embedding_dim=128, num_layers=1, loss_type="bce", n_neg=1, optimizer="Adam", lr=0.01, reg_weight=1e-3,
              weight_decay=0.0),
    "D": dict(embedding_dim=64, num_layers=4, loss_type="bpr", n_neg=1, optimizer="SGD", lr=0.05, reg_weight=1e-4,
              weight_decay=0.0),
}


class LGConv(torch.nn.Module):
    """Stand-in for torch_geometric.nn.LGConv (see the module docstring): deg[v] = number of edges with target v;
    w_e = deg^-1/2[src] * deg^-1/2[dst] with inf -> 0; out[dst] += w_e * x[src]; everything in x's dtype."""

    def forward(self, x, edge_index):
        src, dst = edge_index[0], edge_index[1]
        deg = torch.zeros(x.shape[0], dtype=x.dtype).index_add_(0, dst, torch.ones(dst.numel(), dtype=x.dtype))
        dis = deg.pow(-0.5)
        dis[torch.isinf(dis)] = 0.0
        w = dis[src] * dis[dst]
        return torch.zeros_like(x).index_add_(0, dst, w.unsqueeze(1) * x[src])


def load_class(path, name, ns):
    """exec one top-level class of a reference file, unchanged, in `ns`."""
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    assert len(node) == 1, name
    exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, val in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)


def synthetic_pairs(rng):
    """(train [N_TRAIN, 2] in item-major order, test [*, 2]): see the module docstring."""
    users = [u for u in range(N_USERS) if u != ISO_USER]
    items = [i for i in range(N_ITEMS) if i != ISO_ITEM]
    weight = 1.0 / (3.0 + rng.permutation(len(items)))           # skewed popularity: a few items far above the mean
    weight /= weight.sum()
    pairs = {(u, int(rng.choice(items, p=weight))) for u in users}
    pairs |= {(int(rng.choice(users)), i) for i in items}
    pairs |= {(HEAVY_USER, int(i)) for i in rng.choice(items, HEAVY_USER_DEG, replace=False)}
    while len(pairs) < N_TRAIN - N_DUP:
        pairs.add((int(rng.choice(users)), int(rng.choice(items, p=weight))))
    pairs = sorted(pairs)
    dup = [pairs[k] for k in rng.choice(len(pairs), N_DUP - 1, replace=False)]
    dup.append(dup[0])                                            # one pair three times
    train = np.array(sorted(pairs + dup, key=lambda p: (p[1], p[0])), dtype=np.int64)
    have = set(pairs)
    test = [(ISO_USER, 5), (3, ISO_ITEM), (ISO_USER, ISO_ITEM)]
    while len(test) < 40:
        p = (int(rng.choice(users)), int(rng.choice(items)))
        if p not in have and p not in test:
            test.append(p)
    return train, np.array(test, dtype=np.int64)


class Reference:
    def __init__(self, train, test):
        self.ns = load_defs(PATH, {"load_data"})
        self.ns.update(pd=pd, LGConv=LGConv)
        load_class(PATH, "LightGCN", self.ns)
        self.build = load_stmts(PATH, "train_model", 79, 80)
        self.body = load_stmts(PATH, "train_model", 84, 120)
        tmp = tempfile.mkdtemp()
        for name, arr in (("train.txt", train), ("test.txt", test)):
            with open(os.path.join(tmp, name), "w") as f:
                f.writelines(f"{u} {i} 1\n" for u, i in arr)
        self.data = self.ns["load_data"](os.path.join(tmp, "train.txt"), os.path.join(tmp, "test.txt"))

    def run(self, config, init, dtype, steps=STEPS):
        """lightgcn.py:79-80, the fixture's tables, then lightgcn.py:84-120 `steps` times ->
        (losses [steps], neg_i [steps, E(, n_neg)], step-0 gradients, final tables), tables as float64 numpy."""
        edge_index, train_df, test_df, num_users, num_items = self.data
        env = dict(self.ns, config=dict(config), edge_index=edge_index, train_df=train_df, test_df=test_df,
                   num_users=num_users, num_items=num_items)
        exec(self.build, env)
        model = env["model"].to(dtype)
        params = {"user": model.user_embedding.weight, "item": model.item_embedding.weight}
        with torch.no_grad():
            for k in TABLES:
                params[k].copy_(init[k].to(dtype))
        assert type(env["optimizer"]) is getattr(torch.optim, config["optimizer"])
        model.train()
        torch.manual_seed(NEG_SEED)
        losses, negs, grad0 = [], [], None
        for epoch in range(steps):
            env["epoch"] = epoch
            exec(self.body, env)
            losses.append(float(env["loss"].item()))
            negs.append(env["neg_i"].numpy().astype(np.int32))
            if epoch == 0:
                grad0 = {k: params[k].grad.detach().double().numpy().copy() for k in TABLES}
        final = {k: params[k].detach().double().numpy().copy() for k in TABLES}
        return np.array(losses, dtype=np.float64), np.stack(negs), grad0, final


def xavier_tables(d, seed):
    torch.manual_seed(seed)
    return {"user": torch.nn.init.xavier_uniform_(torch.empty(N_USERS, d)),
            "item": torch.nn.init.xavier_uniform_(torch.empty(N_ITEMS, d))}


def smallest_first_grad(grad0, init, weight_decay):
    """Smallest |g| of the gradient Adam's first step sees, g = step-0 gradient + weight_decay x table, outside the
    isolated user's row (no edge and never a negative: 0, or weight_decay x the row, which float32 rounds relatively)."""
    g = {k: grad0[k] + weight_decay * init[k].numpy().astype(np.float64) for k in TABLES}
    gu = np.delete(g["user"], ISO_USER, axis=0)
    return float(min(np.abs(gu).min(), np.abs(g["item"]).min()))


def main(out_dir):
    torch.set_num_threads(1)
    rng = np.random.default_rng(20261019)
    train, test = synthetic_pairs(rng)
    ref = Reference(train, test)
    edge_index, train_df, _, num_users, num_items = ref.data
    assert (num_users, num_items, len(train_df)) == (N_USERS, N_ITEMS, N_TRAIN)
    assert ISO_USER not in train[:, 0] and ISO_ITEM not in train[:, 1]
    assert ISO_USER in test[:, 0] and ISO_ITEM in test[:, 1]
    assert set(range(N_USERS)) - set(train[:, 0].tolist()) == {ISO_USER}
    assert set(range(N_ITEMS)) - set(train[:, 1].tolist()) == {ISO_ITEM}
    uniq, counts = np.unique(train, axis=0, return_counts=True)
    assert len(train) - len(uniq) == N_DUP and counts.max() == 3
    deg_u, deg_i = np.bincount(train[:, 0], minlength=N_USERS), np.bincount(train[:, 1], minlength=N_ITEMS)
    assert (deg_u > HUB_DEGREE).sum() >= 1 and (deg_i > HUB_DEGREE).sum() >= 2, (deg_u.max(), np.sort(deg_i)[-3:])
    user_major = np.lexsort((train[:, 1], train[:, 0]))
    assert not np.array_equal(user_major, np.arange(N_TRAIN))
    print(f"graph: {N_TRAIN} pairs, {N_DUP} copies, hub users {np.flatnonzero(deg_u > HUB_DEGREE).tolist()} "
          f"hub items {np.flatnonzero(deg_i > HUB_DEGREE).tolist()} (degrees {deg_i[deg_i > HUB_DEGREE].tolist()})")

    out = dict(train_user=train[:, 0].astype(np.int32), train_item=train[:, 1].astype(np.int32),
               test_user=test[:, 0].astype(np.int32), test_item=test[:, 1].astype(np.int32),
               num_users=num_users, num_items=num_items, steps=STEPS, configs=np.array(sorted(CONFIGS)),
               iso_user=ISO_USER, iso_item=ISO_ITEM, n_dup=N_DUP, hub_degree=HUB_DEGREE, neg_seed=NEG_SEED,
               min_first_grad=MIN_FIRST_GRAD)

    # one pair of tables per width; the seed scanned as the module docstring says
    inits = {}
    for d in sorted({cfg["embedding_dim"] for cfg in CONFIGS.values()}):
        adam = [c for c, cfg in CONFIGS.items() if cfg["embedding_dim"] == d and cfg["optimizer"] == "Adam"]
        for seed in range(100 + d, 100 + d + 50000):
            init = xavier_tables(d, seed)
            first = min(smallest_first_grad(ref.run(CONFIGS[c], init, torch.float64, steps=1)[2], init,
                                            CONFIGS[c]["weight_decay"]) for c in adam)
            if first >= MIN_FIRST_GRAD:
                break
        else:
            raise AssertionError(f"d = {d}: no table seed satisfies the first-step gradient condition")
        print(f"d = {d}: table seed {seed} (scanned from {100 + d}), smallest step-0 |gradient| of {adam}: {first:.3g}")
        inits[d] = init
        out[f"table_seed_d{d}"], out[f"first_grad_d{d}"] = seed, first
        for k in TABLES:
            out[f"init_d{d}/{k}"] = init[k].numpy()
            assert out[f"init_d{d}/{k}"].dtype == np.float32

    for c, cfg in CONFIGS.items():
        pre = f"{c}/"
        init = inits[cfg["embedding_dim"]]
        out.update({pre + k: v for k, v in cfg.items()})
        l64, n64, g64, p64 = ref.run(cfg, init, torch.float64)
        l32, n32, g32, p32 = ref.run(cfg, init, torch.float32)
        assert np.array_equal(n64, n32), "the float32 and float64 runs drew different negatives"
        assert n64.shape == ((STEPS, N_TRAIN) if cfg["n_neg"] == 1 else (STEPS, N_TRAIN, cfg["n_neg"]))
        assert n64.min() >= 0 and n64.max() < N_ITEMS and (n64 == ISO_ITEM).any()
        assert np.isfinite(l64).all() and (np.abs(l32 - l64) <= 1e-5 * np.abs(l64)).all()
        out[pre + "neg_i"], out[pre + "f64/loss"], out[pre + "f32/loss"] = n64, l64, l32
        print(f"config {c} {cfg}\n  f64 loss {[f'{x:.9f}' for x in l64]}")
        reruns = {"reg": ref.run(dict(cfg, reg_weight=0.0), init, torch.float64)[3]}
        if cfg["weight_decay"]:
            reruns["wd"] = ref.run(dict(cfg, weight_decay=0.0), init, torch.float64)[3]
        for k in TABLES:
            out[f"{pre}f64/grad0/{k}"] = g64[k]
            drift = out[f"{pre}drift/{k}"] = float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max())
            moved = out[f"{pre}moved/{k}"] = float(np.abs(p64[k] - init[k].numpy().astype(np.float64)).max())
            slack = sg.record_table(out, pre, "lightgcn", k, p64[k], p32[k], reruns, init=init[k].numpy(), store_init=False,
                                    exact=4e-9, factor=sp.DROPPED_CPU, extra=f" grad drift {drift:.3g} moved {moved:.3g}")
            assert sp.has_moved(moved, max(slack, sp.FLOOR)), (c, k, moved, slack)
        # the isolated user: no gradient at all; the isolated item: a gradient that comes through no edge
        assert not g64["user"][ISO_USER].any() and g64["item"][ISO_ITEM].any()

    sg.save(out_dir, "lightgcn_steps", out, write=save_npz)


if __name__ == "__main__":
    main(sg.out_dir())
