#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/diffnet_steps.npz: six training steps of univariate/diffnet.py run by the
reference itself, and one component case per width for the fused layer kernels.

Runs ONLY where the reference sources are (like scripts/gen_golden_mhcn_steps.py; the data set and the helpers are
scripts/step_golden.py's); the fixture is plain data.  diffnet.py imports numba for one decorator of a function nothing
here calls: an inert stand-in module takes its place and the file imports as it is.  A `DiffNet` is constructed on
`step_golden.synthetic_lists` (the social list deep-copied: the cleaning of :903-908 deletes from it in place); `initModel`
draws the tables and the weights under a seed; the optimizer statement :1096-1100 and the loop body :1103-1119 are lifted
with `oracle.gen_golden.load_stmts` and executed unchanged, once per batch.  The batches are the first six of the
reference's own sampler (seeded), one per pass: the batch is the whole training list (1401 triples), because the
loss is a sum and the weights' first-step gradients, products of 0.005-scale tables, only reach Adam's eps range at that size.

Per configuration (n_layer 2, d 64) and (n_layer 3, d 32), from the same float32 initial parameters, what tests/step_pins.py
describes: a float64 run (parameters, S and A cast; per step rec / reg / total, the finals as float32(final - init)), a
float32 run (terms, per-table slack) and float64 reruns with one part dropped: `social` (S's values zeroed: the S X half
of every layer), `rating` (A's values zeroed: the A items addend), `reg` (regU = 0).  'regU' is in the conf, so regU =
reg_lambda = 0.1 (the top of the reference's grid, :1164) with lr = 1e-4: step_pins' sensitivity rule holds by orders of magnitude,
which is asserted; at lr = 1e-3 and above the two precisions' Adam trajectories part by more than the ReLU margin allows
(Adam moves an element by about lr whatever its gradient's size, min |pre-activation| over the run is about 1e-7).

The seed of the initial state is scanned from 3 + c upward for the first that meets two conditions, both stored:
  * Adam: the smallest non-zero |gradient| of the float64 run's FIRST step is at least 1e-7 (10 x Adam's eps; below it the
    update depends on eps in a way float32 cannot follow);
  * ReLU margin: over every layer and step, min |pre-activation| of the float64 run is at least 8 x max |f32 - f64| of
    those pre-activations in the reference's own two runs (otherwise the two runs, and any float32 implementation, may
    take different ReLU masks and a gradient pin compares two different functions).  The pre-activations are what the
    reference hands to `torch.relu`, recorded by a wrapper.

Component cases, d in {32, 64, 128}, n = 70 rows: S has an empty row, a degree-1 row, a self-loop, a 300-entry row with
repeated columns and a non-empty last row; x, w, g are drawn by tests/diffnet_fixture.py's `component_inputs` (the file
stores the seed, not the arrays), g with exact zeros.  The statements :1127-1130 of `DiffNet.forward` run once under
float64 autograd; h, dx, dw are stored with the float32 drift of each (max |f32 - f64| / max |f64|).  The seed is scanned
for the same ReLU margin."""
import copy
import itertools
import os
import random
import sys
import types

import numpy as np
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from oracle.gen_golden import REF, load_stmts  # noqa: E402  (puts the reference's univariate/ on sys.path)
import diffnet_fixture as dfx  # noqa: E402

sys.modules.setdefault("numba", types.SimpleNamespace(jit=lambda *a, **k: (lambda f: f)))
import diffnet as ref  # noqa: E402

PATH = os.path.join(REF, "univariate", "diffnet.py")
BATCH, STEPS, BATCH_SEED, SCAN = sg.N_TRAIN + 1, 6, 7, 20000
MIN_FIRST_GRAD, RELU_MARGIN = 1e-7, 8.0
BASE = {"lr": 1e-4, "reg_lambda": 1e-1}
CONFIGS = [dict(n_layer=2, d=64), dict(n_layer=3, d=32)]
OPTIMIZER = load_stmts(PATH, "DiffNet.trainModel", 1096, 1100)
BODY = load_stmts(PATH, "DiffNet.trainModel", 1103, 1119)
LAYER = load_stmts(PATH, "DiffNet.forward", 1127, 1130)
WEIGHTS = load_stmts(PATH, "DiffNet.initModel", 1087, 1090)
DROPS = ("social", "rating", "reg")


def conf_of(cfg, hp):
    return {"evaluation.setup": "off", "emb_size": cfg["d"], "batch_size": BATCH, "factors": 10, "lr": hp["lr"],
            "reg_lambda": hp["reg_lambda"], "reg_lambda_u": 0.0, "reg_lambda_i": 0.0, "reg_lambda_b": 0.0, "reg_lambda_s": 0.0,
            "n_layer": cfg["n_layer"], "regU": 1}


def names_of(cfg):
    return ["user_embeddings", "item_embeddings"] + [f"weights.{k}" for k in range(cfg["n_layer"])]


def params_of(m):
    return dict(zip(["user_embeddings", "item_embeddings"] + [f"weights.{k}" for k in range(len(m.weights))],
                    [m.user_embeddings, m.item_embeddings, *m.weights]))


def params_to_double(m):
    m.user_embeddings = torch.nn.Parameter(m.user_embeddings.detach().double())
    m.item_embeddings = torch.nn.Parameter(m.item_embeddings.detach().double())
    m.weights = torch.nn.ParameterList([torch.nn.Parameter(w.detach().double()) for w in m.weights])


def redraw(m, seed):
    """The draws of `initModel` in its order (the tables, :935-938, then the weights, :1087-1090) on a model whose S and A
    are built already (building them consumes no draw): what the seed scan repeats instead of a whole construction."""
    torch.manual_seed(seed)
    ref.DeepRecommender.initModel(m)
    exec(WEIGHTS, dict(vars(ref), self=m))


def build(train, social, cfg, hp, dtype, seed, drop=None):
    m = ref.DiffNet(conf_of(cfg, hp), train, train[:10], copy.deepcopy(social))
    torch.manual_seed(seed)
    m.initModel()
    if dtype == torch.float64:
        params_to_double(m)
        m.S, m.A = m.S.double(), m.A.double()
    if drop == "social":
        m.S = m.S * 0.0
    if drop == "rating":
        m.A = m.A * 0.0
    if drop == "reg":
        m.regU = 0.0
    return m


def run(train, social, cfg, hp, dtype, seed, batches, steps=STEPS, drop=None, m=None):
    """The reference's loop body over the batches -> (terms [steps, 3], final parameters in float64, the pre-activations
    handed to torch.relu [steps * n_layer] in float64, the smallest non-zero |gradient| of the first step).  m: a model
    built and drawn already (the seed scan)."""
    m = m or build(train, social, cfg, hp, dtype, seed, drop)
    env = dict(vars(ref), self=m)
    exec(OPTIMIZER, env)
    real_relu, pre, terms, first = torch.relu, [], [], None

    def recording_relu(t):
        pre.append(t.detach().double().numpy().copy())
        return real_relu(t)

    torch.relu = recording_relu
    try:
        for n, batch in enumerate(batches[:steps]):
            env.update(batch=batch, n=n, epoch=0)
            exec(BODY, env)
            rec = -torch.sum(torch.log(torch.sigmoid(env["y"])))
            reg = m.regU * (torch.norm(env["u_embedding"], 2) + torch.norm(env["v_embedding"], 2)
                            + torch.norm(env["neg_item_embedding"], 2))
            terms.append([float(rec), float(reg), float(env["loss"])])
            if n == 0:
                first = min(float(g[g != 0].min()) for g in (p.grad.abs() for p in params_of(m).values()) if (g != 0).any())
    finally:
        torch.relu = real_relu
    assert len(pre) == steps * cfg["n_layer"]
    final = {k: p.detach().double().numpy().copy() for k, p in params_of(m).items()}
    return np.array(terms), final, pre, first


def relu_margin(pre64, pre32):
    """(min |f64 pre-activation|, max |f32 - f64| of the pre-activations) over every recorded call."""
    return min(float(np.abs(p).min()) for p in pre64), max(float(np.abs(a - b).max()) for a, b in zip(pre32, pre64))


def component_graph(rng, n=dfx.COMP_N):
    """COO (row, col) of the component S in entry order: row 0 empty, row 1 one entry, row 2 a self-loop among others, row 3
    with 300 entries over 40 columns (repeats), the last row not empty, the others 0-9 entries."""
    rows, cols = [], []
    for r in range(n):
        deg = 0 if r == 0 else 1 if r == 1 else 300 if r == 3 else int(rng.integers(0, 10))
        if r == n - 1:
            deg = max(deg, 3)
        c = rng.integers(0, 40 if r == 3 else n, deg)
        if r == 2:
            c = np.concatenate([c, [2]])
        rows += [r] * len(c)
        cols += c.tolist()
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)


def component_case(out, d, rng):
    row, col = component_graph(rng)
    val = rng.uniform(0.05, 1.0, row.size).astype(np.float32)
    n = dfx.COMP_N
    assert (np.bincount(row, minlength=n)[[0, 1, 3]] == [0, 1, 300]).all() and ((row == 2) & (col == 2)).any() and row[-1] == n - 1
    assert len(set(col[row == 3].tolist())) < 300
    for seed in range(100, 400):
        x, w, g = dfx.component_inputs(d, seed)
        res, pre = {}, {}
        for dtype in (torch.float64, torch.float32):
            s = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([row, col])), torch.from_numpy(val).to(dtype), (n, n))
            xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
            wt = torch.from_numpy(w).to(dtype).requires_grad_(True)
            holder = types.SimpleNamespace(S=s, weights=[wt])
            real_relu, seen = torch.relu, []
            torch.relu = lambda t: (seen.append(t.detach().double().numpy().copy()), real_relu(t))[1]
            try:
                env = dict(vars(ref), self=holder, user_embeddings=xt, k=0)
                exec(LAYER, env)
            finally:
                torch.relu = real_relu
            h = env["user_embeddings"]
            (h * torch.from_numpy(g).to(dtype)).sum().backward()
            res[dtype] = dict(h=h.detach().double().numpy(), dx=xt.grad.double().numpy(), dw=wt.grad.double().numpy())
            pre[dtype] = seen
        lo, err = relu_margin(pre[torch.float64], pre[torch.float32])
        if lo >= RELU_MARGIN * err:
            break
    else:
        raise AssertionError(f"d = {d}: no component seed meets the ReLU margin")
    pfx = f"comp{d}/"
    out.update({pfx + "row": row.astype(np.int16), pfx + "col": col.astype(np.int16), pfx + "val": val, pfx + "seed": seed,
                pfx + "min_pre": lo, pfx + "pre_err": err})
    for k, v in res[torch.float64].items():
        scale = float(np.abs(v).max())
        drift = float(np.abs(res[torch.float32][k] - v).max()) / scale
        out[pfx + f"f64/{k}"], out[pfx + f"scale/{k}"], out[pfx + f"drift/{k}"] = v, scale, drift
        print(f"component d = {d} seed {seed} {k}: scale {scale:.3g} reference f32 drift {drift:.3g}"
              f" (ReLU margin {lo / err:.1f})")


def main(out_dir):
    rng = np.random.default_rng(20261018)
    train, social = sg.synthetic_lists(rng)
    probe = build(train, social, CONFIGS[0], BASE, torch.float32, 0)
    data = probe.data
    assert (data.trainingSize()) == (sg.N_USERS, sg.N_ITEMS, sg.N_TRAIN + 1)
    assert len(probe.social.relation) == len(social) - 2, "the two pairs naming unknown users must be dropped"
    data.user_num, data.item_num = sg.N_USERS, sg.N_ITEMS          # `step_golden.id_arrays` reads these two names
    random.seed(BATCH_SEED)
    passes = itertools.chain.from_iterable(probe.next_batch_pairwise() for _ in range(STEPS))
    batches = sg.first_batches((b for b in passes if len(b[0]) == BATCH), STEPS, BATCH)

    s, a = probe.S, probe.A
    out = dict(sg.id_arrays(train, data, social), steps=STEPS, batch_size=BATCH, configs=len(CONFIGS), batch_seed=BATCH_SEED,
               min_first_grad=MIN_FIRST_GRAD, relu_margin=RELU_MARGIN, **{f"hp/{k}": v for k, v in BASE.items()},
               S_row=s._indices()[0].numpy().astype(np.int16), S_col=s._indices()[1].numpy().astype(np.int16),
               S_val=s._values().numpy(), A_row=a._indices()[0].numpy().astype(np.int16),
               A_col=a._indices()[1].numpy().astype(np.int16), A_val=a._values().numpy())
    assert out["S_row"].size == len(social) - 2 and out["A_row"].size == len(train)
    dense_s = s.to_dense()
    assert float(dense_s.sum(1).max()) > 1.0 + 1e-6, "the repeated social pair must make a row of S sum to more than 1"
    for n, (users, pos, neg) in enumerate(batches):         # a batch = a permutation of A's entries + the negatives
        out[f"batch{n}_perm"] = dfx.batch_perm(users, pos, out["A_row"], out["A_col"])
        out[f"batch{n}_neg"] = np.asarray(neg).astype(np.int16)
    for k in ("train_user", "train_item", "user_ids", "item_ids", "social_follower", "social_followee"):
        out[k] = out[k].astype(np.int32)

    for c, cfg in enumerate(CONFIGS):
        pre = f"c{c}/"
        out.update({pre + k: v for k, v in cfg.items()})
        scan = build(train, social, cfg, BASE, torch.float64, 0)
        for seed in range(3 + c, 3 + c + SCAN):
            redraw(scan, seed)
            params_to_double(scan)
            first = run(train, social, cfg, BASE, torch.float64, seed, batches, steps=1, m=scan)[3]
            if first < MIN_FIRST_GRAD:
                continue
            l64, p64, pre64, _ = run(train, social, cfg, BASE, torch.float64, seed, batches)
            l32, p32, pre32, _ = run(train, social, cfg, BASE, torch.float32, seed, batches)
            lo, err = relu_margin(pre64, pre32)
            print(f"config {c}: seed {seed}: first-step |gradient| >= {first:.3g}, min |pre| {lo:.3g}, f32 error {err:.3g}"
                  f" (ratio {lo / err:.1f})")
            if lo >= RELU_MARGIN * err:
                break
        else:
            raise AssertionError("no seed satisfies the Adam condition and the ReLU margin")
        out.update({pre + "table_seed": seed, pre + "first_grad": first, pre + "min_pre": lo, pre + "pre_err": err})
        assert np.isfinite(l64).all() and (np.abs(l32 - l64) <= 1e-5 * np.abs(l64)).all(), (l32, l64)
        out[pre + "f64/losses"], out[pre + "f32/losses"] = l64, l32
        print(f"config {c} {cfg}: f64 terms\n{l64}\n  max rel |f32 - f64| per term {(np.abs(l32 - l64) / np.abs(l64)).max(0)}")
        finals = {k: run(train, social, cfg, BASE, torch.float64, seed, batches, drop=k)[1] for k in DROPS}
        init = {k: p.detach().numpy().copy() for k, p in params_of(build(train, social, cfg, BASE, torch.float32, seed)).items()}
        redraw(scan, seed)
        assert all(np.array_equal(p.detach().numpy(), init[k]) for k, p in params_of(scan).items()), "redraw != initModel"
        names = names_of(cfg)
        assert list(p64) == names
        out[pre + "names"] = np.array(names)
        with dfx.registered():
            for k in names:
                sg.record_table(out, pre, "diffnet", k, p64[k], p32[k], finals, init=init[k], exact=1e-9)

    for d in dfx.COMP_WIDTHS:
        component_case(out, d, np.random.default_rng(500 + d))
    sg.save(out_dir, "diffnet_steps", out)


if __name__ == "__main__":
    main(sg.out_dir())
