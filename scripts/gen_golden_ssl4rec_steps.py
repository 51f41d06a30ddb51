#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/ssl4rec_steps.npz: six training steps of ssl4rec.py run by the reference itself.

Runs ONLY where the reference sources are (like oracle/gen_golden.py, whose `REF`, `load_defs` and `load_stmts` it uses);
the fixture is plain data.  ssl4rec.py does not import without numba, so its pieces are taken out of its AST and executed
unchanged:
  * the body of the batch loop of `SSL4RecModel.train` (ssl4rec.py:218-225: both towers, batch_softmax_loss,
    `cl_rate * model.cal_cl_loss(i)`, l2_reg_loss, zero_grad / backward / `torch.optim.Adam(lr)` step), once per batch, in
    a namespace holding `batch`, `optimizer`, `device` and a `self` that carries the model and the hyper-parameters;
  * the classes `DNNEncoder` and `Interaction` (ClassDef nodes) and the functions `InfoNCE`, `batch_softmax_loss`,
    `l2_reg_loss`, `next_batch_pairwise`.

The one stand-in is dropout: after construction `model.dropout` (nn.Dropout, ssl4rec.py:167) is replaced by a module
that applies RECORDED masks, `x * keep / (1 - p)`, two per step in call order (ssl4rec.py:195).  The masks are seeded
numpy draws `u >= p`, stored as packed bits with bit i * emb + c of a word stream for element (i, c) —
gcr_edge_mask_bits' order — so that the float32 and float64 runs see the same draws and the product can replay them.

Initial state: the constructor's draw rounded to a 2^-12 grid (so that it compresses), except the matrices with a
1024-wide side, which tests/ssl4rec_fixture.py regenerates from a seed (see there); their finals are stored at a seeded
sample.  Per configuration:
  * a float64 run: per-step losses and final parameters, what the tests compare against;
  * a float32 run, kept as slack = max |f32 - f64| per parameter (over the whole tensor) and its losses;
  * two float64 reruns with alpha = 0 and reg.weight = 0: max |delta final| per parameter, what a dropped term moves.
Asserted here, relied on by the tests: float32 losses within 2.5e-6 relative of float64; for each dropped term some
parameter with delta >= 10 x (4 x max(slack, 1e-7)); every parameter moved by more than 100 x slack (at the stored entries).
The initial draw of a configuration is the first (seeds tried in order) for which that holds and for which slack is a
stable measure: four more float32 runs of the reference with the rows of every batch permuted — the same sums in another
order, which is all that the HIP step is — stay within 2 x max(slack, 1e-7) of the float64 run.  Both criteria read the
reference's runs only.  learning.rate is 1e-5: see the comment at `LR`."""
import ast
import os
import random
import types
from collections import defaultdict

import numpy as np
import scipy.sparse as sp
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from oracle.gen_golden import REF, load_defs, load_stmts  # noqa: E402  (puts the reference directory on sys.path)
import ssl4rec_fixture as fx  # noqa: E402
import step_pins as pins  # noqa: E402

SRC = os.path.join(REF, "ssl4rec.py")

N_USERS, N_ITEMS, N_TRAIN, BATCH, STEPS = 160, 96, 1000, 128, 6
# learning.rate: the smallest value of ssl4rec.py:278's grid.  An Adam step moves an element by lr x m / sqrt(v), so a
# RELATIVE error rho of a gradient is an error lr x rho of the parameter, and float32 gives a gradient that is a cancelled
# sum of terms of size S the relative error 2^-24 x S / |g|.  Among N elements some have |g| / S near 1 / N, so the worst
# element of a tensor is off by about lr x 2^-24 x N, with a tail like 1 / x: which element is worst, and by how much,
# changes with the summation order of every GEMM (the same float32 run of the reference with its batch rows reordered
# drifts 2 ... 20 x as far from float64, `permuted_drift` below).  The tests' tolerance is 4 x max(slack, 1e-7), whose floor
# is absolute: at lr = 1e-3 that noise (5e-7 at N = 5120) lies above the floor and the tolerance rests on one sample of
# a heavy-tailed quantity; at lr = 1e-5 it lies two orders below it, while one step with a wrong gradient still moves an
# element by up to lr = 25 x the floor, and a dropped loss term by what `delta_*` records (asserted below: >= 10 x the
# tolerance).
LR = 1e-5
# ssl4rec.py:274-284's grid: every drop / tau / alpha value once, n.layers 1-3, reg.weight 1e-4 / 1e-2 / 1e-2 (at the
# default 1e-4 the regulariser moves the parameters by less than the float32 tolerance, so config 0 cannot show it)
CONFIGS = [dict(n_layers=1, emb=64, drop=0.1, tau=0.07, alpha=0.1, reg_weight=1e-4),
           dict(n_layers=2, emb=32, drop=0.2, tau=0.1, alpha=0.2, reg_weight=1e-2),
           dict(n_layers=3, emb=32, drop=0.3, tau=0.2, alpha=0.3, reg_weight=1e-2)]


def load_classes(ns, names):
    """exec the named top-level ClassDef nodes of ssl4rec.py, unchanged, in `ns` (next to the functions they call)."""
    tree = ast.parse(open(SRC).read())
    wanted = [node for node in tree.body if isinstance(node, ast.ClassDef) and node.name in names]
    assert len(wanted) == len(names)
    exec(compile(ast.Module(body=wanted, type_ignores=[]), SRC, "exec"), ns)


class RecordedDropout(torch.nn.Module):
    """Stand-in for nn.Dropout(p) in training mode: the k-th call applies the k-th recorded mask."""

    def __init__(self, p, masks):
        super().__init__()
        self.p, self.masks, self.calls = p, masks, 0

    def forward(self, x):
        keep = self.masks[self.calls].reshape(x.shape).to(x.dtype)
        self.calls += 1
        return x * keep / (1 - self.p)


def run(ref, data, cfg, init, masks, batches, dtype, alpha=None, reg_weight=None):
    """The reference's loop body over the batches; returns (per-step losses, final state as float64 numpy)."""
    model = ref["DNNEncoder"](data, cfg["emb"], cfg["drop"], cfg["tau"], cfg["n_layers"]).to(dtype)
    model.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in init.items()})
    model.dropout = RecordedDropout(cfg["drop"], [torch.from_numpy(m) for m in masks])
    optimizer = torch.optim.Adam(model.parameters(), lr=LR)
    self = types.SimpleNamespace(model=model, tau=cfg["tau"], cl_rate=cfg["alpha"] if alpha is None else alpha,
                                 reg_weight=cfg["reg_weight"] if reg_weight is None else reg_weight)
    body = load_stmts(SRC, "SSL4RecModel.train", 218, 225)
    ns = dict(ref, self=self, optimizer=optimizer)
    model.train()
    losses = {k: [] for k in fx.TERMS}
    for batch in batches:
        ns.update(batch=batch)
        exec(body, ns)
        for k in losses:
            losses[k].append(float(ns[k].item()))
    assert model.dropout.calls == 2 * len(batches)
    return losses, {k: v.detach().to(torch.float64).numpy() for k, v in model.state_dict().items()}


def permuted_drift(ref, data, cfg, init, masks, batches, f64, trials=4):
    """max |f32 - f64| per parameter over `trials` float32 runs whose batch rows (and mask rows) are permuted."""
    rng = np.random.default_rng(77)
    worst = {k: 0.0 for k in f64}
    for _ in range(trials):
        pb, pm = [], []
        for n, (u, i, j) in enumerate(batches):
            p = rng.permutation(len(u))
            pb.append(([u[r] for r in p], [i[r] for r in p], j))
            pm += [masks[2 * n + v].reshape(len(u), -1)[p].reshape(-1) for v in range(2)]
        _, fp = run(ref, data, cfg, init, pm, pb, torch.float32)
        for k in worst:
            worst[k] = max(worst[k], float(np.abs(fp[k] - f64[k]).max()))
    return worst


def main(out_dir):
    ref = load_defs(SRC, {"next_batch_pairwise", "l2_reg_loss", "InfoNCE", "batch_softmax_loss"})
    ref.update(shuffle=random.shuffle, choice=random.choice, sp=sp, defaultdict=defaultdict)   # ssl4rec.py:6-8
    load_classes(ref, {"DNNEncoder", "Interaction"})
    rng = np.random.default_rng(20261017)
    pairs = sg.synthetic_pairs(rng, N_USERS, N_ITEMS, N_TRAIN, 4)
    raw_u = rng.choice(np.arange(10_000, 99_999), N_USERS, replace=False)       # raw ids in no order: first-seen ids
    raw_i = rng.choice(np.arange(100_000, 999_999), N_ITEMS, replace=False)     # differ from the sorted ones
    train = [[str(raw_u[u]), str(raw_i[i]), 1.0] for u, i in pairs]
    data = ref["Interaction"](list(train), [])          # a copy: the sampler shuffles data.training_data in place
    assert (data.user_num, data.item_num) == (N_USERS, N_ITEMS)

    # the batches: the reference's own sampler (ssl4rec.py:33-50), seeded; full batches only
    random.seed(11)
    batches = sg.first_batches(ref["next_batch_pairwise"](data, BATCH), STEPS, BATCH, lambda b: tuple(list(t) for t in b))

    out = dict(sg.id_arrays(train, data),
               steps=STEPS, batch_size=BATCH, learning_rate=LR, configs=len(CONFIGS))
    sg.store_batches(out, batches, ("users", "items"), np.int64)

    for c, cfg in enumerate(CONFIGS):
        pre = f"c{c}/"
        out.update({pre + k: v for k, v in cfg.items()})
        mrng = np.random.default_rng(5000 + c)
        masks = [mrng.random(BATCH * cfg["emb"]) >= cfg["drop"] for _ in range(2 * STEPS)]
        out[pre + "keep_bits"] = np.stack([fx.pack_bits(m) for m in masks]).reshape(STEPS, 2, -1)
        out[pre + "kept_share"] = float(np.mean(masks))
        # Initial draws are tried in order (deterministic) until the reference's own float32 run stays within 1 / 100 of
        # every parameter's movement.  Adam multiplies the error of a gradient far below its eps by lr / eps = 1e5, so an
        # element whose gradient is a cancelled sum carries rounding noise into the parameter; a draw with such an element
        # would make the tests' tolerance (4 x slack) too wide to say anything about that parameter ...
        for attempt in range(200):
            torch.manual_seed(100 + c + 1000 * attempt)
            built = ref["DNNEncoder"](data, cfg["emb"], cfg["drop"], cfg["tau"], cfg["n_layers"])
            names = list(built.state_dict())
            out[pre + "names"] = np.array(names)
            init = {}
            for j, (k, v) in enumerate(built.state_dict().items()):
                out[f"{pre}shape/{k}"] = np.array(v.shape, dtype=np.int64)
                if fx.is_wide(v.shape):
                    seed = 1_000_000 * (c + 1) + 1000 * j + 10 * attempt
                    init[k] = fx.wide_init(v.shape, seed)
                    out[f"{pre}init_seed/{k}"], out[f"{pre}init_crc/{k}"] = seed, fx.crc(init[k])
                    out[f"{pre}sample_seed/{k}"] = seed + 1
                    out[f"{pre}sample_crc/{k}"] = fx.crc(fx.sample_index(v.numel(), seed + 1))
                else:
                    init[k] = out[f"{pre}init/{k}"] = (torch.round(v / fx.GRID) * fx.GRID).numpy().astype(np.float32)
            l64, f64 = run(ref, data, cfg, init, masks, batches, torch.float64)
            l32, f32 = run(ref, data, cfg, init, masks, batches, torch.float32)
            cf = fx.Config({k: np.asarray(v) for k, v in out.items()}, c)      # the reader's view of what is stored so far
            slack = {k: float(np.abs(f32[k] - f64[k]).max()) for k in names}
            moved = {k: float(np.abs(cf.at(k, f64[k]) - cf.at(k, init[k])).max()) for k in names}
            if not all(pins.has_moved(moved[k], slack[k]) for k in names):
                print(f"config {c} draw {attempt}: worst slack / moved", max(slack[k] / moved[k] for k in names))
                continue
            loss_rel = max(float(np.max(np.abs(np.array(l32[k]) - np.array(l64[k])) / np.abs(np.array(l64[k])))) for k in fx.TERMS)
            if loss_rel > 2.5e-6:
                print(f"config {c} draw {attempt}: float32 loss off float64 by {loss_rel:.3g} relative")
                continue
            # ... and until that slack is a stable measure of float32 drift: the same float32 run with the rows of every
            # batch in another order (the same sums, added in another order) must stay within 2 x slack of float64
            spread = permuted_drift(ref, data, cfg, init, masks, batches, f64)
            worst = max(spread[k] / max(slack[k], pins.FLOOR) for k in names)
            if worst <= 2.0:
                break
            print(f"config {c} draw {attempt}: a reordered float32 run drifts {worst:.2f} x slack")
        else:
            raise AssertionError(f"config {c}: no initial draw with every parameter moved by more than 100 x slack")
        out[pre + "init_draw"] = attempt
        for k in names:
            out[f"{pre}f64/final/{k}"] = cf.at(k, f64[k])
            out[f"{pre}slack/{k}"] = slack[k]
        print(f"config {c} {cfg}: kept share {out[pre + 'kept_share']:.4f}")
        for k in fx.TERMS:
            out[f"{pre}f64/{k}"], out[f"{pre}f32/{k}"] = np.array(l64[k]), np.array(l32[k])
            rel = float(np.max(np.abs(np.array(l32[k]) - np.array(l64[k])) / np.abs(np.array(l64[k]))))
            assert rel <= 2.5e-6, f"config {c} {k}: float32 loss off float64 by {rel:.3g} relative"
            print(f"  f64 {k}", [f"{x:.6f}" for x in l64[k]], f"f32 rel diff {rel:.2g}")
        print("  slack max |f32 - f64|:", {k: f"{v:.2g}" for k, v in slack.items()})
        for term in fx.SENSITIVITY:
            _, final = run(ref, data, cfg, init, masks, batches, torch.float64, **{term: 0.0})
            ratios = []
            for k in names:
                delta = out[f"{pre}delta_{term}/{k}"] = float(np.abs(cf.at(k, final[k]) - cf.at(k, f64[k])).max())
                ratios.append(delta / pins.atol_floor_4(slack[k]))
            print(f"  sensitivity {term} = 0: max |delta final| / tolerance per parameter:", [f"{r:.1f}" for r in ratios])
            # at the default reg.weight = 1e-4 the regulariser is below the tolerance (config 0): no claim made there
            if term == "alpha" or cfg["reg_weight"] >= 1e-3:
                assert max(ratios) >= pins.DROPPED_CPU, f"config {c}: dropping {term} stays inside 10 x the tolerance"

    sg.save(out_dir, "ssl4rec_steps", out)


if __name__ == "__main__":
    main(sg.out_dir())
