#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/mhcn_steps.npz: six training steps of univariate/mhcn.py run by the
reference itself.

Runs ONLY where the reference sources are (like oracle/gen_golden.py, whose `load_stmts` / `_lift_class_methods` it
uses); the fixture is plain data.  mhcn.py does not import (tensorflow), so its pieces are taken out of its AST and
executed unchanged:
  * `Interaction`, `Relation`, `Graph`, `TFGraphInterface`, `bpr_loss`, `next_batch_pairwise` (top level);
  * MHCN's `build` (xavier everywhere, zero biases, the four operators), `build_hyper_adj_mats`, the gates, the
    attention, `forward`, `hierarchical_self_supervision`, as methods of a class that is also an `nn.Module`, so that
    `named_parameters()` is the reference's;
  * the body of the batch loop of `MHCN.train_epoch` (mhcn.py:528-539: forward, bpr_loss, the 20 norms, zero_grad,
    backward, `torch.optim.Adam(lr)` step), once per batch.
The batches are the first six of the reference's own sampler (seeded); the nine `torch.randperm` draws of every step are
recorded (a seeded generator stands in for the global one, the same draws in every run).

The data: 200 users, 120 items with a planted group structure; one repeated interaction (2 in Y), one repeated social
pair (2 in S), two social pairs naming a user that is not in the training set (dropped by `Relation.__initialize`).
Asserted: H_p is not empty, and every channel operator has users with an empty row.

Per configuration, from the same float32 initial parameters, what tests/step_pins.py describes: a float64 run (operators
cast too; the 20 finals as float32(final - init), |delta| < 1e-2, exact to 1e-9), a float32 run, float64 reruns with
ss_rate = 0 and with reg_lambda = 0.  Asserted when the file is written: losses of f32 and f64 within 1e-5 relative; its
sensitivity rule; `sgating_bias.4` stays exactly 0 and `sgating_weights.4` moves through the regulariser alone."""
import copy
import math
import os
import random
from collections import defaultdict

import numpy as np
import scipy.sparse as sp
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from oracle.gen_golden import REF, _lift_class_methods, load_stmts  # noqa: E402
from step_golden import N_ITEMS, N_TRAIN, N_USERS  # noqa: E402
from step_pins import MHCN_TERMS as TERMS, MHCN_UNREACHED as UNREACHED  # noqa: E402

PATH = os.path.join(REF, "univariate", "mhcn.py")

BATCH, STEPS = 128, 6
# mhcn.py:564-571's grid; reg_lambda = 1e-2 so that the 20 norms move every parameter well past float32 rounding
BASE = {"lr": 1e-3, "reg_lambda": 1e-2, "ss_rate": 0.01}
CONFIGS = [dict(n_layer=2, d=64), dict(n_layer=3, d=32)]
METHODS = {"build", "build_hyper_adj_mats", "self_gating", "self_supervised_gating", "channel_attention", "forward",
           "hierarchical_self_supervision", "sparse_mx_to_torch_sparse_tensor"}


class Reference:
    def __init__(self):
        self.cls, self.ns = _lift_class_methods(
            PATH, "MHCN", METHODS, extra_ns={"defaultdict": defaultdict, "math": math, "random": random},
            top_level=("TFGraphInterface", "Graph", "Relation", "Interaction", "bpr_loss", "next_batch_pairwise"))
        self.body = load_stmts(PATH, "MHCN.train_epoch", 528, 539)
        self.model_cls = type("LiftedMHCNModule", (self.cls, torch.nn.Module), {})

    def model(self, train, social, cfg, hp, dtype, seed):
        m = self.model_cls()
        m.data = self.ns["Interaction"]({}, train, train[:10])
        m.social_data = self.ns["Relation"]({}, copy.deepcopy(social), m.data.user)      # __initialize deletes in place
        m.emb_size, m.n_layers, m.ss_rate, m.reg = cfg["d"], cfg["n_layer"], hp["ss_rate"], hp["reg_lambda"]
        m.batch_size, m.lRate = BATCH, hp["lr"]
        torch.manual_seed(seed)
        m.build()
        if dtype == torch.float64:
            m.double()
            for k in ("H_s", "H_j", "H_p", "R"):
                setattr(m, k, getattr(m, k).double())
        return m

    def run(self, train, social, cfg, hp, dtype, seed, batches):
        """The reference's loop body over the batches -> (losses [steps, 4], final parameters in float64, recorded
        permutations [steps, 9, n], the model)."""
        m = self.model(train, social, cfg, hp, dtype, seed)
        opt = torch.optim.Adam(m.parameters(), lr=m.lRate)
        g = torch.Generator().manual_seed(99)
        real, drawn = torch.randperm, []

        def recording_randperm(n, **kw):
            p = real(n, generator=g)
            drawn.append(p.numpy().copy())
            return p

        losses = []
        torch.randperm = recording_randperm
        try:
            for user_idx, i_idx, j_idx in batches:
                env = dict(self.ns, self=m, user_idx=user_idx, i_idx=i_idx, j_idx=j_idx, optimizer=opt)
                exec(self.body, env)
                losses.append([float(env[k]) for k in TERMS])
        finally:
            torch.randperm = real
        final = {k: p.detach().double().numpy().copy() for k, p in m.named_parameters()}
        perms = np.stack(drawn).reshape(len(batches), 9, -1)
        return np.array(losses), final, perms, m


def main(out_dir):
    ref = Reference()
    rng = np.random.default_rng(20261018)
    train, social = sg.synthetic_lists(rng)
    probe = ref.model(train, social, CONFIGS[0], BASE, torch.float32, 0)
    data = probe.data
    assert (data.user_num, data.item_num) == (N_USERS, N_ITEMS) and len(train) == N_TRAIN + 1
    kept = probe.social_data.relation
    assert len(kept) == len(social) - 2, "the two pairs naming unknown users must be dropped"
    S = probe.social_data.get_social_mat()
    assert S.max() == 2.0 and data.interaction_mat.max() == 2.0, "one repeated social pair and one repeated interaction"

    # the batches: the reference's own sampler (mhcn.py:13-31), seeded; the first six (all full)
    random.seed(7)
    batches = sg.first_batches(ref.ns["next_batch_pairwise"](data, BATCH), STEPS, BATCH)

    out = dict(sg.id_arrays(train, data, social),
               S_row=np.array([data.user[p[0]] for p in kept], dtype=np.int16),
               S_col=np.array([data.user[p[1]] for p in kept], dtype=np.int16),
               steps=STEPS, batch_size=BATCH, configs=len(CONFIGS), **{f"hp/{k}": v for k, v in BASE.items()})
    sg.store_batches(out, batches, ("users", "pos", "neg"), np.int16)
    nnz = {}
    for name in ("H_s", "H_j", "H_p", "R"):
        t = getattr(probe, name).coalesce()
        mat = sp.csr_matrix((t.values().numpy(), tuple(t.indices().numpy())), shape=tuple(t.shape))
        out.update(sg.csr_dict(name, mat))
        nnz[name] = int(out[f"{name}_data"].size)
        if name != "R":
            assert nnz[name] > 0 and (np.diff(out[f"{name}_indptr"]) == 0).any(), f"{name}: needs entries and an empty row"
    print("nnz", nnz)

    for c, cfg in enumerate(CONFIGS):
        pre, seed = f"c{c}/", 3 + c
        out.update({pre + k: v for k, v in cfg.items()})
        l64, p64, perms, m64 = ref.run(train, social, cfg, BASE, torch.float64, seed, batches)
        l32, p32, perms32, _ = ref.run(train, social, cfg, BASE, torch.float32, seed, batches)
        assert np.array_equal(perms, perms32)
        names = list(p64)
        assert len(names) == 20
        init = {k: v.detach().numpy().copy() for k, v in ref.model(train, social, cfg, BASE, torch.float32, seed).named_parameters()}
        out[pre + "names"] = np.array(names)
        out[pre + "perms"] = perms.astype(np.int16)
        out[pre + "f64/losses"], out[pre + "f32/losses"] = l64, l32
        assert np.isfinite(l64).all() and (np.abs(l32 - l64) <= 1e-5 * np.abs(l64)).all()
        print(f"config {c} {cfg}: f64 losses\n{l64}\n  max rel |f32 - f64| per term {(np.abs(l32 - l64) / np.abs(l64)).max(0)}")
        finals = {"ss": ref.run(train, social, cfg, dict(BASE, ss_rate=0.0), torch.float64, seed, batches)[1],
                  "reg": ref.run(train, social, cfg, dict(BASE, reg_lambda=0.0), torch.float64, seed, batches)[1]}
        for k in names:
            sg.record_table(out, pre, "mhcn", k, p64[k], p32[k], finals, init=init[k], exact=1e-9, unreached=UNREACHED)
            assert np.abs(out[f"{pre}f64/delta/{k}"]).max() < 1e-2 or k == "sgating_bias.4"
        assert not p64["sgating_bias.4"].any() and not init["sgating_bias.4"].any()
        assert np.abs(p64["sgating_weights.4"] - init["sgating_weights.4"]).max() > 1e-3

    sg.save(out_dir, "mhcn_steps", out)


if __name__ == "__main__":
    main(sg.out_dir())
