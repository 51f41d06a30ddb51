#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/ncl_steps.npz: six training steps of ncl.py run by the reference itself.

Runs ONLY where the reference sources are (like oracle/gen_golden.py, whose `load_defs` / `load_stmts` it uses); the
fixture is plain data: a seeded synthetic graph, initial tables, six sampled batches, fixed centroids, and what the
reference computed on them.  ncl.py does not import without numba and faiss, so its pieces are taken out of its AST and
executed unchanged:
  * the body of the batch loop of `NCLModel.train` (ncl.py:311-329: forward, BPR, context-layer pick, structure contrast,
    e_step, prototype contrast, `l2_reg_loss(...) / self.batch_size`, backward, `torch.optim.Adam(lr)` step), once per
    batch, in a namespace holding `model`, `optimizer`, `batch`, `n`, `device` and a `self` that carries the
    hyper-parameters and the lifted `NCLModel.ssl_layer_loss` / `NCLModel.ProtoNCE_loss`;
  * `next_batch_pairwise`, `bpr_loss`, `l2_reg_loss`, `InfoNCE` (ncl.py:91-130);
  * `Interaction` and `LGCNEncoder` come from directau.py, which imports here and is textually ncl.py's.

The one deviation from the reference: `self.e_step()` (ncl.py:324, faiss k-means) becomes a stand-in with FIXED
centroids (stored, exact in float32).  `user_2cluster` / `item_2cluster` are still the nearest centroid (squared L2) of
the CURRENT encoder output, which is what `kmeans.index.search(x, 1)` returns (ncl.py:355).  For every row that
`ProtoNCE_loss` reads, the best and second-best distances must differ by more than 1e-3 relative in both runs, so that
an f32 / f64 near-tie cannot flip an assignment; the smallest gap is stored.

Per configuration, two runs from the same float32 initial tables (the sparse adjacency cast to the run's dtype too):
  * float64: the trajectory tests compare against (per-step losses and the final tables);
  * float32: kept as one number per table, slack = max |f32 - f64| of the final table (tests size their tolerance on it).
Then three float64 reruns with ssl_reg = 0, proto_reg = 0 and reg = 0 store max |delta final| per table: what a dropped
term would move; the sensitivity rule of tests/step_pins.py is asserted on them when the file is written."""
import os
import random
import types

import numpy as np
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from oracle.gen_golden import REF, load_defs, load_stmts  # noqa: E402  (puts the reference directory on sys.path)
from step_pins import NCL_TERMS as TERMS  # noqa: E402

N_USERS, N_ITEMS, N_TRAIN, BATCH, STEPS = 200, 120, 1000, 128, 6
# the raw 0/1 adjacency (ncl.py:76-85) multiplies row norms by about the degree per layer: the xavier tables are scaled
# down so that after three layers the BPR score differences stay O(1) (no saturated sigmoid), a power of two keeps them
# exact in float32
INIT_SCALE = 2.0 ** -4
# ncl.py:350-351 clamps self.k to max(2, n // 39) and keeps it: from the loop's first e_step on, 3 for users and items
K_USER, K_ITEM = 3, 3
MIN_GAP = 1e-3
# ncl.py:444-457's grid except reg.lambda: at B = 128, l2_reg_loss(...) / batch_size weighs the norms by reg / B^2, and at
# the grid's 1e-3 dropping the term moves the final tables by ~4e-8, under any float32 tolerance.  lr = 1e-4 keeps the
# per-step moves small against the tables (~1e-2), so that no batch row drifts onto a centroid boundary
BASE = {"learning.rate": 1e-4, "reg.lambda": 0.5, "NCL.tau": 0.2, "NCL.ssl_reg": 1e-3, "NCL.proto_reg": 1e-3,
        "NCL.alpha": 0.5}
CONFIGS = [dict(n_layers=3, hyper_layers=1, d=64),      # context = emb_list[2], an interior layer
           dict(n_layers=3, hyper_layers=2, d=64),      # hyper_layers * 2 >= len(emb_list): emb_list[-1]
           dict(n_layers=2, hyper_layers=1, d=128)]     # emb_list[2] is the last layer, reached by index; d = 128 engine
SENSITIVITY = ("ssl_reg", "proto_reg", "reg")


def nearest(x, cent):
    """(index of the nearest centroid, relative gap (d2 - d1) / d2 between the two smallest squared distances), in f64."""
    dist = torch.cdist(x.double(), cent.double()).square()
    two = dist.topk(2, dim=1, largest=False).values
    return dist.argmin(1), (two[:, 1] - two[:, 0]) / two[:, 1]


def lloyd(x, k, g, iters=10):
    """k centroids of x: Lloyd's iterations from k seeded rows (float64, only to place the fixed centroids)."""
    cent = x[torch.randperm(x.shape[0], generator=g)[:k]].clone()
    for _ in range(iters):
        a = torch.cdist(x, cent).argmin(1)
        for j in range(k):
            if bool((a == j).any()):
                cent[j] = x[a == j].mean(0)
    return cent


def run(ref, directau, data, cfg, hp, init, cents, batches, dtype):
    """The reference's loop body over the batches; returns (per-step losses, final tables, smallest assignment gap,
    assignments of the rows ProtoNCE_loss read per step, largest |pos - neg score| of BPR)."""
    d = cfg["d"]
    model = directau.LGCNEncoder(data, d, cfg["n_layers"])
    model.sparse_norm_adj = model.sparse_norm_adj.to(dtype)
    for key in ("user_emb", "item_emb"):
        model.embedding_dict[key] = torch.nn.Parameter(init[key].to(dtype, copy=True))  # Adam updates in place
    optimizer = torch.optim.Adam(model.parameters(), lr=hp["learning.rate"])
    self = types.SimpleNamespace(data=data, batch_size=BATCH, reg=hp["reg.lambda"], ssl_temp=hp["NCL.tau"],
                                 ssl_reg=hp["NCL.ssl_reg"], proto_reg=hp["NCL.proto_reg"], alpha=hp["NCL.alpha"],
                                 hyper_layers=cfg["hyper_layers"], n_layers=cfg["n_layers"], emb_size=d)
    self.ssl_layer_loss = types.MethodType(ref["ssl_layer_loss"], self)
    self.ProtoNCE_loss = types.MethodType(ref["ProtoNCE_loss"], self)
    cu, ci = cents["user"].to(dtype), cents["item"].to(dtype)
    state = {"gap": np.inf, "assign": []}

    def e_step():                                     # stand-in for ncl.py:340-345 (see the module docstring)
        user_emb, item_emb, _ = model()
        self.user_centroids, self.item_centroids = cu, ci
        self.user_2cluster, gu = nearest(user_emb.detach(), cu)
        self.item_2cluster, gi = nearest(item_emb.detach(), ci)
        u, p = state["batch"][0], state["batch"][1]
        state["gap"] = min(state["gap"], float(gu[u].min()), float(gi[p].min()))
        state["assign"].append(np.concatenate([self.user_2cluster[u].numpy(), self.item_2cluster[p].numpy()]))

    self.e_step = e_step
    body = load_stmts(os.path.join(REF, "ncl.py"), "NCLModel.train", 311, 329)
    ns = dict(ref, model=model, optimizer=optimizer, self=self, device=torch.device("cpu"))
    model.train()
    losses = {k: [] for k in TERMS}
    score_gap = 0.0
    for n, batch in enumerate(batches):
        state["batch"] = batch
        ns.update(n=n, batch=batch)
        exec(body, ns)
        for k in losses:
            losses[k].append(float(ns[k].item()))
        diff = (ns["user_emb"] * (ns["pos_emb"] - ns["neg_emb"])).sum(1).detach().abs().max()
        score_gap = max(score_gap, float(diff))
    final = {k: model.embedding_dict[k].detach().to(torch.float64).numpy() for k in ("user_emb", "item_emb")}
    return losses, final, state["gap"], np.stack(state["assign"]), score_gap


def main(out_dir):
    import directau                                  # reference module, imported as-is (its Interaction / LGCNEncoder)
    ref = load_defs(os.path.join(REF, "ncl.py"), {"next_batch_pairwise", "bpr_loss", "l2_reg_loss", "InfoNCE"},
                    methods={"NCLModel.ssl_layer_loss", "NCLModel.ProtoNCE_loss"})
    ref.update(shuffle=random.shuffle, choice=random.choice)     # ncl.py:5 `from random import shuffle, choice`
    rng = np.random.default_rng(20261016)
    pairs = sg.synthetic_pairs(rng, N_USERS, N_ITEMS, N_TRAIN, 5)
    raw_u = rng.choice(np.arange(10_000, 99_999), N_USERS, replace=False)      # raw ids: their sorted order is the dense one
    raw_i = rng.choice(np.arange(100_000, 999_999), N_ITEMS, replace=False)
    train = [[int(raw_u[u]), int(raw_i[i]), 1.0] for u, i in pairs]
    data = directau.Interaction({}, train, [])
    assert (data.user_num, data.item_num) == (N_USERS, N_ITEMS)

    # the batches: the reference's own sampler (ncl.py:91-114), seeded; full batches only (len(batch) == batch.size)
    random.seed(7)
    batches = sg.first_batches(ref["next_batch_pairwise"](data, BATCH), STEPS, BATCH,
                               lambda b: tuple(torch.tensor(t, dtype=torch.int64) for t in b))

    out = dict(sg.id_arrays(train, data),
               steps=STEPS, batch_size=BATCH, init_scale=INIT_SCALE, min_gap_required=MIN_GAP, configs=len(CONFIGS),
               **{f"hp/{k}": v for k, v in BASE.items()})
    sg.store_batches(out, batches, ("users", "pos", "neg"), np.int64)

    inits = {}
    for c, cfg in enumerate(CONFIGS):
        d = cfg["d"]
        if d not in inits:
            torch.manual_seed(100 + d)
            enc = directau.LGCNEncoder(data, d, 1)
            inits[d] = {k: (v.detach() * INIT_SCALE).contiguous() for k, v in enc.embedding_dict.items()}
            for k, v in inits[d].items():
                out[f"init_d{d}/{k}"] = v.numpy()
        init = inits[d]
        with torch.no_grad():
            enc = directau.LGCNEncoder(data, d, cfg["n_layers"])
            for key in ("user_emb", "item_emb"):
                enc.embedding_dict[key] = torch.nn.Parameter(init[key].double())
            enc.sparse_norm_adj = enc.sparse_norm_adj.double()
            fu, fi, _ = enc()
        # fixed centroids: k-means (Lloyd, float64) of the initial encoder output from seeded draws, rounded to float32.
        # Draws are tried in order until no row that ProtoNCE_loss reads comes near a tie at any step (deterministic)
        for attempt in range(200):
            g = torch.Generator().manual_seed(1000 * (c + 1) + attempt)
            cents = {"user": lloyd(fu, K_USER, g).float(), "item": lloyd(fi, K_ITEM, g).float()}
            res = {"f64": run(ref, directau, data, cfg, BASE, init, cents, batches, torch.float64)}
            if res["f64"][2] > 2 * MIN_GAP:
                break
        res["f32"] = run(ref, directau, data, cfg, BASE, init, cents, batches, torch.float32)
        pre = f"c{c}/"
        out.update({pre + k: v for k, v in cfg.items()})
        out[pre + "centroid_draw"] = attempt
        out[pre + "user_centroids"], out[pre + "item_centroids"] = cents["user"].numpy(), cents["item"].numpy()
        assert np.array_equal(res["f64"][3], res["f32"][3]), "f32 / f64 cluster assignments differ"
        gap = min(res["f64"][2], res["f32"][2])
        assert gap > MIN_GAP, f"config {c}: assignment gap {gap:.3g} <= {MIN_GAP}"
        out[pre + "min_gap"] = gap
        out[pre + "max_score_diff"] = max(res["f64"][4], res["f32"][4])
        for k in res["f64"][0]:
            out[f"{pre}f64/{k}"] = np.array(res["f64"][0][k], dtype=np.float64)
            out[f"{pre}f32/{k}"] = np.array(res["f32"][0][k], dtype=np.float64)
        print(f"config {c} {cfg}: min assignment gap {gap:.3g}, max |pos - neg score| {out[pre + 'max_score_diff']:.3g}")
        print("  f64 losses", {k: [f"{x:.6f}" for x in v] for k, v in res["f64"][0].items()})
        reruns = {term: run(ref, directau, data, cfg, dict(BASE, **{("reg.lambda" if term == "reg" else f"NCL.{term}"): 0.0}),
                            init, cents, batches, torch.float64)[1] for term in SENSITIVITY}
        for k, v in res["f64"][1].items():
            sg.record_table(out, pre, "ncl", k, v, res["f32"][1][k], reruns)

    sg.save(out_dir, "ncl_steps", out)


if __name__ == "__main__":
    main(sg.out_dir())
