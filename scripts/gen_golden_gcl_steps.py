#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/gcl_steps.npz: five training steps of gcl.py run by the reference itself.

Runs ONLY where the reference sources are (like oracle/gen_golden.py, whose `load_stmts` it uses); the fixture is plain
data: a seeded synthetic graph, the initial weights of GRACEModel, five sampled batches, and what the reference computed
on them.  gcl.py is imported as-is; the body of the batch loop of `GCLTuner.run` (gcl.py:208-225: zero_grad, two
EdgeRemoving views, forward, symmetric InfoNCE over all users and all items, BPR by logsigmoid, regulariser, backward,
`torch.optim.Adam(lr, weight_decay)` step) is lifted out of its AST and executed unchanged, once per batch.

Two runs from the same initial weights and batches:
  * float64 — the reference functions are dtype-agnostic; this is the trajectory tests compare against;
  * float32 — kept whole: how far plain fp32 arithmetic drifts from float64 over the same five steps is the slack the
    tests size their parameter tolerance from (tests/step_pins.py; this fixture stores f32/final in place of a slack).
EdgeRemoving's draws do not reach the outputs: GRACEModel.encode ignores its edges (gcl.py:53-57), so z1 == z2."""
import os
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from oracle.gen_golden import REF, load_stmts  # noqa: E402  (puts the reference directory on sys.path)
from step_pins import GCL_TERMS as TERMS  # noqa: E402

N_USERS, N_ITEMS, N_TRAIN, N_TEST = 300, 200, 3000, 400
EMB, LAYERS, STEPS = 64, 2, 5
CONFIG = dict(embedding_size=EMB, num_layers=LAYERS, lr=0.005, weight_decay=1e-4, ssl_temp=0.2, drop_edge=0.2,
              reg_weight=1e-4, ssl_weight=1.0, batch_size=256, max_epoch=1)


def synthetic_graph(rng):
    """Unique (user, item) pairs with a planted group structure.  Training holds one pair of every user and of every item
    (dense ids, gcl.py:67-78) plus a random share of the rest; the test split is the remainder."""
    groups = 5
    cover = {(u, int(rng.integers(0, N_ITEMS))) for u in range(N_USERS)}
    cover |= {(int(rng.integers(0, N_USERS)), i) for i in range(N_ITEMS)}
    extra = set()
    while len(cover) + len(extra) < N_TRAIN + N_TEST:
        u = int(rng.integers(0, N_USERS))
        i = int(rng.integers(0, N_ITEMS // groups)) * groups + u % groups if rng.random() < 0.8 \
            else int(rng.integers(0, N_ITEMS))
        if (u, i) not in cover:
            extra.add((u, i))
    extra = sorted(extra)
    rng.shuffle(extra)
    n_rest = N_TRAIN - len(cover)
    train = sorted(cover) + extra[:n_rest]
    rng.shuffle(train)
    return np.array(train, dtype=np.int64), np.array(extra[n_rest:], dtype=np.int64)


def main(out_dir):
    import gcl                                                # the reference module, imported as-is
    rng = np.random.default_rng(20261016)
    train, test = synthetic_graph(rng)
    tmp = tempfile.mkdtemp()
    for name, arr in (("train.txt", train), ("test.txt", test)):
        with open(os.path.join(tmp, name), "w") as f:
            f.writelines(f"{u} {i} 1\n" for u, i in arr)
    edge_index, train_df, test_df, num_users, num_items = gcl.load_data(os.path.join(tmp, "train.txt"),
                                                                       os.path.join(tmp, "test.txt"))
    assert (num_users, num_items) == (N_USERS, N_ITEMS)
    user_pos = gcl.get_user_pos(train_df)

    # the batches: the reference's own sampler (gcl.py:111-125), seeded
    np.random.seed(7)
    batches = sg.first_batches(gcl.next_batch_pairwise(train_df, CONFIG["batch_size"], num_users, num_items, user_pos), STEPS,
                               CONFIG["batch_size"], lambda b: tuple(t.clone() for t in b))

    torch.manual_seed(11)
    init = gcl.GRACEModel(num_users, num_items, emb_size=EMB, num_layers=LAYERS)
    init_state = {k: v.detach().clone() for k, v in init.state_dict().items()}

    body = load_stmts(os.path.join(REF, "gcl.py"), "GCLTuner.run", 208, 225)
    out = dict(train_user=train[:, 0], train_item=train[:, 1], test_user=test[:, 0], test_item=test[:, 1],
               num_users=num_users, num_items=num_items, steps=STEPS,
               **{f"config_{k}": v for k, v in CONFIG.items()})
    for k, v in init_state.items():
        out[f"init/{k}"] = v.numpy()
    sg.store_batches(out, batches, ("users", "pos", "neg"), np.int64)

    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        model = gcl.GRACEModel(num_users, num_items, emb_size=EMB, num_layers=LAYERS)
        model.load_state_dict(init_state)
        model = model.to(dtype)
        optimizer = torch.optim.Adam(model.parameters(), lr=CONFIG["lr"], weight_decay=CONFIG["weight_decay"])
        ns = dict(torch=torch, F=F, device=torch.device("cpu"), model=model, optimizer=optimizer,
                  aug=gcl.EdgeRemoving(pe=CONFIG["drop_edge"]), edge_index_dev=edge_index, num_users=num_users,
                  info_nce_loss=gcl.info_nce_loss, config=dict(CONFIG))
        torch.manual_seed(3)                                  # EdgeRemoving's draws (no effect on the outputs)
        model.train()
        rec = {k: [] for k in TERMS}
        for n, (u, p, q) in enumerate(batches):
            ns.update(n=n, users=u, pos_items=p, neg_items=q)
            exec(body, ns)
            for k in rec:
                rec[k].append(float(ns[k].item()))
        for k, v in rec.items():
            out[f"{tag}/{k}"] = np.array(v, dtype=np.float64)
        for k, v in model.state_dict().items():
            out[f"{tag}/final/{k}"] = v.detach().numpy()
        print(tag, {k: [f"{x:.6f}" for x in v] for k, v in rec.items()})

    drift = {k: float(np.abs(out[f"f32/final/{k}"] - out[f"f64/final/{k}"]).max()) for k in init_state}
    print("max |f32 - f64| of the final parameters:", drift)
    sg.save(out_dir, "gcl_steps", out)


if __name__ == "__main__":
    main(sg.out_dir())
