"""GCLModel (recommendation_amd/gcl.py): gcl.py's training loop on the HIP path, pinned to what the reference computed.

  * trajectory: five steps of the faithful (linear) form from tests/golden/gcl_steps.npz — the reference's own loop body
    (gcl.py:208-225, torch.optim.Adam with weight_decay) run in float64 on the same weights and batches;
  * evaluation: gcl.py:87-108's metric definitions, restated in numpy on the same embeddings;
  * the lightgcn form: one step against the autograd composition of the library's differentiable ops on explicitly
    masked operators, and drop_edge = 0 giving two identical views;
  * convergence: train() on a planted-structure graph beats a random ranking by a wide margin."""
import numpy as np
import pytest
import torch

import step_pins as sp

pytestmark = pytest.mark.gpu

CONFIG_KEYS = ("embedding_size", "num_layers", "lr", "weight_decay", "ssl_temp", "drop_edge", "reg_weight", "ssl_weight",
               "batch_size", "max_epoch")


@pytest.fixture(scope="module")
def golden():
    return sp.load("gcl")


def test_trajectory_matches_reference_float64(golden):
    """Five train_steps of GCLModel(encoder="linear") from the fixture's weights on its batches: every loss term at
    rel 1e-5 of the float64 reference run, and the final parameters, by the rule of tests/step_pins.py (family "gcl").

    Parameter tolerance: Adam divides by sqrt(v), so an element whose gradient is near zero moves by up to lr per step
    whatever its size, and fp32 rounding of such a gradient is amplified instead of damped.  How much that is over these
    five steps is measured, not guessed: the fixture's float32 run of the reference itself drifts from the float64 run
    by `slack` (max |f32 - f64| per parameter).  The HIP step is another fp32 evaluation of the same arithmetic in a
    different summation order, so its drift is allowed 4 x the reference's own (floored at 1e-7 for the biases, whose
    reference drift is at the rounding level: `atol_floor_4`).  A wrong gradient moves an element by O(lr) = 5e-3 — far
    outside that; and every parameter moved by more than 100 x that slack (the step is not a no-op)."""
    from recommendation_amd.gcl import GCLModel
    g = golden
    config = {k: g[f"config_{k}"].item() for k in CONFIG_KEYS}
    model = GCLModel(config, (g["train_user"], g["train_item"]), (g["test_user"], g["test_item"]), device="cuda",
                     encoder="linear", num_users=int(g["num_users"]), num_items=int(g["num_items"]))
    names = [k for k in model.model.state_dict()]
    model.model.load_state_dict({k: torch.from_numpy(g[f"init/{k}"]) for k in names})
    got = []
    for n in range(int(g["steps"])):
        out = model.train_step(*sp.batch(g, n, ("users", "pos", "neg")))
        got.append(torch.stack([v.reshape(()) for v in out]))
    final = {k: v.detach().cpu().numpy() for k, v in model.model.state_dict().items()}
    sp.check(sp.record("gcl", g), torch.stack(got).cpu().numpy(), final)


def _numpy_gcl_evaluate(user_emb, item_emb, test_u, test_i, train_u, train_i, ks):
    """gcl.py:87-108, restated: scores, training positives at -inf, argsort, HR / P / R / un-normalised DCG, averaged
    over the test users."""
    scores = user_emb.astype(np.float64) @ item_emb.astype(np.float64).T
    known = {}
    for u, i in zip(train_u, train_i):
        known.setdefault(int(u), set()).add(int(i))
    metrics = {k: {"HR": 0.0, "P": 0.0, "R": 0.0, "NDCG": 0.0} for k in ks}
    users = list(dict.fromkeys(int(u) for u in test_u))
    for user in users:
        test_items = {int(i) for u, i in zip(test_u, test_i) if u == user}
        s = scores[user].copy()
        s[list(known.get(user, ()))] = -np.inf
        rank = np.argsort(-s, kind="stable")
        for k in ks:
            topk = rank[:k]
            hits = len(set(topk.tolist()) & test_items)
            metrics[k]["HR"] += int(hits > 0)
            metrics[k]["P"] += hits / k
            metrics[k]["R"] += hits / len(test_items)
            metrics[k]["NDCG"] += sum(1 / np.log2(i + 2) if topk[i] in test_items else 0 for i in range(k))
    return {k: {m: v / len(users) for m, v in metrics[k].items()} for k in ks}


def test_evaluate_matches_gcl_metric_definitions():
    """evaluate() == gcl.py:87-108 on a tiny graph.  Ties are excluded by construction: the convs are identities and
    every score is a small integer plus the item's own multiple of 1/1024 — exact in fp32 and distinct within a row — so
    the device ranking and the numpy argsort see the same order."""
    from recommendation_amd.gcl import GCLModel
    rng = np.random.default_rng(4)
    n_u, n_i, d = 40, 130, 64
    train = {(int(rng.integers(0, n_u)), int(rng.integers(0, n_i))) for _ in range(400)}
    train |= {(u, u) for u in range(n_u)} | {(i % n_u, i) for i in range(n_i)}
    test = {(int(rng.integers(0, n_u)), int(rng.integers(0, n_i))) for _ in range(240)} - train
    train, test = np.array(sorted(train)), np.array(sorted(test))
    rng.shuffle(test)
    config = dict(embedding_size=d, num_layers=2, lr=1e-3, weight_decay=0.0, ssl_temp=0.2, drop_edge=0.2,
                  reg_weight=1e-4, batch_size=64, max_epoch=1)
    model = GCLModel(config, (train[:, 0], train[:, 1]), (test[:, 0], test[:, 1]), device="cuda", num_users=n_u,
                     num_items=n_i)
    ue = rng.integers(-3, 4, (n_u, d)).astype(np.float32)
    ie = rng.integers(-3, 4, (n_i, d)).astype(np.float32)
    ue[:, -1] = 1.0
    ie[:, -1] = rng.permutation(n_i) / 1024.0
    with torch.no_grad():
        model.model.user_emb.weight.copy_(torch.from_numpy(ue))
        model.model.item_emb.weight.copy_(torch.from_numpy(ie))
        for conv in model.model.convs:
            conv.weight.copy_(torch.eye(d))
            conv.bias.zero_()
    u_emb, i_emb = model.embeddings()
    assert np.array_equal(u_emb.cpu().numpy(), ue) and np.array_equal(i_emb.cpu().numpy(), ie)
    ks = [10, 20, 30, 50]
    got = model.evaluate(ks)
    ref = _numpy_gcl_evaluate(ue, ie, test[:, 0], test[:, 1], train[:, 0], train[:, 1], ks)
    assert set(got) == set(ks)
    for k in ks:
        assert set(got[k]) == {"HR", "P", "R", "NDCG"}
        for m in ("HR", "P", "R", "NDCG"):
            assert got[k][m] == pytest.approx(ref[k][m], rel=1e-12, abs=1e-12), (k, m)
    assert got[10]["HR"] > 0 and got[10]["NDCG"] > 0


def _lightgcn_model(drop_edge, seed=0):
    from recommendation_amd.gcl import GCLModel
    from oracle import oracle_np as O
    n_u, n_i = 150, 90
    u, i = O.synthetic_interactions(n_u, n_i, 1500, seed=2)
    config = dict(embedding_size=64, num_layers=3, lr=1e-3, weight_decay=1e-4, ssl_temp=0.2, drop_edge=drop_edge,
                  reg_weight=1e-3, ssl_weight=0.5, batch_size=128, max_epoch=1)
    return GCLModel(config, (u, i), (u[:10], i[:10]), device="cuda", seed=seed, encoder="lightgcn", num_users=n_u,
                    num_items=n_i)


def _unpack(bits, n):
    shifts = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits.unsqueeze(1) >> shifts) & 1).reshape(-1)[:n].bool()


def test_lightgcn_step_equals_autograd_composition():
    """One train_step of the lightgcn form == lightgcn_propagate over each view's explicitly masked operator (its own
    device transpose for the backward) + proj_head + info_nce_loss + bpr_sums, by autograd: loss terms and every
    parameter's gradient to 2e-6."""
    import recommendation_amd as ra
    from recommendation_amd.gcl import GRACEModel
    from recommendation_amd import functional as Fn
    from recommendation_amd import losses as Ls
    m = _lightgcn_model(0.25)
    graph, n_u = m.model.graph, m.num_users
    rng = np.random.default_rng(1)
    b = 128
    users = torch.from_numpy(rng.integers(0, n_u, b)).cuda()
    pos = torch.from_numpy(rng.integers(0, m.num_items, b)).cuda()
    neg = torch.from_numpy(rng.integers(0, m.num_items, b)).cuda()
    ref_model = GRACEModel(m.num_users, m.num_items, m.emb_size, m.num_layers, device="cuda")
    ref_model.load_state_dict(m.model.state_dict())
    v1, v2 = m.views()
    assert not torch.equal(v1.keep_bits, v2.keep_bits)
    got = m.train_step(users, pos, neg, views=(v1, v2))

    def masked(view):
        keep = _unpack(view.keep_bits, graph.nnz)
        assert 0.6 < float(keep.float().mean()) < 0.9
        return ra.CsrGraph(graph.rowptr_host, graph.col, graph.val * keep.float(), graph.n_rows, graph.n_cols, "cuda",
                           symmetric=False)

    x = torch.cat([ref_model.user_emb.weight, ref_model.item_emb.weight])
    z1 = ref_model.proj_head(Fn.lightgcn_propagate(masked(v1), x, m.num_layers, "mean"))
    z2 = ref_model.proj_head(Fn.lightgcn_propagate(masked(v2), x, m.num_layers, "mean"))
    ssl = Ls.info_nce_loss(z1[:n_u], z2[:n_u], m.ssl_temp) + Ls.info_nce_loss(z1[n_u:], z2[n_u:], m.ssl_temp)
    s = Fn.bpr_sums(z1[:n_u].contiguous(), z1[n_u:].contiguous(), users, pos, neg, Fn.BPR_LOGSIGMOID)
    bpr, reg = s[0] / b, (s[1] + s[2] + s[3]) / b
    total = m.ssl_weight * ssl + bpr + m.reg_weight * reg
    total.backward()
    for name, a, r in zip(("ssl", "bpr", "reg", "total"), got, (ssl, bpr, reg, total)):
        assert float(a) == pytest.approx(float(r.detach()), rel=2e-6), name
    ref_grads = dict(ref_model.named_parameters())
    for name, p in m.model.named_parameters():
        rg = ref_grads[name].grad
        if name.startswith("convs."):
            assert p.grad is None and rg is None
            continue
        rg = rg.cpu().numpy()
        np.testing.assert_allclose(p.grad.cpu().numpy(), rg, rtol=2e-6, atol=2e-6 * np.abs(rg).max(), err_msg=name)


def test_lightgcn_views_identical_without_edge_drop():
    """drop_edge = 0: both views keep every edge, so the two propagated-and-projected views are bit-identical (and with
    drop_edge > 0 they are not)."""
    m = _lightgcn_model(0.0)
    v1, v2 = m.views()
    z1, z2 = m.model(v1, v2)
    assert z1 is not z2 and torch.equal(z1, z2)
    m = _lightgcn_model(0.2)
    z1, z2 = m.model(*m.views())
    assert not torch.equal(z1, z2)


def test_gcl_model_trains_end_to_end():
    """GCLModel(config, train, test).train() (gcl.py:195-236 protocol) on a block-structured toy set: every stage on
    the HIP path, gcl.py's metric keys, and it learns — Recall@10 far above a random ranking's (10 of ~100 unseen
    items: ~0.1).  ssl_weight = 0.01 (the univariate key): with gcl.py's fixed weight of 1 the uniformity term of the
    faithful form (z1 == z2) dominates BPR and the reference itself stays near chance on this graph."""
    from recommendation_amd.gcl import GCLModel
    rng = np.random.default_rng(0)
    n_u, n_i, groups = 300, 120, 6
    pairs = set()
    while len(pairs) < 7000:
        u = int(rng.integers(0, n_u))
        g = u % groups
        i = int(rng.integers(0, n_i // groups)) * groups + g if rng.random() < 0.9 else int(rng.integers(0, n_i))
        pairs.add((u, i))
    pairs = np.array(sorted(pairs))
    rng.shuffle(pairs)
    train, test = pairs[:6000], pairs[6000:]
    config = dict(embedding_size=64, num_layers=2, lr=0.01, weight_decay=1e-4, ssl_temp=0.2, drop_edge=0.2,
                  reg_weight=1e-4, ssl_weight=0.01, batch_size=256, max_epoch=10)
    model = GCLModel(config, (train[:, 0], train[:, 1]), (test[:, 0], test[:, 1]), device="cuda", seed=1)
    metrics = model.train()
    print("GCL end-to-end metrics:", metrics)
    assert set(metrics) == {10, 20, 30, 50}
    assert all(set(v) == {"HR", "P", "R", "NDCG"} for v in metrics.values())
    assert metrics[10]["R"] > 0.4, metrics
    assert metrics[50]["HR"] >= metrics[10]["HR"]
