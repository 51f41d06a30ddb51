"""DirectAU on the GPU against tests/golden/directau_steps.npz — numbers the reference itself computed in float64
(scripts/gen_golden_directau.py): the fused alignment + uniformity sums and their gradients, FusedSGD, six training
steps per configuration, evaluate() and one end-to-end run.

Tolerances.  Values: rtol 1e-5, the project's parity bound.  Gradients and final tables: 4 x max(slack, floor), slack
being the drift of the reference's OWN float32 run from its float64 run, floor 1e-7 x max |ref| for a gradient tensor and
1e-7 for a table (the trajectory rule of tests/step_pins.py, family "directau").  In the two zero-row cases the all-zero row, whose gradient
is ~1e10 (F.normalize divides by eps), is bounded apart from the other rows: slack and max |ref| of the other rows
exclude it, so the rows it is paired with are held to a bound of their own size.  calculate_loss, the training loss and `mix` are differences
of an alignment (> 0) and uniformities (< 0): like `loss` in the trajectories they are held to 1e-5 x the sum of the
sizes of their parts, not of their own size."""
import math

import numpy as np
import pytest
import torch

import directau_fixture as fx
import step_pins as sp

pytestmark = pytest.mark.gpu

_, CASES, CONFIGS = fx.load()


def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _mix(Fn, Ls, c, ut, it, u, i, j):
    s = Fn.au_sums(ut, it, u, i, j, t=c.t)
    unif = Ls._log_mean_pairs(s[2:5], c.batch) if c.batch >= 2 else torch.zeros(3, device=s.device)
    return s[0] / c.batch + fx.MIX_NEG * s[1] / c.batch + c.gamma * (unif[0] + fx.MIX_P * unif[1] + fx.MIX_N * unif[2])


@pytest.mark.parametrize("k", range(len(CASES)), ids=[repr(c) for c in CASES])
def test_components_against_reference_float64(k):
    """au_sums, alignment, uniformity and directau_loss on the fixture's seeded tables and batches (duplicate ids in
    every batch of 512 and more, a zero row in two cases, d = 100 zero-padded): values at rtol 1e-5 of the reference's
    float64, table gradients of the training loss and of `mix` within 4 x max(slack, 1e-7 x max |ref|).
    In the zero-row cases the bound of the ordinary rows is taken without the zero row, which is checked apart.
    Measured on an MI355X (the ratios this test prints): values within 0.062 x, gradients within 0.37 x the tolerance
    (d = 16, B = 1, `mix`, item table); zero-row cases: ordinary rows 0.092 x, the zero row itself 0.392 x its own bound."""
    from recommendation_amd import functional as Fn, losses as Ls
    c = CASES[k]
    ut_np, it_np, u_np, i_np, j_np = c.inputs()
    u, i, j = _dev(u_np), _dev(i_np), _dev(j_np)
    ut, it = _dev(ut_np, True), _dev(it_np, True)
    B = c.batch

    sums = _np(Fn.au_sums(ut, it, u, i, j, t=c.t))
    ref = c.value("sums")
    worst = 0.0
    for n in range(8):
        if ref[n] == 0:
            assert sums[n] == 0
        else:
            worst = max(worst, abs(sums[n] - ref[n]) / abs(ref[n]) / 1e-5)
    print(f"{c}: au_sums worst rel err / 1e-5 = {worst:.3f}")
    got = {}
    with torch.no_grad():
        ue, pe, ne = Fn.gather_rows(ut, u), Fn.gather_rows(it, i), Fn.gather_rows(it, j)
        got["align_pos"], got["align_neg"] = Ls.alignment(ue, pe), Ls.alignment(ue, ne)
        got["unif_u"], got["unif_p"], got["unif_n"] = (Ls.uniformity(x, c.t) for x in (ue, pe, ne))
    for name, v in got.items():
        r = float(c.value(name))
        if B == 1 and name.startswith("unif"):
            assert float(v) == 0.0 and not v.requires_grad               # directau.py:251: no pair
            continue
        ratio = abs(float(v) - r) / abs(r) / 1e-5
        worst = max(worst, ratio)
        print(f"{c}: {name} rel err / 1e-5 = {ratio:.3f}")
    np.testing.assert_allclose(sums, ref, rtol=1e-5, atol=0)
    for name, v in got.items():
        np.testing.assert_allclose(float(v), float(c.value(name)), rtol=1e-5, atol=0, err_msg=name)

    # the training loss of directau.py:223-226 (batch.size = B) and its gradient
    pos, neg, l2, loss = Ls.directau_loss(ut, it, u, i, j, c.gamma, c.reg, B)
    size_pos = abs(c.value("align_pos")) + abs(c.value("calc_pos") - c.value("align_pos"))
    size_neg = abs(c.value("align_neg")) + abs(c.value("calc_neg") - c.value("align_neg"))
    l2_ref = c.reg * np.sqrt(ref[5:8]).sum() / B
    for name, v, r, size in (("calc_pos", pos, c.value("calc_pos"), size_pos), ("calc_neg", neg, c.value("calc_neg"), size_neg),
                             ("l2", l2, l2_ref, abs(l2_ref)), ("train", loss, c.value("train"), size_pos + size_neg + l2_ref / B)):
        err = abs(float(v.detach()) - float(r))
        print(f"{c}: {name} err / (1e-5 x size of parts) = {err / (1e-5 * float(size)):.3f}")
        assert err <= 1e-5 * float(size), name
    loss.backward()
    grads = {"train": {"user_emb": _np(ut.grad), "item_emb": _np(it.grad)}}
    ut.grad = it.grad = None
    mix = _mix(Fn, Ls, c, ut, it, u, i, j)
    size_mix = abs(c.value("align_pos")) + fx.MIX_NEG * abs(c.value("align_neg")) + c.gamma * (
        abs(c.value("unif_u")) + fx.MIX_P * abs(c.value("unif_p")) + fx.MIX_N * abs(c.value("unif_n")))
    assert abs(float(mix.detach()) - float(c.value("mix"))) <= 1e-5 * float(size_mix)
    mix.backward()
    grads["mix"] = {"user_emb": _np(ut.grad), "item_emb": _np(it.grad)}
    report, bad = [], []
    for obj in fx.OBJECTIVES:
        for tab in fx.TABLES:
            assert np.all(np.isfinite(grads[obj][tab]))
            tol = sp.F32 * max(c.grad_slack(obj, tab), sp.FLOOR * c.grad_max(obj, tab))
            err = float(np.abs(c.at(tab, grads[obj][tab]) - c.grad(obj, tab)).max())
            report.append(f"{c}: grad {obj}/{tab} max err {err:.3g}, tolerance {tol:.3g} ({err / tol:.3f}x), max |ref| {c.grad_max(obj, tab):.3g}")
            if err > tol:
                bad.append(report[-1])
            if c.zero_row:
                # the all-zero row on its own: F.normalize's backward multiplies its gradient by 1 / eps = 1e12, so it
                # gets a bound from its own slack and size and takes no part in the bound of the rows above
                zg, zslack, zmax = c.zero_grad(obj, tab)
                ztol = sp.F32 * max(zslack, sp.FLOOR * zmax)
                zerr = float(np.abs(grads[obj][tab][c.zero_index(tab)] - zg).max())
                report.append(f"{c}: grad {obj}/{tab} ZERO ROW max err {zerr:.3g}, tolerance {ztol:.3g} ({zerr / ztol:.3f}x), max |ref| {zmax:.3g}")
                if zerr > ztol:
                    bad.append(report[-1])
    print("\n".join(report))
    assert not bad, "\n".join(bad)


def test_single_row_and_two_set_forms():
    """uniformity of fewer than two rows is exactly 0.0 without a gradient; au_sums without j covers two sets and leaves
    the third's entries 0; a [B, d] tensor without index vectors addresses its own rows."""
    from recommendation_amd import functional as Fn, losses as Ls
    rng = np.random.default_rng(5)
    x = _dev(rng.standard_normal((1, 64)).astype(np.float32), True)
    v = Ls.uniformity(x)
    assert float(v) == 0.0 and not v.requires_grad
    a = _dev(rng.standard_normal((77, 48)).astype(np.float32), True)
    b = _dev(rng.standard_normal((77, 48)).astype(np.float32), True)
    s2 = Fn.au_sums(a, b, None, None)
    idx = torch.arange(77, device="cuda")
    s3 = Fn.au_sums(a, b, idx, idx, idx)
    assert s2[1] == 0 and s2[4] == 0 and s2[7] == 0
    assert torch.equal(s2[[0, 2, 3, 5, 6]], s3[[0, 2, 3, 5, 6]]) and float(s3[1]) == float(s3[0]) and float(s3[4]) == float(s3[3])
    an, bn = torch.nn.functional.normalize(a.detach().double(), dim=-1), torch.nn.functional.normalize(b.detach().double(), dim=-1)
    assert float(Ls.alignment(a, b)) == pytest.approx(float(torch.sum((an - bn) ** 2, dim=1).mean()), rel=1e-5)
    ref_u = torch.log(torch.mean(torch.exp(-2.0 * torch.pdist(an) ** 2)) + 1e-8)
    assert float(Ls.uniformity(a)) == pytest.approx(float(ref_u), rel=1e-5)
    from recommendation_amd import _lib
    with pytest.raises(_lib.GcrError):
        Fn.au_sums(a.detach().cpu(), b.detach().cpu(), None, None)


def test_out_of_range_ids_give_zero_rows_and_no_gradient():
    """An id outside its table behaves as in gather_rows: a zero row in the forward, nothing added by the backward.  The
    same batch with those positions pointed at an appended all-zero row gives bit-equal sums and the same gradients."""
    from recommendation_amd import functional as Fn
    rng = np.random.default_rng(6)
    n_u, n_i, d, B = 50, 40, 64, 200
    ut_np = (rng.standard_normal((n_u, d)) * 0.1).astype(np.float32)
    it_np = (rng.standard_normal((n_i, d)) * 0.1).astype(np.float32)
    u, i, j = rng.integers(0, n_u, B), rng.integers(0, n_i, B), rng.integers(0, n_i, B)
    bad_u, bad_i, bad_j = u.copy(), i.copy(), j.copy()
    bad_u[[3, 150]], bad_i[[7]], bad_j[[7, 199]] = [-1, n_u + 5], [n_i], [-(2 ** 40), 2 ** 40]
    ok_u, ok_i, ok_j = u.copy(), i.copy(), j.copy()
    ok_u[[3, 150]], ok_i[[7]], ok_j[[7, 199]] = n_u, n_i, n_i
    w = _dev(np.array([1.0, -0.7, 0.3, 0.2, -0.4, 0.01, 0.02, 0.03], dtype=np.float32))

    def run(ut_np, it_np, u, i, j):
        ut, it = _dev(ut_np, True), _dev(it_np, True)
        s = Fn.au_sums(ut, it, _dev(u), _dev(i), _dev(j))
        (s * w).sum().backward()
        return s.detach(), ut.grad, it.grad

    s_bad, gu_bad, gi_bad = run(ut_np, it_np, bad_u, bad_i, bad_j)
    zero = np.zeros((1, d), np.float32)
    s_ok, gu_ok, gi_ok = run(np.concatenate([ut_np, zero]), np.concatenate([it_np, zero]), ok_u, ok_i, ok_j)
    assert torch.equal(s_bad, s_ok) and torch.isfinite(s_bad).all()
    for got, ref in ((gu_bad, gu_ok[:n_u]), (gi_bad, gi_ok[:n_i])):
        assert torch.isfinite(got).all()
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("d,B", [(64, 2048), (512, 300), (32, 127)])
def test_forward_is_bitwise_reproducible(d, B):
    """Two forwards give the same bits in all eight sums (and in r / o, through the gradient-side buffers): fixed-order
    reductions, no float atomics."""
    from recommendation_amd import functional as Fn
    rng = np.random.default_rng(d + B)
    ut = _dev((rng.standard_normal((500, d)) * 0.1).astype(np.float32), True)
    it = _dev((rng.standard_normal((400, d)) * 0.1).astype(np.float32), True)
    u, i, j = (_dev(rng.integers(0, n, B)) for n in (500, 400, 400))
    a = Fn.au_sums(ut, it, u, i, j)
    b = Fn.au_sums(ut, it, u, i, j)
    with torch.no_grad():
        c = Fn.au_sums(ut, it, u, i, j)
    assert torch.equal(a, b)
    # the sums-only launch skips the o slices: the same pair tiles in the same order for the first slice
    np.testing.assert_allclose(_np(c), _np(a), rtol=1e-6)
    saved_a, saved_b = a.grad_fn.saved_tensors, b.grad_fn.saved_tensors
    for x, y in zip(saved_a[5:], saved_b[5:]):                         # inv_norm, r, o
        assert torch.equal(x, y)


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_fused_sgd_against_float64_torch_sgd(weight_decay):
    """Five steps of FusedSGD against torch.optim.SGD(momentum=0.9) run in float64 on the same float32 gradients.

    Bound, from the operations of one step: the kernel rounds three times per element — g' = grad + wd p, buf = mu buf +
    g', p = p - lr buf (each one fused multiply-add, u = 2^-24 relative).  With M = max(|buf|, |g'|) and P = max |p| over the
    run, buf after k steps is off by at most 2 u M k (its two roundings per step, the older ones damped by mu < 1), so
    p after n steps by at most  u (n P + lr M n (n + 1)):  n roundings of p itself plus lr x the buffer errors summed."""
    from recommendation_amd.optim import FusedSGD
    torch.manual_seed(3)
    n, lr, mu = 5, 0.05, 0.9
    p32 = torch.nn.Parameter(torch.randn(301, 67, device="cuda"))            # 20167 elements: exercises the n % 4 tail
    p64 = torch.nn.Parameter(p32.detach().double().clone())
    ours = FusedSGD([p32], lr=lr, momentum=mu, weight_decay=weight_decay)
    theirs = torch.optim.SGD([p64], lr=lr, momentum=mu, weight_decay=weight_decay)
    big_p, big_m = float(p64.abs().max()), 0.0
    for step in range(n):
        g = torch.randn(301, 67, device="cuda")
        p32.grad, p64.grad = g.clone(), g.double()
        ours.step()
        theirs.step()
        buf64 = theirs.state[p64]["momentum_buffer"]
        big_p = max(big_p, float(p64.abs().max()))
        big_m = max(big_m, float(buf64.abs().max()), float((g.double().abs() + weight_decay * p64.abs()).max()))
        if step == 0 and weight_decay == 0.0:
            assert torch.equal(ours.state[p32]["momentum_buffer"], g)         # buf = g on the first step
    u = 2.0 ** -24
    tol_p = u * (n * big_p + lr * big_m * n * (n + 1))
    tol_m = 2 * u * big_m * n
    err_p = float((p32.detach().double() - p64.detach()).abs().max())
    err_m = float((ours.state[p32]["momentum_buffer"].double() - theirs.state[p64]["momentum_buffer"]).abs().max())
    print(f"wd {weight_decay}: param err {err_p:.3g} (bound {tol_p:.3g}), buffer err {err_m:.3g} (bound {tol_m:.3g})")
    assert err_p <= tol_p and err_m <= tol_m
    assert float((p64.detach() - p32.detach().double()).abs().max()) < 1e-3 * float((p64.detach()).abs().max())


@pytest.mark.parametrize("c", range(len(CONFIGS)), ids=[repr(c) for c in CONFIGS])
def test_trajectory_matches_reference_float64(c):
    """Six train_steps from the fixture's state on its batches, by the rule of tests/step_pins.py: pos_loss, neg_loss and l2
    at rtol 1e-5 of the reference's float64 run, loss (their difference) within 1e-5 x (|pos_loss| + |neg_loss|); both
    tables within 4 x max(slack, 1e-7) of their float64 finals and moved by more than 100 x slack.  The fixture runs at learning.rate 5e-3, the largest
    value of the reference's grid (scripts/gen_golden_directau.py, `LR_GRID`)."""
    from recommendation_amd.directau import DirectAUModel
    g = np.load(fx.GOLDEN, allow_pickle=False)
    cf = CONFIGS[c]
    model = DirectAUModel(cf.conf(), fx.train_records(g), [], device="cuda")
    # sorted dense ids (directau.py:116-117): the fixture's batches index these rows
    sp.assert_dense_id_order(model, g)
    assert type(model.optimizer).__name__ == {"adam": "FusedAdam", "sgd": "FusedSGD"}[cf.optimizer]
    with torch.no_grad():
        for k in fx.TABLES:
            model.model.embedding_dict[k].copy_(_dev(cf.init(k)))
    got = []
    for batch in fx.batches(g):
        out = model.train_step(tuple(_dev(b) for b in batch))
        assert not any(v.requires_grad for v in out)
        got.append(torch.stack([v.reshape(()) for v in out]))
    sp.check(cf.record(), torch.stack(got).cpu().numpy(), {k: _np(model.model.embedding_dict[k]) for k in fx.TABLES})


def _numpy_ranking_evaluation(query, items, train, test, top_n):
    """directau.py:167-178 and 39-64, restated: per test user the n best unseen items; Hit Ratio = hits over all test
    items, Precision = hits / (users x n), Recall = mean of hits / test items of the user, NDCG = mean DCG / IDCG; all
    rounded to 5 places."""
    scores = query.astype(np.float64) @ items.astype(np.float64).T
    known, origin = {}, {}
    for u, i in train:
        known.setdefault(int(u), set()).add(int(i))
    for u, i in test:
        origin.setdefault(int(u), set()).add(int(i))
    hits, recall, ndcg = 0, 0.0, 0.0
    for u, ts in origin.items():
        s = scores[u].copy()
        s[list(known[u])] = -1e8
        top = np.argsort(-s, kind="stable")[:top_n]
        h = [int(t) in ts for t in top]
        hits += sum(h)
        recall += sum(h) / len(ts)
        dcg = sum(1 / math.log2(r + 2) for r, hit in enumerate(h) if hit)
        idcg = sum(1 / math.log2(r + 2) for r in range(min(top_n, len(ts))))
        ndcg += dcg / idcg
    q = len(origin)
    return {"Hit Ratio": round(hits / sum(len(t) for t in origin.values()), 5), "Precision": round(hits / (q * top_n), 5),
            "Recall": round(recall / q, 5), "NDCG": round(ndcg / q, 5)}


def test_evaluate_and_predict():
    """evaluate() == the numpy restatement of the metric definitions on tie-free embeddings (small integers plus the
    item's own multiple of 1/1024, exact in fp32): the LAST cut-off's four metrics, as the reference's dict
    comprehension leaves them (directau.py:266); predict() is the user's score row; calculate_loss is one fused forward."""
    from recommendation_amd.directau import DirectAUModel
    rng = np.random.default_rng(4)
    n_u, n_i, d = 40, 130, 32
    train = {(int(rng.integers(0, n_u)), int(rng.integers(0, n_i))) for _ in range(400)}
    train |= {(u, u) for u in range(n_u)} | {(i % n_u, i) for i in range(n_i)}
    test = {(int(rng.integers(0, n_u)), int(rng.integers(0, n_i))) for _ in range(240)} - train
    train, test = sorted(train), sorted(test)
    conf = {"embedding.size": d, "batch.size": 64, "item.ranking.topN": [10, 20], "DirectAU": {"gamma": 1.0, "n_layers": 2}}
    model = DirectAUModel(conf, [(f"u{u}", f"i{i}", 1.0) for u, i in train], [(f"u{u}", f"i{i}", 1.0) for u, i in test],
                          device="cuda")
    assert model.reg == 1e-4 and model.lRate == 1e-3 and model.topN == [10, 20] and model.max_N == 20
    assert type(model.optimizer).__name__ == "FusedAdam"
    data = model.data
    ue, ie = model.embeddings()
    assert ue.shape == (n_u, d) and ie.shape == (n_i, d) and not ue.requires_grad
    u_ref, i_ref, _ = model.model()                                     # the encoder's own forward (all layers kept)
    torch.testing.assert_close(ue, u_ref.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ie, i_ref.detach(), rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        cl = model.calculate_loss(ue[:33], ie[:33])
        un, in_ = torch.nn.functional.normalize(ue[:33].double(), dim=-1), torch.nn.functional.normalize(ie[:33].double(), dim=-1)
        align = torch.sum((un - in_) ** 2, dim=1).mean()
        unif = [torch.log(torch.mean(torch.exp(-2.0 * torch.pdist(x) ** 2)) + 1e-8) for x in (un, in_)]
    want, size = float(align + 0.5 * (unif[0] + unif[1])), float(align + 0.5 * (unif[0].abs() + unif[1].abs()))
    assert abs(float(cl) - want) <= 1e-5 * size

    qe = rng.integers(-3, 4, (n_u, d)).astype(np.float32)
    ie_np = rng.integers(-3, 4, (n_i, d)).astype(np.float32)
    qe[:, -1] = 1.0
    ie_np[:, -1] = rng.permutation(n_i) / 1024.0
    model.user_emb, model.item_emb = _dev(qe), _dev(ie_np)
    got = model.evaluate()
    tr = [(data.user[f"u{u}"], data.item[f"i{i}"]) for u, i in train]
    te = [(data.user[f"u{u}"], data.item[f"i{i}"]) for u, i in test]
    ref = _numpy_ranking_evaluation(qe, ie_np, tr, te, 20)
    assert set(got) == {"Hit Ratio", "Precision", "Recall", "NDCG"}
    for k in ref:
        assert got[k] == pytest.approx(ref[k], abs=1.1e-5), (k, got, ref)
    assert got["Recall"] > 0
    uid = data.user["u7"]
    assert np.array_equal(model.predict("u7"), (model.user_emb[uid] @ model.item_emb.T).cpu().numpy())


def test_directau_trains_end_to_end():
    """DirectAUModel(conf, train, test).train() on the block-structured toy set of the GCL / SSL4Rec convergence tests,
    same bar: Recall@10 > 0.4 where a random ranking gives ~0.1.  The reference trains ONE epoch (directau.py:217), so
    the configuration is taken from its grid to make 6000 pairs enough: batch.size 64 (94 steps), learning.rate 5e-3,
    Adam, one layer, gamma 0.5.  The reference itself, run on the CPU with these settings, reaches Recall@10 0.83 from
    0.09 - 0.27 untrained (two seeds)."""
    from recommendation_amd.directau import DirectAUModel
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
    conf = {"embedding.size": 64, "batch.size": 64, "learning.rate": 5e-3, "optimizer": "adam", "item.ranking.topN": [10],
            "DirectAU": {"gamma": 0.5, "n_layers": 1}}
    model = DirectAUModel(conf, [(int(u), int(i), 1.0) for u, i in train], [(int(u), int(i), 1.0) for u, i in test],
                          device="cuda", seed=1)
    before = model.evaluate()
    del model.user_emb, model.item_emb
    metrics = model.train()
    print("DirectAU end-to-end metrics:", metrics, "untrained:", before)
    assert set(metrics) == {"Hit Ratio", "Precision", "Recall", "NDCG"}
    assert metrics["Recall"] > 0.4, metrics
    assert model.user_emb.shape == (n_u, 64) and model.item_emb.shape == (n_i, 64)
