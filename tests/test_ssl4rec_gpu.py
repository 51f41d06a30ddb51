"""SSL4Rec on the GPU (recommendation_amd/ssl4rec.py and the fused gather + dropout-views kernel behind it):

  * kernel forward: bit-equal to gather_rows x the unpacked gcr_edge_mask_bits draw x 1 / (1 - p), replay of recorded
    bits, distinct masks per view and seed;
  * kernel backward: float64 autograd of that composition, per-element bound from the number of addends;
  * both again where the entry points take their other kernel (one column per lane instead of 16 bytes per lane): widths
    that are no multiple of four, a table and a gradient that start 4 bytes past a 16-byte boundary (equal to the 16-byte
    kernels' results: keep1 against keep4), and more batch rows than the grid cap holds waves;
  * trajectory: six train_steps per fixture config (tests/golden/ssl4rec_steps.npz: ssl4rec.py's own loop body run in
    float64 by the reference, the dropout masks recorded) — loss terms and final parameters;
  * evaluation: embeddings() and the metric definitions of ssl4rec.py:104-123 restated in numpy;
  * convergence: train() on the planted-structure graph of the GCL convergence test, same bar."""
import math

import numpy as np
import pytest
import torch

import ssl4rec_fixture as fx
import step_pins as sp

pytestmark = pytest.mark.gpu

NS = (1, 127, 2048, 4096)
PS = (0.0, 0.1, 0.3, 1.0)
ODD_WIDTHS = (1, 3, 50, 101, 130)                 # d % 4 != 0: the one-column-per-lane kernels, forward and backward
N_CAPPED = 32768 + 37                             # more rows than 8192 workgroups x 4 waves: the second grid-stride trip


def _unpack(bits, n):
    shifts = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits.unsqueeze(1) >> shifts) & 1).reshape(-1)[:n].bool()


def _scale(p):
    """1.0f / (1.0f - p) as the kernel's host side computes it."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def _ids(rng, n, n_rows):
    """Ids with duplicates (n_rows < n for the larger n) and, from four rows on, ids outside the table."""
    idx = rng.integers(0, n_rows, n)
    if n >= 4:
        idx[[0, n // 2, n - 1]] = [-1, n_rows, n_rows + 5]
        idx[1] = idx[2]
    return torch.from_numpy(idx).cuda()


def _composition(table, idx, p, seed, n_views):
    """[(1 + V) n, d] from the parent ops: gather_rows, then each view = where(keep_v, rows * scale, 0)."""
    from recommendation_amd import functional as Fn
    n, d = idx.numel(), table.shape[1]
    rows = Fn.gather_rows(table, idx)
    blocks, keeps = [rows], []
    scale = torch.tensor(_scale(p) if p < 1 else np.float32(np.inf), device="cuda")
    for v in range(n_views):
        keep = _unpack(Fn.edge_mask_bits(n * d, p, seed + v, "cuda"), n * d).view(n, d)
        keeps.append(keep)
        blocks.append(torch.where(keep, rows * scale, torch.zeros_like(rows)))
    return torch.cat(blocks), keeps


def _composition_indexed(table, idx, p, seed, n_views):
    """`_composition` with the clean rows from plain torch indexing instead of gather_rows (whose own choice of kernel by
    width and alignment must not decide what the reference is); the keep masks are the same independent statement of
    "bit i * d + c of the flat stream of seed + v"."""
    from recommendation_amd import functional as Fn
    n, d = idx.numel(), table.shape[1]
    ok = ((idx >= 0) & (idx < table.shape[0])).unsqueeze(1)
    rows = torch.where(ok, table[idx.clamp(0, table.shape[0] - 1)], torch.zeros((), device=table.device))
    blocks = [rows]
    scale = torch.tensor(_scale(p) if p < 1 else np.float32(np.inf), device="cuda")
    for v in range(n_views):
        keep = _unpack(Fn.edge_mask_bits(n * d, p, seed + v, "cuda"), n * d).view(n, d)
        blocks.append(torch.where(keep, rows * scale, torch.zeros_like(rows)))
    return torch.cat(blocks)


def _misaligned(shape, rng):
    """A contiguous float32 tensor of this shape, 4 bytes past a 16-byte boundary, and an aligned copy of it."""
    numel = int(np.prod(shape))
    buf = torch.from_numpy(rng.standard_normal(numel + 8).astype(np.float32)).cuda()
    t = buf[1:1 + numel].view(*shape)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()                # otherwise the vec4 kernel runs and nothing is tested
    aligned = t.clone()
    assert aligned.data_ptr() % 16 == 0
    return t, aligned


@pytest.mark.parametrize("d", ODD_WIDTHS)
def test_gather_dropout_forward_at_widths_that_are_no_multiple_of_four(d):
    """gather_dropout_kernel (one column per lane, keep1): bit-equal to the composition over indexed rows, replay of the
    recorded bits included, zero rows for ids outside the table in every block."""
    from recommendation_amd import functional as Fn
    rng = np.random.default_rng(1000 + d)
    n_rows = 300
    table = torch.from_numpy(rng.standard_normal((n_rows, d)).astype(np.float32)).cuda()
    for n in NS:
        idx = _ids(rng, n, n_rows)
        assert torch.equal(_composition_indexed(table, idx, 0.0, 0, 1)[:n], Fn.gather_rows(table, idx))
        for p in PS:
            seed = 1000 * n + int(100 * p) + 7
            got = Fn.gather_dropout_views(table, idx, p, seed, 2)
            assert got.shape == (3 * n, d)
            assert torch.equal(got, _composition_indexed(table, idx, p, seed, 2)), (d, n, p)
            if n >= 4:
                bad = torch.tensor([0, n // 2, n - 1], device="cuda")
                assert not got.view(3, n, d)[:, bad].any()
            if 0 < p < 1:
                bits = torch.stack([Fn.edge_mask_bits(n * d, p, seed + v, "cuda") for v in range(2)])
                assert torch.equal(Fn.gather_dropout_views(table, idx, p, seed + 12345, 2, keep_bits=bits), got)
    if d == 50:
        idx = _ids(rng, 127, n_rows)
        for n_views in (1, 3, 4):
            got = Fn.gather_dropout_views(table, idx, 0.3, 5, n_views)
            assert torch.equal(got, _composition_indexed(table, idx, 0.3, 5, n_views)), n_views


def test_gather_dropout_forward_from_a_misaligned_table():
    """d = 64 from a table that starts 4 bytes past a 16-byte boundary takes the one-column-per-lane kernel; its aligned copy
    takes the vec4 kernel.  Equal outputs: keep1 is component e & 3 of keep4, for drawn and for recorded bits."""
    from recommendation_amd import functional as Fn
    rng = np.random.default_rng(64)
    table, aligned = _misaligned((300, 64), rng)
    for n in (127, 2048):
        idx = _ids(rng, n, 300)
        got = Fn.gather_dropout_views(table, idx, 0.3, 11, 2)
        assert torch.equal(got, Fn.gather_dropout_views(aligned, idx, 0.3, 11, 2))
        assert torch.equal(got, _composition_indexed(aligned, idx, 0.3, 11, 2))
        bits = torch.stack([Fn.edge_mask_bits(n * 64, 0.3, 500 + v, "cuda") for v in range(2)])
        rec = Fn.gather_dropout_views(table, idx, 0.3, 0, 2, keep_bits=bits)
        assert torch.equal(rec, Fn.gather_dropout_views(aligned, idx, 0.3, 0, 2, keep_bits=bits))
        assert torch.equal(rec, _composition_indexed(aligned, idx, 0.3, 500, 2)) and not torch.equal(rec, got)


@pytest.mark.parametrize("d", [32, 50])
def test_gather_dropout_beyond_the_grid_cap(d):
    """N_CAPPED rows over a 300-row table: the waves of both forward and both backward kernels (d = 32: vec4, d = 50: one
    column per lane) take a second trip, and a table row collects about a hundred duplicates."""
    from recommendation_amd import functional as Fn
    rng = np.random.default_rng(d)
    table = torch.from_numpy(rng.standard_normal((300, d)).astype(np.float32)).cuda()
    idx = _ids(rng, N_CAPPED, 300)
    got = Fn.gather_dropout_views(table, idx, 0.3, 21, 2)
    assert torch.equal(got, _composition_indexed(table, idx, 0.3, 21, 2))
    _check_backward(d, N_CAPPED, 0.3, 2)


@pytest.mark.parametrize("d", [32, 64, 100, 1024])
def test_gather_dropout_forward_is_bit_equal_to_the_composition(d):
    from recommendation_amd import functional as Fn
    rng = np.random.default_rng(d)
    n_rows = 300
    table = torch.from_numpy(rng.standard_normal((n_rows, d)).astype(np.float32)).cuda()
    for n in NS:
        idx = _ids(rng, n, n_rows)
        for p in PS:
            seed = 1000 * n + int(100 * p) + 7
            got = Fn.gather_dropout_views(table, idx, p, seed, 2)
            ref, keeps = _composition(table, idx, p, seed, 2)
            assert got.shape == (3 * n, d)
            assert torch.equal(got, ref), (d, n, p)
            assert torch.equal(got[:n], Fn.gather_rows(table, idx))
            if p == 0.0:
                assert torch.equal(got[n:2 * n], got[:n]) and torch.equal(got[2 * n:], got[:n])
            if p == 1.0:
                assert not got[n:].any()
            if n >= 4:
                bad = torch.tensor([0, n // 2, n - 1], device="cuda")
                assert not got.view(3, n, d)[:, bad].any()
            if 0 < p < 1:
                # replay of the recorded bits under another seed == the seeded draw
                bits = torch.stack([Fn.edge_mask_bits(n * d, p, seed + v, "cuda") for v in range(2)])
                assert torch.equal(Fn.gather_dropout_views(table, idx, p, seed + 12345, 2, keep_bits=bits), got)
                if n * d >= 4096:
                    assert not torch.equal(keeps[0], keeps[1])                       # the views differ
                    other = Fn.gather_dropout_views(table, idx, p, seed + 1, 2)      # another seed: other masks ...
                    assert not torch.equal(other[n:2 * n], got[n:2 * n])
                    assert torch.equal(other[n:2 * n], got[2 * n:])                  # ... view 0 of seed + 1 is view 1 of seed
                    share = float(keeps[0].float().mean())
                    assert abs(share - (1 - p)) < 4 * math.sqrt(p * (1 - p) / (n * d))


@pytest.mark.parametrize("n_views", [1, 3, 4])
def test_gather_dropout_view_counts(n_views):
    from recommendation_amd import functional as Fn
    rng = np.random.default_rng(n_views)
    for d in (64, 100):
        table = torch.from_numpy(rng.standard_normal((50, d)).astype(np.float32)).cuda()
        idx = _ids(rng, 127, 50)
        got = Fn.gather_dropout_views(table, idx, 0.3, 5, n_views)
        ref, _ = _composition(table, idx, 0.3, 5, n_views)
        assert torch.equal(got, ref)
    with pytest.raises(ValueError):
        Fn.gather_dropout_views(table, idx, 0.3, 5, 5)
    with pytest.raises(ValueError):
        Fn.gather_dropout_views(table, idx, 0.3, 5, 2, keep_bits=torch.zeros(2, 3, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("d,n,p,n_views", [(32, 127, 0.1, 2), (64, 2048, 0.3, 2), (64, 4096, 0.1, 2), (100, 127, 0.3, 2),
                                           (100, 2048, 0.1, 3), (1024, 127, 0.3, 2), (1024, 2048, 0.1, 1), (64, 1, 0.3, 2),
                                           (64, 2048, 0.0, 2), (64, 2048, 1.0, 2), (32, 4096, 0.3, 4)])
def test_gather_dropout_backward_against_float64_autograd(d, n, p, n_views):
    _check_backward(d, n, p, n_views)


@pytest.mark.parametrize("d,n,p,n_views", [(50, 127, 0.3, 2), (50, 2048, 0.1, 3), (101, 2048, 0.3, 2), (3, 4096, 0.3, 4),
                                           (1, 127, 0.3, 2), (50, 2048, 1.0, 2)])
def test_gather_dropout_backward_at_widths_that_are_no_multiple_of_four(d, n, p, n_views):
    """gather_dropout_bwd_kernel (one column per lane, keep1) by the rule of `_check_backward`."""
    _check_backward(d, n, p, n_views)


def test_gather_dropout_backward_from_a_misaligned_gradient():
    """d = 64 with a grad_out that starts 4 bytes past a 16-byte boundary takes the one-column-per-lane kernel.  The entry point
    is called directly, as tests/test_tri_gpu.py calls its own: autograd is free to hand the node a copy of the gradient."""
    from recommendation_amd import _lib
    rng = np.random.default_rng(640)
    d, n, n_rows, p, seed, n_views = 64, 2048, 300, 0.3, 99, 2
    idx = _ids(rng, n, n_rows)
    g_mis, g_al = _misaligned(((1 + n_views) * n, d), rng)
    table = torch.from_numpy(rng.standard_normal((n_rows, d)).astype(np.float32)).cuda()
    ref, bound, count = _float64_gradient(table, idx, p, seed, n_views, g_al)
    L = _lib.lib()
    got = []
    for g in (g_mis, g_al):
        gt = torch.zeros(n_rows, d, device="cuda")
        _lib.check(L.gcr_gather_dropout_bwd_f32(_lib.dptr(g), _lib.dptr(idx), n, d, n_rows, p, seed, n_views, None,
                                                _lib.dptr(gt), _lib.cur_stream(gt.device)), "gcr_gather_dropout_bwd_f32")
        assert bool(((gt.double() - ref).abs() <= bound).all())
        got.append(gt.double())
    worst = float(((got[0] - got[1]).abs() / bound.clamp(min=1e-300)).max())
    print(f"misaligned grad_out d={d} n={n}: max |misaligned - aligned| / bound = {worst:.3f}")
    assert bool(((got[0] - got[1]).abs() <= bound).all()), worst
    assert bool((got[0][count.squeeze(1) == 0] == 0).all())


def _float64_gradient(table, idx, p, seed, n_views, g_out):
    """(grad_table of the composition by float64 autograd, the bound of `_check_backward` per table element, duplicates per
    table row)."""
    from recommendation_amd import functional as Fn
    n, (n_rows, d) = idx.numel(), table.shape
    ok = ((idx >= 0) & (idx < n_rows))
    safe = idx.clamp(0, n_rows - 1)
    scale = float(_scale(p)) if p < 1 else 0.0
    keeps = [_unpack(Fn.edge_mask_bits(n * d, p, seed + v, "cuda"), n * d).view(n, d).double() for v in range(n_views)]

    def compose(t64, weight):
        rows = t64[safe] * ok.double().unsqueeze(1)
        blocks = [rows] + [rows * k * scale for k in keeps]
        return (torch.cat(blocks) * weight).sum()

    t64 = table.detach().double().requires_grad_(True)
    compose(t64, g_out.double()).backward()
    ref = t64.grad
    # sum |terms| per table element: the same composition is linear in the table, so its gradient under |g| is that sum
    ones = torch.ones_like(t64).requires_grad_(True)
    compose(ones, g_out.double().abs()).backward()
    sum_abs = ones.grad
    count = torch.bincount(safe[ok], minlength=n_rows).double().unsqueeze(1)
    m = count * (1 + n_views)
    bound = (m - 1).clamp(min=0) * 2.0 ** -23 * sum_abs
    return ref, bound, count


def _check_backward(d, n, p, n_views):
    """grad_table against float64 autograd of the composition (index gather, mask, scale, stack).  Per element the
    kernel and the atomics add m = duplicates x (1 + V) float32 terms: the error is at most (m - 1) roundings of 2^-24
    relative to a partial sum, each partial sum at most sum |terms|, and forming a term (one multiply by the scale) is
    one more rounding each — together under (m - 1) x 2^-23 x sum |terms| (m >= 2).  Replay of the bits gives the
    same gradient to that bound as well."""
    from recommendation_amd import functional as Fn
    rng = np.random.default_rng(d * 7 + n)
    n_rows = 300
    table = torch.from_numpy(rng.standard_normal((n_rows, d)).astype(np.float32)).cuda().requires_grad_(True)
    idx = _ids(rng, n, n_rows)
    seed = 99
    g_out = torch.from_numpy(rng.standard_normal(((1 + n_views) * n, d)).astype(np.float32)).cuda()
    out = Fn.gather_dropout_views(table, idx, p, seed, n_views)
    out.backward(g_out)
    got = table.grad.double()
    ref, bound, count = _float64_gradient(table, idx, p, seed, n_views, g_out)
    m = count * (1 + n_views)
    err = (got - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"d={d} n={n} p={p} V={n_views}: max err / bound = {worst:.3f}, max m = {int(m.max())}")
    assert bool((err <= bound).all()), worst
    assert bool((got[count.squeeze(1) == 0] == 0).all())
    if 0 < p < 1:
        table.grad = None
        bits = torch.stack([Fn.edge_mask_bits(n * d, p, seed + v, "cuda") for v in range(n_views)])
        Fn.gather_dropout_views(table, idx, p, 0, n_views, keep_bits=bits).backward(g_out)
        assert bool(((table.grad.double() - ref).abs() <= bound).all())


def _train_list(g):
    return [(str(u), str(i), 1.0) for u, i in zip(g["train_user"], g["train_item"])]


@pytest.mark.parametrize("c", [0, 1, 2])
def test_trajectory_matches_reference_float64(c):
    """Six train_steps from the fixture's state on its batches and recorded masks, by the rule of tests/step_pins.py
    (family "ssl4rec"): every loss term at rtol 1e-5 of the reference's float64 run; every parameter within
    4 x max(slack, 1e-7) (`atol_floor_4`) of its float64 final, slack being the drift of the reference's own float32 run;
    every parameter moved by more than 100 x slack.  Matrices with a 1024-wide side are compared at the fixture's seeded sample of entries.

    The fixture runs at learning.rate 1e-5, the smallest value of the reference's grid (why: the comment at `LR` in
    scripts/gen_golden_ssl4rec_steps.py — an Adam step turns a relative gradient error rho into lr x rho, and at 1e-3
    the worst element of a tensor, a cancelled sum, lies above the tolerance's absolute floor in a summation-order
    dependent way).  Measured on an MI355X: loss terms within 5.1e-7 relative, every parameter within 1.92 x
    max(slack, 1e-7) (config 1 initial_user; all others <= 0.65 x), movement 6e-5 = 150 x the tolerance floor."""
    from recommendation_amd.ssl4rec import SSL4RecModel
    g, configs = fx.load()
    cf = configs[c]
    model = SSL4RecModel(cf.conf(), _train_list(g), [], device="cuda")
    # first-seen dense ids (ssl4rec.py:69-75): the fixture's batches index these rows
    sp.assert_dense_id_order(model, g)
    assert list(model.model.state_dict()) == cf.names
    model.model.load_state_dict({k: torch.from_numpy(cf.init(k)) for k in cf.names})
    got = []
    model.model.train()
    for n in range(int(g["steps"])):
        out = model.train_step(*sp.batch(g, n, ("users", "items")), keep_bits=torch.from_numpy(cf.keep_bits[n]).cuda())
        assert not any(v.requires_grad for v in out)
        got.append(torch.stack([v.reshape(()) for v in out]))
    final = {k: cf.at(k, v.detach().cpu().numpy()) for k, v in model.model.state_dict().items()}
    sp.check(cf.record(), torch.stack(got).cpu().numpy(), final)


def test_seeded_steps_draw_new_masks_and_need_no_recorded_bits():
    """Without keep_bits the step draws its own masks: two models with one seed see the same draws, the contrastive term
    changes from step to step on one batch, and another seed gives another draw."""
    from recommendation_amd.ssl4rec import SSL4RecModel
    g, configs = fx.load()
    cf = configs[0]
    u, i = (torch.from_numpy(g[f"batch0_{s}"]).cuda() for s in ("users", "items"))

    def first_losses(seed):
        m = SSL4RecModel(cf.conf(), _train_list(g), [], device="cuda", seed=seed)
        m.model.load_state_dict({k: torch.from_numpy(cf.init(k)) for k in cf.names})
        with torch.no_grad():
            return [float(m.losses(u, i)[1]) for _ in range(3)]

    a, b, other = first_losses(3), first_losses(3), first_losses(4)
    assert a == pytest.approx(b, rel=1e-6)
    assert min(abs(x - y) for x, y in ((a[0], a[1]), (a[1], a[2]), (a[0], a[2]), (a[0], other[0]))) > 1e-4 * abs(a[0])


def _numpy_ranking_evaluation(query, items, train, test, top_n):
    """ssl4rec.py:143-153 and 104-123, restated: per test user the n best unseen items; Hit Ratio = hits over all test
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


def test_embeddings_and_evaluate(monkeypatch):
    """embeddings() == both towers over all rows (also when the pass is cut into row blocks); evaluate() == the numpy
    restatement on tie-free embeddings (small integers plus the item's own multiple of 1/1024, exact in fp32); predict()
    is the user's score row."""
    from recommendation_amd import ssl4rec
    rng = np.random.default_rng(4)
    n_u, n_i = 40, 130
    train = {(int(rng.integers(0, n_u)), int(rng.integers(0, n_i))) for _ in range(400)}
    train |= {(u, u) for u in range(n_u)} | {(i % n_u, i) for i in range(n_i)}
    test = {(int(rng.integers(0, n_u)), int(rng.integers(0, n_i))) for _ in range(240)} - train
    train, test = sorted(train), sorted(test)
    conf = {"embedding.size": 32, "batch.size": 64, "learning.rate": 1e-3, "reg.lambda": 1e-4, "max.epoch": 1,
            "item.ranking.topN": [10, 20], "n.layers": 2, "SSL4Rec": {"alpha": 0.1, "tau": 0.2, "drop": 0.1}}
    model = ssl4rec.SSL4RecModel(conf, [(f"u{u}", f"i{i}", 1.0) for u, i in train], [(f"u{u}", f"i{i}", 1.0) for u, i in test],
                                 device="cuda")
    assert model.n_layers == 2 and model.reg_weight == 1e-4 and model.topN == [10, 20] and model.max_N == 20
    enc, data = model.model, model.data
    q, it = model.embeddings()
    assert q.shape == (n_u, 128) and it.shape == (n_i, 128) and not q.requires_grad
    with torch.no_grad():
        q_ref, it_ref = enc(torch.arange(n_u, device="cuda"), torch.arange(n_i, device="cuda"))
    assert torch.equal(q, q_ref) and torch.equal(it, it_ref)
    monkeypatch.setattr(ssl4rec, "_TOWER_ROWS", 48)
    q_cut, it_cut = model.embeddings()
    torch.testing.assert_close(q_cut, q_ref, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(it_cut, it_ref, rtol=1e-6, atol=1e-6)

    d = 128
    qe = rng.integers(-3, 4, (n_u, d)).astype(np.float32)
    ie = rng.integers(-3, 4, (n_i, d)).astype(np.float32)
    qe[:, -1] = 1.0
    ie[:, -1] = rng.permutation(n_i) / 1024.0
    model.query_emb, model.item_emb = torch.from_numpy(qe).cuda(), torch.from_numpy(ie).cuda()
    got = model.evaluate()
    # dense ids are first-seen: map the raw pairs through the model's own maps
    tr = [(data.user[f"u{u}"], data.item[f"i{i}"]) for u, i in train]
    te = [(data.user[f"u{u}"], data.item[f"i{i}"]) for u, i in test]
    ref = _numpy_ranking_evaluation(qe, ie, tr, te, 20)                  # the last cut-off's metrics, as the reference returns
    assert set(got) == {"Hit Ratio", "Precision", "Recall", "NDCG"}
    for k in ref:
        assert got[k] == pytest.approx(ref[k], abs=1.1e-5), (k, got, ref)
    assert got["Recall"] > 0
    uid = data.user["u7"]
    assert np.array_equal(model.predict("u7"), (model.query_emb[uid] @ model.item_emb.T).cpu().numpy())


def test_ssl4rec_trains_end_to_end():
    """SSL4RecModel(conf, train, test).train() on the block-structured toy set of the GCL convergence test, same bar:
    Recall@10 far above a random ranking's (~0.1)."""
    from recommendation_amd.ssl4rec import SSL4RecModel
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
    conf = {"embedding.size": 64, "batch.size": 256, "learning.rate": 0.01, "reg.lambda": 1e-4, "max.epoch": 10,
            "item.ranking.topN": [10], "SSL4Rec": {"alpha": 0.1, "tau": 0.2, "drop": 0.1}}
    model = SSL4RecModel(conf, [(int(u), int(i), 1.0) for u, i in train], [(int(u), int(i), 1.0) for u, i in test],
                         device="cuda", seed=1)
    metrics = model.train()
    print("SSL4Rec end-to-end metrics:", metrics, "best epoch", model.best_epoch)
    assert set(metrics) == {"Hit Ratio", "Precision", "Recall", "NDCG"}
    assert metrics["Recall"] > 0.4, metrics
    assert model.best_query_emb.shape == (n_u, 128) and model.best_item_emb.shape == (n_i, 128)
    assert model.steps >= 24                      # 6000 pairs / 256 per batch, at least one epoch
