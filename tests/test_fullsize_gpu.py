"""Parity at BASELINE.json's full single-GPU sizes (cfg2 / cfg3: 1M users x 100K items, 10M
interactions, nnz = 20M, d = 64, B = 2048) against the C restatement of the reference arithmetic
(oracle/oracle.c, fp32 like the CPU PyTorch path), plus size-independent properties.  The graphs come
from the bench's device generator (same recipe as oracle_np.synthetic_interactions)."""
import numpy as np
import pytest
import torch

from oracle import oracle_c as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cfg2():
    import bench
    import recommendation_amd as ra
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["cfg2"]
    users, items = bench.synth_interactions_device(wl["users"], wl["items"], wl["edges"], bench.SEED, dev)
    graph = ra.CsrGraph.bipartite_sym_norm(users, items, wl["users"], wl["items"], dev)
    n = wl["users"] + wl["items"]
    x0 = torch.empty(n, 64, device=dev)
    torch.nn.init.xavier_uniform_(x0, generator=torch.Generator(device=dev).manual_seed(0))
    return dict(graph=graph, x0=x0, n_u=wl["users"], n_i=wl["items"], users=users, items=items)


def test_cfg2_three_layer_propagation_matches_c_oracle(cfg2):
    """BASELINE configs[1]: LightGCN 3-layer d=64 over the 20M-nnz operator, every output element."""
    from recommendation_amd import functional as Fn
    g, x0 = cfg2["graph"], cfg2["x0"]
    assert g.nnz == 20_000_000
    # integer structure: sorted by (row, col), symmetric, every pair once
    rows = torch.repeat_interleave(torch.arange(g.n_rows, device=x0.device), g.rowptr[1:] - g.rowptr[:-1])
    key = rows * g.n_rows + g.col
    assert bool((key[1:] > key[:-1]).all())
    assert torch.equal(torch.sort(g.col.to(torch.int64) * g.n_rows + rows).values, key)
    with torch.no_grad():
        final, layers = Fn.lightgcn_propagate(g, x0, 3, combine="mean", return_layers=True)
    ref = C.lightgcn_propagate(g.rowptr_host, g.col.cpu().numpy(), g.val.cpu().numpy(), x0.cpu().numpy(), 3, "mean")
    got = final.cpu().numpy()
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-5 * scale
    # 8192 sampled rows + the 64 longest (hub item) rows at PER-ROW tolerance: a small row cannot hide behind the global
    # maximum.  Both sides sum a row's terms in fp32 in different orders (the C oracle front to back, the kernel in chunks of
    # 512 non-zeros), so the bar is 1e-5 of the row's own largest element
    deg = np.diff(g.rowptr_host)
    rs = np.concatenate([np.random.default_rng(4).integers(0, g.n_rows, 8192), np.argsort(deg)[-64:]])
    denom = np.abs(ref[rs]).max(1, keepdims=True) + 1e-30
    worst = (np.abs(got[rs] - ref[rs]) / denom).max()
    assert worst <= 1e-5, worst
    # row-sum identity on the last layer input: A 1 = rowsum(val)
    ones = Fn.spmm(g, torch.ones_like(x0))
    rowsum = torch.zeros(g.n_rows, device=x0.device, dtype=torch.float64).index_add_(0, rows, g.val.double())
    assert float((ones[:, 0].double() - rowsum).abs().max()) <= 1e-5 * float(rowsum.max())


def test_cfg3_structure_contrast_matches_c_oracle(cfg2):
    """BASELINE configs[2] shape (ncl.py:358-367): 2048 anchors against ALL 1M user rows + 100K item rows."""
    from recommendation_amd import functional as Fn
    x0, n_u = cfg2["x0"], cfg2["n_u"]
    gen = torch.Generator(device="cuda").manual_seed(3)
    ctx = x0 + 0.05 * torch.randn(x0.shape, device="cuda", generator=gen)
    uidx = torch.randint(0, n_u, (2048,), device="cuda", generator=gen)
    with torch.no_grad():
        lse, pos = Fn.infonce_stats(ctx[:n_u][uidx], x0[:n_u], uidx, 0.1, True)
    # the C oracle over 2048 x 1M pairs takes ~10 s of host time: check a 256-anchor sample
    sel = torch.arange(0, 2048, 8, device="cuda")
    ref_lse, ref_pos = C.row_lse(ctx[:n_u][uidx][sel].cpu().numpy(), x0[:n_u].cpu().numpy(), uidx[sel].cpu().numpy(), 10.0, True)
    np.testing.assert_allclose(lse[sel].cpu().numpy(), ref_lse, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(pos[sel].cpu().numpy(), ref_pos, rtol=1e-5, atol=2e-5)
    assert bool((lse >= pos).all())            # the positive is one of the summed terms


def test_cfg2_full_batch_bpr_and_sampler(cfg2):
    """lightgcn.py:86-108 full batch (B = E = 10M): BPR value vs the C oracle; negatives never hit a
    training positive across all 10M slots."""
    from recommendation_amd import functional as Fn
    g, x0, n_u, n_i = cfg2["graph"], cfg2["x0"], cfg2["n_u"], cfg2["n_i"]
    users, items = cfg2["users"], cfg2["items"]
    rowptr_u = g.rowptr[: n_u + 1].contiguous()
    items_u = (g.col[: int(rowptr_u[-1])] - n_u).contiguous()
    neg = Fn.neg_sample(rowptr_u, items_u, users, 1, n_i, 2025, 0, 101)
    assert int(neg.min()) >= 0 and int(neg.max()) < n_i
    pos_keys = torch.sort(users * n_i + items).values
    hit = torch.searchsorted(pos_keys, users * n_i + neg)
    hit = pos_keys[hit.clamp(max=pos_keys.numel() - 1)] == users * n_i + neg
    assert not bool(hit.any())
    ut, it = x0[:n_u].contiguous(), x0[n_u:].contiguous()
    with torch.no_grad():
        sums = Fn.bpr_sums(ut, it, users, items, neg, Fn.BPR_LOG_SIGMOID)
    ref = C.bpr_loss(ut.cpu().numpy(), it.cpu().numpy(), users.cpu().numpy(), items.cpu().numpy(), neg.cpu().numpy(), 2)
    assert float(sums[0]) / users.numel() == pytest.approx(ref, rel=1e-5)
    assert float(sums[4]) == 0.0


def test_cfg2_full_batch_bce_value_and_gradients(cfg2):
    """lightgcn.py:109-113 on the full batch of the benchmark graph (E = 10M samples x I = 100K items = 10^12 logits in
    the reference; 10^11 pairs here, by distinct user): the loss against a float64 evaluation of ALL U x I scores on the
    GPU (slabs of 4096 users), the gradient rows of 512 sampled users and 256 sampled items against float64."""
    from recommendation_amd import functional as Fn
    g, x0, n_u, n_i = cfg2["graph"], cfg2["x0"], cfg2["n_u"], cfg2["n_i"]
    users, items = cfg2["users"], cfg2["items"]
    e = users.numel()
    with torch.no_grad():                                     # scores of a trained-model magnitude (|s| up to a few units)
        table = Fn.lightgcn_propagate(g, x0 * 40.0, 3, combine="sum")
    table = table.clone().requires_grad_(True)
    loss = Fn.bce_edge_loss(g, table, n_u)
    loss.backward()
    grad = table.grad
    a64, b64 = table.detach()[:n_u].double(), table.detach()[n_u:].double()
    deg = g.row_degrees()[:n_u].double()
    soft = torch.zeros((), dtype=torch.float64, device=table.device)
    for u0 in range(0, n_u, 4096):
        sc = a64[u0:u0 + 4096] @ b64.T
        soft += (torch.nn.functional.softplus(sc).sum(1) * deg[u0:u0 + 4096]).sum()
    pos = torch.zeros((), dtype=torch.float64, device=table.device)
    for k0 in range(0, e, 1 << 21):
        pos += (a64[users[k0:k0 + (1 << 21)]] * b64[items[k0:k0 + (1 << 21)]]).sum()
    ref = float((soft - pos) / (float(e) * n_i))
    assert float(loss.detach()) == pytest.approx(ref, rel=1e-5)
    gen = torch.Generator(device=table.device).manual_seed(5)
    norm = float(e) * n_i
    # users: deg_u sum_i sigmoid(s_ui) b_i - sum_{i in N(u)} b_i
    su = torch.randint(0, n_u, (512,), device=table.device, generator=gen)
    want_u = (torch.sigmoid(a64[su] @ b64.T) @ b64) * deg[su].unsqueeze(1)
    adj_u = torch.zeros(n_u, 64, dtype=torch.float64, device=table.device).index_add_(0, users, b64[items])
    want_u = (want_u - adj_u[su]) / norm
    del adj_u
    got_u = grad[su].double()
    assert float((got_u - want_u).abs().max()) <= 1e-5 * float(want_u.abs().max())
    # items: sum_u deg_u sigmoid(s_ui) a_u - sum_{u in N(i)} a_u
    si = torch.randint(0, n_i, (256,), device=table.device, generator=gen)
    want_i = torch.zeros(256, 64, dtype=torch.float64, device=table.device)
    for u0 in range(0, n_u, 1 << 16):
        sg = torch.sigmoid(a64[u0:u0 + (1 << 16)] @ b64[si].T) * deg[u0:u0 + (1 << 16)].unsqueeze(1)
        want_i += sg.T @ a64[u0:u0 + (1 << 16)]
    adj_i = torch.zeros(n_i, 64, dtype=torch.float64, device=table.device).index_add_(0, items, a64[users])
    want_i = (want_i - adj_i[si]) / norm
    got_i = grad[n_u:][si].double()
    assert float((got_i - want_i).abs().max()) <= 1e-5 * float(want_i.abs().max())


def test_cfg2_horner_sum_is_the_path_the_bench_times(cfg2):
    """bench.py's timed call: `lightgcn_propagate(graph, x0, 3, combine="sum")` without layer outputs — the
    Horner branch (y = NULL, acc_in = x0) — every element against the C oracle's sum of layers
    (lightgcn.py:21-27)."""
    from recommendation_amd import functional as Fn
    g, x0 = cfg2["graph"], cfg2["x0"]
    with torch.no_grad():
        got = Fn.lightgcn_propagate(g, x0, 3, combine="sum")
    ref = C.lightgcn_propagate(g.rowptr_host, g.col.cpu().numpy(), g.val.cpu().numpy(), x0.cpu().numpy(), 3, "sum")
    assert np.abs(got.cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    # the other branch computes the same thing
    with torch.no_grad():
        other, _ = Fn.lightgcn_propagate(g, x0, 3, combine="sum", return_layers=True)
    assert float((other - got).abs().max()) <= 2e-6 * float(got.abs().max())


def test_cfg2_operator_itself_against_float64_degrees(cfg2):
    """The operator the tests above hand to the C oracle, checked on its own from `users` / `items` with torch ops only
    (nothing the ingest returned enters the reference): the user rows' (row, col) pairs are exactly the distinct
    (u, i + U) pairs in key order, the item rows their mirror; every one of the 20 M values is within rtol 3e-7 of
    m / sqrt(deg_r deg_c), m the pair's multiplicity and deg the float64 `index_add_` of the multiplicities -- the hub item
    rows (`row_dinv_kernel`'s strided loop over ~50 K entries) included, the 64 longest rows reported separately.  Worst
    measured on MI355X: 0.63 of the bar over all values, 0.59 on the 64 longest rows (16 479 to 49 231 entries)."""
    g, users, items, n_u, n_i = cfg2["graph"], cfg2["users"], cfg2["items"], cfg2["n_u"], cfg2["n_i"]
    n, dev = n_u + n_i, users.device
    uk, m = torch.unique(users.to(torch.int64) * n + (items.to(torch.int64) + n_u), return_counts=True)      # sorted keys
    e = uk.numel()
    ru, cu = uk // n, uk % n
    assert g.nnz == 2 * e and int(g.rowptr[n_u]) == e
    rows = torch.repeat_interleave(torch.arange(n, device=dev), g.rowptr[1:] - g.rowptr[:-1])
    got_key = rows * n + g.col.to(torch.int64)
    assert torch.equal(got_key[:e], uk)
    mirror, order = torch.sort(cu * n + ru)                                   # distinct keys: any sort gives this order
    assert torch.equal(got_key[e:], mirror)
    del got_key, mirror, rows
    m64 = m.double()
    deg = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, ru, m64).index_add_(0, cu, m64)
    assert float(deg.max()) < 2 ** 24                                         # the device's fp32 row sums are exact
    ref_u = m64 / torch.sqrt(deg[ru] * deg[cu])
    ref = torch.cat([ref_u, ref_u[order]])
    rel = (g.val.double() - ref).abs() / ref
    worst = float(rel.max())
    top = torch.topk(g.rowptr[1:] - g.rowptr[:-1], 64)
    lo, hi = g.rowptr[top.indices].tolist(), g.rowptr[top.indices + 1].tolist()
    hub_worst = float(torch.stack([rel[a:b].max() for a, b in zip(lo, hi)]).max())
    print(f"cfg2 operator values: worst {worst / 3e-7:.3f} x rtol 3e-7 over {2 * e} values; 64 longest rows "
          f"({int(top.values.min())}-{int(top.values.max())} entries): worst {hub_worst / 3e-7:.3f} x")
    assert worst <= 3e-7, f"worst {worst:.3e} over all values, {hub_worst:.3e} on the 64 longest rows (bar 3e-7)"


@pytest.fixture(scope="module")
def cfg4():
    import bench
    import recommendation_amd as ra
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["cfg4"]
    users, items = bench.synth_interactions_device(wl["users"], wl["items"], wl["edges"], bench.SEED, dev)
    graph = ra.CsrGraph.bipartite_sym_norm(users, items, wl["users"], wl["items"], dev)     # library ingest
    del users, items
    n = wl["users"] + wl["items"]
    x0 = torch.empty(n, 64, device=dev)
    torch.nn.init.xavier_uniform_(x0, generator=torch.Generator(device=dev).manual_seed(0))
    yield dict(graph=graph, x0=x0, n_u=wl["users"], n_i=wl["items"])
    del graph, x0
    torch.cuda.empty_cache()


def test_cfg4_graph_three_layer_propagation(cfg4):
    """BASELINE configs[3]'s graph (10M users x 1M items / 100M interactions, nnz = 200M) on one GPU, the
    bench's timed call: every output element against the C oracle (lightgcn.py:21-27 / ncl.py:415-422
    arithmetic in fp32), plus the size-independent properties: linearity and the row-sum identity."""
    from recommendation_amd import functional as Fn
    g, x0 = cfg4["graph"], cfg4["x0"]
    assert g.nnz == 200_000_000 and g.n_rows == 11_000_000
    with torch.no_grad():
        got = Fn.lightgcn_propagate(g, x0, 3, combine="sum")
    col_h, val_h, x_h = g.col.cpu().numpy(), g.val.cpu().numpy(), x0.cpu().numpy()
    ref = C.lightgcn_propagate(g.rowptr_host, col_h, val_h, x_h, 3, "sum")
    got_h = got.cpu().numpy()
    assert np.abs(got_h - ref).max() <= 1e-5 * np.abs(ref).max()
    del ref, got_h, col_h, val_h, x_h
    # ~4K sampled rows + the 64 longest rows at PER-ROW 1e-5 (small rows are not hidden behind the global maximum) against a
    # float64 referee, layer by layer: z_k[row] = x0[row] + sum_e val_e z_{k-1}[col_e] with the row's sum accumulated in
    # float64 from the kernel's own previous layer (two fp32 summation orders of a 500K-term hub row differ by more than each
    # differs from the exact sum, so the C oracle's fp32 order is no referee for those rows)
    rs = torch.from_numpy(np.random.default_rng(4).integers(0, g.n_rows, 4096)).cuda()
    deg = g.rowptr[1:] - g.rowptr[:-1]
    rs = torch.unique(torch.cat([rs, torch.topk(deg, 64).indices]))
    starts, lens = g.rowptr[rs], deg[rs]
    owner = torch.repeat_interleave(torch.arange(rs.numel(), device="cuda"), lens)
    pos = torch.arange(int(lens.sum()), device="cuda") - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens) + starts[owner]
    col_s, val_s = g.col[pos].to(torch.int64), g.val[pos].double()
    z_prev = x0
    for k in range(3):
        z_k = torch.empty_like(x0)
        Fn.spmm_into(g, z_prev, acc_in=x0, acc_out=z_k)                    # the Horner layer the timed call launches
        ref_rows = x0[rs].double()
        for lo in range(0, pos.numel(), 1 << 22):                         # slabs: [4M, 64] float64 products = 2 GB
            hi = min(pos.numel(), lo + (1 << 22))
            # segment sums by prefix sums (the entries of a row are consecutive; half a million float64 atomics onto one
            # hub row would serialise)
            cs = torch.cumsum(z_prev[col_s[lo:hi]].double() * val_s[lo:hi].unsqueeze(1), 0)
            uniq, cnt = torch.unique_consecutive(owner[lo:hi], return_counts=True)
            ends = torch.cumsum(cnt, 0) - 1
            seg = cs[ends]
            seg[1:] -= cs[ends[:-1]]
            ref_rows[uniq] += seg
            del cs
        denom = ref_rows.abs().max(1, keepdim=True).values + 1e-300
        assert float(((z_k[rs].double() - ref_rows).abs() / denom).max()) <= 1e-5, k
        z_prev = z_k
    assert float((z_prev - got).abs().max()) == 0.0                        # the same three launches as lightgcn_propagate
    del z_prev, z_k, ref_rows, col_s, val_s, pos, owner
    torch.cuda.empty_cache()
    # linearity: P(a x + b z) = a P(x) + b P(z)
    gen = torch.Generator(device="cuda").manual_seed(9)
    z = torch.randn(x0.shape, device="cuda", generator=gen) * x0.std()
    with torch.no_grad():
        pz = Fn.lightgcn_propagate(g, z, 3, combine="sum")
        mix = Fn.lightgcn_propagate(g, 0.5 * x0 - 2.0 * z, 3, combine="sum")
    lin = 0.5 * got - 2.0 * pz
    assert float((mix - lin).abs().max()) <= 2e-5 * float(lin.abs().max())
    del z, pz, mix, lin
    # row-sum identity: A 1 = rowsum(val), and the operator is symmetric: 1^T A x = rowsum^T x
    rows = torch.repeat_interleave(torch.arange(g.n_rows, device="cuda"), g.rowptr[1:] - g.rowptr[:-1])
    rowsum = torch.zeros(g.n_rows, device="cuda", dtype=torch.float64).index_add_(0, rows, g.val.double())
    del rows
    with torch.no_grad():
        ones = Fn.spmm(g, torch.ones_like(x0))
        ax = Fn.spmm(g, x0)
    assert float((ones[:, 0].double() - rowsum).abs().max()) <= 1e-5 * float(rowsum.max())
    lhs, rhs = ax.double().sum(0), (rowsum.unsqueeze(1) * x0.double()).sum(0)
    assert float((lhs - rhs).abs().max()) <= 1e-6 * float((rowsum.unsqueeze(1) * x0.double().abs()).sum(0).max())
