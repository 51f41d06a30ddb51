"""GPU parity of the HIP SpMM / LightGCN propagation (through the C ABI) against the CPU oracle
and the reference-generated golden fixtures.  Tolerance: 1e-5 relative fp32 (north_star),
measured against the row scale max|y| (sums of products; the fp64 oracle is the truth)."""
import numpy as np
import pytest
import torch

from f64_pins import pins
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

RT = 1e-5


def close(got, ref, rt=RT):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else got
    scale = max(np.abs(ref).max(), 1e-30)
    np.testing.assert_allclose(got, ref, rtol=rt, atol=rt * scale)


def rand_csr(rng, n_rows, n_cols, degs):
    rowptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    nnz = int(rowptr[-1])
    col = rng.integers(0, n_cols, nnz).astype(np.int32)
    val = rng.standard_normal(nnz).astype(np.float32)
    return rowptr, col, val


@pytest.fixture(scope="module")
def ra():
    import recommendation_amd as ra
    return ra


@pytest.mark.parametrize("d", [64, 32, 128, 100, 256, 1])
def test_spmm_matches_oracle_skewed_degrees(ra, d):
    rng = np.random.default_rng(d)
    n_rows, n_cols = 700, 500
    degs = rng.poisson(9, n_rows)
    degs[[3, 77, 200]] = [5000, 257, 256]     # long rows (split into chunks) and the boundary
    degs[[0, 1, 2, 10, 11, 699]] = 0          # empty rows incl. first / last
    rowptr, col, val = rand_csr(rng, n_rows, n_cols, degs)
    x = rng.standard_normal((n_cols, d)).astype(np.float32)
    g = ra.CsrGraph(rowptr, col, val, n_rows, n_cols, "cuda")
    y = ra.functional.spmm(g, torch.from_numpy(x).cuda())
    close(y, O.spmm_csr(rowptr, col, val, x))
    # all-ones values (raw adjacency) path
    g1 = ra.CsrGraph(rowptr, col, None, n_rows, n_cols, "cuda")
    close(ra.functional.spmm(g1, torch.from_numpy(x).cuda()), O.spmm_csr(rowptr, col, np.ones_like(val), x))


def test_spmm_many_empty_rows_and_tiny(ra):
    rng = np.random.default_rng(0)
    degs = np.zeros(1000, dtype=np.int64)
    degs[500] = 3
    rowptr, col, val = rand_csr(rng, 1000, 17, degs)
    x = rng.standard_normal((17, 64)).astype(np.float32)
    g = ra.CsrGraph(rowptr, col, val, 1000, 17, "cuda")
    close(ra.functional.spmm(g, torch.from_numpy(x).cuda()), O.spmm_csr(rowptr, col, val, x))
    g0 = ra.CsrGraph(np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 4, "cuda")
    y = ra.functional.spmm(g0, torch.ones(4, 64, device="cuda"))
    assert y.shape == (5, 64) and float(y.abs().max()) == 0.0


def test_spmm_edge_mask_scale_and_transpose_backward(ra):
    rng = np.random.default_rng(1)
    n_rows, n_cols, d = 300, 200, 64
    degs = rng.poisson(20, n_rows)
    degs[5] = 1500
    rowptr, col, val = rand_csr(rng, n_rows, n_cols, degs)
    nnz = col.size
    keep = O.edge_keep_mask(nnz, 0.3, seed=9)
    bits = np.packbits(keep, bitorder="little")
    bits = np.concatenate([bits, np.zeros((-bits.size) % 4, np.uint8)]).view(np.int32)
    x = rng.standard_normal((n_cols, d)).astype(np.float32)
    g = ra.CsrGraph(rowptr, col, val, n_rows, n_cols, "cuda")
    xt = torch.from_numpy(x).cuda()
    y = torch.empty(n_rows, d, device="cuda")
    ra.functional.spmm_into(g, xt, y=y, keep_bits=torch.from_numpy(bits).cuda(), val_scale=1.0 / 0.7)
    close(y, O.spmm_csr(rowptr, col, val, x, keep=keep, scale=1 / 0.7))
    # backward through the (asymmetric, rectangular) operator uses the transposed CSR
    xt.requires_grad_(True)
    w = rng.standard_normal((n_rows, d)).astype(np.float32)
    (ra.functional.spmm(g, xt) * torch.from_numpy(w).cuda()).sum().backward()
    close(xt.grad, O.spmm_backward(rowptr, col, val, w, n_cols))


def test_row_l2norm_epilogue(ra):
    rng = np.random.default_rng(2)
    degs = rng.poisson(6, 400)
    degs[7] = 900
    degs[9] = 0
    rowptr, col, val = rand_csr(rng, 400, 400, degs)
    x = rng.standard_normal((400, 64)).astype(np.float32)
    g = ra.CsrGraph(rowptr, col, val, 400, 400, "cuda")
    y = ra.functional.spmm_l2norm(g, torch.from_numpy(x).cuda())
    close(y, O.row_l2_normalize(O.spmm_csr(rowptr, col, val, x)))


def _golden_raw_graph(ra, golden):
    g = golden("graph_build.npz")
    nu, ni = len(g["sorted_user_ids"]), len(g["sorted_item_ids"])
    umap = {u: k for k, u in enumerate(g["sorted_user_ids"].tolist())}
    imap = {i: k for k, i in enumerate(g["sorted_item_ids"].tolist())}
    uid = np.array([umap[u] for u in g["train_user"].tolist()])
    iid = np.array([imap[i] for i in g["train_item"].tolist()])
    graph = ra.CsrGraph.bipartite_raw(uid, iid, nu, ni, "cuda")
    # integer neighbour indexing is bit-exact with the reference's COO (stable by-row order)
    rp, c, _, _ = O.coo_to_csr_stable(g["coo_row"], g["coo_col"], g["coo_data"], nu + ni)
    assert np.array_equal(graph.rowptr.cpu().numpy(), rp) and np.array_equal(graph.col.cpu().numpy(), c)
    return graph, nu, ni


@pytest.mark.parametrize("k", [1, 2, 3])
def test_golden_lgcn_encoder_raw_adjacency(ra, golden, k):
    """directau.LGCNEncoder.forward (= ncl.py:415-422) outputs and autograd gradients."""
    p = golden("propagation.npz")
    graph, nu, ni = _golden_raw_graph(ra, golden)
    x0 = torch.from_numpy(p["x0"]).cuda().requires_grad_(True)
    final, layers = ra.functional.lightgcn_propagate(graph, x0, k, combine="mean", return_layers=True)
    close(final, p[f"raw_mean_K{k}"].astype(np.float64), rt=2e-5)
    close(layers[-1], p[f"raw_last_K{k}"].astype(np.float64), rt=2e-5)
    (final * torch.from_numpy(p["w"]).cuda()).sum().backward()
    close(x0.grad, p[f"raw_grad_K{k}"].astype(np.float64), rt=2e-5)
    f64 = pins("propagation")           # the reference's own float64 run (tests/f64_pins.py)
    f64.check(f"raw_mean_K{k}", final)
    f64.check(f"raw_last_K{k}", layers[-1])
    f64.check(f"raw_grad_K{k}", x0.grad)


@pytest.mark.parametrize("k", [2, 3])
def test_golden_lgcn_encoder_normalised(ra, golden, k):
    """selfcf.LGCN_Encoder.forward on D^-1/2 A D^-1/2 (selfcf.py:475-485) + its gradient."""
    g, p = golden("graph_build.npz"), golden("propagation.npz")
    umap = {u: k_ for k_, u in enumerate(g["seen_user_ids"].tolist())}
    imap = {i: k_ for k_, i in enumerate(g["seen_item_ids"].tolist())}
    uid = np.array([umap[u] for u in g["train_user"].tolist()])
    iid = np.array([imap[i] for i in g["train_item"].tolist()])
    graph = ra.CsrGraph.bipartite_sym_norm(uid, iid, len(umap), len(imap), "cuda")
    assert np.array_equal(graph.rowptr.cpu().numpy(), g["norm_indptr"])
    assert np.array_equal(graph.col.cpu().numpy().astype(np.int64), g["norm_indices"])
    np.testing.assert_allclose(graph.val.cpu().numpy(), g["norm_data"], rtol=3e-7)
    xs = torch.from_numpy(p["xs"]).cuda().requires_grad_(True)
    final = ra.functional.lightgcn_propagate(graph, xs, k, combine="mean")
    close(final, p[f"norm_mean_K{k}"].astype(np.float64), rt=2e-5)
    (final * torch.from_numpy(p["w"][: xs.shape[0]]).cuda()).sum().backward()
    close(xs.grad, p[f"norm_grad_K{k}"].astype(np.float64), rt=2e-5)
    pins("propagation").check(f"norm_mean_K{k}", final)
    pins("propagation").check(f"norm_grad_K{k}", xs.grad)


def test_golden_sept_encoder(ra, golden):
    """sept.SEPT.encoder (sept.py:220-226): per-layer row normalise, mean over layers, + gradient."""
    g, p = golden("graph_build.npz"), golden("propagation.npz")
    n = len(g["sorted_user_ids"]) + len(g["sorted_item_ids"])
    graph = ra.CsrGraph.from_coo(g["coo_row"], g["coo_col"], g["coo_data"], n, n, "cuda", coalesce=True, symmetric=True)
    x0 = torch.from_numpy(p["x0"]).cuda().requires_grad_(True)
    embs, e = [x0], x0
    for _ in range(2):
        e = ra.functional.spmm_l2norm(graph, e)
        embs.append(e)
    final = torch.stack(embs, 0).mean(0)
    close(final, p["sept_mean_K2"].astype(np.float64), rt=2e-5)
    (final * torch.from_numpy(p["w"]).cuda()).sum().backward()
    close(x0.grad, p["sept_grad_K2"].astype(np.float64), rt=5e-5)
    pins("propagation").check("sept_mean_K2", final)
    pins("propagation").check("sept_grad_K2", x0.grad)


def test_cfg1_lightgcn_forward_sum_of_layers(ra):
    """BASELINE cfg1 (ML-100K-sized, K=2, d=64): lightgcn.py:21-27 semantics (gcn_norm weights,
    sum over layers) against the oracle restatement; LGConv itself is 'parity unpinned'."""
    u, i = O.synthetic_interactions(943, 1682, 80000, seed=20250919)
    ei = O.build_edge_index(u, i, 943)
    rng = np.random.default_rng(0)
    uw = (rng.standard_normal((943, 64)) * 0.1).astype(np.float32)
    iw = (rng.standard_normal((1682, 64)) * 0.1).astype(np.float32)
    graph = ra.CsrGraph.from_edge_index_gcn_norm(ei, 943 + 1682, "cuda", symmetric=True)
    x0 = torch.from_numpy(np.concatenate([uw, iw])).cuda()
    final = ra.functional.lightgcn_propagate(graph, x0, 2, combine="sum")
    ru, ri = O.lightgcn_forward(ei, uw, iw, 2)
    close(final, np.concatenate([ru, ri]))


def test_linearity_and_determinism_at_scale(ra):
    """Size-independent properties at a size the numpy oracle would take minutes for:
    A(ax + by) = a Ax + b Ay, run-to-run bitwise determinism (no atomics), and the row-sum
    identity A 1 = rowsum(val)."""
    n_u, n_i, e = 200_000, 20_000, 2_000_000
    uu, ii = O.synthetic_interactions(n_u, n_i, e, seed=5)
    graph = ra.CsrGraph.bipartite_sym_norm(uu, ii, n_u, n_i, "cuda")
    n = n_u + n_i
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(n, 64, device="cuda", generator=gen)
    z = torch.randn(n, 64, device="cuda", generator=gen)
    f = ra.functional.spmm
    lhs = f(graph, 2.0 * x - 0.5 * z)
    rhs = 2.0 * f(graph, x) - 0.5 * f(graph, z)
    assert float((lhs - rhs).abs().max()) <= 2e-5 * float(rhs.abs().max())
    assert torch.equal(f(graph, x), f(graph, x))
    ones = f(graph, torch.ones(n, 64, device="cuda"))
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), graph.rowptr[1:] - graph.rowptr[:-1])
    rowsum = torch.zeros(n, device="cuda", dtype=torch.float64).index_add_(0, rows, graph.val.double())
    assert float((ones[:, 0].double() - rowsum).abs().max()) <= 1e-5 * float(rowsum.abs().max())
    assert float((ones - ones[:, :1]).abs().max()) == 0.0


def test_hipgraph_capture_and_replay(ra):
    """The C ABI allocates nothing and never synchronises, so a whole cfg1 forward step (2-layer
    propagation + full-batch BPR, lightgcn.py:85-108) can be captured into a hipGraph and replayed."""
    u, i = O.synthetic_interactions(943, 1682, 80000, seed=20250919)
    g = ra.CsrGraph.bipartite_sym_norm(u, i, 943, 1682, "cuda")
    x = torch.randn(943 + 1682, 64, device="cuda")
    ut, it = torch.from_numpy(u).cuda(), torch.from_numpy(i).cuda()
    jt = torch.randint(0, 1682, (80000,), device="cuda")

    def step():
        f = ra.functional.lightgcn_propagate(g, x, 2, combine="sum")
        return ra.functional.bpr_sums(f[:943].contiguous(), f[943:].contiguous(), ut, it, jt, 2)

    with torch.no_grad():
        ref = step().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        x.mul_(2.0)                       # new input values, same buffers
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, step())   # replay == eager on the updated input
        assert not torch.equal(out, ref)
