"""Device graph ingest and the streaming ops around the hot path against references that never see a device result.

Every reference here is numpy (or torch float64 where a test says so) computed from the COO INPUT: the structure from
O.coo_to_csr_stable / O.coalesce_csr, the degrees from O.coo_sums_f64, the values from O.sym_norm_values_f64 /
O.row_norm_values_f64 (each pinned to the reference's own outputs in tests/test_oracle_golden.py).  The shapes are the
smallest at which the named branch runs: sort-bit boundaries of the radix sort (`bits_for(max_key)`), rows longer than one
trip of `row_dinv_kernel`'s 16-lane loop, and the second grid-stride trip of every capped launch:
    scale_values_kernel     16384 x 256 threads        nnz    > 4 194 304
    row_dinv_kernel         262144 blocks x 16 rows    n_rows > 4 194 304
    gather / scatter_add    65536 blocks x 4 rows      n      >   262 144
    spgemm_expand           65536 blocks x 16 nnz      a_nnz  > 1 048 576
    csr_lookup              65536 x 256 threads        nnz    > 16 777 216
    adam / sgd float4 loop  65536 x 256 float4         n      > 67 108 864
Deliberately left out: the caps of `gcr_coo_to_csr`'s own kernels and of `gcr_dense_ids_u64` (262 144 blocks x 256
threads = 67 108 864 entries) -- a second trip there needs a 67 M-entry COO and a host sort of it as the reference, which
no test of a few seconds can afford.
"""
import numpy as np
import pytest
import torch

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

RTOL = 3e-7          # the bar tests/test_graph_gpu.py holds the 80-node golden to: two 1/sqrtf and two multiplications


@pytest.fixture(scope="module")
def G():
    from recommendation_amd import graph
    return graph


def _np(t):
    return t.cpu().numpy()


def _int_vals(rng, n):
    """Small integers as float32: sums of duplicates are exact in fp32 in any order, so coalesced values are bit-exact."""
    return rng.integers(1, 4, n).astype(np.float32)


def _check_stable(G, row, col, val, n_rows, n_cols):
    rp, c, v, perm = G.coo_to_csr_device(row, col, val, n_rows, n_cols, "cuda", want_perm=True)
    rrp, rc, rv, order = O.coo_to_csr_stable(row, col, val, n_rows)
    assert rp.dtype == torch.int64 and c.dtype == torch.int32 and v.dtype == torch.float32 and perm.dtype == torch.int64
    assert np.array_equal(_np(rp), rrp), "stable rowptr"
    assert np.array_equal(_np(c), rc), "stable col"
    assert np.array_equal(_np(v), rv), "stable val"
    assert np.array_equal(_np(perm), order), "stable perm"


def _check_coalesced(G, row, col, val, n_rows, n_cols):
    rp, c, v, _ = G.coo_to_csr_device(row, col, val, n_rows, n_cols, "cuda", coalesce=True)
    rrp, rc, rv = O.coalesce_csr(row, col, val, n_rows)
    assert np.array_equal(_np(rp), rrp), "coalesced rowptr"
    assert np.array_equal(_np(c), rc), "coalesced col"
    assert np.array_equal(_np(v), rv), "coalesced val (integer-valued: exact in any order)"


def _check_both(G, row, col, val, n_rows, n_cols):
    _check_stable(G, row, col, val, n_rows, n_cols)
    _check_coalesced(G, row, col, val, n_rows, n_cols)


# ------------------------------------------------------------------------------------------------------------------------
# 1. coo_to_csr structure, both modes
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [255, 256, 257])
@pytest.mark.parametrize("n_rows", [255, 256, 257])
def test_coo_to_csr_at_sort_bit_boundaries(G, n_rows, n_cols):
    """The radix sort runs over `bits_for(max_key)` bits: max_key = n_rows (stable) crosses 8 -> 9 bits at 256, max_key =
    n_rows * n_cols (coalesced) crosses 16 -> 17 bits at 256 x 256.  20 000 entries with duplicates, the largest row and
    column ids present, rowptr / col / val / perm bit-exact."""
    rng = np.random.default_rng(n_rows * 1000 + n_cols)
    nnz = 20_000
    row, col = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz)
    row[:3000], col[:3000] = row[3000:6000], col[3000:6000]
    row[-4:], col[-4:] = [n_rows - 1, n_rows - 1, 0, n_rows - 1], [n_cols - 1, 0, n_cols - 1, n_cols - 1]
    _check_both(G, row, col, _int_vals(rng, nnz), n_rows, n_cols)


@pytest.mark.parametrize("n_rows", [1, 2])
def test_coo_to_csr_one_and_two_rows(G, n_rows):
    """n_rows = 1 and 2: the stable key has 1 and 2 significant bits (every key 0 when n_rows = 1)."""
    rng = np.random.default_rng(n_rows)
    nnz, n_cols = 5000, 300
    row, col = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz)
    _check_both(G, row, col, _int_vals(rng, nnz), n_rows, n_cols)


def test_coo_to_csr_columns_at_the_top_of_int32(G):
    """5 rows x (2^31 - 1) columns: the coalesce key r * n_cols + c exceeds 2^32 (34 sort bits), `split_key_kernel`'s
    `ukey % mul` and the int32 `col_out` hold column ids up to 2^31 - 2."""
    rng = np.random.default_rng(5)
    n_rows, n_cols, nnz = 5, 2 ** 31 - 1, 3000
    edge = np.array([0, 1, 65_535, 65_536, 2 ** 24, 2 ** 30, 2 ** 31 - 2], dtype=np.int64)
    col = np.concatenate([np.tile(edge, 200), rng.integers(0, n_cols, nnz - 1400)])
    row = rng.integers(0, n_rows, nnz)
    row[:7], row[7:14] = 4, 0                                          # every edge column in the last and the first row
    _check_both(G, row, col, _int_vals(rng, nnz), n_rows, n_cols)
    assert int(O.coalesce_csr(row, col, np.ones(nnz, np.float32), n_rows)[1].max()) == 2 ** 31 - 2


def test_coo_to_csr_stable_70000_rows(G):
    """Stable mode with n_rows = 70 000 > 2^16: 17 sort bits, most rows empty or single."""
    rng = np.random.default_rng(70)
    n_rows, n_cols, nnz = 70_000, 900, 50_000
    row, col = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz)
    row[:2] = [n_rows - 1, 65_536]
    _check_stable(G, row, col, _int_vals(rng, nnz), n_rows, n_cols)


@pytest.mark.parametrize("placement", ["row0", "last_row", "ends_empty", "every_1000th", "single"])
def test_coo_to_csr_placement(G, placement):
    """Where `rowptr_fill_kernel`'s inner loop closes many rows at once: all entries in row 0 (one thread writes every
    later rowptr), all in the last row, first and last rows empty, entries only in every 1000th row, nnz = 1."""
    rng = np.random.default_rng(len(placement))
    n_rows, n_cols, nnz = 5001, 700, 4000
    col = rng.integers(0, n_cols, nnz)
    if placement == "row0":
        row = np.zeros(nnz, dtype=np.int64)
    elif placement == "last_row":
        row = np.full(nnz, n_rows - 1, dtype=np.int64)
    elif placement == "ends_empty":
        row = rng.integers(1, n_rows - 1, nnz)
    elif placement == "every_1000th":
        row = rng.integers(0, 6, nnz) * 1000
    else:
        row, col, nnz = np.array([2500]), np.array([n_cols - 1]), 1
    _check_both(G, row, col, _int_vals(rng, nnz), n_rows, n_cols)


def test_coalesce_one_pair_repeated_10000_times(G):
    """One (row, col) pair repeated K = 10 000 times with random float values among 20 000 distinct ordinary entries:
    the reduce-by-key sum lies within (K - 1) 2^-24 sum|v_i| of the float64 sum (the bound for an fp32 sum in ANY order),
    every non-repeated entry is bit-exact.  Measured on MI355X: 6.8e-7 off, 1.4e-7 of the bound (4.76)."""
    rng = np.random.default_rng(10)
    n_rows, n_cols, K, n_other = 600, 500, 10_000, 20_000
    key = rng.choice(n_rows * n_cols, n_other + 1, replace=False)
    hot, key = int(key[0]), key[1:]
    row = np.concatenate([key // n_cols, np.full(K, hot // n_cols)])
    col = np.concatenate([key % n_cols, np.full(K, hot % n_cols)])
    val = rng.standard_normal(n_other + K).astype(np.float32)
    mix = rng.permutation(n_other + K)
    row, col, val = row[mix], col[mix], val[mix]
    rp, c, v, _ = G.coo_to_csr_device(row, col, val, n_rows, n_cols, "cuda", coalesce=True)
    rrp, rc, rv = O.coalesce_csr(row, col, val, n_rows)
    assert np.array_equal(_np(rp), rrp) and np.array_equal(_np(c), rc)
    rows = np.repeat(np.arange(n_rows), np.diff(rrp))
    at = int(np.flatnonzero((rows == hot // n_cols) & (rc == hot % n_cols))[0])
    got = _np(v)
    others = np.arange(got.size) != at
    assert np.array_equal(got[others], rv[others])
    rep = val[(row == hot // n_cols) & (col == hot % n_cols)].astype(np.float64)
    assert rep.size == K
    bound = (K - 1) * 2.0 ** -24 * np.abs(rep).sum()
    err = abs(float(got[at]) - rep.sum())
    print(f"repeated pair: |sum - f64| = {err:.3e} = {err / bound:.4f} x bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------------------
# 2. normalised values, one by one
# ------------------------------------------------------------------------------------------------------------------------
def _ratio(name, got, ref, rtol=RTOL):
    """Worst |got - ref| / (rtol |ref|) over the non-zero references, printed; exact zeros must be exact."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    zero = ref == 0
    assert not got[zero].any(), f"{name}: a value that must be exactly 0 is not"
    worst = float((np.abs(got - ref)[~zero] / (rtol * np.abs(ref[~zero]))).max()) if (~zero).any() else 0.0
    print(f"{name}: worst error {worst:.3f} x rtol {rtol:g} over {int((~zero).sum())} values ({int(zero.sum())} exact zeros)")
    return worst


ROW_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1000)
N_U, N_I, HUB = 62_000, 8_000, 60_000


@pytest.fixture(scope="module")
def degree_graph():
    """A 70 000-node bipartite graph (62 000 users, 8 000 items): item 0 is a hub with 60 000 distinct users, users
    60 000 + k have exactly ROW_LENGTHS[k] distinct items, the other rows are short; every distinct pair is repeated 1-3
    times.  Returns the interactions and the float64 references of the coalesced symmetric operator."""
    rng = np.random.default_rng(2)
    pu = [np.arange(HUB), np.repeat(np.arange(HUB), 2)[rng.random(2 * HUB) < 0.4]]
    pi = [np.zeros(HUB, dtype=np.int64), None]
    pi[1] = rng.integers(1100, N_I, pu[1].size)
    for k, length in enumerate(ROW_LENGTHS):
        pu.append(np.full(length, HUB + k))
        pi.append(1 + np.arange(length))
    rest = np.arange(HUB + len(ROW_LENGTHS), N_U)
    pu.append(np.repeat(rest, 3))
    pi.append(rng.integers(1, N_I, 3 * rest.size))
    key = np.unique(np.concatenate(pu) * N_I + np.concatenate(pi))           # distinct pairs
    mult = rng.integers(1, 4, key.size)
    key = rng.permutation(np.repeat(key, mult))
    uid, iid = key // N_I, key % N_I
    n = N_U + N_I
    row, col = np.concatenate([uid, iid + N_U]), np.concatenate([iid + N_U, uid])
    rp, c, v = O.coalesce_csr(row, col, np.ones(row.size, np.float32), n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    lens = np.diff(rp)
    assert set(ROW_LENGTHS) | {HUB} <= set(lens.tolist()) and lens.max() == HUB
    assert set(np.unique(v).tolist()) == {1.0, 2.0, 3.0}
    deg_w = O.coo_sums_f64(row, None, n)                                      # multiplicities summed: from the COO
    assert deg_w.max() < 2 ** 24                                              # fp32 row sums are exact in any order
    return dict(uid=uid, iid=iid, row=row, col=col, n=n, rp=rp, c=c, v=v, rows=rows,
                ref_w=O.sym_norm_values_f64(rows, c, v, deg_w),
                ref_1=O.sym_norm_values_f64(rows, c, np.ones(c.size), lens.astype(np.float64)))


def test_sym_norm_values_over_the_degree_ladder(G, degree_graph):
    """`graph.sym_norm_device` on 70 000 nodes whose row lengths include 0, 1, 15-17, 31-33, 47-49, 1000 and one hub of
    60 000 (`row_dinv_kernel`'s strided 16-lane loop: 0 to 3750 trips, partial last trips, the four `__shfl_xor`): every
    stored value against float64 d_r v d_c with the degrees summed from the COO, rtol 3e-7.  Once with val = None (row
    length as the degree), once with the multiplicities 1-3 that coalescing produced, and the same graph through
    `CsrGraph.bipartite_sym_norm`.  Worst measured on MI355X, as a multiple of the bar: 0.41 (val = None), 0.51
    (multiplicities), 0.51 (bipartite_sym_norm), 0.37 on the hub row alone."""
    d = degree_graph
    rp, c, v, _ = G.coo_to_csr_device(d["row"], d["col"], None, d["n"], d["n"], "cuda", coalesce=True)
    assert np.array_equal(_np(rp), d["rp"]) and np.array_equal(_np(c), d["c"]) and np.array_equal(_np(v), d["v"])
    got_1 = _np(G.sym_norm_device(rp, c, None, d["n"]))
    got_w = _np(G.sym_norm_device(rp, c, v, d["n"]))
    g = G.CsrGraph.bipartite_sym_norm(d["uid"], d["iid"], N_U, N_I, "cuda")
    assert np.array_equal(g.rowptr_host, d["rp"]) and np.array_equal(_np(g.col), d["c"])
    worst = [_ratio("val=None", got_1, d["ref_1"]), _ratio("multiplicities", got_w, d["ref_w"]),
             _ratio("bipartite_sym_norm", _np(g.val), d["ref_w"])]
    hub = slice(int(d["rp"][N_U]), int(d["rp"][N_U + 1]))
    assert hub.stop - hub.start == HUB
    _ratio("hub row alone", got_w[hub], d["ref_w"][hub])
    assert max(worst) <= 1.0, worst


def test_gcn_norm_on_a_directed_edge_list(G):
    """`from_edge_index_gcn_norm(symmetric=False)` on a DIRECTED edge list with repeated edges: rows = targets in stable
    order, w = deg^-1/2[src] deg^-1/2[dst] with deg the in-degree from the edge list in float64.  A source that is no
    edge's target has d = 0, so its out-edges weigh exactly 0 (O.gcn_norm_weights), never inf or NaN.
    Worst measured on MI355X: 0.50 of the bar."""
    rng = np.random.default_rng(8)
    n, e = 20_000, 120_000
    src = rng.integers(0, n, e)
    dst = rng.integers(0, n // 2, e)                    # the upper half of the nodes are sources only
    dst[:20_000] = rng.integers(0, 40, 20_000)          # rows of a few hundred entries
    src[100:200], dst[100:200] = src[:100], dst[:100]   # repeated edges
    ei = np.stack([src, dst])
    g = G.CsrGraph.from_edge_index_gcn_norm(ei, n, "cuda", symmetric=False)
    w64 = O.sym_norm_values_f64(dst, src, np.ones(e), O.coo_sums_f64(dst, None, n))
    w32 = O.gcn_norm_weights(ei, n)
    assert np.array_equal(w64 == 0, w32 == 0) and (w64 == 0).sum() > 10_000 and (w64 != 0).sum() > 10_000
    rp, c, _, order = O.coo_to_csr_stable(dst, src, w32, n)
    assert np.array_equal(g.rowptr_host, rp) and np.array_equal(_np(g.col), c)
    assert _ratio("directed gcn_norm", _np(g.val), w64[order]) <= 1.0


def test_row_normalised_signs_and_cancelling_rows(G):
    """`CsrGraph.row_normalised` (`row_dinv_kernel` with 1 / s): every value against float64 v / rowsum with the row sums
    from the COO.  Values of both signs with duplicates; rows whose entries cancel to exactly 0 come out all 0 (1 / 0 -> inf
    -> 0), never inf or NaN; rows with a negative sum; one row of 5000 entries, rows of 15-17 and 31-33.
    Worst measured on MI355X: 0.30 of the bar."""
    rng = np.random.default_rng(9)
    n_rows, n_cols, nnz = 2000, 6000, 60_000
    row, col = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz)
    val = rng.choice(np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32), nnz)
    keep = (row >= 40) & (row % 97 != 0)                                      # rows 0-39 are built below, some stay empty
    row, col, val = [row[keep]], [col[keep]], [val[keep]]
    for r, length in enumerate((15, 16, 17, 31, 32, 33)):                    # zero-sum rows: +a and -a on distinct columns
        row += [np.full(2 * length, r)]
        col += [np.arange(2 * length) * 7]
        val += [np.concatenate([np.arange(1, length + 1), -np.arange(1, length + 1)]).astype(np.float32)]
    row += [np.full(5000, 10), np.full(17, 11), np.array([12, 12])]          # long row, negative row, +2 -2 on ONE pair
    col += [rng.choice(n_cols, 5000, replace=False), np.arange(17), np.array([5, 5])]
    val += [rng.choice(np.array([-1, 1, 2, 3], dtype=np.float32), 5000), np.full(17, -2, np.float32), np.array([2, -2], np.float32)]
    row, col, val = np.concatenate(row), np.concatenate(col), np.concatenate(val)
    rowsum = O.coo_sums_f64(row, val, n_rows)
    assert (rowsum[:6] == 0).all() and rowsum[11] == -34 and rowsum[12] == 0 and (rowsum < 0).sum() > 100
    g = G.CsrGraph.row_normalised(row, col, val, n_rows, n_cols, "cuda")
    rp, c, v = O.coalesce_csr(row, col, val, n_rows)                          # integer values: v is exact
    assert np.array_equal(g.rowptr_host, rp) and np.array_equal(_np(g.col), c)
    rows = np.repeat(np.arange(n_rows), np.diff(rp))
    ref = O.row_norm_values_f64(rows, v, rowsum)
    got = _np(g.val)
    assert not got[rows < 6].any() and not got[rows == 12].any()
    assert (ref[rows == 11] == 1.0 / 17).all()
    assert _ratio("row_normalised", got, ref) <= 1.0


@pytest.fixture(scope="module")
def second_trip_graph():
    """4 200 000 nodes, node 0 a hub with 60 000 neighbours, 2 090 000 further distinct undirected edges: nnz = 4 300 000."""
    rng = np.random.default_rng(42)
    n, n_hub, n_other = 4_200_000, 60_000, 2_090_000
    a, b = rng.integers(1, n, n_other + 4096), rng.integers(1, n, n_other + 4096)
    key = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    key = key[key // n != key % n]
    key = key[rng.permutation(key.size)[:n_other]]
    assert key.size == n_other
    a = np.concatenate([np.zeros(n_hub, dtype=np.int64), key // n])
    b = np.concatenate([1 + np.arange(n_hub), key % n])
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    assert src.size == 4_300_000
    return dict(n=n, src=src, dst=dst, deg=O.coo_sums_f64(dst, None, n))


@pytest.mark.parametrize("mode", ["stable_val_none", "coalesced_val"])
def test_sym_norm_second_grid_stride_trip(G, second_trip_graph, mode):
    """n_rows = 4 200 000 > 262 144 blocks x 16 rows and nnz = 4 300 000 > 16 384 x 256 threads: `row_dinv_kernel` and
    `scale_values_kernel` both take a second grid-stride trip (module-level functions only: no CsrGraph / HubPlan is
    built).  `stable_val_none`: by-row stable CSR, degree = row length, against O.coo_to_csr_stable + float64 gcn_norm
    weights; `coalesced_val`: (row, col)-sorted with stored values, `row_dinv_kernel`'s summing loop over the 60 000-entry
    hub row, against O.coalesce_csr + float64.  Every one of the 4.3 M values at rtol 3e-7; the values of the second trip
    (positions past 4 194 304) are reported on their own.  Worst measured on MI355X, both modes: 0.50 of the bar over all
    values, 0.31 over the second trip (the numpy restatement in fp32 sits at 0.50 too)."""
    d = second_trip_graph
    n, src, dst = d["n"], d["src"], d["dst"]
    if mode == "stable_val_none":
        w64 = O.sym_norm_values_f64(dst, src, np.ones(src.size), d["deg"])
        rp, c, _, _ = G.coo_to_csr_device(dst, src, None, n, n, "cuda")
        rrp, rc, _, order = O.coo_to_csr_stable(dst, src, np.ones(src.size, np.float32), n)
        ref = w64[order]
        got = G.sym_norm_device(rp, c, None, n)
    else:
        rp, c, v, _ = G.coo_to_csr_device(dst, src, None, n, n, "cuda", coalesce=True)
        rrp, rc, rv = O.coalesce_csr(dst, src, np.ones(src.size, np.float32), n)
        assert np.array_equal(_np(v), rv) and rv.size == src.size           # distinct pairs: nothing merged
        rows = np.repeat(np.arange(n), np.diff(rrp))
        ref = O.sym_norm_values_f64(rows, rc, rv, d["deg"])
        got = G.sym_norm_device(rp, c, v, n)
    assert np.array_equal(_np(rp), rrp) and np.array_equal(_np(c), rc)
    assert ref.size > 16_384 * 256 and n > 262_144 * 16
    got = _np(got)
    worst = _ratio(mode, got, ref)
    _ratio(mode + " second trip", got[16_384 * 256:], ref[16_384 * 256:])
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------------
# 3. C ABI branches no Python caller reaches
# ------------------------------------------------------------------------------------------------------------------------
def _raw_coo_to_csr(row, col, val, n_rows, n_cols, coalesce):
    """gcr_coo_to_csr called directly: (rowptr, col_out, val_out, perm_out, nnz_out, n_errors) as numpy, the outputs
    pre-filled with a sentinel."""
    from recommendation_amd import _lib
    L = _lib.lib()
    nnz = int(row.size)
    r = torch.from_numpy(np.ascontiguousarray(row, dtype=np.int64)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(col, dtype=np.int64)).cuda()
    v = torch.from_numpy(np.ascontiguousarray(val, dtype=np.float32)).cuda()
    rowptr = torch.full((n_rows + 1,), -7, dtype=torch.int64, device="cuda")
    col_out = torch.full((nnz,), -7, dtype=torch.int32, device="cuda")
    val_out = torch.full((nnz,), -7.0, dtype=torch.float32, device="cuda")
    perm = None if coalesce else torch.full((nnz,), -7, dtype=torch.int64, device="cuda")
    meta = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(L.gcr_coo_to_csr_workspace_bytes(nnz)), dtype=torch.uint8, device="cuda")
    _lib.check(L.gcr_coo_to_csr(_lib.dptr(r), _lib.dptr(c), _lib.dptr(v), nnz, n_rows, n_cols, int(coalesce),
                                _lib.dptr(rowptr), _lib.dptr(col_out), _lib.dptr(val_out), _lib.dptr(perm),
                                _lib.dptr(meta[0:1]), _lib.dptr(meta[1:2]), _lib.dptr(ws), _lib.cur_stream(r.device)),
               "gcr_coo_to_csr")
    n_out, n_err = (int(x) for x in meta.tolist())
    return _np(rowptr), _np(col_out), _np(val_out), None if perm is None else _np(perm), n_out, n_err


@pytest.mark.parametrize("coalesce", [False, True])
@pytest.mark.parametrize("where", ["start", "middle", "end", "all_invalid"])
def test_coo_to_csr_drops_invalid_entries(where, coalesce):
    """include/gcr.h: entries with an id outside the matrix sort to the end and are dropped, `n_errors` counts them,
    `nnz_out` the valid ones -- `rowptr_fill_kernel`'s `prev >= n_rows` / `cur > n_rows` branches and `split_key_kernel`'s
    `n_valid`, whose outputs Python never reads (it raises on n_errors).  Invalid = a negative row, row = n_rows, a negative
    column, col = n_cols, placed at the start, in the middle or at the end of the COO; the result equals the conversion of
    the valid subset alone (perm in positions of the FULL input).  `all_invalid`: rowptr all zeros, nnz_out 0.  The ids
    are range-checked before any use, so this is defined behaviour."""
    rng = np.random.default_rng(3)
    n_rows, n_cols, nnz = 37, 29, 900
    row, col = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz)
    if where == "middle":
        row %= 30                                      # rows 30-36 empty: the first invalid entry closes all of them
    else:
        row[rng.random(nnz) < 0.3] = n_rows - 1        # a long last row, next to the invalid tail
    val = _int_vals(rng, nnz)
    bad_r = np.array([-1, n_rows, 3, 5, -1, n_rows, n_rows, 0])
    bad_c = np.array([2, 4, -1, n_cols, -1, n_cols, 0, n_cols])
    bad_v = np.full(bad_r.size, 64.0, dtype=np.float32)
    if where == "all_invalid":
        row, col, val, valid = bad_r, bad_c, bad_v, np.zeros(bad_r.size, dtype=bool)
    else:
        at = {"start": 0, "middle": nnz // 2, "end": nnz}[where]
        row, col, val = (np.insert(a, at, b) for a, b in ((row, bad_r), (col, bad_c), (val, bad_v)))
        valid = np.ones(row.size, dtype=bool)
        valid[at:at + bad_r.size] = False
    assert np.array_equal(valid, (row >= 0) & (row < n_rows) & (col >= 0) & (col < n_cols))
    rp, c, v, perm, n_out, n_err = _raw_coo_to_csr(row, col, val, n_rows, n_cols, coalesce)
    assert n_err == int((~valid).sum()) == bad_r.size
    pos = np.flatnonzero(valid)
    if coalesce:
        rrp, rc, rv = O.coalesce_csr(row[valid], col[valid], val[valid], n_rows)
    else:
        rrp, rc, rv, order = O.coo_to_csr_stable(row[valid], col[valid], val[valid], n_rows)
        assert np.array_equal(perm[:n_out], pos[order])
    assert n_out == rc.size == int(rrp[-1])
    assert np.array_equal(rp, rrp)
    assert np.array_equal(c[:n_out], rc) and np.array_equal(v[:n_out], rv)
    if where == "all_invalid":
        assert n_out == 0 and not rp.any()


def test_rectangular_sym_norm_with_transposed_csr():
    """`gcr_csr_sym_norm_f32` with `rowptr_t` / `val_t` / `dinv_col` (no Python caller): D_r^-1/2 A D_c^-1/2 on a
    3000 x 500 operator with empty rows and empty columns, the transposed CSR from `coo_to_csr_device` on the swapped COO.
    Values, dinv_row and dinv_col against float64 from the COO at rtol 3e-7, exact zeros for the empty rows / columns.
    Worst measured on MI355X: 0.60 (values), 0.22 (dinv_row), 0.26 (dinv_col) of the bar."""
    from recommendation_amd import _lib, graph as G
    rng = np.random.default_rng(12)
    n_rows, n_cols, nnz = 3000, 500, 40_000
    row, col = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz)
    keep = (row % 50 != 7) & (col % 25 != 3) & (row != n_rows - 1) & (col != 0)
    row, col = row[keep], col[keep]
    val = _int_vals(rng, row.size)
    rowsum, colsum = O.coo_sums_f64(row, val, n_rows), O.coo_sums_f64(col, val, n_cols)
    assert (rowsum == 0).sum() >= 60 and (colsum == 0).sum() >= 20
    rp, c, v, _ = G.coo_to_csr_device(row, col, val, n_rows, n_cols, "cuda", coalesce=True)
    rpt, _, vt, _ = G.coo_to_csr_device(col, row, val, n_cols, n_rows, "cuda", coalesce=True)
    rrp, rc, rv = O.coalesce_csr(row, col, val, n_rows)
    assert np.array_equal(_np(rp), rrp) and np.array_equal(_np(c), rc) and np.array_equal(_np(v), rv)
    dinv_r = torch.full((n_rows,), -7.0, device="cuda")
    dinv_c = torch.full((n_cols,), -7.0, device="cuda")
    out = torch.full((c.numel(),), -7.0, device="cuda")
    _lib.check(_lib.lib().gcr_csr_sym_norm_f32(_lib.dptr(rp), _lib.dptr(c), _lib.dptr(v), n_rows, n_cols, _lib.dptr(rpt),
                                               _lib.dptr(vt), _lib.dptr(dinv_r), _lib.dptr(dinv_c), _lib.dptr(out),
                                               _lib.cur_stream(rp.device)), "gcr_csr_sym_norm_f32")
    rows = np.repeat(np.arange(n_rows), np.diff(rrp))
    dinv64 = lambda s: np.divide(1.0, np.sqrt(s), out=np.zeros_like(s), where=s > 0)      # noqa: E731
    worst = [_ratio("rectangular values", _np(out), O.sym_norm_values_f64(rows, rc, rv, rowsum, colsum)),
             _ratio("dinv_row", _np(dinv_r), dinv64(rowsum)), _ratio("dinv_col", _np(dinv_c), dinv64(colsum))]
    assert max(worst) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------------
# 4. second grid-stride trips of the streaming ops
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [33, 100])
def test_gather_rows_second_trip(d):
    """n = 262 144 + 37 indices > 65 536 blocks x 4 rows: `gather_rows_kernel` and `scatter_add_rows_kernel` take a second
    trip (d = 33: one partial pass of the 64 lanes, d = 100: two).  A few out-of-range ids, also among the last 37.
    Forward `torch.equal` to table[idx] with zero rows for the bad ids; backward against the float64 index_add_ at 1e-6 x
    max (the upstream gradient is a multiple of 1/8, so the atomic sums are exact in any order)."""
    from recommendation_amd import functional as Fn
    n, n_tab = 262_144 + 37, 1000
    g = torch.Generator(device="cuda").manual_seed(d)
    table = torch.randn(n_tab, d, device="cuda", generator=g).requires_grad_(True)
    idx = torch.randint(0, n_tab, (n,), device="cuda", generator=g)
    bad = torch.tensor([0, 5, 131_072, 262_143, 262_144, 262_150, n - 1], device="cuda")
    idx[bad] = torch.tensor([-1, n_tab, 2 ** 40, -5, n_tab, -(2 ** 40), n_tab + 7], device="cuda")
    ok = (idx >= 0) & (idx < n_tab)
    assert int((~ok).sum()) == bad.numel()
    out = Fn.gather_rows(table, idx)
    want = table.detach()[idx.clamp(0, n_tab - 1)] * ok.unsqueeze(1)
    assert torch.equal(out.detach(), want)
    w = torch.randint(-32, 33, (n, d), device="cuda", generator=g).float() / 8
    (out * w).sum().backward()
    ref = torch.zeros(n_tab, d, dtype=torch.float64, device="cuda").index_add_(0, idx[ok], w[ok].double())
    err, scale = float((table.grad.double() - ref).abs().max()), max(float(ref.abs().max()), 1.0)
    print(f"gather_rows backward d={d}: err {err:.3e} = {err / (1e-6 * scale):.3f} x bound")
    assert err <= 1e-6 * scale


def test_spgemm_expand_second_trip():
    """`Sp.__matmul__` with a_nnz = 1 048 576 + 1000 > 65 536 blocks x 16 non-zeros: `spgemm_expand_kernel` takes a second
    trip.  B is a permutation scaled by 1-3 with rows of length 0, 16, 17, 33 and 1000 (the 16-lane loop: no trip, one
    full, one full + 1, two full + 1, 62.5), their extra entries in columns of their own.  So A @ B is A with permuted
    columns and scaled values plus the known extra columns, with no two products on one (row, col): structure and (integer)
    values exact against torch index arithmetic."""
    from recommendation_amd.graph_ops import Sp
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(4)
    R, C, nnz = 2048, 4096, 1_048_576 + 1000
    key = torch.sort(torch.randperm(R * C, device=dev, generator=gen)[:nnz]).values
    a_row, a_col = key // C, key % C
    a_val = torch.randint(1, 4, (nnz,), device=dev, generator=gen).float()
    rp = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    rp[1:] = torch.cumsum(torch.bincount(a_row, minlength=R), 0)
    A = Sp(rp, a_col.to(torch.int32), a_val, R, C)
    perm = torch.randperm(C, device=dev, generator=gen)
    scale = torch.randint(1, 4, (C,), device=dev, generator=gen).float()
    special = {100: 0, 200: 16, 300: 17, 400: 33, 500: 1000}           # row of B -> its length
    b_row, b_col, b_val, nxt = [torch.arange(C, device=dev)], [perm], [scale], C
    for k, length in special.items():
        if length:
            b_row.append(torch.full((length - 1,), k, device=dev))
            b_col.append(torch.arange(nxt, nxt + length - 1, device=dev))
            b_val.append(torch.randint(1, 4, (length - 1,), device=dev, generator=gen).float())
            nxt += length - 1
    b_row, b_col, b_val = torch.cat(b_row), torch.cat(b_col), torch.cat(b_val)
    live = b_row != 100                                                  # the empty row
    b_row, b_col, b_val = b_row[live], b_col[live], b_val[live]
    order = torch.argsort(b_row * nxt + b_col)
    b_row, b_col, b_val = b_row[order], b_col[order], b_val[order]
    brp = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    brp[1:] = torch.cumsum(torch.bincount(b_row, minlength=C), 0)
    assert sorted((brp[1:] - brp[:-1])[list(special)].tolist()) == sorted(special.values())
    B = Sp(brp, b_col.to(torch.int32), b_val, C, nxt)
    P = A @ B
    # expectation: every (A non-zero, B entry of its column's row) pair, no two on one (row, col)
    e_row, e_col, e_val = [], [], []
    on = a_col != 100
    e_row.append(a_row[on]), e_col.append(perm[a_col[on]]), e_val.append(a_val[on] * scale[a_col[on]])
    for k, length in special.items():
        if length:
            hit = torch.nonzero(a_col == k).reshape(-1)
            lo = int(brp[k])
            extra = torch.arange(lo, lo + length, device=dev)
            extra = extra[b_col[extra] >= C]                              # the entries besides the permutation's
            assert extra.numel() == length - 1
            e_row.append(a_row[hit].repeat_interleave(length - 1))
            e_col.append(b_col[extra].repeat(hit.numel()))
            e_val.append((a_val[hit].unsqueeze(1) * b_val[extra].unsqueeze(0)).reshape(-1))
    e_row, e_col, e_val = torch.cat(e_row), torch.cat(e_col), torch.cat(e_val)
    ekey, order = torch.sort(e_row * nxt + e_col)
    assert bool((ekey[1:] != ekey[:-1]).all())
    assert P.nnz == ekey.numel() > nnz
    assert torch.equal(P.row_of().to(torch.int64) * nxt + P.col.to(torch.int64), ekey)
    erp = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    erp[1:] = torch.cumsum(torch.bincount(e_row, minlength=R), 0)
    assert torch.equal(P.rowptr, erp) and torch.equal(P.val, e_val[order])


def test_csr_lookup_second_trip():
    """`Sp.__mul__` with nnz = 131 072 rows x 129 ascending columns = 16 908 288 > 65 536 x 256 threads:
    `csr_lookup_kernel` takes a second trip.  A * A = val^2 exactly on the same structure; A * B with B = A minus its
    odd-position entries keeps exactly the even positions (the binary search misses every other column)."""
    from recommendation_amd.graph_ops import Sp
    dev = torch.device("cuda")
    R, L, C = 131_072, 129, 1000
    e = torch.arange(R * L, device=dev)
    r, j = e // L, e % L
    col = (r % 7 + 7 * j).to(torch.int32)
    val = (1 + e % 5).float()
    rp = torch.arange(R + 1, device=dev, dtype=torch.int64) * L
    A = Sp(rp, col, val, R, C)
    assert A.nnz == 16_908_288 > 65_536 * 256
    sq = A * A
    assert torch.equal(sq.rowptr, rp) and torch.equal(sq.col, col) and torch.equal(sq.val, val * val)
    del sq
    even = j % 2 == 0
    vb = (2 + e % 3).float()[even]
    B = Sp(torch.arange(R + 1, device=dev, dtype=torch.int64) * 65, col[even].contiguous(), vb, R, C)
    AB = A * B
    assert torch.equal(AB.rowptr, B.rowptr) and torch.equal(AB.col, B.col) and torch.equal(AB.val, val[even] * vb)
    del A, B, AB
    torch.cuda.empty_cache()


N_OPT = 67_108_864 + 1203        # > 65 536 blocks x 256 threads x 4 floats; n % 4 = 3: the scalar tail runs too


def test_fused_adam_second_trip():
    """FusedAdam on a 1-D parameter of 67 108 864 + 1203 elements: the `float4` loop of `adam_step_kernel` takes a second
    trip (the benchmark's 70.4 M-element table runs this regime every step) and the n % 4 tail follows it.  Two steps
    against torch.optim.Adam at the bar of test_fused_adam_matches_torch_adam: 2e-6 x max|p|, exp_avg_sq within 1e-6.
    Measured on MI355X: 0.04 of the parameter bound, exp_avg_sq 5.0e-7."""
    from recommendation_amd.optim import FusedAdam
    g = torch.Generator(device="cuda").manual_seed(1)
    p0 = torch.randn(N_OPT, device="cuda", generator=g)
    pa, pb = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0)
    ref, opt = torch.optim.Adam([pa], lr=1e-2, weight_decay=1e-4), FusedAdam([pb], lr=1e-2, weight_decay=1e-4)
    for _ in range(2):
        gr = torch.randn(N_OPT, device="cuda", generator=g)
        pa.grad, pb.grad = gr, gr.clone()
        ref.step()
        opt.step()
    del gr
    diff = (pa.detach() - pb.detach()).abs_()
    err, scale = float(diff.max()), float(pa.detach().abs().max())
    err_tail = float(diff[4 * 65_536 * 256:].max())
    del diff
    err_v = float((ref.state[pa]["exp_avg_sq"] - opt.state[pb]["exp_avg_sq"]).abs_().max())
    print(f"adam: param err {err:.3e} = {err / (2e-6 * scale):.3f} x bound (second trip + tail {err_tail:.3e}), "
          f"exp_avg_sq err {err_v:.3e}")
    del ref, opt, pa, pb, p0
    torch.cuda.empty_cache()
    assert err <= 2e-6 * scale and err_v <= 1e-6


def test_fused_sgd_second_trip():
    """FusedSGD on the same size (`sgd_momentum_step_kernel`'s `float4` loop takes a second trip, then the n % 4 tail): two
    steps against torch.optim.SGD(momentum=0.9) in float64 under the bound of
    test_fused_sgd_against_float64_torch_sgd: param u (n P + lr M n (n + 1)), buffer 2 u M n with u = 2^-24.
    Measured on MI355X: 0.58 of the parameter bound, 0.31 of the buffer bound."""
    from recommendation_amd.optim import FusedSGD
    gen = torch.Generator(device="cuda").manual_seed(3)
    n, lr, mu, wd = 2, 0.05, 0.9, 1e-4
    p32 = torch.nn.Parameter(torch.randn(N_OPT, device="cuda", generator=gen))
    p64 = torch.nn.Parameter(p32.detach().double())
    ours = FusedSGD([p32], lr=lr, momentum=mu, weight_decay=wd)
    theirs = torch.optim.SGD([p64], lr=lr, momentum=mu, weight_decay=wd)
    big_p, big_m = float(p64.detach().abs().max()), 0.0
    for _ in range(n):
        g = torch.randn(N_OPT, device="cuda", generator=gen)
        p32.grad, p64.grad = g, g.double()
        big_m = max(big_m, float(g.abs().max()) + wd * big_p)            # >= max |grad + wd p| before the step
        ours.step()
        theirs.step()
        big_p = max(big_p, float(p64.detach().abs().max()))
        big_m = max(big_m, float(theirs.state[p64]["momentum_buffer"].abs().max()))
        p32.grad = p64.grad = None
    del g
    u = 2.0 ** -24
    tol_p, tol_m = u * (n * big_p + lr * big_m * n * (n + 1)), 2 * u * big_m * n
    err_p = float((p32.detach().double() - p64.detach()).abs_().max())
    err_m = float((ours.state[p32]["momentum_buffer"].double() - theirs.state[p64]["momentum_buffer"]).abs_().max())
    print(f"sgd: param err {err_p:.3e} = {err_p / tol_p:.3f} x bound, buffer err {err_m:.3e} = {err_m / tol_m:.3f} x bound")
    del ours, theirs, p32, p64
    torch.cuda.empty_cache()
    assert err_p <= tol_p and err_m <= tol_m


# ------------------------------------------------------------------------------------------------------------------------
# 6. motif algebra beyond 60 users
# ------------------------------------------------------------------------------------------------------------------------
def test_motif_adjacency_400_users():
    """`graph_ops.build_hyper_graphs` at 400 users x 300 items (the golden has 60 users): about 5000 directed social pairs
    with 800 reciprocated and 50 repeated, 12 000 interactions with repeats, against O.mhcn_motif_adjacency on the dense
    count matrices: structure exact, values at rtol 2e-6 / atol 1e-7 (test_motif_adjacency_matches_reference's bar).
    Many rows of U = S - B hold more than 16 entries, so `spgemm_expand_kernel`'s 16-lane loop takes a second trip; the
    `> 3` filter of H_p keeps some entries and drops others; no operator is empty."""
    from recommendation_amd import graph_ops
    rng = np.random.default_rng(0)
    n_u, n_i = 400, 300
    s = (n_u * rng.random(6000) ** 2).astype(np.int64) * n_u + rng.integers(0, n_u, 6000)     # sources skewed to low ids
    s = s[np.sort(np.unique(s, return_index=True)[1])]                                       # distinct, in drawn order
    s = s[s // n_u != s % n_u][:4200]
    s_row, s_col = s // n_u, s % n_u
    s_row, s_col = (np.concatenate([s_row, s_col[:800], s_row[1000:1050]]),          # + 800 reciprocated, + 50 repeated
                    np.concatenate([s_col, s_row[:800], s_col[1000:1050]]))
    y_row, y_col = rng.integers(0, n_u, 12_000), rng.integers(0, n_i, 12_000)
    S, Y = np.zeros((n_u, n_u)), np.zeros((n_u, n_i))
    np.add.at(S, (s_row, s_col), 1.0)
    np.add.at(Y, (y_row, y_col), 1.0)
    assert S.max() == 2 and Y.max() >= 2 and ((S > 0) & (S.T > 0)).sum() >= 1600
    U = S - S * S.T
    print(f"S {int((S != 0).sum())} pairs, rows of U with more than 16 entries: {int(((U != 0).sum(1) > 16).sum())}")
    assert ((U != 0).sum(1) > 16).sum() > 20                    # second trips of the 16-lane loop in U @ U, B @ U ...
    ref = dict(zip(("H_s", "H_j", "H_p"), O.mhcn_motif_adjacency(S, Y)))
    ref["R"] = np.divide(Y, Y.sum(1, keepdims=True), out=np.zeros_like(Y), where=Y.sum(1, keepdims=True) > 0)
    yy = Y @ Y.T
    a10 = yy - yy * (S * S.T) - (yy * U + (yy * U).T)
    assert 0 < (a10 > 3).sum() < (a10 > 0).sum()               # the filter keeps some entries and drops others
    hs, hj, hp, r = graph_ops.build_hyper_graphs(s_row, s_col, y_row, y_col, n_u, n_i, "cuda")
    for name, g in (("H_s", hs), ("H_j", hj), ("H_p", hp), ("R", r)):
        want = ref[name]
        got = np.zeros_like(want)
        rows = np.repeat(np.arange(g.n_rows), np.diff(g.rowptr_host))
        got[rows, _np(g.col)] = _np(g.val)
        print(f"{name}: {g.nnz} non-zeros")
        assert g.nnz > 0 and g.nnz == int((want != 0).sum()), name
        assert np.array_equal(got != 0, want != 0), name
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-7, err_msg=name)


# ------------------------------------------------------------------------------------------------------------------------
# 7. exact-count dropout, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", [1, 31, 32, 33, 64, 100_003])
def test_exact_count_dropout_bits_match_oracle(nnz):
    """`gcr_edge_mask_exact_bits` bit for bit against O.edge_keep_exact (Philox key (x << 32) | y of ctr (e, 1, 'EDGE'),
    stable ascending sort, the first n_keep kept): n_keep in {0, 1, nnz - 1, nnz} and the int(nnz (1 - rate)) of rates
    0.1 / 0.25 / 0.5 / 0.9; the bits past nnz are clear; two calls give the same bits."""
    from recommendation_amd import functional as Fn
    seed = 7 + (1 << 40)                                         # both key words non-zero
    keeps = sorted({0, 1, nnz - 1, nnz} | {int(nnz * (1 - r)) for r in (0.1, 0.25, 0.5, 0.9)})
    for n_keep in keeps:
        if not 0 <= n_keep <= nnz:
            continue
        bits = Fn.edge_mask_exact_bits(nnz, n_keep, seed, "cuda")
        again = Fn.edge_mask_exact_bits(nnz, n_keep, seed, "cuda")
        assert torch.equal(bits, again)
        got = np.unpackbits(_np(bits).view(np.uint8), bitorder="little").astype(bool)
        assert got.size == 32 * ((nnz + 31) // 32) and not got[nnz:].any()
        want = O.edge_keep_exact(nnz, n_keep, seed)
        assert np.array_equal(got[:nnz], want), (nnz, n_keep, int(got[:nnz].sum()))
