"""The row-wise glue kernels off their one tested shape, each against the float64 restatement of tests/rowops_rules.py
under the project's rule (err / S <= max(4 x drift, 2^-20) and <= 1e-5; the exact kernels by array_equal):
  gcr_infonce.hip   row_inv_norm, pos_logit, infonce_pos_bwd, normalize_bwd
  gcr_dense.hip     normalize_bwd_n / _raw, rows_dot_vec, weighted_colsum, gram_tn
  gcr_ops.hip       gather_rows / scatter_add_rows, bitmap_set, csr_lookup
Through the `functional` wrapper where there is one; through `_lib.call` on the raw entry where the wrapper hides the path.
What each shape is chosen against is said where rowops_rules.py lists it and checked by tests/test_rowops_rules_cpu.py."""
import numpy as np
import pytest
import torch

import rowops_rules as R

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ids(shapes):
    return ["-".join(str(int(v) if isinstance(v, bool) else v) for v in s) for s in shapes]


@pytest.mark.parametrize("shape", R.INV_NORM_SHAPES, ids=ids(R.INV_NORM_SHAPES))
def test_row_inv_norm(shape):
    from recommendation_amd import functional as Fn
    c = R.inv_norm_case(*shape)
    out = Fn.row_inv_norm(dev(c["x"]), eps=R.EPS)
    R.check_rows(out, c["ref"], c["f32"], f"row_inv_norm:{shape}")
    assert float(out[3]) == float(out[7]) == float(np.float32(1.0) / np.float32(R.EPS))      # both clamped rows: 1 / eps


@pytest.mark.parametrize("shape", R.POS_LOGIT_SHAPES, ids=ids(R.POS_LOGIT_SHAPES))
def test_pos_logit(shape):
    from recommendation_amd import functional as Fn
    c = R.pos_logit_case(*shape)
    out = Fn.pos_logit_raw(dev(c["a"]), dev(c["sa"]), dev(c["b"]), dev(c["sb"]), dev(c["pos"]), c["scale"]).cpu().numpy()
    nan = np.isnan(c["ref"])
    assert np.array_equal(np.isnan(out), nan) and nan.sum() == (2 if shape[3] else 0)      # NaN in those rows and nowhere else
    R.check(out[~nan], c["ref"][~nan], c["f32"][~nan], f"pos_logit:{shape}")


@pytest.mark.parametrize("mode", ["gx", "gy", "both"])
@pytest.mark.parametrize("shape", R.POS_BWD_SHAPES, ids=ids(R.POS_BWD_SHAPES))
def test_infonce_pos_bwd(shape, mode):
    """gx is added to, not overwritten (it starts from random contents, and so does gy); either may be NULL; ids outside
    [0, ny) change nothing; HOT_ANCHORS anchors add into one row of gy with atomics."""
    from recommendation_amd import _lib
    c = R.pos_bwd_case(*shape)
    mx, ny, d = shape[:3]
    gx = dev(c["gx_in"]) if mode != "gy" else None
    gy = dev(c["gy_in"]) if mode != "gx" else None
    x = dev(c["x"])
    _lib.call("gcr_infonce_pos_bwd_f32", x, dev(c["sx"]), dev(c["y"]), dev(c["sy"]), dev(c["pos"]), dev(c["coef"]), mx, ny, d,
              c["inv_tau"], gx, gy, on=x)
    torch.cuda.synchronize()
    if gx is not None:
        R.check(gx, c["ref"][0], c["f32"][0], f"pos_bwd:{shape} {mode} gx")
        # what was added, against the same scale: gx_out - gx_in is the anchor-side term itself
        R.check(gx.cpu().numpy().astype(np.float64) - c["gx_in"], c["ref"][0] - c["gx_in"], c["f32"][0] - c["gx_in"],
                f"pos_bwd:{shape} {mode} gx_out - gx_in", scale=float(np.abs(c["ref"][0]).max()))
        if c["pos"] is not None:
            assert np.array_equal(gx[:4].cpu().numpy(), c["gx_in"][:4])                      # ids -1 and ny: untouched
    if gy is not None:
        R.check(gy, c["ref"][1], c["f32"][1], f"pos_bwd:{shape} {mode} gy")
        if c["pos"] is not None:
            unnamed = np.setdiff1d(np.arange(ny), c["pos"])
            assert np.array_equal(gy.cpu().numpy()[unnamed], c["gy_in"][unnamed])


@pytest.mark.parametrize("shape", R.NORMALIZE_BWD_SHAPES, ids=ids(R.NORMALIZE_BWD_SHAPES))
def test_normalize_bwd(shape):
    """gcr_normalize_bwd_f32 out of place and in place (out == ghat): the two bitwise equal."""
    from recommendation_amd import _lib
    c = R.normalize_bwd_case(*shape)
    n, d = shape
    x, inv, g = dev(c["x"]), dev(c["inv"]), dev(c["g"])
    out = torch.full_like(g, float("nan"))
    _lib.call("gcr_normalize_bwd_f32", x, inv, g, n, d, out, on=x)
    assert torch.equal(g, dev(c["g"]))                                                       # out of place: ghat is read only
    R.check(out, c["ref"], c["f32"], f"normalize_bwd:{shape}", apart=c["apart"], scale=c["scale"])
    _lib.call("gcr_normalize_bwd_f32", x, inv, g, n, d, g, on=x)
    assert torch.equal(g, out)


@pytest.mark.parametrize("from_raw", [False, True], ids=["n", "raw"])
@pytest.mark.parametrize("shape", R.NORMALIZE_BWD_N_SHAPES, ids=ids(R.NORMALIZE_BWD_N_SHAPES))
def test_normalize_bwd_n_and_raw(shape, from_raw):
    """Fn.normalize_bwd_n (gcr_normalize_bwd_n_f32, and gcr_normalize_bwd_raw_f32 with from_raw) out of place, with out = g_n
    and with out = g_raw: all bitwise equal; the clamped row is compared, against its own scale."""
    from recommendation_amd import functional as Fn
    c = R.normalize_bwd_n_case(*shape, from_raw)
    src, inv, g, g_raw = dev(c["src"]), dev(c["inv"]), dev(c["g"]), dev(c["g_raw"])
    out = Fn.normalize_bwd_n(src, inv, g, g_raw, from_raw=from_raw)
    assert torch.equal(g, dev(c["g"])) and (g_raw is None or torch.equal(g_raw, dev(c["g_raw"])))
    R.check(out, c["ref"], c["f32"], f"normalize_bwd_{'raw' if from_raw else 'n'}:{shape}", apart=c["apart"])
    g2 = g.clone()
    assert Fn.normalize_bwd_n(src, inv, g2, g_raw, out=g2, from_raw=from_raw) is g2 and torch.equal(g2, out)
    if g_raw is not None:
        r2 = g_raw.clone()
        assert Fn.normalize_bwd_n(src, inv, g, r2, out=r2, from_raw=from_raw) is r2 and torch.equal(r2, out)


@pytest.mark.parametrize("shape", R.ROWS_DOT_VEC_SHAPES, ids=ids(R.ROWS_DOT_VEC_SHAPES))
def test_rows_dot_vec(shape):
    """Fn.rows_dot_vec forward, and its gradient of v (gcr_weighted_colsum_f32; torch's beyond d = 256) under the same rule."""
    from recommendation_amd import functional as Fn
    c = R.dot_case(*shape)
    x, v = dev(c["x"]), dev(c["v"]).requires_grad_(True)
    out = Fn.rows_dot_vec(x, v)
    assert (type(out.grad_fn).__name__.startswith("_RowsDotVec")) == (shape[1] <= 256)
    R.check(out, c["ref"], c["f32"], f"rows_dot_vec:{shape}")
    out.backward(dev(c["w"]))
    R.check(v.grad, c["ref_colsum"], c["f32_colsum"], f"rows_dot_vec:{shape} grad v")


@pytest.mark.parametrize("shape", R.COLSUM_SHAPES, ids=ids(R.COLSUM_SHAPES))
def test_weighted_colsum(shape):
    from recommendation_amd import _lib
    c = R.dot_case(*shape)
    n, d = shape
    x, w = dev(c["x"]), dev(c["w"])
    out = torch.full((d,), float("nan"), device="cuda")
    ws = _lib.workspace("gcr_weighted_colsum_workspace_bytes", n, d, device=x.device)
    _lib.call("gcr_weighted_colsum_f32", x, w, n, d, out, ws, on=x)
    R.check(out, c["ref_colsum"], c["f32_colsum"], f"weighted_colsum:{shape}")
    again = torch.empty_like(out)
    _lib.call("gcr_weighted_colsum_f32", x, w, n, d, again, ws, on=x)
    assert torch.equal(out, again)


@pytest.mark.parametrize("dx,dg", R.GRAM_PAIRS)
def test_gram_tn_every_pair(dx, dg):
    """All 16 width pairs around the 8-pair unroll and at two and three workgroups; two calls bitwise equal; n = 0 zeros."""
    from recommendation_amd import functional as Fn
    for n in R.GRAM_SMALL_N:
        c = R.gram_case(n, dx, dg)
        x, g = dev(c["x"]), dev(c["g"])
        out = Fn.gram_tn(x, g)
        R.check(out, c["ref"], c["f32"], f"gram_tn:{(n, dx, dg)}")
        assert torch.equal(out, Fn.gram_tn(x, g))
    zero = Fn.gram_tn(torch.empty(0, dx, device="cuda"), torch.empty(0, dg, device="cuda"))
    assert zero.shape == (dx, dg) and not zero.any()


@pytest.mark.parametrize("shape", [(R.OVER_CAP_GRAM, 32, 32), (257, 48, 64)], ids=["over_cap", "library_width"])
def test_gram_tn_over_the_cap_and_outside_the_table(shape):
    """262147 rows: 1024 workgroups of 258 rows.  A width outside {32, 64, 96, 128} goes to the library product and meets
    the same rule."""
    from recommendation_amd import functional as Fn
    c = R.gram_case(*shape)
    x, g = dev(c["x"]), dev(c["g"])
    out = Fn.gram_tn(x, g)
    R.check(out, c["ref"], c["f32"], f"gram_tn:{shape}")
    if shape[1] in R.GRAM_DIMS:
        assert torch.equal(out, Fn.gram_tn(x, g))


@pytest.mark.parametrize("shape", R.GATHER_SHAPES, ids=ids(R.GATHER_SHAPES))
def test_gather_rows_and_scatter_backward(shape):
    """Fn.gather_rows as documented: an id outside [0, N) gives a zero row (exact) and is skipped by the backward."""
    from recommendation_amd import functional as Fn
    c = R.gather_case(*shape)
    table = dev(c["table"]).requires_grad_(True)
    out = Fn.gather_rows(table, dev(c["idx"]))
    assert np.array_equal(out.detach().cpu().numpy(), c["fwd"])
    out.backward(dev(c["up"]))
    R.check(table.grad, c["ref"], c["f32"], f"scatter_add_rows:{shape}")
    untouched = np.setdiff1d(np.arange(shape[0]), c["idx"])
    assert not table.grad.cpu().numpy()[untouched].any()


@pytest.mark.parametrize("n_bits", [1, 32, 70, 1000])
def test_bitmap_set(n_bits):
    """Duplicates, ids outside [0, n_bits) (n_bits itself, the rest of the last word, negative, huge), a last word that is
    partly used, and bits already there: atomicOr keeps them."""
    from recommendation_amd import _lib
    rng = np.random.default_rng(n_bits)
    n_words = (n_bits + 31) // 32 + 2                                       # two words past the end: never written
    words = rng.integers(0, 1 << 32, n_words, dtype=np.uint64).astype(np.uint32) & np.uint32(0x11111111)
    idx = np.concatenate([rng.integers(0, n_bits, 3 * n_bits), rng.integers(0, n_bits, 5).repeat(40),
                          [n_bits, n_bits + 1, 32 * ((n_bits + 31) // 32) - 1 + (n_bits % 32 == 0), -1, -33, 1 << 40, 0, n_bits - 1]])
    idx = rng.permutation(idx).astype(np.int64)
    bits = torch.from_numpy(words.view(np.int32).copy()).cuda()
    didx = dev(idx)
    _lib.call("gcr_bitmap_set", didx, idx.size, n_bits, bits, on=didx)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), R.bitmap(idx, n_bits, words))
    # and through the wrapper, from zeros
    from recommendation_amd import functional as Fn
    got = Fn.active_rows_bitmap(didx, n_bits).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, R.bitmap(idx, n_bits, np.zeros((n_bits + 31) // 32, dtype=np.uint32)))


@pytest.mark.parametrize("with_val", [True, False])
def test_csr_lookup(with_val):
    """Every (row, column) of a 40 x 50 grid against the dense mask: row 0 is empty, row 1 holds one entry, row 2 only its
    first and last column, so queries fall below the first and above the last stored column; m_val NULL answers 1."""
    from recommendation_amd import _lib
    rng = np.random.default_rng(5)
    dense = ((rng.random((40, 50)) < 0.2) * rng.integers(1, 9, (40, 50))).astype(np.float32)
    dense[0], dense[1], dense[2] = 0.0, 0.0, 0.0
    dense[1, 17], dense[2, 0], dense[2, 49] = 3.0, 4.0, 5.0
    dense[3, :2], dense[3, 48:], dense[3, 20] = 0.0, 0.0, 6.0                # nothing at either end of row 3
    rowptr, col, val = R.csr_of(dense)
    r, c = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(40), np.arange(50), indexing="ij"))
    out = torch.full((r.size,), float("nan"), device="cuda")
    dr = dev(r)
    _lib.call("gcr_csr_lookup_f32", dr, dev(c), r.size, dev(rowptr), dev(col), dev(val) if with_val else None, out, on=dr)
    want = dense if with_val else (dense != 0).astype(np.float32)
    assert np.array_equal(out.cpu().numpy(), want[r, c])

