"""Bit-for-bit pin of gcr_spmm_csr_acc2_f32's summation order around every point where the kernel's load pipeline
changes shape: row ends, 16-gather batch boundaries, 64-non-zero block boundaries, partition tails, chunked rows, masks.

The expected bits come from a replay of the documented order over `graph.plan.desc_host` and the long-row lists with the
float32 fma of tests/test_spmm_order_cpu.py: per partition, the kept non-zeros of a row (or chunk) in stored order, one fma
each from 0; chunk partials of a split row summed per wave (chunks w, w+4, ...) and the four wave sums added in wave order;
then `* val_scale`, then `(acc_in [+ acc_in2 * s] + y) * acc_scale`.  Scheduling changes in the kernel (prefetched
`acc_in`, prefetched col/val blocks, batched tails) must leave every one of these bits alone.  The float64 oracle stays
beside it at the stress test's 1e-5.  The row L2-normalise goes through a wave reduction and a division and keeps its
tolerance (not bit-pinned)."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from test_spmm_order_cpu import fma32

pytestmark = pytest.mark.gpu

F32 = np.float32
N_COLS = 700
P_MAX = 8          # longer than any acc_in prefetch queue the kernel could afford in registers


def _degrees(kind, L):
    if kind == "deg1_64":
        return [1] * 64                                            # 64 rows, 64 non-zeros: one full partition at L = 64
    if kind == "deg1_many":
        return [1] * 200                                           # kMaxRowsPerPart closes the partitions (L = 512)
    if kind == "all_empty":
        return [0] * 50
    assert kind == "composite"
    deg = [0] * (P_MAX + 3) + [3, 2]                                # empty run at the start of a partition
    deg += [5] + [0] * (P_MAX + 1) + [4, 1, 1]                      # ... in the middle
    deg += [15, 1, 16, 17, 1, 63, 1, 64, 65, 2]                     # row ends on batch (16) and block (64) boundaries
    deg += [L // 2, L // 2]                                         # a row ending exactly at the partition's last non-zero
    deg += [L, 5, L, 16, L, 17, L, 69, L, 80, L, 81, L - 1, L]      # one-row partitions; tails of < UNR, UNR, UNR + 1
    deg += [L + 1, 3, 2 * L + 1, 7 * L + 3, 1, 1]                   # chunked rows (no flush), neighbours on both sides
    deg += [9, 11, 10, 12, 8, 13, 7, 10, 10, 10, 31, 33, 1, 0, 2]   # the mean-degree-10 regime of the user rows
    deg += [6] + [0] * (P_MAX + 2)                                  # empty run at the end of the partition and the matrix
    return deg


class _Case:
    """One matrix + plan, its device graph, and a cache of replayed raw sums per mask."""

    def __init__(self, kind, L, d, has_val):
        import recommendation_amd as ra
        seed = sum(map(ord, kind)) * 7 + L + 13 * d + int(has_val)
        rng = np.random.default_rng(seed)
        deg = np.asarray(_degrees(kind, L), dtype=np.int64)
        self.n_rows, self.d, self.L = deg.size, d, L
        assert self.n_rows <= 900
        self.rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        self.nnz = int(self.rowptr[-1])
        self.col = rng.integers(0, N_COLS, self.nnz).astype(np.int32)
        self.val = rng.standard_normal(self.nnz).astype(F32) if has_val else None
        self.w = self.val if has_val else np.ones(self.nnz, F32)
        self.x = rng.standard_normal((N_COLS, d)).astype(F32)
        self.acc_in = rng.standard_normal((self.n_rows, d)).astype(F32)
        self.acc_in2 = rng.standard_normal((self.n_rows, d)).astype(F32)
        self.g = ra.CsrGraph(self.rowptr, self.col, self.val, self.n_rows, N_COLS, "cuda", nnz_per_part=L)
        self.xt = torch.from_numpy(self.x).cuda()
        self.rng = rng

    def replay(self, keep, x=None):
        """Raw float32 row sums (before val_scale) in the kernel's order; keep: bool [nnz]."""
        x = self.x if x is None else x
        plan = self.g.plan
        desc = plan.desc_host
        seg_a, seg_b, seg_row, seg_slot = [], [], [], []
        for a, b, rowinfo, slot in desc.tolist():
            row0, nrows = rowinfo & 0xFFFFFFFF, rowinfo >> 32
            if slot < 0:
                assert a == self.rowptr[row0] and b == self.rowptr[row0 + nrows]
                for r in range(row0, row0 + nrows):
                    seg_a.append(self.rowptr[r]); seg_b.append(self.rowptr[r + 1]); seg_row.append(r); seg_slot.append(-1)
            else:
                seg_a.append(a); seg_b.append(b); seg_row.append(row0); seg_slot.append(slot)
        seg_a, seg_b = np.asarray(seg_a, np.int64), np.asarray(seg_b, np.int64)
        seg_slot = np.asarray(seg_slot, np.int64)
        # the kept non-zeros of every segment, in stored order
        seg_of = np.repeat(np.arange(seg_a.size), seg_b - seg_a)
        e_all = np.concatenate([np.arange(a, b) for a, b in zip(seg_a, seg_b)]) if seg_a.size else np.zeros(0, np.int64)
        assert e_all.size == self.nnz and np.array_equal(np.sort(e_all), np.arange(self.nnz))     # covered exactly once
        kept = keep[e_all]
        seg_of, e_all = seg_of[kept], e_all[kept]
        first = np.searchsorted(seg_of, np.arange(seg_a.size))
        rank = np.arange(e_all.size) - first[seg_of]
        acc = np.zeros((seg_a.size, self.d), F32)
        for k in range(int(rank.max()) + 1 if rank.size else 0):
            sel = rank == k
            s, e = seg_of[sel], e_all[sel]
            acc[s] = fma32(self.w[e][:, None], x[self.col[e]], acc[s])
        raw = np.zeros((self.n_rows, self.d), F32)
        whole = seg_slot < 0
        raw[np.asarray(seg_row)[whole]] = acc[whole]
        partial = np.zeros((max(plan.n_slots, 1), self.d), F32)
        partial[seg_slot[~whole]] = acc[~whole]
        long_row = plan.long_row.cpu().numpy()
        slot0 = plan.long_slot0.cpu().numpy()
        for i in range(plan.n_long):
            waves = []
            for wv in range(4):
                t = np.zeros(self.d, F32)
                for s in range(slot0[i] + wv, slot0[i + 1], 4):
                    t = t + partial[s]
                waves.append(t)
            raw[long_row[i]] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
        return raw

    def oracle(self, keep, scale, x=None):
        return O.spmm_csr(self.rowptr, self.col, self.w, self.x if x is None else x, keep=keep, scale=scale)


def _row_end_offsets(c):
    """Local offsets (from the partition's first non-zero) at which the non-empty rows of whole-row partitions end, as
    (offset, partition length) pairs: what decides whether a flush meets a 16-gather batch or a 64-non-zero block boundary."""
    out = []
    for a, b, rowinfo, slot in c.g.plan.desc_host.tolist():
        if slot >= 0:
            continue
        row0, nrows = rowinfo & 0xFFFFFFFF, rowinfo >> 32
        for r in range(row0, row0 + nrows):
            if c.rowptr[r + 1] > c.rowptr[r]:
                out.append((int(c.rowptr[r + 1] - a), int(b - a)))
    return out


def _bits_equal(got_t, want, what):
    got = got_t.cpu().numpy()
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} words differ, first at {np.argwhere(~same)[0]}"


def _epilogue(raw, val_scale, acc_in, acc_in2, s2, acc_scale):
    y = raw * F32(val_scale)
    prev = np.zeros_like(y) if acc_in is None else acc_in
    if acc_in2 is not None:
        prev = fma32(acc_in2, F32(s2), prev)
    return y, (prev + y) * F32(acc_scale)


def _near_oracle(got_t, ref, extra=0.0):
    np.testing.assert_allclose(got_t.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * max(np.abs(ref).max(), extra, 1e-30))


KINDS = ["composite", "deg1_64", "deg1_many", "all_empty"]


@pytest.mark.parametrize("has_val", [True, False], ids=["val", "ones"])
@pytest.mark.parametrize("d", [64, 48, 128])
@pytest.mark.parametrize("L", [64, 512])
@pytest.mark.parametrize("kind", KINDS)
def test_order_is_pinned(kind, L, d, has_val):
    from recommendation_amd import functional as Fn
    c = _Case(kind, L, d, has_val)
    dev = lambda a: torch.from_numpy(a).cuda()
    empty = lambda: torch.full((c.n_rows, d), float("nan"), device="cuda")
    if kind == "composite":
        # the plan, not the degree list, decides where a row ends: the cases named above must really be in it
        ends = _row_end_offsets(c)
        assert any(o % 16 == 0 and o % 64 != 0 and o < n for o, n in ends), "no row end on an interior batch boundary"
        assert any(o % 64 == 0 for o, n in ends), "no row end on a block boundary"
        assert any(o % 16 == 1 and o < n for o, n in ends) and any(o % 16 == 15 for o, n in ends)   # one past / one short
        assert any(o == n and n == L for o, n in ends), "no row ending at the last non-zero of a full partition"
        if L > 64:
            assert any(o % 64 == 0 and o < n for o, n in ends), "no row end on an interior block boundary"
    all_keep = np.ones(c.nnz, bool)
    raw = c.replay(all_keep)
    ref64 = c.oracle(None, 1.0)
    a_in, a_in2 = dev(c.acc_in), dev(c.acc_in2)

    # -- epilogue variants, no mask ---------------------------------------------------------------------------------
    y = empty()
    Fn.spmm_into(c.g, c.xt, y=y)                                                        # y only
    _bits_equal(y, _epilogue(raw, 1.0, None, None, 0, 1.0)[0], "y only")
    _near_oracle(y, ref64)
    out = empty()
    Fn.spmm_into(c.g, c.xt, acc_in=a_in, acc_out=out)                                   # acc_out only (the Horner layer)
    _bits_equal(out, _epilogue(raw, 1.0, c.acc_in, None, 0, 1.0)[1], "acc_out only")
    _near_oracle(out, c.acc_in + ref64, np.abs(c.acc_in).max())
    y, out = empty(), empty()
    Fn.spmm_into(c.g, c.xt, y=y, acc_in=a_in, acc_out=out, acc_scale=0.25, val_scale=1.0 / 0.65)   # y + acc_out, both scales
    ey, eo = _epilogue(raw, 1.0 / 0.65, c.acc_in, None, 0, 0.25)
    _bits_equal(y, ey, "y of y + acc_out")
    _bits_equal(out, eo, "acc_out of y + acc_out")
    _near_oracle(y, ref64 / 0.65)
    inplace = a_in.clone()
    Fn.spmm_into(c.g, c.xt, acc_in=inplace, acc_out=inplace, acc_scale=0.5)             # in place
    _bits_equal(inplace, _epilogue(raw, 1.0, c.acc_in, None, 0, 0.5)[1], "in place")
    out = empty()
    Fn.spmm_into(c.g, c.xt, acc_in=None, acc_out=out, acc_scale=3.0, val_scale=0.7)     # acc_in = None
    _bits_equal(out, _epilogue(raw, 0.7, None, None, 0, 3.0)[1], "acc_in None")
    y, out = empty(), empty()
    Fn.spmm_into(c.g, c.xt, y=y, acc_in=a_in, acc_in2=a_in2, acc_in2_scale=1.0 / 3.0, acc_out=out, acc_scale=0.25)   # second addend
    ey, eo = _epilogue(raw, 1.0, c.acc_in, c.acc_in2, 1.0 / 3.0, 0.25)
    _bits_equal(y, ey, "y with acc_in2")
    _bits_equal(out, eo, "acc_out with acc_in2")
    _near_oracle(out, (c.acc_in + c.acc_in2 / 3.0 + ref64) * 0.25, np.abs(c.acc_in).max())
    inplace = a_in.clone()
    Fn.spmm_into(c.g, c.xt, acc_in=inplace, acc_in2=a_in2, acc_in2_scale=-2.0, acc_out=inplace)    # second addend, in place
    _bits_equal(inplace, _epilogue(raw, 1.0, c.acc_in, c.acc_in2, -2.0, 1.0)[1], "in place with acc_in2")
    # row normalise: tolerance only (wave reduction + division), the stress test's bounds
    inv = torch.empty(c.n_rows, device="cuda")
    y = empty()
    Fn.spmm_into(c.g, c.xt, y=y, l2norm=True, inv_norm_out=inv)
    nrm = np.sqrt((ref64 ** 2).sum(1))
    big = nrm > 1e-6 * max(nrm.max(), 1e-30)
    np.testing.assert_allclose(y.cpu().numpy()[big], (ref64 / np.maximum(nrm, 1e-12)[:, None])[big], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(inv.cpu().numpy()[big], 1.0 / nrm[big], rtol=1e-4)

    if c.nnz == 0:
        return
    # -- masks (y + acc_out, in the Horner layer's form) ---------------------------------------------------------------
    desc = c.g.plan.desc_host
    block = np.ones(c.nnz, bool)
    for p, (a, b, _, _) in enumerate(desc.tolist()):               # whole 64-blocks cleared, row ends inside them
        if p % 3 == 1:
            block[a:min(a + 64, b)] = False
        elif p % 3 == 2 and b - a > 64:
            block[a + 64:min(a + 128, b)] = False
    masks = {"p=0.35": c.rng.random(c.nnz) >= 0.35, "cleared blocks": block, "all clear": np.zeros(c.nnz, bool)}
    for name, keep in masks.items():
        bits = Fn.pack_bits(dev(keep))
        y, out = empty(), empty()
        Fn.spmm_into(c.g, c.xt, y=y, acc_in=a_in, acc_out=out, keep_bits=bits, val_scale=1.0 / 0.65)
        ey, eo = _epilogue(c.replay(keep), 1.0 / 0.65, c.acc_in, None, 0, 1.0)
        _bits_equal(y, ey, f"y, mask {name}")
        _bits_equal(out, eo, f"acc_out, mask {name}")
        _near_oracle(y, c.oracle(keep, 1.0 / 0.65))
    # column bitmap: x is zero outside a handful of rows, their non-zeros are skipped before the gather
    active = np.sort(c.rng.choice(N_COLS, 9, replace=False))
    xs = np.zeros_like(c.x)
    xs[active] = c.x[active]
    cbits = Fn.active_rows_bitmap(dev(active.astype(np.int64)), N_COLS)
    keep = np.isin(c.col, active)
    out = empty()
    Fn.spmm_into(c.g, dev(xs), acc_in=a_in, acc_out=out, acc_scale=0.25, col_active_bits=cbits)
    _bits_equal(out, _epilogue(c.replay(keep, xs), 1.0, c.acc_in, None, 0, 0.25)[1], "col_active_bits")
    _near_oracle(out, (c.acc_in + c.oracle(None, 1.0, xs)) * 0.25, np.abs(c.acc_in).max())


@pytest.mark.parametrize("combine", ["mean", "sum"])
def test_propagate_twice_is_bitwise_equal(combine):
    import recommendation_amd as ra
    from recommendation_amd import functional as Fn
    n_u, n_i, k, d = 300, 200, 3, 64
    u, i = O.synthetic_interactions(n_u, n_i, 4000, seed=5)
    g = ra.CsrGraph.bipartite_sym_norm(u, i, n_u, n_i, "cuda")
    x0 = torch.randn(n_u + n_i, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    with torch.no_grad():
        a = Fn.lightgcn_propagate(g, x0, k, combine=combine)
        b = Fn.lightgcn_propagate(g, x0, k, combine=combine)
        fa, la = Fn.lightgcn_propagate(g, x0, k, combine=combine, return_layers=True)
        fb, lb = Fn.lightgcn_propagate(g, x0, k, combine=combine, return_layers=True)
    assert torch.equal(a, b) and torch.equal(fa, fb) and all(torch.equal(p, q) for p, q in zip(la, lb))
    rowptr, col, val = O.norm_adj_csr(u, i, n_u, n_i)
    ref, _ = O.lgcn_encoder_forward(rowptr, col, val, x0.cpu().numpy(), k, combine=combine)
    for got in (a, fa):
        assert np.abs(got.cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
