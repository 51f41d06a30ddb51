"""The one-launch windowed SpMM (gcr_spmm_windowed_f32, d <= 64) against the three entries it replaces.

A windowed launch used to be gcr_spmm_hub_parts_f32 (the companion, then its split segments), gcr_spmm_hub_reduce_f32 and
gcr_spmm_rows_f32 (the main plan, then its split rows): five kernels.  The new entry walks both plans in one grid, sums both
plans' split rows in a second and reduces the hub rows in a third.  The partitions, the order inside a partition, the order of
every partial sum and the epilogue are unchanged, so every word it writes -- y, acc_out, the hub partials and both split-row
workspaces, all NaN-filled beforehand -- must equal, as uint32, what the three entries write when called in that order; in
either order of the two block ranges, and with the main plan's descriptors permuted (graph.long_rows_first_order).

The graphs are tests/spmm_fused_common.py's: the four kinds of spmm_window_common.make_matrix, a graph of hub rows only (an
empty main range), one whose main plan has split rows as well as the companion, and one whose two partition counts are odd
(the seam between the ranges falls inside a block, and the padding to a multiple of 8 blocks is not empty)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from spmm_fused_common import CASES, build_graph, case_matrix, companion_plan
from spmm_raw import Out, assert_words_equal, nan
from spmm_window_common import F32, N_COLS

pytestmark = pytest.mark.gpu

# (y, acc_in: None | 'given' | 'inplace', acc_out, val_scale, acc_scale): the forms of
# test_spmm_window_gpu.test_windowed_order_is_pinned
FORMS = {
    "y_only": (True, None, False, 1.0, 1.0),
    "acc_out_only": (False, "given", True, 1.0, 1.0),
    "both_scaled": (True, "given", True, 1.0 / 0.65, 0.25),
    "in_place": (False, "inplace", True, 1.0, 0.5),
    "acc_in_none": (False, None, True, 0.7, 3.0),
}
CELLS = {"hub_first": (0, False), "main_first": (1, False), "hub_first_long_rows_first": (0, True),
         "main_first_long_rows_first": (1, True)}


@functools.lru_cache(maxsize=None)
def _graph(case, has_val):
    g = build_graph(case, has_val, "cuda")
    return g, companion_plan(g, case)


class _Buffers(Out):
    """One launch's outputs and workspaces, NaN-filled; acc_in is a copy the launch may overwrite (in place)."""

    def __init__(self, g, hp, main, d, form, acc_in):
        super().__init__(g.n_rows, d, FORMS[form], acc_in)
        self.part, self.h_ws, self.m_ws = nan(g.hub.H.n_rows, d), nan(hp.n_slots, d), nan(main.n_slots, d)

    def words(self):
        named = (("y", self.y), ("acc_out", self.acc_out), ("hub partials", self.part),
                 ("companion workspace", self.h_ws), ("main workspace", self.m_ws))
        return {k: t for k, t in named if t is not None}


def _old_entries(g, hp, main, xt, d, b):
    """Today's order: the companion and its split segments, the hub reduction, the main plan and its split rows."""
    from recommendation_amd import spmm_launch as L
    hub, H = g.hub, g.hub.H
    L.hub_parts(H, hp, x=xt, d=d, y=b.part, partials=b.h_ws, on=xt)
    L.hub_reduce(hub, partials=b.part, d=d, n_rows=g.n_rows, on=xt, **b.kw())
    L.rows(g, main, x=xt, d=d, partials=b.m_ws, on=xt, **b.kw())


def _new_entry(g, hp, main, xt, d, b, main_first):
    from recommendation_amd import spmm_launch as L
    L.windowed(g.hub.H, hp, g, main, g.hub, hub_split=b.h_ws, partials=b.m_ws, hub_partials=b.part, x=xt, d=d,
               main_first=main_first, on=xt, **b.kw())


@functools.lru_cache(maxsize=None)
def _inputs(case, d, has_val):
    g, _ = _graph(case, has_val)
    rng = np.random.default_rng(13 * d + int(has_val) + sum(map(ord, case)))
    x = rng.standard_normal((N_COLS, d)).astype(F32)
    acc_in = rng.standard_normal((g.n_rows, d)).astype(F32)
    return x, torch.from_numpy(x).cuda(), torch.from_numpy(acc_in).cuda()


@functools.lru_cache(maxsize=None)
def _reference(case, d, has_val):
    """form -> words of the three old entries: computed once per graph and width, shared by every cell, never written to."""
    g, hp = _graph(case, has_val)
    _, xt, a_in = _inputs(case, d, has_val)
    ref = {}
    for form in FORMS:
        b = _Buffers(g, hp, g.hub.main, d, form, a_in)
        _old_entries(g, hp, g.hub.main, xt, d, b)
        ref[form] = b.words()
    return ref


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert_words_equal(got[k], want[k], f"{what}, {k}")


def _assert_counts(case, g, hp):
    main = g.hub.main
    if case == "all_hub":
        assert g.hub.n_hub == g.n_rows and main.n_parts == 0 and main.n_long == 0
    if case in ("dup", "main_split"):
        assert hp.n_long > 0, "no split segment in the companion"
    if case == "main_split":
        assert g.hub.min_degree > main.nnz_per_part == 64 and main.n_long > 0, "no split row in the main plan"
    if case == "odd_counts":
        for plan in (hp, main):                       # the seam falls inside a block, the padding is not empty
            assert plan.n_parts % 4 != 0 and ((plan.n_parts + 3) // 4) % 8 != 0
        assert (hp.n_parts, main.n_parts) == (133, 49)


@pytest.mark.parametrize("cell", sorted(CELLS))
@pytest.mark.parametrize("has_val", [True, False], ids=["val", "ones"])
@pytest.mark.parametrize("d", [64, 48])
@pytest.mark.parametrize("case", CASES)
def test_every_word_is_the_three_entries(case, d, has_val, cell):
    from recommendation_amd.graph import long_rows_first_order
    g, hp = _graph(case, has_val)
    _assert_counts(case, g, hp)
    main_first, permute = CELLS[cell]
    main = g.hub.main
    if permute:
        order = long_rows_first_order(main.desc_host)
        if case in ("main_split", "odd_counts"):
            assert not np.array_equal(order, np.arange(main.n_parts)), "the permutation moves nothing"
        main = main.permuted(order)
    _, xt, a_in = _inputs(case, d, has_val)
    ref = _reference(case, d, has_val)
    for form in FORMS:
        assert not any(bool(torch.isnan(w).any()) for k, w in ref[form].items() if k in ("y", "acc_out", "hub partials")), \
            f"{form}: the old entries left a word unwritten"
        first = _Buffers(g, hp, main, d, form, a_in)
        _new_entry(g, hp, main, xt, d, first, main_first)
        _same(first.words(), ref[form], f"{case} {form}")
        second = _Buffers(g, hp, main, d, form, a_in)
        _new_entry(g, hp, main, xt, d, second, main_first)
        _same(second.words(), first.words(), f"{case} {form}, second launch")


@pytest.mark.parametrize("main_first", [0, 1], ids=["hub_first", "main_first"])
def test_output_matches_the_float64_oracle(main_first):
    case, d = "base", 64
    rowptr, col, val, _ = case_matrix(case)
    g, hp = _graph(case, True)
    x, xt, a_in = _inputs(case, d, True)
    ref64 = O.spmm_csr(rowptr, col, val, x, keep=None, scale=1.0)
    b = _Buffers(g, hp, g.hub.main, d, "both_scaled", a_in)
    _new_entry(g, hp, g.hub.main, xt, d, b, main_first)
    acc_in = a_in.cpu().numpy()
    yref = ref64 / 0.65
    for got, ref, extra in ((b.y, yref, 0.0), (b.acc_out, (acc_in + yref) * 0.25, np.abs(acc_in).max())):
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * max(np.abs(ref).max(), extra, 1e-30))


def test_spmm_into_takes_the_new_entry_and_wider_launches_do_not():
    from recommendation_amd import _lib
    from recommendation_amd import functional as Fn
    g, hp = _graph("dup", True)
    _, xt, a_in = _inputs("dup", 64, True)
    L = _lib.lib()
    calls = []
    real = L.gcr_spmm_windowed_f32

    def counted(*a):
        calls.append(a[23])                                          # d
        return real(*a)

    L.gcr_spmm_windowed_f32 = counted
    try:
        out = torch.full((g.n_rows, 64), float("nan"), device="cuda")
        Fn.spmm_into(g, xt, acc_in=a_in, acc_out=out)
        assert calls == [64]
        want = _reference("dup", 64, True)["acc_out_only"]
        assert_words_equal(out, want["acc_out"], "spmm_into, acc_out")
        assert_words_equal(g.hub.partials(64), want["hub partials"], "spmm_into, hub partials")
        keep = torch.full(((g.nnz + 31) // 32,), -1, dtype=torch.int32, device="cuda")
        Fn.spmm_into(g, xt, y=torch.empty(g.n_rows, 64, device="cuda"), keep_bits=keep)
        assert calls == [64], "a masked launch keeps the classic plan"
        x128 = torch.randn(N_COLS, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        Fn.spmm_into(g, x128, y=torch.empty(g.n_rows, 128, device="cuda"))
        assert calls == [64], "d > 64 keeps the generic kernels"
    finally:
        L.gcr_spmm_windowed_f32 = real
    # called directly, a wider launch is refused before anything is launched
    b = _Buffers(g, hp, g.hub.main, 128, "y_only", None)
    b.y.fill_(7.0), b.part.fill_(7.0)
    with pytest.raises(_lib.GcrError, match="code -2"):              # GCR_EUNSUPPORTED
        _new_entry(g, hp, g.hub.main, x128, 128, b, 0)
    torch.cuda.synchronize()
    assert bool((b.y == 7.0).all()) and bool((b.part == 7.0).all()), "a refused call launched something"
