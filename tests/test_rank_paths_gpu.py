"""Full-ranking evaluation (csrc/gcr_rank.hip, evaluate.py) on the launch shapes, branches and contracts that
tests/test_evaluate.py never reaches, each at the smallest shape that gets there.

Every ranking is judged by tests/rank_rules.py: `check_topk`'s bound for standard-normal embeddings (float64 scores,
eps from the CPU's own float32 drift, no share of rows or positions exempt) and equality with a stable argsort for
`integer_case` embeddings, whose scores are exact in any float32 order.  Where a case is built so that a row stays on the
fused path or leaves it, gcr_rank_fused_f32 is called as evaluate.py calls it and `status` is asserted first.
gcr_rank_metrics is compared with a plain float64 loop over the header's definition.

Nothing at module level touches a device."""
import functools

import numpy as np
import pytest
import torch

import rank_rules as R
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("integer", "normal")


def cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def embeddings(kind, rng, n_u, n_i, d):
    if kind == "integer":
        return R.integer_case(rng, n_u, n_i, d)
    return rng.standard_normal((n_u, d)).astype(np.float32), rng.standard_normal((n_i, d)).astype(np.float32)


def csr(train, n_u):
    if train is None:
        return None, None
    rowptr, items = R.train_csr(train, n_u)
    return cuda(rowptr), cuda(items)


def rank(ue, ie, uids, train, k, **kw):
    from recommendation_amd.evaluate import rank_topk
    rp, it = csr(train, ue.shape[0])
    gi, gs = rank_topk(cuda(ue), cuda(ie), np.asarray(uids, dtype=np.int64), rp, it, k, **kw)
    assert gi.shape == (len(uids), k) and gi.dtype == torch.int64 and gs.dtype == torch.float32
    return gi.cpu().numpy(), gs.cpu().numpy()


def judge(kind, gi, gs, ue, ie, uids, train, k, tag):
    if kind == "integer":
        R.check_rows_exact(gi, gs, ue, ie, uids, train, k, f"{tag}_integer")
    else:
        R.check_rows(gi, gs, ue, ie, uids, train, k, f"{tag}_normal")


def fused_raw(ue, ie, uids, train, k):
    """gcr_rank_fused_f32 as evaluate.rank_topk issues it (one call, no fallback) -> (items, scores, status)."""
    from recommendation_amd import _lib
    n_u, d = ue.shape
    assert _lib.call("gcr_rank_fused_supported", ie.shape[0], d, k)
    q = n_u if uids is None else len(uids)
    uet, iet, ids = cuda(ue), cuda(ie), None if uids is None else cuda(np.asarray(uids, dtype=np.int64))
    rp, it = csr(train, n_u)
    ws = _lib.workspace("gcr_rank_fused_workspace_bytes", q, device=uet.device, dtype=torch.uint8)
    top_i = torch.full((q, k), -7, dtype=torch.int64, device=DEV)
    top_s = torch.full((q, k), 7.0, dtype=torch.float32, device=DEV)
    status = torch.full((q,), 7, dtype=torch.int32, device=DEV)
    _lib.call("gcr_rank_fused_f32", uet, ids, q, n_u, iet, ie.shape[0], d, rp, it, k, top_i, top_s, status, ws, on=uet)
    return top_i.cpu().numpy(), top_s.cpu().numpy(), status.cpu().numpy()


def two_call_raw(ue, ie, uids, train, k):
    """gcr_score_rows_f32 + gcr_topk_masked_f32 as evaluate._rank_two_call issues them, in one chunk."""
    from recommendation_amd import _lib
    n_u, d = ue.shape
    q = n_u if uids is None else len(uids)
    uet, iet, ids = cuda(ue), cuda(ie), None if uids is None else cuda(np.asarray(uids, dtype=np.int64))
    rp, it = csr(train, n_u)
    scores = torch.empty(q, ie.shape[0], dtype=torch.float32, device=DEV)
    top_i = torch.full((q, k), -7, dtype=torch.int64, device=DEV)
    top_s = torch.full((q, k), 7.0, dtype=torch.float32, device=DEV)
    _lib.call("gcr_score_rows_f32", uet, ids, q, n_u, iet, ie.shape[0], d, scores, on=uet)
    _lib.call("gcr_topk_masked_f32", scores, q, ie.shape[0], ids, n_u, rp, it, k, top_i, top_s, on=uet)
    return top_i.cpu().numpy(), top_s.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------
# two-call path (n_items < 16384)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [256, 200, 100, 48])
@pytest.mark.parametrize("n_u, n_i, k", [(70, 129, 20), (33, 1000, 256)])
def test_two_call_width_256_and_padded_widths(n_u, n_i, k, d, kind):
    """score_rows_kernel<256> (one item tile per wave, 128 items per block: 129 items leave a block with one item) and
    the widths `_pad_dim` widens: 200 -> 256, 100 -> 128, 48 -> 64."""
    rng = np.random.default_rng(7 * d + n_i)
    ue, ie = embeddings(kind, rng, n_u, n_i, d)
    train = R.random_train(rng, n_u, n_i, 25)
    uids = rng.permutation(n_u)
    gi, gs = rank(ue, ie, uids, train, k, chunk_bytes=4 * n_i * 31)            # chunks of 31 rows, a ragged last one
    judge(kind, gi, gs, ue, ie, uids, train, k, f"two_call_{n_u}x{n_i}_d{d}_k{k}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_i, k", [(300, 256), (200, 256), (300, 1)])
def test_two_call_largest_and_smallest_k(n_i, k, kind):
    """k = 256 (kMaxK: the gather and the bitonic sort fill their buffers), k = 256 on 200 items (56 slots of tail
    beyond the catalogue on top of the masked items), and k = 1."""
    rng = np.random.default_rng(n_i + k)
    ue, ie = embeddings(kind, rng, 20, n_i, 64)
    train = R.random_train(rng, 20, n_i, 12)
    uids = np.arange(20)
    gi, gs = rank(ue, ie, uids, train, k)
    judge(kind, gi, gs, ue, ie, uids, train, k, f"two_call_20x{n_i}_d64_k{k}")
    if k > n_i:
        assert (gi[:, n_i - 12:] == -1).all() and (gi[:, :n_i - 12] >= 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_fewer_than_k_eligible_items_are_padded(kind):
    """include/gcr.h: "rows with fewer than k finite items are padded with (-1, -inf)".  User 0 has 30 of the 40 items
    in training (10 real entries + 10 padding), user 1 all 40 (all padding), user 2 none (20 real).  Before the
    write-out compared the selected score with -inf, the masked training items came back as ids with score -inf."""
    rng = np.random.default_rng(40)
    ue, ie = embeddings(kind, rng, 3, 40, 64)
    train = {0: np.sort(rng.choice(40, 30, replace=False)), 1: np.arange(40), 2: np.zeros(0, dtype=np.int64)}
    gi, gs = rank(ue, ie, [0, 1, 2, 1, 0], train, 20)
    real = (gi >= 0).sum(1).tolist()
    print(f"RANKPIN fewer_than_k_{kind} real entries per row = {real}")
    assert real == [10, 0, 20, 0, 10], (real, gi)
    assert (gi[0, 10:] == -1).all() and (gs[0, 10:] == -np.inf).all() and (gi[1] == -1).all() and (gs[1] == -np.inf).all()
    judge(kind, gi, gs, ue, ie, [0, 1, 2, 1, 0], train, 20, "fewer_than_k")


@pytest.mark.parametrize("kind", KINDS)
def test_two_call_grid_stride_second_trip(kind):
    """topk_masked_kernel launches at most 65536 blocks: 65536 + 77 query rows (50 users in a cycle, one chunk at the
    default chunk_bytes) send 77 blocks round their loop a second time.  The first 50 rows are judged by the rule; every
    other row, those of the second trip included, must equal the first row of its user bit for bit."""
    n_u, n_i, d, k, q = 50, 40, 32, 10, 65536 + 77
    rng = np.random.default_rng(65536)
    ue, ie = embeddings(kind, rng, n_u, n_i, d)
    train = R.random_train(rng, n_u, n_i, 8)
    uids = np.arange(q) % n_u
    gi, gs = rank(ue, ie, uids, train, k)
    judge(kind, gi[:n_u], gs[:n_u], ue, ie, uids[:n_u], train, k, "grid_stride_first_rows")
    assert np.array_equal(gi, gi[:n_u][uids]), np.nonzero((gi != gi[:n_u][uids]).any(1))[0][:10]
    assert np.array_equal(gs.view(np.uint32), gs[:n_u][uids].view(np.uint32))
    assert np.array_equal(gi[65536:], gi[uids[65536:]]) and (gi[65536:] >= 0).all()


NSPLIT_ROWS = (0, 31, 32, 63, 64, 1055, 1056, 2047, 2048, 2098, 2099)


@pytest.mark.parametrize("kind", KINDS)
def test_two_call_second_nsplit_rule(kind):
    """launch_score's second rule: 32768 + 129 items at d = 256 are 258 item blocks (> 256), and 2100 query rows are 66
    query tiles, so nsplit = ceil(66 / 64) = 2 with 33 tiles each; the last item block holds one item, the last query tile
    20 rows, and n_items % 4 == 1 takes the candidate filter's scalar loop.  All rows: the structural items of the rule
    and bit equality with the first row of the same user; the float64 items on the rows at the tile and split edges."""
    n_u, n_i, d, k, q = 300, 32768 + 129, 256, 50, 2100
    rng = np.random.default_rng(258)
    ue, ie = embeddings(kind, rng, n_u, n_i, d)
    train = R.random_train(rng, n_u, n_i, 20)
    uids = np.arange(q) % n_u
    gi, gs = rank(ue, ie, uids, train, k)                                       # one chunk: a 276 MB score buffer
    for r in range(q):
        assert R.check_structure(gi[r], gs[r], n_i, train[int(uids[r])], k) == k
    assert np.array_equal(gi, gi[:n_u][uids]) and np.array_equal(gs.view(np.uint32), gs[:n_u][uids].view(np.uint32))
    rows = list(NSPLIT_ROWS)
    if kind == "integer":
        R.check_rows_exact(gi[rows], gs[rows], ue, ie, uids[rows], train, k, "nsplit2_edge_rows_integer")
    else:
        R.check_rows(gi, gs, ue, ie, uids, train, k, "nsplit2_edge_rows_normal", rows=rows)


# ------------------------------------------------------------------------------------------------------------
# fused path (n_items >= 16384)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k, d", [(1, 32), (50, 64), (256, 128)])
@pytest.mark.parametrize("n_i", [16384, 16383])
def test_catalogue_edge_16384_and_16383(n_i, k, d, kind):
    """16384 items is the first catalogue gcr_rank_fused_supported accepts (and the first row length at which
    topk_masked_kernel filters by a prefix threshold); 16383 is the longest row of the full radix select."""
    from recommendation_amd import _lib
    assert bool(_lib.call("gcr_rank_fused_supported", n_i, d, k)) == (n_i == 16384)
    n_u = 64
    rng = np.random.default_rng(n_i + k)
    ue, ie = embeddings(kind, rng, n_u, n_i, d)
    train = R.random_train(rng, n_u, n_i, 40)
    uids = rng.permutation(n_u)[:48]
    gi, gs = rank(ue, ie, uids, train, k)
    judge(kind, gi, gs, ue, ie, uids, train, k, f"edge_{n_i}_d{d}_k{k}")


@pytest.mark.parametrize("kind", KINDS)
def test_fused_chunk_loop_with_a_ragged_last_chunk(kind, monkeypatch):
    """rank_topk's loop over FUSED_CHUNK_USERS: 100 queries in chunks of 37 (37 + 37 + 26) reuse one workspace and write
    slices of `status`; the result must be the one-chunk result bit for bit."""
    from recommendation_amd import evaluate
    n_u, n_i, d, k = 80, 20000, 64, 50
    rng = np.random.default_rng(37)
    ue, ie = embeddings(kind, rng, n_u, n_i, d)
    train = R.random_train(rng, n_u, n_i, 30)
    uids = rng.integers(0, n_u, 100)
    whole_i, whole_s = rank(ue, ie, uids, train, k)
    monkeypatch.setattr(evaluate, "FUSED_CHUNK_USERS", 37)
    gi, gs = rank(ue, ie, uids, train, k)
    assert np.array_equal(gi, whole_i) and np.array_equal(gs.view(np.uint32), whole_s.view(np.uint32))
    judge(kind, gi, gs, ue, ie, uids, train, k, "fused_chunks_of_37")


@pytest.mark.parametrize("kind", KINDS)
def test_fused_training_rows_around_the_lds_staging_limit(kind):
    """rank_finish_kernel stages a training row of up to 2048 items in LDS and searches longer ones in global memory:
    users with 2048, 2049 and 5000 training items.  Half of each user's true top-100 is in training, so masked candidates
    reach the search (the rest of the row is drawn from the lower half of the user's scores, which keeps the sample's
    threshold high and the candidate list short): the rows must stay on the fused path."""
    n_i, d, k = 20000, 64, 50
    rng = np.random.default_rng(2048)
    ue, ie = embeddings(kind, rng, 3, n_i, d)
    s64 = ue.astype(np.float64) @ ie.astype(np.float64).T
    train = {}
    for u, n_train in enumerate((2048, 2049, 5000)):
        order = np.argsort(-s64[u], kind="stable")
        top = rng.choice(order[:100], 50, replace=False)
        low = rng.choice(order[n_i // 2:], n_train - 50, replace=False)
        train[u] = np.sort(np.concatenate([top, low]))
        assert len(np.unique(train[u])) == n_train
    gi, gs, status = fused_raw(ue, ie, [0, 1, 2], train, k)
    assert status.tolist() == [0, 0, 0], status
    judge(kind, gi, gs, ue, ie, [0, 1, 2], train, k, "fused_n_train_2048_2049_5000")
    for u in range(3):                                     # the masked half of the top-100 is really missing
        assert not set(gi[u].tolist()) & set(train[u].tolist())


def test_fused_without_training_rows_and_without_user_ids():
    """user_rowptr = user_items_sorted = NULL on the fused entry, and user_ids = NULL (query q is user q) on both raw
    entries."""
    n_u, n_i, d, k = 70, 20000, 32, 50
    rng = np.random.default_rng(70)
    ue, ie = embeddings("normal", rng, n_u, n_i, d)
    uids = rng.permutation(n_u)[:40]
    gi, gs, status = fused_raw(ue, ie, uids, None, k)
    assert not status.any(), status
    R.check_rows(gi, gs, ue, ie, uids, None, k, "fused_no_training_rows")
    train = R.random_train(rng, n_u, n_i, 30)
    gi, gs, status = fused_raw(ue, ie, None, train, k)
    assert not status.any(), status
    R.check_rows(gi, gs, ue, ie, np.arange(n_u), train, k, "fused_no_user_ids")
    ue2, ie2 = embeddings("normal", rng, n_u, 1000, d)
    train2 = R.random_train(rng, n_u, 1000, 30)
    gi, gs = two_call_raw(ue2, ie2, None, train2, k)
    R.check_rows(gi, gs, ue2, ie2, np.arange(n_u), train2, k, "two_call_no_user_ids")
    ui, ei = R.integer_case(rng, n_u, 1000, d)
    gi, gs = two_call_raw(ui, ei, None, train2, k)
    R.check_rows_exact(gi, gs, ui, ei, np.arange(n_u), train2, k, "two_call_no_user_ids_integer")


def test_fused_designed_overflow_reports_status_1():
    """Scores ascending in item id make the 4096-item sample the row's minimum: every item passes the threshold, the
    candidate regions overflow and the row must ask for the fallback; the mirrored user (scores descending) has all its
    winners in the sample and stays.  Through rank_topk both rows are exact."""
    n_i, d, k = 30000, 64, 50
    rng = np.random.default_rng(1)
    ie = np.zeros((n_i, d), dtype=np.float32)
    ie[:, 0] = np.sort(rng.standard_normal(n_i).astype(np.float32))
    ue = np.zeros((2, d), dtype=np.float32)
    ue[0, 0], ue[1, 0] = 1.0, -1.0
    train = R.random_train(rng, 2, n_i, 30)
    gi, gs, status = fused_raw(ue, ie, [0, 1], train, k)
    assert status.tolist() == [1, 0], status
    R.check_rows(gi, gs, ue, ie, [0, 1], train, k, "fused_overflow_row_that_stayed", rows=[1])
    gi, gs = rank(ue, ie, [0, 1], train, k)
    R.check_rows(gi, gs, ue, ie, [0, 1], train, k, "fused_overflow_through_fallback")


# ------------------------------------------------------------------------------------------------------------
# invalid user ids
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_i, d", [(300, 64), (20000, 64)])
def test_user_ids_outside_the_table_get_padding_rows(n_i, d):
    """include/gcr.h: a query whose user id is outside [0, n_users) gets an all-padding row; the valid rows beside it are
    what they are without it.  Small catalogue: the two-call path; 20000 items: the fused path, where the row is final
    (status 0) without a fallback."""
    n_u, k = 10, 10
    rng = np.random.default_rng(n_i)
    ue, ie = embeddings("normal", rng, n_u, n_i, d)
    train = R.random_train(rng, n_u, n_i, 20)
    uids = [3, n_u, -1, 5, 2 ** 40, -2 ** 40]
    gi, gs = rank(ue, ie, uids, train, k)
    print(f"RANKPIN invalid_ids_{n_i} rows of ids {uids}: items[:, :3] = {gi[:, :3].tolist()}")
    for r in (1, 2, 4, 5):
        assert (gi[r] == -1).all() and (gs[r] == -np.inf).all(), (r, gi[r], gs[r])
    ok_i, ok_s = rank(ue, ie, [3, 5], train, k)
    assert np.array_equal(gi[[0, 3]], ok_i) and np.array_equal(gs[[0, 3]].view(np.uint32), ok_s.view(np.uint32))
    R.check_rows(gi, gs, ue, ie, uids, train, k, f"invalid_ids_{n_i}_valid_rows", rows=[0, 3])
    if n_i >= 16384:
        fi, fs, status = fused_raw(ue, ie, uids, train, k)
        assert status.tolist() == [0] * 6, status
        assert np.array_equal(fi, gi) and np.array_equal(fs.view(np.uint32), gs.view(np.uint32))
    else:
        ti, ts = two_call_raw(ue, ie, uids, train, k)
        assert np.array_equal(ti, gi) and np.array_equal(ts.view(np.uint32), gs.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------
# gcr_rank_metrics against a float64 loop
# ------------------------------------------------------------------------------------------------------------
def cutoff_sets(k):
    return [[1], [5, 10, 20], [k], [k, k + 30], [10, 10], list(range(1, 321, 5))]          # the last: 64 distinct cut-offs


@functools.lru_cache(maxsize=None)
def metrics_case(n_query, k):
    """Ranked lists with duplicates and tail padding, test rows of 0, 1, k and k + 7 items, and the per-position prefix
    sums of the header's definition in float64 (hits on sets, a gain at every hit position, -1 never hits)."""
    rng = np.random.default_rng(1000 * n_query + k)
    n_names = 2 * k + 20
    top = rng.integers(0, n_names, (n_query, k)).astype(np.int64)                          # few names: repeats are common
    for r in range(0, n_query, 3):
        top[r, rng.integers(0, k + 1):] = -1
    lens = np.array([(0, 1, k, k + 7)[r % 4] for r in range(n_query)])
    tests = [np.sort(rng.choice(n_names, n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    test_items = np.concatenate(tests).astype(np.int32)
    hits = np.zeros((n_query, k + 1), dtype=np.int64)
    dcg = np.zeros((n_query, k + 1), dtype=np.float64)
    repeated_hits = 0
    for r in range(n_query):
        wanted, seen, h, d = set(tests[r].tolist()), set(), 0, 0.0
        for p, it in enumerate(top[r].tolist()):
            if it >= 0 and it in wanted:
                d += 1.0 / np.log2(p + 2.0)
                if it not in seen:
                    seen.add(it)
                    h += 1
                else:
                    repeated_hits += 1
            hits[r, p + 1], dcg[r, p + 1] = h, d
    assert repeated_hits > 0 or k == 1                      # the set rule and the per-position gain really differ
    return top, rowptr, test_items, lens, hits, dcg


@pytest.mark.parametrize("n_query, k", [(1, 1), (257, 20), (1000, 256)])
def test_rank_metrics_match_a_float64_loop(n_query, k):
    """hits exactly; dcg and idcg within 1e-12 relative: at most 256 double terms, each gain within 2 ulp of the loop's
    (a division and a log2), give 256 * 2 * 2.2e-16 = 1.1e-13.  257 and 1000 query rows: a second block of 256 threads
    with one row, and four blocks with a ragged last one.  Cut-offs above k see the whole list and the longer ideal."""
    from recommendation_amd.evaluate import rank_metric_terms
    top, rowptr, test_items, lens, ref_hits, ref_dcg = metrics_case(n_query, k)
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(400) + 2.0))])
    top_d = cuda(top)
    worst = 0.0
    for cuts in cutoff_sets(k):
        cut, hits, dcg, idcg = rank_metric_terms(top_d, rowptr, test_items, cuts)
        assert cut.tolist() == sorted(cuts)
        hits, dcg, idcg = hits.cpu().numpy(), dcg.cpu().numpy(), idcg.cpu().numpy()
        for c, n in enumerate(sorted(cuts)):
            assert np.array_equal(hits[:, c], ref_hits[:, min(n, k)]), (cuts, n)
            want_d, want_i = ref_dcg[:, min(n, k)], ideal[np.minimum(lens, n)]
            assert ((dcg[:, c] == 0) == (want_d == 0)).all() and ((idcg[:, c] == 0) == (want_i == 0)).all()
            err = max(float(np.abs(dcg[:, c] - want_d).max() / max(want_d.max(), 1e-300)),
                      float(np.abs(idcg[:, c] - want_i).max() / max(want_i.max(), 1e-300)))
            worst = max(worst, err)
            assert np.all(np.abs(dcg[:, c] - want_d) <= 1e-12 * np.abs(want_d)), (cuts, n)
            assert np.all(np.abs(idcg[:, c] - want_i) <= 1e-12 * np.abs(want_i)), (cuts, n)
    print(f"RANKPIN metrics_q{n_query}_k{k} worst relative error {worst:.3e} bound 1e-12 ratio={worst / 1e-12:.3f}")


def test_rank_metrics_refuses_65_cutoffs_and_k_0():
    from recommendation_amd import _lib
    from recommendation_amd.evaluate import rank_metric_terms
    top, rowptr, test_items = metrics_case(257, 20)[:3]
    rank_metric_terms(cuda(top), rowptr, test_items, range(1, 65))
    with pytest.raises(_lib.GcrError):
        rank_metric_terms(cuda(top), rowptr, test_items, range(1, 66))
    with pytest.raises(_lib.GcrError):
        rank_metric_terms(cuda(top[:, :0]), rowptr, test_items, [1])


def test_ranking_evaluation_matches_the_oracle_report_on_random_dictionaries():
    """300 users with string names: lists shorter than the cut-off, users of `origin` that were never ranked (they count
    in the Hit Ratio's denominator only), repeated items in a list.  A ranked user that `origin` does not know makes the
    reference's own report raise (its NDCG loop indexes origin[u], ncl.py:158-159), and so the oracle; the package
    leaves that user out, and its lines are those of the report without the user."""
    from recommendation_amd.evaluate import ranking_evaluation
    rng = np.random.default_rng(300)
    names = [f"i{j}" for j in range(400)]
    origin, res = {}, {}
    for u in range(300):
        origin[f"u{u}"] = {names[j]: 1 for j in rng.choice(400, int(rng.integers(1, 40)), replace=False)}
        if u % 7 == 3:
            continue                                                             # in origin, never ranked
        n = int(rng.integers(0, 60)) if u % 5 == 0 else 60                       # some lists end before the cut-off
        res[f"u{u}"] = [(names[j], float(60 - p)) for p, j in enumerate(rng.integers(0, 400, n))]
    cuts = [10, 20, 50, 80]
    got = ranking_evaluation(origin, res, cuts)
    assert got == O.ranking_report(origin, res, cuts)
    assert len(got) == 5 * len(cuts) and got[0] == "Top 10\n"
    stray = dict(res)
    stray["nobody"] = [(names[j], 1.0) for j in range(30)]
    with pytest.raises(KeyError):
        O.ranking_report(origin, stray, cuts)
    assert ranking_evaluation(origin, stray, cuts) == got
