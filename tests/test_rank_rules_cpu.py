"""tests/rank_rules.py judged on the CPU: the rule must accept a correct float32 ranking whose scores were summed in
another order than numpy's (8-column chunks, added left to right) on every shape the GPU cases use it at, and must
reject each way a selector goes subtly wrong."""
import functools

import numpy as np
import pytest

import rank_rules as R

# (users, items, d, k): the two-call widths, kMaxK, the catalogue edge, the second nsplit rule's catalogue, a plain one
SHAPES = [(70, 129, 256, 20), (33, 1000, 256, 256), (64, 16384, 32, 256), (40, 32897, 256, 50), (50, 5000, 64, 50)]


def chunked_f32_scores(ue, ie, uids):
    """The same product in float32 with another summation order: partial sums over 8 columns, accumulated in float32."""
    acc = np.zeros((len(uids), ie.shape[0]), dtype=np.float32)
    for c in range(0, ue.shape[1], 8):
        acc += ue[uids][:, c:c + 8] @ ie[:, c:c + 8].T
    return acc


def rank_rows(scores32, uids, train, k):
    """A correct selector on given float32 scores: training positives out, (score desc, id asc), (-1, -inf) padding."""
    out_i = np.empty((len(uids), k), dtype=np.int64)
    out_s = np.empty((len(uids), k), dtype=np.float32)
    for r, u in enumerate(uids):
        out_i[r], out_s[r] = R.exact_topk(scores32[r], train[int(u)], k)
    return out_i, out_s


@functools.lru_cache(maxsize=None)
def _case(n_u, n_i, d, k):
    rng = np.random.default_rng(1000 * d + n_i)
    ue = rng.standard_normal((n_u, d)).astype(np.float32)
    ie = rng.standard_normal((n_i, d)).astype(np.float32)
    train = R.random_train(rng, n_u, n_i, 30)
    uids = np.arange(n_u)
    items, scores = rank_rows(chunked_f32_scores(ue, ie, uids), uids, train, k)
    return ue, ie, train, uids, items, scores


@pytest.mark.parametrize("n_u, n_i, d, k", SHAPES)
def test_rule_accepts_a_second_float32_order(n_u, n_i, d, k):
    ue, ie, train, uids, items, scores = _case(n_u, n_i, d, k)
    worst = R.check_rows(items, scores, ue, ie, uids, train, k, f"cpu_chunked_{n_u}x{n_i}_d{d}_k{k}")
    # the other order sits well inside the bound (0.11 - 0.17 of eps when this was written): a rule that a correct
    # implementation only just meets would be a coin toss on the GPU
    assert worst[0] <= 0.5, worst


def _row():
    """One row of the plain shape with its accepted result and the quantities the mutations need."""
    n_u, n_i, d, k = SHAPES[-1]
    ue, ie, train, uids, items, scores = _case(n_u, n_i, d, k)
    u = 7
    s64, s32 = (x[0] for x in R.reference_scores(ue, ie, [u]))
    eps = max(4.0 * float(np.abs(s32 - s64).max()), R.FLOOR * float(np.abs(s64).max()))
    return ue, ie, u, train[u], k, items[u].copy(), scores[u].copy(), s64, eps


def test_rule_accepts_the_unmutated_row():
    ue, ie, u, t, k, items, scores, s64, eps = _row()
    R.check_topk(items, scores, ue, ie, u, t, k)


def test_rule_rejects_a_worse_item_swapped_in():
    ue, ie, u, t, k, items, scores, s64, eps = _row()
    elig = R.eligible_mask(len(s64), t)
    elig[items] = False
    worse = np.nonzero(elig & (s64 < s64[items[-1]] - 2.0 * eps))[0]
    j = worse[np.argmax(s64[worse])]                       # the best of the items that are too bad: the narrowest miss
    items[-1], scores[-1] = j, np.float32(s64[j])
    with pytest.raises(AssertionError, match="a better item was left out"):
        R.check_topk(items, scores, ue, ie, u, t, k)


def test_rule_rejects_a_training_positive():
    ue, ie, u, t, k, items, scores, s64, eps = _row()
    j = t[np.argmax(s64[t])]
    p = min(int(np.searchsorted(-s64[items], -s64[j])), k - 1)     # where it would rank: order and scores stay consistent
    items = np.concatenate([items[:p], [j], items[p:-1]])
    scores = np.concatenate([scores[:p], [np.float32(s64[j])], scores[p:-1]]).astype(np.float32)
    with pytest.raises(AssertionError, match="a training positive in the list"):
        R.check_topk(items, scores, ue, ie, u, t, k)


def test_rule_rejects_a_duplicate():
    ue, ie, u, t, k, items, scores, s64, eps = _row()
    items[4], scores[4] = items[3], scores[3]
    with pytest.raises(AssertionError, match="a duplicate in the list"):
        R.check_topk(items, scores, ue, ie, u, t, k)


def test_rule_rejects_two_positions_out_of_order():
    ue, ie, u, t, k, items, scores, s64, eps = _row()
    p = next(p for p in range(k - 1) if s64[items[p]] - s64[items[p + 1]] > 2.0 * eps)
    items[[p, p + 1]] = items[[p + 1, p]]
    with pytest.raises(AssertionError, match="a returned score is off"):      # ids swapped under sorted scores
        R.check_topk(items, scores, ue, ie, u, t, k)
    scores[[p, p + 1]] = scores[[p + 1, p]]
    # pairs swapped.  (Scores that never increase and each sit within eps of their float64 value already put two
    # neighbours within 2 * eps of the right order, so the float64 order clause cannot fire before one of these two.)
    with pytest.raises(AssertionError, match="returned scores increase"):
        R.check_topk(items, scores, ue, ie, u, t, k)


def test_rule_rejects_an_item_id_in_a_padding_slot():
    rng = np.random.default_rng(5)
    ue, ie = rng.standard_normal((3, 32)).astype(np.float32), rng.standard_normal((40, 32)).astype(np.float32)
    t = np.arange(30)                                       # 10 eligible items, k = 20
    s32 = R.reference_scores(ue, ie, [1])[1]
    items, scores = R.exact_topk(s32[0], t, 20)
    assert (items[10:] == -1).all() and (items[:10] >= 30).all()
    R.check_topk(items, scores, ue, ie, 1, t, 20)
    bad = items.copy()
    bad[10] = 4                                             # what the kernel did: a masked training item, score -inf
    with pytest.raises(AssertionError, match="an item id in a padding slot"):
        R.check_topk(bad, scores, ue, ie, 1, t, 20)
    bad_s = scores.copy()
    bad_s[10] = np.float32(0.0)
    with pytest.raises(AssertionError, match="a score in a padding slot"):
        R.check_topk(items, bad_s, ue, ie, 1, t, 20)


def test_rule_rejects_an_equal_score_pair_in_descending_id_order():
    rng = np.random.default_rng(9)
    ue, ie = R.integer_case(rng, 4, 200, 32)
    s = ue.astype(np.float64) @ ie.astype(np.float64).T
    items, scores = R.exact_topk(s[2], None, 30)
    R.check_topk(items, scores, ue, ie, 2, None, 30)
    p = next(p for p in range(29) if scores[p] == scores[p + 1])
    items[[p, p + 1]] = items[[p + 1, p]]
    with pytest.raises(AssertionError, match="an equal-score pair in descending id order"):
        R.check_topk(items, scores, ue, ie, 2, None, 30)


def test_integer_case_is_exact_in_float32_and_in_another_order():
    rng = np.random.default_rng(11)
    ue, ie = R.integer_case(rng, 9, 1000, 256)
    s64, s32 = R.reference_scores(ue, ie, np.arange(9))
    assert np.array_equal(s64, s32.astype(np.float64)) and np.abs(s64).max() <= 1024
    assert np.array_equal(chunked_f32_scores(ue, ie, np.arange(9)), s32)
    train = R.random_train(rng, 9, 1000, 30)
    items, scores = rank_rows(s32, np.arange(9), train, 256)
    R.check_rows_exact(items, scores, ue, ie, np.arange(9), train, 256, "cpu_integer")
    items[4, [10, 11]] = items[4, [11, 10]]
    with pytest.raises(AssertionError):
        R.check_rows_exact(items, scores, ue, ie, np.arange(9), train, 256, "cpu_integer_mutated")
