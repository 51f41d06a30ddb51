"""One rule for "this is a correct masked top-k", shared by tests/test_rank_rules_cpu.py (the rule against a second
float32 summation order and against mutations), tests/test_rank_paths_gpu.py and tests/test_evaluate.py.

`check_topk` judges one query row from the float32 inputs alone.  With s64 the float64 scores of the row and s32 the
same product by numpy in float32 on the CPU:

    S = max |s64|,  drift = max |s32 - s64|,  eps = max(4 * drift, 2^-20 * S),  eps <= 1e-5 * S      (tests/f64_pins.py's rule)

drift is the CPU's rounding, never measured on the code under test.  E = the items that are no training positive,
kk = min(k, |E|).  Then, with no share of rows or positions exempt:

    2  items[:kk] distinct and all in E; items[kk:] == -1; scores[kk:] == -inf
    3  |scores[p] - s64[items[p]]| <= eps                                             for p < kk
    4  min s64 over the returned items >= max s64 over the non-returned items of E - 2 * eps
       (a selector that sees every score within eps of s64 cannot prefer an item more than 2 * eps worse)
    5  s64[items[p]] >= s64[items[p + 1]] - 2 * eps; where scores[p] and scores[p + 1] are the same bits, items[p] < items[p + 1]

`integer_case` draws embeddings from {-2 .. 2}: every score is an integer of magnitude <= 4 * d <= 1024, exact in float32,
in three bf16 planes and in any summation order, so those cases compare with `exact_topk` (a stable argsort) for equality,
ties and ids included, with no tolerance.

Nothing here touches a device."""
import numpy as np

FLOOR = 2.0 ** -20
NORTH_STAR = 1e-5


def reference_scores(ue, ie, uids):
    """(s64, s32) [len(uids), n_items]: the float64 scores and numpy's float32 product of the same float32 inputs."""
    uids = np.asarray(uids, dtype=np.int64)
    s64 = ue[uids].astype(np.float64) @ ie.astype(np.float64).T
    s32 = ue[uids].astype(np.float32) @ ie.astype(np.float32).T
    assert s32.dtype == np.float32
    return s64, s32


def eligible_mask(n_items, train_items):
    m = np.ones(n_items, dtype=bool)
    if train_items is not None and len(train_items):
        m[np.asarray(train_items, dtype=np.int64)] = False
    return m


def check_structure(items, scores, n_items, train_items, k):
    """Item 2 and the part of item 5 that needs no reference: returned scores never increase, and equal bits keep
    ascending ids.  Returns kk."""
    items, scores = np.asarray(items), np.asarray(scores)
    assert items.shape == (k,) and scores.shape == (k,) and scores.dtype == np.float32
    elig = eligible_mask(n_items, train_items)
    kk = min(k, int(elig.sum()))
    head = items[:kk]
    assert ((head >= 0) & (head < n_items)).all(), ("an id outside the catalogue", head)
    assert len(np.unique(head)) == kk, "a duplicate in the list"
    assert elig[head].all(), ("a training positive in the list", head[~elig[head]])
    assert (items[kk:] == -1).all(), ("an item id in a padding slot", items[kk:])
    assert (scores[kk:] == -np.inf).all(), ("a score in a padding slot", scores[kk:])
    assert np.isfinite(scores[:kk]).all()
    assert (scores[:kk][:-1] >= scores[:kk][1:]).all(), "returned scores increase"
    bits = scores[:kk].view(np.uint32)
    tie = bits[:-1] == bits[1:]
    assert (head[:-1][tie] < head[1:][tie]).all(), "an equal-score pair in descending id order"
    return kk


def check_topk(items, scores, ue, ie, uid, train_items, k, s64=None, s32=None):
    """The rule of the module docstring for one query row.  (s64, s32): that row of `reference_scores`, when the caller
    has computed it for several rows at once.  Returns (score error, selection deficit, order deficit), each as a
    share of its bound (eps, 2 * eps, 2 * eps); a deficit of 0 means the float64 order agrees outright."""
    items, scores = np.asarray(items), np.asarray(scores)
    if s64 is None:
        s64, s32 = (x[0] for x in reference_scores(ue, ie, [uid]))
    n_items = s64.shape[0]
    S = float(np.abs(s64).max())
    drift = float(np.abs(s32.astype(np.float64) - s64).max())
    eps = max(4.0 * drift, FLOOR * S)
    assert eps <= NORTH_STAR * S, ("the float32 product itself drifts past 1e-5", eps, S)
    kk = check_structure(items, scores, n_items, train_items, k)           # item 2, and item 5's tie order
    if kk == 0:
        return 0.0, 0.0, 0.0
    head = items[:kk]
    h64 = s64[head]
    err = float(np.abs(scores[:kk].astype(np.float64) - h64).max())
    assert err <= eps, ("a returned score is off", err, eps)                # item 3
    rest = eligible_mask(n_items, train_items)
    rest[head] = False
    select = float(s64[rest].max() - h64.min()) if rest.any() else -np.inf
    assert select <= 2.0 * eps, ("a better item was left out", select, 2.0 * eps)      # item 4
    order = float((h64[1:] - h64[:-1]).max()) if kk > 1 else -np.inf
    assert order <= 2.0 * eps, ("two positions are out of order", order, 2.0 * eps)   # item 5
    unit = eps if eps > 0 else 1.0
    return err / unit, max(select, 0.0) / (2.0 * unit), max(order, 0.0) / (2.0 * unit)


def check_rows(got_items, got_scores, ue, ie, uids, train, k, tag, rows=None):
    """`check_topk` on every row (or on `rows`) of a [Q, k] result; train: {user id: training items} or a list indexed
    by user id.  Prints the worst err / eps of the case, as the BTPIN / F64PIN lines do."""
    uids = np.asarray(uids, dtype=np.int64)
    rows = list(range(len(uids))) if rows is None else list(rows)
    s64, s32 = reference_scores(ue, ie, uids[rows])
    worst = np.zeros(3)
    for n, r in enumerate(rows):
        u = int(uids[r])
        t = train.get(u) if isinstance(train, dict) else (train[u] if train is not None else None)
        try:
            worst = np.maximum(worst, check_topk(got_items[r], got_scores[r], ue, ie, u, t, k, s64=s64[n], s32=s32[n]))
        except AssertionError as e:
            raise AssertionError(f"{tag}: query row {r} (user {u}): {e}") from None
    print(f"RANKPIN {tag} rows={len(rows)} score_err/eps={worst[0]:.3f} select/2eps={worst[1]:.3f} order/2eps={worst[2]:.3f}")
    return worst


def integer_case(rng, n_u, n_i, d):
    """Embeddings from {-2 .. 2}: every score is an integer of magnitude <= 4 * d, exact in any float32 order."""
    assert 4 * d <= 1024
    return (rng.integers(-2, 3, (n_u, d)).astype(np.float32), rng.integers(-2, 3, (n_i, d)).astype(np.float32))


def exact_topk(row, train_items, k):
    """(items int64 [k], scores float32 [k]) of one exact score row: stable argsort (ties -> smaller id) over the
    eligible items, (-1, -inf) behind them."""
    elig = eligible_mask(row.shape[0], train_items)
    masked = np.where(elig, row.astype(np.float64), -np.inf)
    kk = min(k, int(elig.sum()))
    order = np.argsort(-masked, kind="stable")[:kk]
    items = np.full(k, -1, dtype=np.int64)
    scores = np.full(k, -np.inf, dtype=np.float32)
    items[:kk], scores[:kk] = order, masked[order]
    return items, scores


def check_rows_exact(got_items, got_scores, ue, ie, uids, train, k, tag):
    """Every row equals `exact_topk` of the (exact) integer scores, ids, ties and padding included."""
    uids = np.asarray(uids, dtype=np.int64)
    s64 = ue.astype(np.float64) @ ie.astype(np.float64).T
    assert (s64 == np.round(s64)).all() and np.abs(s64).max() <= 1024
    cache = {}
    for r, u in enumerate(uids.tolist()):
        if u not in cache:
            t = train.get(u) if isinstance(train, dict) else (train[u] if train is not None else None)
            cache[u] = exact_topk(s64[u], t, k)
        ref_i, ref_s = cache[u]
        assert np.array_equal(got_items[r], ref_i), (tag, r, u, got_items[r], ref_i)
        assert np.array_equal(got_scores[r], ref_s), (tag, r, u, got_scores[r], ref_s)
    print(f"RANKPIN {tag} rows={len(uids)} exact")


def train_csr(train, n_users):
    """(rowptr int64 [n_users + 1], items int32) of {user: items} / a list by user id; rows sorted ascending."""
    rows = [np.sort(np.asarray((train.get(u, []) if isinstance(train, dict) else train[u]), dtype=np.int64)) for u in range(n_users)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    items = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return rowptr, items


def random_train(rng, n_u, n_i, per_user):
    """{user: sorted training items}, `per_user` of them (capped at half the catalogue) drawn without replacement."""
    n = min(per_user, n_i // 2)
    return {u: np.sort(rng.choice(n_i, n, replace=False)) for u in range(n_u)}
