"""Every centroid-update path of `run_kmeans` against a float64 Lloyd step, one step at a time.

run_kmeans takes one of five code paths ("paths of run_kmeans"), each with an accumulation kernel of its own:

  A  image search + incremental 64-bit fixed-point sums (d in {32, 64}, n_train * k <= 2^28: the default)
  B  image search + float-atomic rows into private copies (A with INCREMENTAL_UPDATE off)
  C  tiled search with the accumulation fused in (d <= 128 otherwise)
  D  tiled search, then one float-atomic row per point into private copies (d = 256)
  E  tiled search, sort by cluster, one float-atomic row per run (n_train >= SORTED_UPDATE_MIN_POINTS)

A whole float64 trajectory cannot be compared (a flipped near-tie moves centroids and the run is chaotic), so every
single step is pinned instead: from the GPU's own centroids C_{t-1} the float64 distances of all points are taken, the
points whose two nearest centroids lie within a factor 1 + 1e-4 of one another are set aside (ten times the 1e-5 near-tie
allowance test_kmeans_gpu.py grants the search; never more than 1 % of the points), and ONE run_kmeans iteration over the
rest must return, per cluster, the float64 mean of its float64 arg-min members.  Which path ran is read off the libgcr
entry points the call went through.

Bounds (none of them taken from what the kernels give):
  * path A: |err| <= max|x| * 2^-28 + 2^-23 * |expected| — the sums are exact integers of q = round(x * 2^e) with
    max|x| * 2^e in [2^29, 2^30), so a mean is off by at most half a quantum 2^-e <= max|x| * 2^-29, and the quotient is
    rounded to float32 once (2^-24 relative); a factor 2 of slack on each.  run_kmeans caps e at 125 (max|x| < 2^-96): the
    quantum stays 2^-125 there, and the first term becomes 2^-125 (half a quantum, the same factor 2);
  * paths B-E (float sums): rtol = atol = 1e-5 on inputs with max|x| <= 16, the float-path bound of
    test_lloyd_iterations_match_restatement;
  * rows rewritten by the empty-cluster re-seed: rtol = 2e-6, atol = 1e-6 of test_split_step_matches_restatement_bit_for_bit
    where that is the wider of the two (one more float32 product on top of the mean).
References are torch float64 (on the host; on the device for the one case above 10^6 points) and oracle_np's split.
"""
import numpy as np
import pytest
import torch

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-4          # a point is ambiguous when d2_second < d2_best * (1 + NEAR_TIE)
MAX_EXCLUDED = 0.01      # share of the points a step may set aside
SEED = 1234

ENTRY_POINTS = ("gcr_kmeans_search_image_incr_f32", "gcr_kmeans_lloyd_update_q_f32", "gcr_kmeans_search_image_f32",
                "gcr_kmeans_assign_accumulate_f32", "gcr_kmeans_assign_f32", "gcr_kmeans_lloyd_update_f32", "gcr_sort_index",
                "gcr_kmeans_centroid_image_f32")


class EntryPointSpy:
    """Counts (and keeps the arguments of) the calls run_kmeans makes into libgcr; the real entry point still runs."""

    def __init__(self, monkeypatch):
        from recommendation_amd import _lib
        L = _lib.lib()
        self.calls = {name: [] for name in ENTRY_POINTS}
        for name in ENTRY_POINTS:
            monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))

    def _wrap(self, name, real):
        def call(*args):
            self.calls[name].append(args)
            return real(*args)
        return call

    def reset(self):
        for v in self.calls.values():
            v.clear()

    def n(self, name):
        return len(self.calls[name])

    def assert_path(self, path, copies=None):
        """The calls of ONE run_kmeans: the kernels of `path` ran and those of the other paths did not."""
        n = self.n
        # gcr_kmeans_lloyd_update_f32(x, n, d, assign, keys_sorted, perm, k, cent, half, sums, counts, n_copies, ...)
        upd = self.calls["gcr_kmeans_lloyd_update_f32"]
        if path == "A":
            assert n("gcr_kmeans_search_image_incr_f32") >= 1 and n("gcr_kmeans_lloyd_update_q_f32") >= 1
            assert not upd and not n("gcr_kmeans_search_image_f32") and not n("gcr_kmeans_assign_accumulate_f32")
            assert not n("gcr_sort_index")
            return
        assert not n("gcr_kmeans_search_image_incr_f32") and not n("gcr_kmeans_lloyd_update_q_f32")
        assert len(upd) >= 1
        for a in upd:
            if path in "BC":
                assert a[3] is None and a[4] is None and a[5] is None       # sums arrive accumulated by the search
            elif path == "D":
                assert a[3] is not None and a[4] is None and a[5] is None and a[11] > 1
            else:
                assert a[4] is not None and a[5] is not None and a[11] == 1
            if copies is not None:
                assert a[11] == copies, (a[11], copies)
        assert (n("gcr_kmeans_search_image_f32") >= 1) == (path == "B")
        assert (n("gcr_kmeans_assign_accumulate_f32") >= 1) == (path == "C")
        assert (n("gcr_sort_index") >= 1) == (path == "E")


@pytest.fixture
def spy(monkeypatch):
    return EntryPointSpy(monkeypatch)


def blob_fixture(n, k, d, blobs, spread):
    rng = np.random.default_rng(1)
    cen = rng.standard_normal((blobs, d)) * spread
    x = (cen[rng.integers(0, blobs, n)] + rng.standard_normal((n, d))).astype(np.float32)
    init = x[rng.choice(n, k, replace=False)]
    return x, init


def nearest_two(x, c, chunk=1 << 15):
    """float64 squared distances of the rows of x (float32, any device) to the rows of c: (d2_best, d2_second, ids [n, 2])."""
    c = c.to(device=x.device, dtype=torch.float64)
    cc = (c * c).sum(1)
    n = x.shape[0]
    best = torch.empty(n, dtype=torch.float64, device=x.device)
    second = torch.empty_like(best)
    ids = torch.empty(n, 2, dtype=torch.int64, device=x.device)
    for s in range(0, n, chunk):
        xs = x[s:s + chunk].double()
        d2 = ((xs * xs).sum(1, keepdim=True) - 2.0 * (xs @ c.t()) + cc[None]).clamp_min_(0.0)
        v, i = torch.topk(d2, 2, dim=1, largest=False)
        best[s:s + chunk], second[s:s + chunk], ids[s:s + chunk] = v[:, 0], v[:, 1], i
    return best, second, ids


def float64_means(x, members, k, keep_rows):
    """Per-cluster float64 mean of the rows of x (float32) listed in `members`; an empty cluster keeps `keep_rows`."""
    sums = torch.zeros(k, x.shape[1], dtype=torch.float64, device=x.device).index_add_(0, members, x.double())
    cnt = torch.bincount(members, minlength=k)
    mean = torch.where(cnt[:, None] > 0, sums / cnt.clamp_min(1)[:, None].double(), keep_rows.to(x.device).double())
    return mean.cpu().numpy(), cnt.cpu().numpy().astype(np.float64)


def fixed_point_bound(max_abs, expect):
    return max(max_abs * 2.0 ** -28, 2.0 ** -125) + 2.0 ** -23 * np.abs(expect)


def float_sum_bound(max_abs, expect):
    assert max_abs <= 16.0            # the scale the bound was stated for
    return 1e-5 + 1e-5 * np.abs(expect)


def reseed_bound(expect):
    return 1e-6 + 2e-6 * np.abs(expect)


def assert_float64_argmin(got, best, ids, x, cent, tie_rule=True):
    """test_assignment_is_exact_argmin's rule: the float64 arg-min but for float32 near-ties, where the chosen centroid must
    be as close within 1e-5."""
    agree = got == ids[:, 0]
    assert float(agree.double().mean()) > 0.999
    bad = torch.nonzero(~agree).squeeze(1)
    if bad.numel() and tie_rule:
        d2 = ((x[bad].double() - cent.to(x.device).double()[got[bad]]) ** 2).sum(1)
        assert bool((d2 <= best[bad] * (1 + 1e-5) + 1e-6).all())


def run_steps(x, init, k, steps, path, spy, bound, copies=None, dev="cpu", on_step=None, label="", tie_rule=True):
    """The step loop of the module docstring.  Returns the largest error and the largest error / bound it met."""
    from recommendation_amd import kmeans as K
    xg = torch.from_numpy(x).cuda()
    xr = xg if dev == "cuda" else torch.from_numpy(x)                # the float64 side's copy of the points
    c_prev = torch.from_numpy(init).cuda()
    best, second, ids = nearest_two(xr, c_prev)
    worst_err = worst_ratio = worst_excluded = 0.0
    moved = []
    for t in range(steps):
        amb = second < best * (1 + NEAR_TIE)
        excluded = float(amb.double().mean())
        worst_excluded = max(worst_excluded, excluded)
        assert excluded <= MAX_EXCLUDED, (t, excluded)
        keep = ~amb
        xk = xg[keep.cuda()].contiguous()
        xk_ref = xr[keep]
        members = ids[keep, 0]
        spy.reset()
        c_t, a_t, info = K.run_kmeans(xk, k, niter=1, seed=SEED, init_centroids=c_prev, max_points_per_centroid=0,
                                      return_info=True)
        spy.assert_path(path, copies)
        assert info["k"] == k and info["n_train"] == xk.shape[0] and c_t.shape == (k, x.shape[1])
        expect, cnt = float64_means(xk_ref, members, k, c_prev)
        if on_step is not None:
            on_step(t, cnt)
        plain = expect.copy()
        n_split = O.kmeans_split_clusters(expect, cnt, xk.shape[0], SEED, 0) if (cnt == 0).any() else 0
        assert int(info["n_split"]) == n_split
        reseeded = (expect != plain).any(1)
        limit = bound(float(xk.abs().max()), expect)
        limit[reseeded] = np.maximum(limit[reseeded], reseed_bound(expect[reseeded]))
        got = c_t.double().cpu().numpy()
        assert np.isfinite(got).all()
        err = np.abs(got - expect)
        worst_err, worst_ratio = max(worst_err, float(err.max())), max(worst_ratio, float((err / limit).max()))
        assert (err <= limit).all(), (label, t, float(err.max()), float((err / limit).max()))
        # the returned assignment: against the centroids just returned
        best_t, second_t, ids_t = nearest_two(xr, c_t)
        a_ref = a_t.to(xr.device)
        assert a_t.shape == (xk.shape[0],) and int(a_ref.min()) >= 0 and int(a_ref.max()) < k
        assert_float64_argmin(a_ref, best_t[keep], ids_t[keep], xk_ref, c_t, tie_rule)
        moved.append(int((ids_t[:, 0] != ids[:, 0]).sum()))
        best, second, ids, c_prev = best_t, second_t, ids_t, c_t
    print(f"[kmeans-paths] {label} path {path}: max |err| {worst_err:.3e}, max err/bound {worst_ratio:.3f}, "
          f"max excluded {worst_excluded:.4%}, points changing cluster per step {moved}")
    return worst_err, worst_ratio


# ---------------------------------------------------------------------------------------------------------------------------
# 1. stepwise float64 Lloyd, every path
# ---------------------------------------------------------------------------------------------------------------------------

#        id                (n, k, d, blobs, spread, steps)        path  module switches                          copies
STEP_CASES = [
    ("A-d64",             (8000, 24, 64, 8, 3, 10),               "A", {},                                       None),
    ("A-d64-ncl-shape",   (30000, 120, 64, 40, 2, 25),            "A", {},                                       None),
    ("A-d32",             (8000, 24, 32, 8, 3, 10),               "A", {},                                       None),
    ("A-d48-padded",      (6000, 40, 48, 10, 3, 10),              "A", {},                                       None),
    ("A-110000x300",      (110000, 300, 64, 100, 2, 6),           "A", {},                                       None),
    ("B-16-copies",       (8000, 24, 64, 8, 3, 10),               "B", {"INCREMENTAL_UPDATE": False},            16),
    ("B-1-copy",          (8000, 24, 64, 8, 3, 10),               "B", {"INCREMENTAL_UPDATE": False, "MAX_ATOMIC_COPIES": 1}, 1),
    ("C-d128",            (6000, 40, 128, 10, 3, 10),             "C", {},                                       9),
    ("C-d64-by-pairs",    (8000, 24, 64, 8, 3, 10),               "C", {"IMAGE_SEARCH_MAX_PAIRS": 1},            16),
    ("C-d100-padded",     (6000, 40, 100, 10, 3, 10),             "C", {},                                       9),
    ("D-d256",            (5000, 16, 256, 6, 3, 10),              "D", {},                                       16),
    ("D-d200-padded",     (5000, 16, 200, 6, 3, 10),              "D", {},                                       16),
]


@pytest.mark.parametrize("label,shape,path,switches,copies", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_every_step_is_a_float64_lloyd_step(label, shape, path, switches, copies, spy, monkeypatch):
    from recommendation_amd import kmeans as K
    assert K.IMAGE_SEARCH and K.INCREMENTAL_UPDATE and K.SORTED_UPDATE_MIN_POINTS == 1 << 20
    for name, value in switches.items():
        monkeypatch.setattr(K, name, value)
    n, k, d, blobs, spread, steps = shape
    x, init = blob_fixture(n, k, d, blobs, spread)
    run_steps(x, init, k, steps, path, spy, fixed_point_bound if path == "A" else float_sum_bound, copies=copies, label=label)


def test_every_step_on_the_sorted_path_forced(spy, monkeypatch):
    """Path E below its size threshold: a partial last 64-entry chunk, runs that straddle chunk boundaries, and a cluster
    that starts empty (a far-away start: it is re-seeded in step 0 exactly as oracle_np re-seeds it)."""
    from recommendation_amd import kmeans as K
    monkeypatch.setattr(K, "SORTED_UPDATE_MIN_POINTS", 1000)
    x, init = blob_fixture(8000, 24, 64, 8, 3)
    init = np.concatenate([init, np.full((1, 64), 1e3, np.float32)])
    seen = {}

    def on_step(t, cnt):
        if t == 0:
            starts = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
            seen["partial"] = int(starts[-1]) % 64 != 0
            seen["empty"] = bool((cnt == 0).any())
            # a run [start, end) with a multiple of 64 strictly inside it is split between two chunks
            seen["straddle"] = bool(((starts[1:] - 1) // 64 > starts[:-1] // 64).any())

    run_steps(x, init, 25, 8, "E", spy, float_sum_bound, copies=1, on_step=on_step, label="E-forced")
    assert seen == {"partial": True, "empty": True, "straddle": True}, seen


def test_every_step_on_the_sorted_path_at_its_own_size(spy):
    """Path E where run_kmeans takes it by itself: 2^20 + 4097 points (a partial last chunk), the float64 side on the device."""
    from recommendation_amd import kmeans as K
    assert K.SORTED_UPDATE_MIN_POINTS == 1 << 20
    n = (1 << 20) + 4097
    x, init = blob_fixture(n, 64, 64, 20, 3)
    run_steps(x, init, 64, 2, "E", spy, float_sum_bound, copies=1, dev="cuda", label="E-2^20+4097")


def spectral_fixture(n=20000, dim=6, groups=5):
    """What reorder.py hands to run_kmeans: a few spectral coordinates per row, rows on the unit sphere."""
    rng = np.random.default_rng(1)
    cen = rng.standard_normal((groups, dim)) * 3
    z = cen[rng.integers(0, groups, n)] + 0.5 * rng.standard_normal((n, dim))
    return (z / np.linalg.norm(z, axis=1, keepdims=True)).astype(np.float32)


def test_the_call_shapes_of_the_spectral_renumbering(spy):
    """reorder.py: `run_kmeans(z, ceil(U / 8192), niter=15, seed=...)` on narrow unit rows (padded to 32 columns: path A).
    Stepwise against float64 first, then the call as reorder.py makes it (default cap: 256 training points per centroid)."""
    from recommendation_amd import kmeans as K
    z = spectral_fixture()
    rng = np.random.default_rng(2)
    run_steps(z, z[rng.choice(len(z), 3, replace=False)], 3, 6, "A", spy, fixed_point_bound, label="spectral-6-of-32")
    zg = torch.from_numpy(z).cuda()
    spy.reset()
    cent, labels, info = K.run_kmeans(zg, 3, niter=15, seed=8, return_info=True)
    spy.assert_path("A")
    assert spy.n("gcr_kmeans_search_image_incr_f32") == 15
    assert info["n_train"] == 3 * K.FAISS_MAX_POINTS_PER_CENTROID and info["k"] == 3
    assert cent.shape == (3, 6) and labels.shape == (len(z),) and labels.dtype == torch.int64
    assert bool(torch.isfinite(cent).all())
    best, _, ids = nearest_two(torch.from_numpy(z), cent)
    assert_float64_argmin(labels.cpu(), best, ids, torch.from_numpy(z), cent)
    assert (np.bincount(labels.cpu().numpy(), minlength=3) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the re-seed of empty clusters on the paths without a centroid image
# ---------------------------------------------------------------------------------------------------------------------------

def dead_start_fixture(d, n=6000):
    rng = np.random.default_rng(7)
    centers = rng.standard_normal((8, d)) * 5
    x = (centers[rng.integers(0, 8, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    far = 1e3 * (1 + np.arange(4))[:, None] * np.ones((4, d))
    return x, np.concatenate([centers, far]).astype(np.float32)                  # clusters 8..11 start dead


SPLIT_CASES = [("B", 64, {"INCREMENTAL_UPDATE": False}), ("C", 128, {}), ("D", 256, {}),
               ("E", 64, {"SORTED_UPDATE_MIN_POINTS": 1000})]


@pytest.mark.parametrize("path,d,switches", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_step_matches_restatement_off_the_image_paths(path, d, switches, spy, monkeypatch):
    """test_split_step_matches_restatement_bit_for_bit where kmeans_split_kernel gets no centroid image: the same Philox
    trials, so the same donors; half_sq of the rewritten rows is what the next search uses (no cluster left empty)."""
    from recommendation_amd import kmeans as K
    for name, value in switches.items():
        monkeypatch.setattr(K, name, value)
    k = 12
    x, init = dead_start_fixture(d)
    xg, ig = torch.from_numpy(x).cuda(), torch.from_numpy(init).cuda()
    plain, _ = O.kmeans_lloyd(x, init, niter=1)
    for seed in (1234, 99):
        spy.reset()
        cent, assign, info = K.run_kmeans(xg, k, niter=1, seed=seed, init_centroids=ig, max_points_per_centroid=0,
                                          return_info=True)
        spy.assert_path(path)
        ns = []
        ref_c, ref_a = O.kmeans_lloyd(x, init, niter=1, split_seed=seed, n_split_out=ns)
        assert int(info["n_split"]) == ns[0] == 4
        got = cent.cpu().numpy()
        # donors: a re-seeded row is its donor's mean pushed off by 2^-10 relative, far closer to it than to any other mean
        def donors(c):
            gap = np.linalg.norm(c[8:, None, :] - plain[None, :8, :], axis=2)
            assert (gap.min(1) < 1e-2 * np.linalg.norm(plain[gap.argmin(1)], axis=1)).all()
            return gap.argmin(1).tolist()
        assert donors(got.astype(np.float64)) == donors(ref_c)
        np.testing.assert_allclose(got, ref_c, rtol=2e-6, atol=1e-6)
        cent2, assign2 = K.run_kmeans(xg, k, niter=2, seed=seed, init_centroids=ig, max_points_per_centroid=0)
        assert (np.bincount(assign2.cpu().numpy(), minlength=k) > 0).all()


@pytest.mark.parametrize("form,d,copies", [("accumulated", 64, 3), ("accumulated", 128, 1), ("assign", 256, 5), ("sorted", 64, 1),
                                           ("sorted", 256, 1)])
def test_lloyd_update_reseeds_and_leaves_its_scratch_zeroed(form, d, copies):
    """gcr_kmeans_lloyd_update_f32 through the C ABI in its three forms (sums already accumulated over `copies` private
    copies / an assignment to accumulate / sorted keys): centroids and 0.5 |c|^2 of the re-seeded rows as the restatement
    gives them, and sums / counts — every copy — left zeroed for the next iteration."""
    from recommendation_amd import _lib
    from recommendation_amd import functional as Fn
    k = 12
    x, init = dead_start_fixture(d, n=3001)
    n = x.shape[0]
    a = O.kmeans_lloyd(x, init, niter=0)[1]
    ref_c, _ = O.kmeans_lloyd(x, init, niter=1, split_seed=SEED)
    xg = torch.from_numpy(x).cuda()
    ag = torch.from_numpy(a).cuda()
    cent = torch.from_numpy(init).cuda().clone()
    half = torch.full((k,), -1.0, device="cuda")
    sums = torch.zeros(copies, k, d, device="cuda")
    counts = torch.zeros(copies, k, device="cuda")
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    assign = keys = perm = None
    if form == "accumulated":
        for g in range(copies):                       # rows g, g + copies, ... go to copy g
            sums[g].index_add_(0, ag[g::copies], xg[g::copies])
            counts[g] = torch.bincount(ag[g::copies], minlength=k).float()
    elif form == "assign":
        assign = ag
    else:
        keys, perm, _ = Fn._sorted_order(ag, k)
    L = _lib.lib()
    _lib.check(L.gcr_kmeans_lloyd_update_f32(_lib.dptr(xg), n, d, _lib.dptr(assign), _lib.dptr(keys), _lib.dptr(perm), k,
                                             _lib.dptr(cent), _lib.dptr(half), _lib.dptr(sums), _lib.dptr(counts), copies,
                                             SEED, 0, _lib.dptr(ns), _lib.cur_stream()), "lloyd")
    assert int(ns) == 4
    got = cent.cpu().numpy()
    np.testing.assert_allclose(got, ref_c, rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(half.cpu().numpy(), 0.5 * (got.astype(np.float64) ** 2).sum(1), rtol=1e-5)
    assert float(counts.abs().sum()) == 0.0 and float(sums.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the incremental state after many iterations
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [2, 7, 25])
def test_incremental_sums_after_t_iterations_are_float64_means(t, spy):
    """Path A keeps its sums across the iterations and only moves the points that change cluster.  After t iterations every
    cluster that no ambiguous point has among its two nearest centroids has float64-certain members: its centroid must be
    their float64 mean within the fixed-point bound (the reference is float64 arithmetic, not another GPU search)."""
    from recommendation_amd import kmeans as K
    n, k, d = 30000, 120, 64
    x, init = blob_fixture(n, k, d, 40, 2)
    xg, ig = torch.from_numpy(x).cuda(), torch.from_numpy(init).cuda()
    c_prev, _ = K.run_kmeans(xg, k, niter=t - 1, init_centroids=ig, max_points_per_centroid=0)
    spy.reset()
    c_t, _, info = K.run_kmeans(xg, k, niter=t, init_centroids=ig, max_points_per_centroid=0, return_info=True)
    spy.assert_path("A")
    assert spy.n("gcr_kmeans_search_image_incr_f32") == t
    xr = torch.from_numpy(x)
    best, second, ids = nearest_two(xr, c_prev)
    amb = second < best * (1 + NEAR_TIE)
    unsure = np.zeros(k, dtype=bool)
    unsure[ids[amb].reshape(-1).numpy()] = True
    expect, cnt = float64_means(xr, ids[:, 0], k, c_prev)
    # an empty cluster is re-seeded from a donor and both rows leave their means (this fixture empties four clusters in its
    # second iteration): the split tests and the stepwise case of this shape pin those rows, here they are left out
    reseeded = expect.copy()
    O.kmeans_split_clusters(reseeded, cnt.copy(), n, K.FAISS_SEED, t - 1)
    compared = ~unsure & (cnt > 0) & ~(reseeded != expect).any(1)
    share = compared.mean()
    assert share >= 0.40, share
    err = np.abs(c_t.double().cpu().numpy() - expect)[compared]
    limit = fixed_point_bound(float(xg.abs().max()), expect[compared])
    print(f"[kmeans-paths] incremental t={t}: {compared.sum()} of {k} clusters compared, max |err| {err.max():.3e}, "
          f"max err/bound {(err / limit).max():.3f}, re-seeded {int(info['n_split'])}")
    assert (err <= limit).all(), (float(err.max()), float((err / limit).max()))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the exported update entry points
# ---------------------------------------------------------------------------------------------------------------------------

def update_fixture(d, n=1003, k=9):
    rng = np.random.default_rng(d)
    x = rng.standard_normal((n, d)).astype(np.float32) * 2 + 1
    a = rng.integers(-2, k + 2, n)                        # ids -2, -1, k, k + 1 are out of range: skipped
    a[a == 5] = 6                                         # cluster 5 stays empty: keeps its centroid
    c0 = rng.standard_normal((k, d)).astype(np.float32)
    ok = (a >= 0) & (a < k)
    sums = np.zeros((k, d))
    np.add.at(sums, a[ok], x[ok].astype(np.float64))
    cnt = np.bincount(a[ok], minlength=k)
    assert cnt[5] == 0 and (~ok).sum() > 50 and n % 64 != 0
    expect = np.where(cnt[:, None] > 0, sums / np.maximum(cnt, 1)[:, None], c0.astype(np.float64))
    return x, a, c0, expect


@pytest.mark.parametrize("d", [32, 100, 256])
@pytest.mark.parametrize("entry", ["gcr_kmeans_update_f32", "gcr_kmeans_update_sorted_f32"])
def test_exported_update_entry_points(entry, d):
    """gcr_kmeans_update_f32 (n > 0) and gcr_kmeans_update_sorted_f32: float64 means, out-of-range ids skipped, an empty
    cluster kept, n not a multiple of 64, 0.5 |c|^2 refreshed; the scratch they are handed need not be zero."""
    from recommendation_amd import _lib
    k = 9
    x, a, c0, expect = update_fixture(d)
    n = x.shape[0]
    xg = torch.from_numpy(x).cuda()
    cent = torch.from_numpy(c0).cuda().clone()
    half = torch.full((k,), -1.0, device="cuda")
    sums = torch.full((k, d), 7.0, device="cuda")
    counts = torch.full((k,), 3.0, device="cuda")
    L = _lib.lib()
    if entry == "gcr_kmeans_update_f32":
        ag = torch.from_numpy(a).cuda()
        rc = L.gcr_kmeans_update_f32(_lib.dptr(xg), n, d, _lib.dptr(ag), k, _lib.dptr(cent), _lib.dptr(half), _lib.dptr(sums),
                                     _lib.dptr(counts), _lib.cur_stream())
    else:
        key = np.where(a < 0, k + 3, a)                  # (a negative id is a key >= k as uint32 as well)
        order = np.argsort(key, kind="stable")
        keys = torch.from_numpy(key[order].astype(np.int32)).cuda()
        perm = torch.from_numpy(order.astype(np.int32)).cuda()
        rc = L.gcr_kmeans_update_sorted_f32(_lib.dptr(xg), n, d, _lib.dptr(keys), _lib.dptr(perm), k, _lib.dptr(cent),
                                            _lib.dptr(half), _lib.dptr(sums), _lib.dptr(counts), _lib.cur_stream())
    assert rc == 0
    got = cent.cpu().numpy()
    np.testing.assert_allclose(got, expect, rtol=1e-5, atol=1e-5)
    assert np.array_equal(got[5], c0[5])
    np.testing.assert_allclose(half.cpu().numpy(), 0.5 * (got.astype(np.float64) ** 2).sum(1), rtol=1e-5)


def test_exported_update_entry_points_refuse_bad_arguments():
    """Both entry points check their arguments on the host, before the first memset or launch (csrc/gcr_kmeans.hip): a
    refused call returns non-zero and leaves every buffer as it was."""
    from recommendation_amd import _lib
    k, d, n = 4, 32, 100
    L = _lib.lib()
    st = _lib.cur_stream()
    x = torch.ones(n, 512, device="cuda")
    a = torch.zeros(n, dtype=torch.int64, device="cuda")
    keys = torch.zeros(n, dtype=torch.int32, device="cuda")
    perm = torch.arange(n, dtype=torch.int32, device="cuda")
    cent = torch.full((k, 512), 2.0, device="cuda")
    half = torch.full((k,), -1.0, device="cuda")
    sums = torch.full((k, 512), 7.0, device="cuda")
    counts = torch.full((k,), 3.0, device="cuda")
    p = _lib.dptr
    sorted_bad = [
        (p(x), n, 257, p(keys), p(perm), k, p(cent), p(half), p(sums), p(counts), st),      # d > 256
        (p(x), n, 0, p(keys), p(perm), k, p(cent), p(half), p(sums), p(counts), st),
        (p(x), 0, d, p(keys), p(perm), k, p(cent), p(half), p(sums), p(counts), st),        # n < 1
        (p(x), n, d, p(keys), p(perm), 0, p(cent), p(half), p(sums), p(counts), st),
        (None, n, d, p(keys), p(perm), k, p(cent), p(half), p(sums), p(counts), st),
        (p(x), n, d, None, p(perm), k, p(cent), p(half), p(sums), p(counts), st),
        (p(x), n, d, p(keys), None, k, p(cent), p(half), p(sums), p(counts), st),
        (p(x), n, d, p(keys), p(perm), k, None, p(half), p(sums), p(counts), st),
        (p(x), n, d, p(keys), p(perm), k, p(cent), None, p(sums), p(counts), st),
        (p(x), n, d, p(keys), p(perm), k, p(cent), p(half), None, p(counts), st),
        (p(x), n, d, p(keys), p(perm), k, p(cent), p(half), p(sums), None, st),
    ]
    for args in sorted_bad:
        assert L.gcr_kmeans_update_sorted_f32(*args) != 0, args
    update_bad = [
        (p(x), -1, d, p(a), k, p(cent), p(half), p(sums), p(counts), st),
        (p(x), n, 0, p(a), k, p(cent), p(half), p(sums), p(counts), st),
        (p(x), n, d, p(a), 0, p(cent), p(half), p(sums), p(counts), st),
        (None, n, d, p(a), k, p(cent), p(half), p(sums), p(counts), st),
        (p(x), n, d, None, k, p(cent), p(half), p(sums), p(counts), st),
        (p(x), n, d, p(a), k, None, p(half), p(sums), p(counts), st),
        (p(x), n, d, p(a), k, p(cent), None, p(sums), p(counts), st),
        (p(x), n, d, p(a), k, p(cent), p(half), None, p(counts), st),
        (p(x), n, d, p(a), k, p(cent), p(half), p(sums), None, st),
        (None, 0, d, None, k, None, p(half), None, None, st),                               # the refresh-only form
    ]
    for args in update_bad:
        assert L.gcr_kmeans_update_f32(*args) != 0, args
    torch.cuda.synchronize()
    assert float((cent - 2.0).abs().max()) == 0.0 and float((half + 1.0).abs().max()) == 0.0
    assert float((sums - 7.0).abs().max()) == 0.0 and float((counts - 3.0).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the range of the fixed-point scale
# ---------------------------------------------------------------------------------------------------------------------------

def test_fixed_point_sums_over_a_wide_dynamic_range(spy):
    """One feature column at 1e3, the others at 1e-2: path A resolves every centroid element to max|x| * 2^-28 whatever the
    element's own size (the resolution run_kmeans documents), and stays inside that bound against float64."""
    rng = np.random.default_rng(1)
    n, k, d = 8000, 24, 64
    cen = rng.standard_normal((8, d)) * 3
    x = cen[rng.integers(0, 8, n)] + rng.standard_normal((n, d))
    x *= np.where(np.arange(d) == 0, 1e3, 1e-2)[None, :]
    x = x.astype(np.float32)
    init = x[rng.choice(n, k, replace=False)]
    # the near-tie rule of the other cases measures a flipped assignment against d2 * 1e-5; here |x|^2 is up to 4e7 with d2
    # near 1e6, and a float32 score x.c - |c|^2 / 2 is rounded at 2^-24 |x| |c| ~ 2, which that allowance (~10) does not
    # clear by a safe margin: the assignment is held to the 99.9 % agreement only (the 1e-4 exclusion margin, ~100, is
    # far above the rounding, so the members of every cluster are still float64-certain)
    run_steps(x, init, k, 6, "A", spy, fixed_point_bound, label="A-wide-range", tie_rule=False)


@pytest.mark.parametrize("scale", [0.0, 1e-35])
def test_fixed_point_scale_at_degenerate_magnitudes(scale, spy):
    """An all-zero training set, and one scaled by 1e-35: 29 - floor(log2 max|x|) exceeds 127 there, 2^e is not a float32
    any more (inf, and 0 * inf = NaN), so run_kmeans caps the exponent at 125 and keeps the sums in units of 2^-125.  Squared
    distances near 1e-70 are below float32's range: the search sees exact ties everywhere and answers with the lowest id, so
    what is pinned here is the update — finite centroids that are the float64 means of the members the search names
    (`assign_to_centroids`), re-seeded as oracle_np re-seeds the clusters that search leaves empty."""
    from recommendation_amd import kmeans as K
    n, k, d = 2000, 3, 64
    x, init = blob_fixture(n, k, d, 3, 3)
    x, init = (x * np.float32(scale)).astype(np.float32), (init * np.float32(scale)).astype(np.float32)
    assert scale == 0.0 or (0 < np.abs(x).max() < 2.0 ** -98)
    xg, ig = torch.from_numpy(x).cuda(), torch.from_numpy(init).cuda()
    members = K.assign_to_centroids(xg, ig)
    spy.reset()
    cent, assign, info = K.run_kmeans(xg, k, niter=1, init_centroids=ig, max_points_per_centroid=0, return_info=True)
    spy.assert_path("A")
    expect, cnt = float64_means(torch.from_numpy(x), members.cpu(), k, ig)
    n_split = O.kmeans_split_clusters(expect, cnt, n, K.FAISS_SEED, 0)
    got = cent.double().cpu().numpy()
    assert np.isfinite(got).all()
    assert int(info["n_split"]) == n_split
    # the re-seed multiplies the float32 mean by 1 +- 2^-10 in float32: one more rounding, again with a factor 2 of slack (the
    # absolute part of the re-seed bound of the other tests, 1e-6, would swallow inputs of this size whole)
    limit = fixed_point_bound(float(np.abs(x).max()), expect) + (2.0 ** -23 * np.abs(expect) if n_split else 0.0)
    err = np.abs(got - expect)
    print(f"[kmeans-paths] degenerate scale {scale:g}: max |err| {err.max():.3e}, max err/bound {(err / limit).max():.3f}, "
          f"re-seeded {n_split}")
    assert (err <= limit).all()
    assert int(assign.min()) >= 0 and int(assign.max()) < k
    for niter in (3, 25):
        c, a = K.run_kmeans(xg, k, niter=niter, init_centroids=ig, max_points_per_centroid=0)
        assert bool(torch.isfinite(c).all()) and float(c.abs().max()) <= float(np.abs(x).max()) * 1.1
    c, a = K.run_kmeans(xg, k, niter=2)
    assert bool(torch.isfinite(c).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 6. small belongings
# ---------------------------------------------------------------------------------------------------------------------------

def test_assign_points_false_skips_only_the_final_search(spy):
    from recommendation_amd import kmeans as K
    x, init = blob_fixture(8000, 24, 64, 8, 3)
    xg, ig = torch.from_numpy(x).cuda(), torch.from_numpy(init).cuda()
    c1, a1 = K.run_kmeans(xg, 24, niter=5, init_centroids=ig, max_points_per_centroid=0)
    spy.reset()
    c2, a2 = K.run_kmeans(xg, 24, niter=5, init_centroids=ig, max_points_per_centroid=0, assign_points=False)
    spy.assert_path("A")
    assert a2 is None and spy.n("gcr_kmeans_assign_f32") == 0
    assert torch.equal(c1, c2)
    # (assign_to_centroids recomputes 0.5 |c|^2 with torch: a last-bit difference may flip a float32 near-tie)
    assert float((K.assign_to_centroids(xg, c2) == a1).float().mean()) > 0.999
    c3, a3, info = K.run_kmeans(xg, 24, niter=5, init_centroids=ig, max_points_per_centroid=0, assign_points=False,
                                return_info=True)
    assert a3 is None and torch.equal(c1, c3) and info["k"] == 24


@pytest.mark.parametrize("n,k,want_k,want_train", [(1000, 500, 25, 1000), (100, 2000, 2, 100), (20000, 8, 8, 2048),
                                                    (20000, 600, 512, 20000)])
def test_return_info_reports_the_clamped_sizes(n, k, want_k, want_train):
    """k' = min(k, max(2, n // 39)) (ncl.py:350-351) and the training-set size after faiss' 256-points-per-centroid cap."""
    from recommendation_amd import kmeans as K
    g = torch.Generator(device="cuda").manual_seed(n + k)
    x = torch.randn(n, 64, device="cuda", generator=g)
    cent, assign, info = K.run_kmeans(x, k, niter=2, return_info=True)
    assert want_k == min(k, max(2, n // 39))
    assert info["k"] == want_k and info["n_train"] == want_train
    assert cent.shape == (want_k, 64) and assign.shape == (n,) and int(assign.max()) < want_k and int(assign.min()) >= 0
    assert info["n_split"].shape == (1,) and info["n_split"].dtype == torch.int32
