"""k-means E-step of NCL (ncl.py:340-356) on the GPU: `run_kmeans(x)` -> (centroids, assignment).

The reference delegates to `faiss.Kmeans(d=emb_size, k=k, gpu=False).train(x)` + `kmeans.index.search(x, 1)`
(ncl.py:352-355); faiss is an un-vendored dependency that is not installed here and the reference holds no fixture
for it, so PARITY WITH FAISS IS UNPINNED.  What is implemented is faiss' published `Clustering::train`
(faiss/Clustering.cpp) under the parameter list the reference's call leaves at its defaults — `struct
ClusteringParameters` of faiss/Clustering.h as published for faiss 1.7 / 1.8 (restated from memory of the public
source; not checkable offline, hence explicit arguments here rather than a claim):

    niter = 25, nredo = 1, seed = 1234, spherical = false, int_centroids = false, update_index = false,
    frozen_centroids = false, min_points_per_centroid = 39, max_points_per_centroid = 256

  * n > k * max_points_per_centroid: train on a random subsample of k * 256 points (`subsample_training_set`, a
    random permutation seeded `seed`); n < k * 39 only warns (the reference clamps k so that it does not happen);
  * initial centroids = k training points from a random permutation seeded `seed + 1` (nredo = 1);
  * niter times: nearest centroid under L2 for every training point (IndexFlatL2), centroid = mean of its points
    (an empty cluster keeps its centroid), then `split_clusters`: every empty cluster takes a perturbed copy of a
    cluster picked with probability (size - 1) / (n - k);
  * every point is then assigned against the final centroids (`kmeans.index.search(x, 1)`).
faiss seeds its generator identically in every call (seed = 1234), so the subsample and the initial picks are the SAME
index vectors in every e_step; they are cached here per (n, count, seed).  The random streams themselves are torch's /
Philox, not faiss' Mersenne twister.  Nothing in an e_step reads anything back to the host (hipGraph-capturable);
the nearest-centroid search runs on the MFMA tile engine (gcr_kmeans_assign_f32).
"""
from __future__ import annotations

import torch

from . import _lib
from . import functional as Fn

# faiss/Clustering.h `ClusteringParameters` defaults (see the module docstring for provenance)
FAISS_NITER = 25
FAISS_SEED = 1234
FAISS_MIN_POINTS_PER_CENTROID = 39          # ncl.py:350 clamps k with it: max_k = max(2, n // 39)
FAISS_MAX_POINTS_PER_CENTROID = 256

# centroid update: one float-atomic row per point into `copies` private (sums, counts) pairs (gcr_kmeans_lloyd_update_f32),
# or — for training sets at least this large — from the points ordered by cluster (one atomic per run; needs a sort)
SORTED_UPDATE_MIN_POINTS = 1 << 20
MAX_ATOMIC_COPIES = 16

# the wave-independent search (every wave streams the whole centroid image from L2) pays while the problem is small enough
# to be latency-bound; past this many point-centroid pairs per iteration the tiled kernel's LDS sharing wins
IMAGE_SEARCH = True
IMAGE_SEARCH_LOW_REGISTERS = True      # <= 128 registers per lane: co-resident with the InfoNCE loops of the training step
# cluster sums kept in 64-bit fixed point across the iterations, updated only by the points that changed cluster (exact,
# order-independent: equals a fresh accumulation bit for bit, and makes the e_step run-to-run reproducible)
INCREMENTAL_UPDATE = True
IMAGE_SEARCH_MAX_PAIRS = 1 << 28

_PERM_CACHE = {}


def _perm_prefix(n, count, seed, device):
    """First `count` entries of a random permutation of range(n), fixed by `seed` (faiss: `rand_perm(perm, n, seed)`;
    it re-seeds per call, so the vector is a constant of (n, seed): computed once, kept)."""
    key = (int(n), int(count), int(seed), str(device))
    hit = _PERM_CACHE.get(key)
    if hit is None:
        g = torch.Generator(device=device).manual_seed(int(seed))
        hit = torch.randperm(int(n), device=device, generator=g)[: int(count)].contiguous()
        if len(_PERM_CACHE) >= 16:
            _PERM_CACHE.pop(next(iter(_PERM_CACHE)))
        _PERM_CACHE[key] = hit
    return hit


def kmeans_assign(x, centroids, half_sq):
    n, d = x.shape
    assign = torch.empty(n, dtype=torch.int64, device=x.device)
    _lib.call("gcr_kmeans_assign_f32", x, n, centroids, half_sq, centroids.shape[0], d, assign, None, on=x)
    return assign


def assign_to_centroids(x, centroids):
    """`kmeans.index.search(x, 1)` (ncl.py:355): the nearest centroid (L2) of every row of x, int64 [n]."""
    _lib.require_cuda(x, centroids)
    xp = Fn._pad_dim(x.detach()).contiguous()
    cp = Fn._pad_dim(centroids.detach().to(torch.float32)).contiguous()
    return kmeans_assign(xp, cp, 0.5 * (cp * cp).sum(1))


def run_kmeans(x, k, niter=FAISS_NITER, seed=FAISS_SEED, init_centroids=None,
               max_points_per_centroid=FAISS_MAX_POINTS_PER_CENTROID, return_info=False, assign_points=True):
    """ncl.py:347-356.  x: float32 [n, d] on the GPU.  Returns (centroids [k', d], assignment int64 [n])
    with k' = min(k, max(2, n // 39)) exactly as ncl.py:350-351 clamps it (and, with return_info, a dict holding the
    device counter of re-seeded empty clusters).  assign_points=False skips the final search over all n points and
    returns None for the assignment (`assign_to_centroids` gives it later, for all rows or for a batch's rows only).
    No host synchronisation.

    Resolution.  On the default path (d in {32, 64} after padding, n_train * k <= IMAGE_SEARCH_MAX_PAIRS) the cluster sums
    are 64-bit fixed point in units of 2^-e, max |x| * 2^e in [2^29, 2^30): every centroid element is the float64 mean of
    its members within max|x| * 2^-28 + 2^-23 * |mean|, whatever the element's own size — a column a factor 2^28 below the
    largest entry of the training set is not resolved.  For max |x| < 2^-96 (an all-zero set included) the unit stays at
    2^-125 and the first term becomes 2^-125.  The float-sum paths (d > 64, or past the thresholds above) carry float32
    accumulation error instead (1e-5 relative + 1e-5 absolute on inputs up to |x| = 16).  tests/test_kmeans_paths_gpu.py pins
    every path to these bounds, one Lloyd step at a time.
    Non-finite input (a NaN or an infinity anywhere in x) is UNDEFINED behaviour: centroids and assignment come back
    without an error and mean nothing.  Refusing it would take a read-back of a device flag, and the e_step must not
    synchronise with the host; callers that cannot vouch for their input check it themselves (`torch.isfinite(x).all()`)."""
    _lib.require_cuda(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("x must be float32 [n, d]")
    n, d_orig = x.shape
    k = min(int(k), max(2, n // FAISS_MIN_POINTS_PER_CENTROID))
    xp = Fn._pad_dim(x.detach()).contiguous()
    xt = xp                                            # training set
    if max_points_per_centroid and n > k * max_points_per_centroid:
        xt = xp[_perm_prefix(n, k * max_points_per_centroid, seed, x.device)]
    n_train = xt.shape[0]
    if init_centroids is None:
        cent = xt[_perm_prefix(n_train, k, seed + 1, x.device)].clone()
    else:
        cent = Fn._pad_dim(init_centroids.detach().to(torch.float32)).contiguous().clone()
    k = cent.shape[0]
    d = xp.shape[1]
    dev = x.device
    half_sq = torch.empty(k, dtype=torch.float32, device=dev)
    use_sorted = n_train >= SORTED_UPDATE_MIN_POINTS
    # ~256 points per centroid (faiss' cap) on a few hundred rows: spread the row atomics over private copies
    copies = 1 if use_sorted else max(1, min(MAX_ATOMIC_COPIES, n_train // (16 * k)))
    sums = torch.zeros(copies, k, d, dtype=torch.float32, device=dev)      # zero on entry / exit of every lloyd_update
    counts = torch.zeros(copies, k, dtype=torch.float32, device=dev)
    n_split = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = _lib.cur_stream(dev)
    # 0.5 |c|^2 of the initial centroids (n = 0: refresh only)
    _lib.call("gcr_kmeans_update_f32", None, 0, d, None, k, cent, half_sq, None, None, on=stream)
    fused = not use_sorted and bool(_lib.call("gcr_infonce_engine", d))       # search + accumulate in one launch (d <= 128)
    # small problems (the e_step: 76.8 K sampled points, a few hundred centroids) are latency-bound: wave-independent search
    # over a pre-split centroid image (gcr_kmeans_search_image_f32), the image rebuilt once per iteration
    image = None
    if fused and d in (32, 64) and IMAGE_SEARCH and n_train * k <= IMAGE_SEARCH_MAX_PAIRS:
        image = torch.empty(_lib.call("gcr_kmeans_image_bytes", k, d), dtype=torch.uint8, device=dev)
    incremental = image is not None and INCREMENTAL_UPDATE
    if incremental:
        # fixed-point scale 2^e with max |x| * 2^e in [2^29, 2^30): exact in f32, computed on the device (no read-back).
        # The floor 2^-96 under max |x| bounds e by 125, so 2^e and 2^-e stay finite normal float32 (with the former floor
        # 1e-30 an all-zero set, or any max |x| < 2^-98, gave e > 127: 2^e = inf, 2^-e = 0, 0 * inf = NaN); below it the sums
        # are kept in units of 2^-125.  max |x| < 2^128 gives e >= -98 by itself.
        e = 29.0 - torch.floor(torch.log2(xt.abs().max().clamp_min(2.0 ** -96)))
        qscale = torch.stack([torch.exp2(e), torch.exp2(-e)]).to(torch.float32)
        sums_q = torch.zeros(copies, k, d, dtype=torch.int64, device=dev)
        counts_i = torch.zeros(copies, k, dtype=torch.int32, device=dev)
        prev = torch.full((n_train,), -1, dtype=torch.int32, device=dev)
        counts_f = torch.zeros(k, dtype=torch.float32, device=dev)
        flags = 1 if IMAGE_SEARCH_LOW_REGISTERS else 0
        # the operand image is built once; every iteration's update keeps it current (no image launch per iteration)
        _lib.call("gcr_kmeans_centroid_image_f32", cent, half_sq, k, d, image, on=stream)
        for it in range(int(niter)):
            _lib.call("gcr_kmeans_search_image_incr_f32", xt, n_train, image, k, d, prev, qscale, sums_q, counts_i, copies, flags,
                      on=stream)
            _lib.call("gcr_kmeans_lloyd_update_q_f32", sums_q, counts_i, qscale, k, d, cent, half_sq, counts_f, n_train,
                      int(seed) & (2 ** 64 - 1), it, n_split, image, copies, on=stream)
        niter = 0
    for it in range(int(niter)):
        keys = perm = assign = None
        if image is not None:
            _lib.call("gcr_kmeans_centroid_image_f32", cent, half_sq, k, d, image, on=stream)
            _lib.call("gcr_kmeans_search_image_f32", xt, n_train, image, k, d, None, sums, counts, copies,
                      1 if IMAGE_SEARCH_LOW_REGISTERS else 0, on=stream)
        elif fused:
            _lib.call("gcr_kmeans_assign_accumulate_f32", xt, n_train, cent, half_sq, k, d, None, sums, counts, copies, on=stream)
        else:
            assign = kmeans_assign(xt, cent, half_sq)
            if use_sorted:
                # points ordered by cluster: one row atomic per run instead of one per point
                keys, perm, _ = Fn._sorted_order(assign, k)
        _lib.call("gcr_kmeans_lloyd_update_f32", xt, n_train, d, assign, keys, perm, k, cent, half_sq, sums, counts, copies,
                  int(seed) & (2 ** 64 - 1), it, n_split, on=stream)
    # kmeans.index.search(x, 1) against the final centroids
    assign = kmeans_assign(xp, cent, half_sq) if assign_points else None
    cent = cent[:, :d_orig].contiguous()
    if return_info:
        return cent, assign, {"n_split": n_split, "n_train": n_train, "k": k}
    return cent, assign
