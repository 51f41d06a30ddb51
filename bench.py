#!/usr/bin/env python3
"""Headline benchmark: edges propagated/sec (+ InfoNCE pairs/sec) of the LightGCN d=64 hot path.

Contract (see the task statement): `python bench.py --gpus N --steps K --warmup W`; for N > 1 the
driver launches it under torch.distributed.run, one rank per GPU.  W untimed warm-up steps, then
exactly K timed steps between barrier + synchronize, MAX over ranks, rank 0 prints ONE JSON line.

A "step" is one pass of the hot path over one batch of synthetic input: the K_layers-layer
LightGCN message pass (normalised bipartite adjacency SpMM x embedding table, layer combine
fused) over the whole graph — forward only for the headline `value`.

A plain run does only what the headline line needs: build the workload, warm up, time the K steps
and print the line (its `roofline` block comes from events around the timed launches).  `--full`
adds everything else, each leg timed on its own: memory probes, the InfoNCE roofline, fwd+bwd,
InfoNCE, BPR and training-step rates ("extra"), the CPU baseline, the cfg4 companion line, the
community graphs, cfg5 and the GCL step (N > 1: the GCL step and the strong-scaling cfg4 line).
`--dump-outputs DIR` writes what the last timed step returned as DIR/<name>.npy (float32; a
fixed, seeded sample of the rows of a large output; see dump_outputs).

Workloads:
  cfg2  U=1M  I=100K E=10M  (N=1.1M,  nnz=20M)   K=3 d=64   <- N=1 default (BASELINE configs[1])
  cfg4  U=10M I=1M   E=100M (N=11M,   nnz=200M)  K=3 d=64
  cfg1  U=943 I=1682 E=80K                        K=2 d=64   (plumbing size)
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "cfg1": dict(users=943, items=1682, edges=80_000, layers=2),
    "cfg2": dict(users=1_000_000, items=100_000, edges=10_000_000, layers=3),
    "cfg4": dict(users=10_000_000, items=1_000_000, edges=100_000_000, layers=3),
}
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8.0 TB/s spec
FP32_MFMA_PEAK_TF = 157.3  # MI355X_MICROARCH.md: fp32-input MFMA = vector rate
BF16_MFMA_PEAK_TF = 16 * FP32_MFMA_PEAK_TF   # same guide: bf16 MFMA = 16x the f32 MFMA rate (~2.5 PF dense)
SEED = 20250919


def synth_interactions_device(n_users, n_items, n_edges, seed, device, perm_seed=None):
    """Same recipe as oracle_np.synthetic_interactions (users uniform, items Zipf(1) capped at
    0.5 % each, unique pairs, every user >= 1 edge), generated with torch on the GPU.
    `perm_seed` fixes the popularity-rank -> item-id permutation separately from the draws (the
    ranks of a sharded run share one item popularity law but draw their own users' edges)."""
    g = torch.Generator(device=device).manual_seed(seed)
    p = 1.0 / torch.arange(1, n_items + 1, device=device, dtype=torch.float64)
    p /= p.sum()
    cap = 0.005
    for _ in range(50):
        over = p > cap
        if not bool(over.any()):
            break
        excess = (p[over] - cap).sum()
        p[over] = cap
        p[~over] += excess * p[~over] / p[~over].sum()
    cdf = torch.cumsum(p, 0)
    cdf[-1] = 1.0
    gp = g if perm_seed is None else torch.Generator(device=device).manual_seed(perm_seed)
    perm = torch.randperm(n_items, generator=gp, device=device)

    def draw_items(n):
        r = torch.rand(n, generator=g, device=device, dtype=torch.float64)
        return perm[torch.searchsorted(cdf, r, right=True).clamp_(max=n_items - 1)]

    keys = torch.arange(n_users, device=device, dtype=torch.int64) * n_items + draw_items(n_users)
    need = n_edges - n_users
    while need > 0:
        n = int(need * 1.15) + 16
        k = torch.randint(0, n_users, (n,), generator=g, device=device) * n_items + draw_items(n)
        k = torch.unique(k)
        k = k[~torch.isin(k, keys)]
        if k.numel() > need:
            k = k[torch.randperm(k.numel(), generator=g, device=device)[:need]]
        keys = torch.cat([keys, k])
        need = n_edges - keys.numel()
    keys = keys[torch.randperm(keys.numel(), generator=g, device=device)]
    return keys // n_items, keys % n_items


COMMUNITY = dict(n_comm=128, p_in=0.85)     # cfg2c: the cfg2 sizes with planted taste communities (8K users x 780 items each)


def synth_community_interactions_device(n_users, n_items, n_edges, seed, device, n_comm=128, p_in=0.85):
    """A bipartite graph with the structure real interaction data has and the uniform generator lacks: `n_comm` taste
    communities (equal blocks of users and of items); a user draws an item of its own community with probability p_in
    and any item otherwise, items by the same capped Zipf(1) popularity law as the uniform generator (popular and
    unpopular items in every community).  The ids are then SHUFFLED (random permutations of users and of items), as ids
    of a real data set carry no locality — recovering it is the renumbering's job (recommendation_amd/reorder.py).
    Returns (users, items, hidden_user_community [U], hidden_item_community [I]) in the shuffled ids; unique pairs,
    every user >= 1 interaction."""
    g = torch.Generator(device=device).manual_seed(seed)
    p = 1.0 / torch.arange(1, n_items + 1, device=device, dtype=torch.float64)
    p /= p.sum()
    cap = 0.005
    for _ in range(50):
        over = p > cap
        if not bool(over.any()):
            break
        excess = (p[over] - cap).sum()
        p[over] = cap
        p[~over] += excess * p[~over] / p[~over].sum()
    p = p[torch.randperm(n_items, generator=g, device=device)]           # hidden item id -> popularity (ranks scattered)
    cdf = torch.cumsum(p, 0)
    cdf[-1] = 1.0
    # community c owns hidden users [c U / C, (c + 1) U / C) and hidden items [ceil(c I / C), ceil((c + 1) I / C))
    bounds = (torch.arange(n_comm + 1, device=device, dtype=torch.int64) * n_items + n_comm - 1) // n_comm
    cdf0 = torch.cat([cdf.new_zeros(1), cdf])
    seg_lo, seg_hi = cdf0[bounds[:-1]], cdf0[bounds[1:]]                  # popularity mass interval of every community

    def draw(users_h):
        n = users_h.numel()
        r = torch.rand(n, generator=g, device=device, dtype=torch.float64)
        inside = torch.rand(n, generator=g, device=device) < p_in
        c = users_h * n_comm // n_users
        target = torch.where(inside, seg_lo[c] + r * (seg_hi[c] - seg_lo[c]), r)
        return torch.searchsorted(cdf, target, right=True).clamp_(max=n_items - 1)

    uh = torch.arange(n_users, device=device, dtype=torch.int64)
    keys = uh * n_items + draw(uh)
    need = n_edges - n_users
    while need > 0:
        n = int(need * 1.15) + 16
        u = torch.randint(0, n_users, (n,), generator=g, device=device)
        k = torch.unique(u * n_items + draw(u))
        k = k[~torch.isin(k, keys)]
        if k.numel() > need:
            k = k[torch.randperm(k.numel(), generator=g, device=device)[:need]]
        keys = torch.cat([keys, k])
        need = n_edges - keys.numel()
    keys = keys[torch.randperm(keys.numel(), generator=g, device=device)]
    uh, ih = keys // n_items, keys % n_items
    pu = torch.randperm(n_users, generator=g, device=device)             # hidden -> public id
    pi = torch.randperm(n_items, generator=g, device=device)
    cu = torch.empty(n_users, dtype=torch.int64, device=device)
    ci = torch.empty(n_items, dtype=torch.int64, device=device)
    cu[pu] = torch.arange(n_users, device=device, dtype=torch.int64) * n_comm // n_users
    ci[pi] = torch.searchsorted(bounds, torch.arange(n_items, device=device, dtype=torch.int64), right=True) - 1
    return pu[uh], pi[ih], cu, ci


def community_leg(ra, Fn, dev, name, d=64, reps=10):
    """Secondary workload: the same K-layer forward on a graph WITH community structure, ids shuffled
    as they arrive (`before`) and after recommendation_amd/reorder.py's spectral renumbering + XCD-grouped plan (`after`).
    The uniform headline graph cannot benefit from any numbering; this one shows what the carried permutation buys."""
    from recommendation_amd import reorder as R
    wl = WORKLOADS[name]
    n_u, n_i, n_e, k_layers = wl["users"], wl["items"], wl["edges"], wl["layers"]
    n_comm = max(2, n_u // 8192)
    users, items, _, _ = synth_community_interactions_device(n_u, n_i, n_e, SEED, dev, n_comm, COMMUNITY["p_in"])
    n = n_u + n_i
    x0 = torch.empty(n, d, device=dev)
    torch.nn.init.xavier_uniform_(x0, generator=torch.Generator(device=dev).manual_seed(0))

    def layer_ms(graph):
        with torch.no_grad():
            return _event_ms(lambda: Fn.lightgcn_propagate(graph, x0, k_layers, combine="sum"), reps) / k_layers

    g0 = ra.CsrGraph.bipartite_sym_norm(users, items, n_u, n_i, dev)
    t_before = layer_ms(g0)
    nnz = g0.nnz
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pu, pi, group = R.locality_permutation(users, items, n_u, n_i, dev, graph=g0)
    torch.cuda.synchronize()
    t_reorder = time.perf_counter() - t0
    del g0
    g1 = ra.CsrGraph.bipartite_sym_norm(pu[users], pi[items], n_u, n_i, dev, row_group=group)
    t_after = layer_ms(g1)
    bytes_alg = nnz * (8 + 4 * d) + n * (4 * d + 4)
    out = {"workload": f"{name} sizes with {n_comm} planted communities (p_in = {COMMUNITY['p_in']}), ids shuffled: {n_u} users x "
                       f"{n_i} items / {n_e} interactions (nnz={nnz}), {k_layers}-layer d={d} forward",
           "ms_per_layer_before": round(t_before, 4), "ms_per_layer_after": round(t_after, 4),
           "speedup": round(t_before / t_after, 3), "reorder_s": round(t_reorder, 2),
           "edges_per_s_before": nnz / t_before * 1e3, "edges_per_s_after": nnz / t_after * 1e3,
           "frac_alg_before": round(bytes_alg / t_before / 1e6 / HBM_PEAK_GBS, 4),
           "frac_alg_after": round(bytes_alg / t_after / 1e6 / HBM_PEAK_GBS, 4),
           "traffic_before": None, "traffic_after": None,
           "note": "after = spectral co-clustering renumbering (reorder.py: subspace iteration on the SpMM kernel + the e_step's "
                   "k-means) + work plan walked community by community on one XCD; frac_alg is the no-reuse byte model (cache hits "
                   "make it exceed 1)"}
    for tag in ("before", "after"):
        pmc = _committed_pmc(f"{name}c_{tag}", spmm_source_digest())
        if pmc:
            out[f"traffic_{tag}"] = pmc["bytes_per_launch"]
            out["traffic_source"] = pmc["source"]
    return out


def sym_norm_csr_device(users, items, n_users, n_items):
    """D^-1/2 (R + R^T) D^-1/2 as CSR, built with torch ops on the device (bench plumbing; the
    pairs are unique so no duplicate merge is needed; rows sorted by (row, col) like selfcf.py:297)."""
    n = n_users + n_items
    row = torch.cat([users, items + n_users])
    col = torch.cat([items + n_users, users])
    order = torch.argsort(row * n + col)
    row, col = row[order], col[order]
    deg = torch.bincount(row, minlength=n)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=row.device)
    rowptr[1:] = torch.cumsum(deg, 0)
    dinv = deg.to(torch.float32).pow(-0.5)
    dinv[torch.isinf(dinv)] = 0.0
    val = dinv[row] * dinv[col]
    return rowptr, col.to(torch.int32), val


def _file_digest(paths, salt=""):
    import hashlib
    h = hashlib.sha256(salt.encode())
    for rel in paths:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(rel.encode())
            h.update(f.read())
    return h.hexdigest()[:16]


def spmm_source_digest():
    """Identifies the SpMM kernel + plan a PMC capture belongs to (the .git directory does not travel to
    the GPU box, so the check is on source content, not on a commit id)."""
    from recommendation_amd.graph import DEFAULT_NNZ_PER_PART
    return _file_digest(["recommendation_amd/csrc/gcr_spmm.hip", "recommendation_amd/csrc/gcr_plan.cpp",
                         "recommendation_amd/csrc/gcr_common.h"], salt=f"nnz_per_part={DEFAULT_NNZ_PER_PART}")


def infonce_source_digest():
    return _file_digest(["recommendation_amd/csrc/gcr_infonce.hip", "recommendation_amd/csrc/gcr_common.h"])


def _committed_pmc(key, digest, allow_stale=False):
    """Entry `key` of profiles/pmc_traffic.json, or None when there is none or it was captured on other
    kernel sources than the ones being benchmarked.  allow_stale: return such an entry anyway, marked
    `stale_digest` (the caller must say so in what it reports)."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            ent = json.load(f).get(key)
    except (OSError, ValueError):
        return None
    if not ent:
        return None
    if ent.get("source_digest") != digest:
        if not allow_stale:
            return None
        ent = dict(ent, stale_digest=True)
    return ent


def _event_ms(fn, reps, warm=1):
    """Average device time of fn() in ms, HIP events on the stream the kernels are launched on (torch's
    current stream is the one every gcr_* launch receives).  `warm` untimed calls first: a matrix-core kernel timed over a
    few milliseconds right after a memory-bound phase (or idle) reads 10-15 % slow while the clock ramps
    (scripts/exp/fwd_bimodal_probe.py: 0.93 -> 0.86 ms over four 2.5 ms windows after 0.5 s idle, 0.825 ms sustained)."""
    for _ in range(max(1, warm)):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


DUMP_MAX_BYTES = 48 << 20      # --dump-outputs in all


def dump_outputs(outdir, arrays):
    """--dump-outputs: every [rows, d] tensor of `arrays` (name -> tensor) as <outdir>/<name>.npy in float32.  The byte
    budget is shared equally; a tensor over its share is cut to a sample of its rows drawn from SEED alone (sorted), so
    runs with the same arguments dump the same rows and two builds can be compared output for output."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    share = DUMP_MAX_BYTES // len(arrays)
    for name, t in arrays.items():
        t = t.detach().float()
        row_bytes = 4 * (t.numel() // max(1, t.shape[0]))
        if t.numel() * 4 > share:
            keep = np.random.default_rng(SEED).choice(t.shape[0], share // row_bytes, replace=False)
            t = t[torch.from_numpy(np.sort(keep)).to(t.device)]
        np.save(os.path.join(outdir, name + ".npy"), t.cpu().numpy())


def memory_probes(table, dev):
    """Measured ceilings of this box's memory system (gcr_probe_*): float4 copy / read over 1 GiB buffers
    (far past the 256 MiB Infinity Cache) and the 256-B row gather of the SpMM on `table` itself."""
    from recommendation_amd import _lib
    L = _lib.lib()
    st = _lib.cur_stream(dev)
    n = 1 << 28                                            # 1 GiB of floats
    src = torch.empty(n, device=dev).normal_()
    dst = torch.empty(n, device=dev)
    sink = torch.zeros(1, device=dev)
    t_copy = _event_ms(lambda: _lib.check(L.gcr_probe_copy_f32(_lib.dptr(src), _lib.dptr(dst), n, st), "probe_copy"), 10)
    t_read = _event_ms(lambda: _lib.check(L.gcr_probe_read_f32(_lib.dptr(src), n, _lib.dptr(sink), st), "probe_read"), 10)
    del src, dst
    out = {"copy_GBs": round(2 * n * 4 / t_copy / 1e6, 1), "read_GBs": round(n * 4 / t_read / 1e6, 1),
           "buffer_MiB": n * 4 >> 20}
    rows = table.shape[0]
    if table.shape[1] == 64:
        n_idx = 1 << 24
        idx = torch.randint(0, rows, (n_idx,), device=dev, dtype=torch.int32)
        o = torch.empty(n_idx // 64, 64, device=dev)
        t_g = _event_ms(lambda: _lib.check(L.gcr_probe_gather_rows_f32(_lib.dptr(table), rows, _lib.dptr(idx), n_idx,
                                                                        _lib.dptr(o), st), "probe_gather"), 10)
        out["gather_256B_rows_GBs"] = round((n_idx * 260 + o.numel() * 4) / t_g / 1e6, 1)
        out["gather_table_MB"] = round(table.numel() * 4 / 1e6, 1)
    return out


def measure_propagation(ra, Fn, name, d, dev, steps, warmup):
    """Builds workload `name` through the library ingest and times `steps` K-layer forward passes (the
    Horner form, one launch per layer) with HIP events around every gcr_spmm_csr_f32 launch."""
    wl = WORKLOADS[name]
    n_u, n_i, n_e, k_layers = wl["users"], wl["items"], wl["edges"], wl["layers"]
    n = n_u + n_i
    t_build = time.time()
    users, items = synth_interactions_device(n_u, n_i, n_e, SEED, dev)
    # graph ingest through the library: gcr_coo_to_csr (radix sort + merge) + gcr_csr_sym_norm_f32
    graph = ra.CsrGraph.bipartite_sym_norm(users, items, n_u, n_i, dev)
    del users, items
    nnz = graph.nnz
    x0 = torch.empty(n, d, device=dev)
    torch.nn.init.xavier_uniform_(x0, generator=torch.Generator(device=dev).manual_seed(0))
    torch.cuda.synchronize()
    t_build = time.time() - t_build

    events = []
    Fn.EVENT_SINK = None

    def step():
        with torch.no_grad():
            return Fn.lightgcn_propagate(graph, x0, k_layers, combine="sum")

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    Fn.EVENT_SINK = events          # HIP events around every gcr_spmm_csr_f32 launch (same stream)
    t0 = time.perf_counter()
    for _ in range(steps):
        final = None        # only the last output is kept: each earlier one is released before the next step, as if discarded
        final = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    Fn.EVENT_SINK = None

    launch_ms = [a.elapsed_time(b) for a, b in events]
    avg_launch_ms = sum(launch_ms) / len(launch_ms)
    t_launch = avg_launch_ms * 1e-3
    bytes_alg = nnz * (4 + 4 + 4 * d) + n * (4 * d + 4)      # BASELINE.md §4 / SURVEY §8d, per layer
    bytes_comp = nnz * 8 + (n + 1) * 4 + 2 * n * 4 * d
    achieved = bytes_alg / t_launch / 1e9
    roofline = {
        "bound": "hbm", "kernel": "spmm_parts + spmm_long_rows (one gcr_spmm_csr_f32 launch = one layer)",
        "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
        "frac_basis": "alg: no PMC capture matches these kernel sources, so `achieved` / `frac` are the no-reuse byte "
                      "model (cache-assisted: may exceed 1)",
        "traffic": None,
        "achieved_alg": round(achieved, 1),
        "frac_alg": round(achieved / HBM_PEAK_GBS, 4),
        "frac_alg_note": "SURVEY §8d no-reuse byte model / launch time / 8 TB/s; it is cache-assisted (L2 and the "
                         "Infinity Cache serve repeated gathers), so it may exceed the fabric rate and even 1.0 — "
                         "frac_fabric is the counter-based figure",
        "frac_fabric": None,
        "frac_compulsory": round(bytes_comp / t_launch / 1e9 / HBM_PEAK_GBS, 4),
        "bytes_alg_per_launch": bytes_alg, "avg_launch_ms": round(avg_launch_ms, 4),
        "compulsory_bytes_per_launch": bytes_comp, "launches_timed": len(launch_ms),
    }
    # fabric traffic per launch from the committed rocprofv3 --pmc passes of the SAME workload and the same
    # kernel sources (FETCH_SIZE x2 on gfx950 + WRITE_SIZE, MI355X_MICROARCH.md §HBM); null otherwise
    pmc = _committed_pmc(name, spmm_source_digest(), allow_stale=True) if d == 64 else None
    if pmc:
        roofline["traffic"] = pmc["bytes_per_launch"]
        roofline["frac_fabric"] = round(pmc["bytes_per_launch"] / t_launch / 1e9 / HBM_PEAK_GBS, 4)
        # the headline pair is the PHYSICAL one: bytes the memory-side counters saw per launch / live launch time
        # (never above the fabric's rate); the no-reuse model stays beside it as achieved_alg / frac_alg
        roofline["achieved"] = round(pmc["bytes_per_launch"] / t_launch / 1e9, 1)
        roofline["frac"] = roofline["frac_fabric"]
        roofline["frac_basis"] = "fabric: rocprofv3 FETCH_SIZE x 2 + WRITE_SIZE per launch (profiles/) / live launch time"
        if pmc.get("stale_digest"):
            # the counters were captured on an earlier revision of the kernel sources: still the physical byte count of this
            # access pattern to within the epilogue edits since, and never a fraction above the fabric's rate — but say so
            roofline["traffic_stale"] = {"captured_on": pmc["source_digest"], "benchmarked": spmm_source_digest()}
            roofline["frac_basis"] += " — counters captured on an EARLIER revision of the kernel sources (traffic_stale)"
        roofline["traffic_source"] = pmc["source"]
        roofline["traffic_source_digest"] = pmc["source_digest"]
    else:
        roofline["traffic_note"] = "no committed PMC capture matches these kernel sources (digest %s)" % spmm_source_digest()
    res = {"name": name, "graph": graph, "x0": x0, "final": final, "nnz": nnz, "n": n, "n_u": n_u, "n_i": n_i, "n_e": n_e,
           "k_layers": k_layers, "elapsed": elapsed, "ms_per_step": 1e3 * elapsed / steps,
           "edges_per_s": nnz * k_layers * steps / elapsed, "roofline": roofline, "graph_build_s": round(t_build, 2)}
    return res


def infonce_roofline(Fn, x0, n_u, dev):
    """Dominant InfoNCE kernel at the NCL structure-contrast shape (ncl.py:358-367): B = 2048 anchors against
    all n_u layer-0 user rows, d = 64 — bare kernel launches (gcr_infonce_fwd_ex_f32 / gcr_infonce_bwd_ex_f32),
    HIP events on the launch stream."""
    d = x0.shape[1]
    m = 2048
    gen = torch.Generator(device=dev).manual_seed(11)
    table = x0[:n_u].contiguous()
    anchors = table[torch.randint(0, n_u, (m,), device=dev, generator=gen)] + \
        0.1 * torch.randn(m, d, device=dev, generator=gen) * table.std()
    sa, sb = Fn.row_inv_norm(anchors), Fn.row_inv_norm(table)
    inv_tau = 10.0
    # the rows are normalised by sa / sb, as in every contrast loss of the reference: the launches carry the
    # unit-rows promise and (d <= 64) run on two f16 planes per operand, THREE 16-bit MFMA products per f32 product
    # instead of the six of the three-bf16-plane format
    ef = Fn._resolve_engine(unit_rows=True)
    lse = Fn.infonce_lse_raw(anchors, sa, table, sb, inv_tau, engine_flag=ef)
    w = torch.ones(m, device=dev)
    t_f = _event_ms(lambda: Fn.infonce_lse_raw(anchors, sa, table, sb, inv_tau, engine_flag=ef), 50, warm=20)   # sustained rate
    flops = 2.0 * m * n_u * d
    from recommendation_amd import _lib
    engine = int(_lib.lib().gcr_infonce_engine(d))
    h2 = engine == 1 and d <= 64 and bool(ef & Fn.INFONCE_UNIT_ROWS) and inv_tau <= 20.0
    mult = 3 if h2 else (6 if engine == 1 else 1)        # 16-bit MFMA products per f32 product
    peak = BF16_MFMA_PEAK_TF if engine == 1 else FP32_MFMA_PEAK_TF
    mult2 = mult
    planes = "EngH2: 2 f16 planes, 3 products per f32 product" if h2 else "EngB3: 3 bf16 planes, 6 products"

    def leg(kernel, t_ms, units):
        return {"kernel": kernel, "avg_launch_ms": round(t_ms, 4), "flops_alg_per_launch": units * flops,
                "mfma_products_per_f32_product": mult2,
                "achieved_alg": round(units * flops / t_ms / 1e9, 1), "achieved": round(mult2 * units * flops / t_ms / 1e9, 1),
                "frac": round(mult2 * units * flops / t_ms / 1e9 / peak, 4), "mfma_busy_pct": None}

    # training path of a row-softmax loss (ncl.py:358-367): flash-style forward (lse + weighted row sum, the
    # anchor-side gradient is a scale of it) and ONE backward launch for the table side
    t_b = _event_ms(lambda: Fn._infonce_bwd_raw(table, sb, anchors, sa, inv_tau, None, None, lse, w, engine_flag=ef), 20, warm=5)
    fwd_o = None
    if Fn.infonce_fwd_o_supported(d):
        t_fo = _event_ms(lambda: Fn.infonce_fwd_o_raw(anchors, sa, table, sb, inv_tau, engine_flag=ef), 20, warm=5)
        fwd_o = leg(f"infonce_pipe_kernel<{planes.split(':')[0]}, 64, MODE 1> (score + softmax-weighted row sum; {planes})",
                    t_fo, 2)
    out = {
        "bound": "mfma",
        "kernel": f"infonce_fwd_e_kernel<{planes.split(':')[0]}, 64>" if engine == 1 else "infonce_fwd_kernel<64>",
        "engine": ("split-operand 16-bit MFMA, f32 accumulate (" + planes + ")") if engine == 1 else "f32 MFMA",
        "mfma_products_per_f32_product": mult,
        "shape": f"{m} x {n_u} x {d}", "pairs_per_launch": m * n_u, "flops_alg_per_launch": flops,
        "avg_launch_ms": round(t_f, 4), "pairs_per_s": m * n_u / t_f * 1e3,
        "achieved_alg": round(flops / t_f / 1e9, 1), "achieved": round(mult * flops / t_f / 1e9, 1),
        "peak": peak, "unit": "TFLOP/s", "frac": round(mult * flops / t_f / 1e9 / peak, 4),
        "note": "achieved = 16-bit MFMA flops issued (algorithmic x products per f32 product: 6 on three bf16 planes, "
                "3 on two f16 planes) / launch time; peak = dense bf16 / f16 MFMA",
        "mfma_busy_pct": None,
        "fwd_o": fwd_o,
        "bwd": leg(f"infonce_pipe_kernel<{planes.split(':')[0]}, 64, MODE 0> (table-side gradient: score recomputed once + "
                   f"one product; {planes})", t_b, 2),
    }
    if h2:
        # the same three launches with the promise withheld (three bf16 planes, six products): what the format buys,
        # measured in the same process
        t3_f = _event_ms(lambda: Fn.infonce_lse_raw(anchors, sa, table, sb, inv_tau, engine_flag=0), 5)
        t3_b = _event_ms(lambda: Fn._infonce_bwd_raw(table, sb, anchors, sa, inv_tau, None, None, lse, w, engine_flag=0), 3)
        t3_o = _event_ms(lambda: Fn.infonce_fwd_o_raw(anchors, sa, table, sb, inv_tau, engine_flag=0), 3)
        out["three_bf16_plane_format"] = {
            "avg_launch_ms": {"fwd": round(t3_f, 4), "fwd_o": round(t3_o, 4), "bwd": round(t3_b, 4)},
            "issued_frac_of_peak": {"fwd": round(6 * flops / t3_f / 1e9 / peak, 4), "fwd_o": round(12 * flops / t3_o / 1e9 / peak, 4),
                                    "bwd": round(12 * flops / t3_b / 1e9 / peak, 4)},
            "note": "EngH2 issues half the MFMA flops for the same f32 result, so its issued fraction of peak is lower "
                    "while its launches are 1.35-1.55x shorter; the limiter moved from the matrix pipe to vector issue "
                    "and waits (DESIGN 4.2b, profiles/r04_infonce_stall_counters.csv)"}
    pmc = _committed_pmc("infonce", infonce_source_digest())
    if pmc:
        out["mfma_busy_pct"] = pmc.get("fwd_mfma_busy_pct")
        out["bwd"]["mfma_busy_pct"] = pmc.get("bwd_mfma_busy_pct")
        if out["fwd_o"] is not None:
            out["fwd_o"]["mfma_busy_pct"] = pmc.get("fwdo_mfma_busy_pct")
        out["mfma_busy_source"] = pmc.get("source")
    return out


def self_launch(n_ranks):
    """`python bench.py --gpus N` without a launcher: run `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port <free> bench.py <same arguments>` as a child process (one rank per GPU, the
    contract's own launch line) and exit with its code.  Called before anything initialises the GPU."""
    import socket
    import subprocess
    with socket.socket() as sock:                     # a free rendezvous port on the loopback interface
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    sys.stdout.flush()
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def init_only(rank, world):
    """GCR_BENCH_INIT_ONLY=1: every rank joins the process group (gloo, CPU), meets at a barrier and rank 0 prints one line
    — the launch path of `--gpus N` exercised without a GPU (tests/test_host_logic_cpu.py)."""
    import torch.distributed as dist
    dist.init_process_group(backend="gloo")
    seen = torch.ones(1)
    dist.all_reduce(seen)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"init_only": True, "dist_backend": dist.get_backend(), "dist_world": dist.get_world_size(),
                          "ranks_seen": int(seen.item())}))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS) + ["cfg5"])
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="N > 1: weak = a cfg2-sized user block per rank; strong = the fixed workload graph over N ranks")
    ap.add_argument("--full", action="store_true",
                    help="after the headline line's steps, also run every secondary leg (probes, rooflines, extra rates, CPU "
                         "baseline, companion workloads); the --no-* options below trim a --full run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32, at most 48 MiB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true")
    ap.add_argument("--no-cfg4", action="store_true", help="skip the 10M x 1M / 100M-edge 1-GPU companion line")
    ap.add_argument("--gcl-full", action="store_true",
                    help="N > 1: run the GCL step leg on the benchmark graph itself (all-pairs user InfoNCE is O(U^2): minutes)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1:
            # plain `python bench.py --gpus N`: start the N ranks ourselves.  Nothing in this process has touched the GPU
            # (importing torch does not), and it never will: the ranks are children, their output is relayed, their exit
            # code is ours.
            return self_launch(args.gpus)
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if os.environ.get("GCR_BENCH_INIT_ONLY") == "1":
        return init_only(rank, world)
    if os.environ.get("GCR_BENCH_REHEARSE_ONE_GPU") == "1":
        local_rank = 0      # rehearsal of the N-rank code path on a one-GPU box: ranks share cuda:0 over gloo
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import recommendation_amd as ra
    from recommendation_amd import functional as Fn

    if world > 1 or os.environ.get("GCR_BENCH_FORCE_DIST") == "1":
        return main_sharded(args, rank, world, dev, ra)
    if args.workload == "cfg5":
        return main_cfg5(args, rank, world, dev, ra)

    name = args.workload or "cfg2"
    d = args.dim
    r = measure_propagation(ra, Fn, name, d, dev, args.steps, args.warmup)
    graph, x0, nnz, n, n_u, n_i, k_layers = r["graph"], r["x0"], r["nnz"], r["n"], r["n_u"], r["n_i"], r["k_layers"]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"final_embeddings": r["final"]})
    del r["final"]
    roofline = r["roofline"]
    extra = {"graph_build_s": r["graph_build_s"], "nnz": nnz, "n_nodes": n,
             "spmm_parts": graph.plan.n_parts, "spmm_split_rows": graph.plan.n_long}
    infonce_pairs_per_s = None
    cpu = None
    if args.full:
        infonce_pairs_per_s, cpu = full_legs(args, ra, Fn, r, name, d, dev, roofline, extra)

    line = {
        "metric": "edges propagated/sec (LightGCN d=%d, %d-layer fwd message pass)" % (d, k_layers),
        "value": r["edges_per_s"], "unit": "edges/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": r["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic", "full": args.full,
        "config": {"workload": f"{name}: LightGCN {k_layers}-layer d={d}, {n_u} users x {n_i} items / {r['n_e']} "
                               f"interactions (nnz={nnz}), sym-normalised CSR, forward propagation + fused layer sum",
                   "users": n_u, "items": n_i, "interactions": r["n_e"], "layers": k_layers, "dim": d},
        "infonce_pairs_per_s": infonce_pairs_per_s,
        "roofline": roofline, "roofline_infonce": roofline.get("infonce"), "cpu_baseline": cpu,
        "dist_backend": None, "dist_world": 1, "extra": extra,
    }
    print(json.dumps(line))


def full_legs(args, ra, Fn, r, name, d, dev, roofline, extra):
    """--full on one GPU: every secondary leg after the headline steps, filling `roofline` and `extra` in place; returns
    (InfoNCE pairs/s, CPU baseline).  Each leg is secondary: a failure is reported in the line, never costs it."""
    graph, x0, nnz, n_u, n_i, k_layers = r["graph"], r["x0"], r["nnz"], r["n_u"], r["n_i"], r["k_layers"]
    try:
        roofline["probe"] = memory_probes(x0, dev)
    except Exception as e:      # noqa: BLE001
        roofline["probe_error"] = repr(e)
    infonce_pairs_per_s = None
    if d == 64 and n_u >= 100000:
        try:
            roofline["infonce"] = infonce_roofline(Fn, x0, n_u, dev)
            infonce_pairs_per_s = roofline["infonce"]["pairs_per_s"]
        except Exception as e:      # noqa: BLE001
            roofline["infonce_error"] = repr(e)
    if not args.no_extra:
        try:
            extra.update(bench_extra(ra, Fn, graph, x0, k_layers, nnz, dev, n_u, n_i))
        except Exception as e:      # noqa: BLE001
            extra["extra_error"] = repr(e)

    cpu = None
    if not args.no_cpu_baseline:
        try:
            cpu = cpu_baseline(graph, x0, k_layers, nnz, n_u, n_i)
        except Exception as e:      # noqa: BLE001
            cpu = {"value": None, "unit": "edges/s", "cores": 0, "kind": "port", "sample": "failed: " + repr(e)}

    # the graph the >= 60 % target is quoted on (10M x 1M / 100M interactions) fits one GPU (~6 GB): same timed
    # step, its own roofline block
    if name != "cfg4" and not args.no_cfg4 and d == 64:
        try:
            del graph, x0
            r4 = measure_propagation(ra, Fn, "cfg4", d, dev, max(3, args.steps // 4), 2)
            try:
                r4["roofline"]["probe"] = memory_probes(r4["x0"], dev)
            except Exception as e:      # noqa: BLE001
                r4["roofline"]["probe_error"] = repr(e)
            roofline["cfg4_graph"] = {
                "workload": "cfg4 on 1 GPU: 10000000 users x 1000000 items / 100000000 interactions (nnz=%d), 3-layer "
                            "d=64 forward" % r4["nnz"],
                "edges_per_s": r4["edges_per_s"], "ms_per_step": r4["ms_per_step"], "graph_build_s": r4["graph_build_s"],
                "spmm_parts": r4["graph"].plan.n_parts, "spmm_split_rows": r4["graph"].plan.n_long,
                **r4["roofline"]}
            del r4
        except Exception as e:      # noqa: BLE001
            roofline["cfg4_graph_error"] = repr(e)

    # secondary workload: graphs with community structure, before / after the locality renumbering
    if not args.no_extra and d == 64 and name in ("cfg2", "cfg4"):
        extra["community_graph"] = {}
        for wl_name in ("cfg2",) if args.no_cfg4 else ("cfg2", "cfg4"):
            try:
                extra["community_graph"][wl_name] = community_leg(ra, Fn, dev, wl_name, d)
            except Exception as e:      # noqa: BLE001
                extra["community_graph"][wl_name] = {"error": repr(e)[:200]}
            torch.cuda.empty_cache()

    # BASELINE configs[3] and [4] at one GPU (their N-rank forms run under --gpus N): the GCL two-view step of gcl.py:205-227
    # through the single-rank sharded path, and MHCN's 2-layer multi-channel pass forward and forward + backward
    if not args.no_extra and d == 64:
        try:
            c5, _ = cfg5_measure(d, 5, 2, 0, 1, dev, ra)
            extra["cfg5"] = {"workload": c5["config"]["workload"], "edges_per_s": c5["value"], "fwd_ms": c5["ms_per_step"],
                             "fwd_bwd_ms": c5["extra"]["fwd_bwd_ms"], "fwd_bwd_over_fwd": c5["extra"]["fwd_bwd_over_fwd"],
                             "frac_alg": c5["roofline"]["frac"]}
        except Exception as e:      # noqa: BLE001
            extra["cfg5"] = {"error": repr(e)[:300]}
        torch.cuda.empty_cache()
        try:
            from recommendation_amd import distributed as gdist
            dist = _init_dist(dev)                                  # one rank: RCCL group of size 1 (no collective moves data)
            try:
                extra["gcl_step"] = gcl_step_leg(ra, gdist, dist, dev, 0, 1, d, None)
            finally:
                dist.destroy_process_group()
        except Exception as e:      # noqa: BLE001
            extra["gcl_step"] = {"error": repr(e)[:300]}
        torch.cuda.empty_cache()
    return infonce_pairs_per_s, cpu


def _init_dist(dev):
    import torch.distributed as dist
    if not dist.is_initialized():
        if "RANK" not in os.environ:             # single process through the sharded path (GCR_BENCH_FORCE_DIST=1)
            os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1",
                              MASTER_PORT=os.environ.get("MASTER_PORT", "29533"))
        if os.environ.get("GCR_BENCH_REHEARSE_ONE_GPU") == "1":
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=dev)
    return dist


def _timed_ranks(dist, dev, step, warmup, steps):
    """W untimed + K timed steps between barrier + synchronize on both sides; (MAX over ranks in seconds, what the last
    step returned)."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = None          # only the last output is kept: each earlier one is released before the next step, as if discarded
        out = step()
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    elapsed = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
    dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    return float(elapsed.item()), out


def build_sharded_bipartite(ra, gdist, dist, dev, rank, world, n_u_local, n_i, users, items):
    """This rank's blocks of the symmetric-normalised bipartite operator from its own (local user id, item id)
    interactions: global item degrees by all-reduce, blocks through the library ingest (gcr_coo_to_csr +
    device transpose, which also gives ShardedEdgeDrop its nnz correspondence)."""
    per_i, i_pad = gdist.shard_bounds(n_i, world)
    deg_i = torch.bincount(items, minlength=n_i)
    dist.all_reduce(deg_i)                                       # global item degrees (integer)
    deg_u = torch.bincount(users, minlength=n_u_local)
    du, di = deg_u.float().pow(-0.5), deg_i.float().pow(-0.5)
    du[torch.isinf(du)] = 0.0
    di[torch.isinf(di)] = 0.0
    r_ui = ra.CsrGraph.from_coo(users, items, du[users] * di[items], n_u_local, i_pad, dev, coalesce=True)
    r_iu = r_ui.t
    return gdist.ShardedBipartiteGraph(r_ui, r_iu, n_u_local, n_i, per_i, rank, world)


def local_interactions(name, scaling, rank, world, dev, gdist):
    """(local user ids, item ids, users on this rank, global users, items, global interactions).
    weak: every rank draws its own `users` x (items * world) block (the item popularity law is shared);
    strong: the ONE global graph of the workload, generated identically on every rank (same seed) and
    filtered to the rank's contiguous user block."""
    wl = WORKLOADS[name]
    if scaling == "weak":
        n_u, n_i = wl["users"], wl["items"] * world
        users, items = synth_interactions_device(n_u, n_i, wl["edges"], SEED + 7919 * (rank + 1), dev, perm_seed=SEED)
        return users, items, n_u, n_u * world, n_i, wl["edges"] * world
    n_ug, n_i = wl["users"], wl["items"]
    per_u, _ = gdist.shard_bounds(n_ug, world)
    users, items = synth_interactions_device(n_ug, n_i, wl["edges"], SEED, dev)
    lo = rank * per_u
    sel = (users >= lo) & (users < lo + per_u)
    return (users[sel] - lo).contiguous(), items[sel].contiguous(), per_u, n_ug, n_i, wl["edges"]


GCL_LEG = dict(users=1 << 18, items=1 << 15, edges=(1 << 18) * 10, layers=3)   # per rank (weak): the step is O(U^2)


def gcl_step_leg(ra, gdist, dist, dev, rank, world, d, full_graph=None):
    """One sharded SSL4Rec / GCL training step (gcl.py:205-227 with the propagation BASELINE config 4 names):
    two edge-dropped views (ShardedEdgeDrop, independent draws per stored non-zero), K-layer sharded
    propagation of each, all-pairs symmetric InfoNCE over users and over items between the views
    (row-sharded anchors against the all-gathered other view: two row-logsumexp launches forward, one both-sided
    backward launch per local table — distributed._ShardedSymInfoNCE), BPR on a batch, backward incl. the reduce-scatter
    of the item gradients, on its own named workload (the all-pairs user InfoNCE is O(U^2))."""
    from recommendation_amd import functional as Fn
    wl = GCL_LEG
    if full_graph is None:
        n_u, n_i, k_layers = wl["users"], wl["items"] * world, wl["layers"]
        users, items = synth_interactions_device(n_u, n_i, wl["edges"], SEED + 104729 * (rank + 1), dev, perm_seed=SEED)
        g = build_sharded_bipartite(ra, gdist, dist, dev, rank, world, n_u, n_i, users, items)
    else:
        g, users, items, k_layers = full_graph
        n_u, n_i = g.n_local_users, g.num_items
    gen = torch.Generator(device=dev).manual_seed(100 + rank)
    bound = (6.0 / (n_u * world + n_i + d)) ** 0.5
    x_u = ((torch.rand(n_u, d, device=dev, generator=gen) * 2 - 1) * bound).requires_grad_(True)
    x_i = ((torch.rand(g.items_per_rank, d, device=dev, generator=gen) * 2 - 1) * bound).requires_grad_(True)
    bsz = 2048
    sel = torch.randint(0, users.numel(), (bsz,), device=dev, generator=gen)
    bu, bi = users[sel], items[sel]
    bj = torch.randint(0, n_i, (bsz,), device=dev, generator=gen)
    pe, temp = 0.2, 0.2
    state = {"n": 0}

    def step():
        state["n"] += 1
        x_u.grad = x_i.grad = None
        v1 = gdist.ShardedEdgeDrop(g, pe, seed=2 * state["n"] + 1)
        v2 = gdist.ShardedEdgeDrop(g, pe, seed=2 * state["n"] + 2)
        u1, i1 = gdist.sharded_lightgcn_propagate(g, x_u, x_i, k_layers, "mean", view=v1)
        u2, i2 = gdist.sharded_lightgcn_propagate(g, x_u, x_i, k_layers, "mean", view=v2)
        ssl = gdist.sharded_info_nce_loss(u1, u2, temp) + gdist.sharded_info_nce_loss(i1, i2, temp)
        items_full = gdist.gather_items(i1)[: n_i]
        sums = Fn.bpr_sums(u1, items_full, bu, bi, bj, Fn.BPR_LOGSIGMOID)
        loss = ssl + sums[0] / bsz + 1e-4 * (sums[1] + sums[2] + sums[3]) / bsz
        loss.backward()

    t, _ = _timed_ranks(dist, dev, step, 1, 2)
    n_edges = torch.tensor([g.r_ui.nnz + g.r_iu.nnz], device=dev, dtype=torch.int64)
    dist.all_reduce(n_edges)
    u_tot, i_tot = n_u * world, g.items_padded
    pairs = u_tot * u_tot + i_tot * i_tot                     # logits of the two all-pairs similarity matrices
    return {"workload": f"gcl step: {u_tot} users ({n_u}/GPU) x {n_i} items, nnz={int(n_edges)}, {k_layers}-layer d={d}, "
                        f"two edge-dropped views (pe={pe}) + all-pairs InfoNCE(users) + InfoNCE(items) + BPR(B={bsz}) + backward",
            "ms_per_step": 1e3 * t / 2, "infonce_pairs_per_s": pairs * 2 / t,
            "edges_per_s_fwd_bwd": int(n_edges) * k_layers * 2 * 2 * 2 / t,
            "pairs_per_step": pairs, "note": "pairs = U^2 + I^2 logits per step (each feeds a row and a column softmax)"}


def main_sharded(args, rank, world, dev, ra):
    """N > 1: one rank per GPU, users row-sharded, items all-gathered / reduce-scattered over xGMI every layer
    (recommendation_amd/distributed.py).  --scaling weak (default): every rank brings its own cfg2-sized block
    (1M users / 10M interactions) and the item side grows with N (100K x N items), so N = 8 is 8M users x 800K
    items / 80M interactions — the cfg4 regime; --scaling strong: the fixed graph of --workload (cfg4: 10M x 1M /
    100M interactions) split over the N ranks."""
    from recommendation_amd import distributed as gdist
    dist = _init_dist(dev)
    if os.environ.get("GCR_BENCH_FORCE_COLLECTIVES") == "1":      # one rank, real RCCL calls (degenerate copies)
        gdist.FORCE_COLLECTIVES = True
    name = args.workload or ("cfg4" if args.scaling == "strong" else "cfg2")
    if name == "cfg5":
        return main_cfg5(args, rank, world, dev, ra)
    k_layers, d = WORKLOADS[name]["layers"], args.dim

    def propagation_leg(wl_name, scaling, steps, warmup):
        """One sharded K-layer forward leg: (rank-local state, whole-job numbers)."""
        users, items, n_u, n_u_total, n_i, n_e_total = local_interactions(wl_name, scaling, rank, world, dev, gdist)
        graph = build_sharded_bipartite(ra, gdist, dist, dev, rank, world, n_u, n_i, users, items)
        nnz_local = graph.r_ui.nnz + graph.r_iu.nnz
        gen = torch.Generator(device=dev).manual_seed(rank)
        bound = (6.0 / (n_u_total + n_i + d)) ** 0.5                  # xavier_uniform of the global table
        x_u = (torch.rand(n_u, d, device=dev, generator=gen) * 2 - 1) * bound
        x_i = (torch.rand(graph.items_per_rank, d, device=dev, generator=gen) * 2 - 1) * bound
        torch.cuda.synchronize()

        def step():
            with torch.no_grad():
                return gdist.sharded_propagate_raw(graph, x_u, x_i, WORKLOADS[wl_name]["layers"], 1.0)

        elapsed, final = _timed_ranks(dist, dev, step, warmup, steps)
        nnz_all = torch.tensor([nnz_local], device=dev, dtype=torch.int64)
        dist.all_reduce(nnz_all)
        return dict(users=users, items=items, graph=graph, n_u=n_u, n_u_total=n_u_total, n_i=n_i, n_e_total=n_e_total,
                    nnz_all=int(nnz_all.item()), elapsed=elapsed, steps=steps, final=final)

    leg = propagation_leg(name, args.scaling, args.steps, args.warmup)
    users, items, graph = leg["users"], leg["items"], leg["graph"]
    n_u, n_u_total, n_i, n_e_total, nnz_all, elapsed = (leg[k] for k in ("n_u", "n_u_total", "n_i", "n_e_total", "nnz_all",
                                                                         "elapsed"))
    if args.dump_outputs and rank == 0:                           # rank 0's user block and item shard
        dump_outputs(args.dump_outputs, {"user_embeddings": leg["final"][0], "item_embeddings": leg["final"][1]})
    del leg["final"]
    gcl = None
    if args.full and not args.no_extra:
        try:
            full = (graph, users, items, k_layers) if args.gcl_full else None
            gcl = gcl_step_leg(ra, gdist, dist, dev, rank, world, d, full)
            del full
        except Exception as e:      # noqa: BLE001  (secondary: never costs the headline line)
            gcl = {"error": repr(e)[:300]}
    # BASELINE configs[3] itself: the FIXED 10M x 1M / 100M-interaction graph split over the N ranks (strong scaling), next
    # to the weak-scaling headline whose N = 1 point is the single-GPU bench line
    cfg4_strong = None
    items_padded = graph.items_padded
    if args.full and not (name == "cfg4" and args.scaling == "strong") and not args.no_cfg4 and d == 64:
        try:
            del users, items, graph
            leg.clear()
            torch.cuda.empty_cache()
            s4 = propagation_leg("cfg4", "strong", max(3, args.steps // 4), 2)
            k4 = WORKLOADS["cfg4"]["layers"]
            t4 = s4["elapsed"] / s4["steps"]
            b4 = s4["nnz_all"] * (8 + 4 * d) + (s4["n_u_total"] + s4["n_i"]) * (4 * d + 4)
            cfg4_strong = {
                "workload": f"cfg4 x{world} (strong): LightGCN {k4}-layer d={d}, {s4['n_u_total']} users (row-sharded, "
                            f"{s4['n_u']}/GPU) x {s4['n_i']} items / {s4['n_e_total']} interactions (nnz={s4['nnz_all']})",
                "scaling": "strong", "edges_per_s": s4["nnz_all"] * k4 / t4, "ms_per_step": 1e3 * t4, "steps": s4["steps"],
                "frac_alg": round(b4 * k4 / t4 / 1e9 / (HBM_PEAK_GBS * world), 4),
                "note": "1-GPU point of this curve: roofline.cfg4_graph of the N = 1 bench line"}
            del s4
        except Exception as e:      # noqa: BLE001  (secondary: never costs the headline line)
            cfg4_strong = {"error": repr(e)[:300]}
    if rank == 0:
        n_nodes = n_u_total + n_i
        bytes_alg = nnz_all * (8 + 4 * d) + n_nodes * (4 * d + 4)
        per_layer_s = elapsed / (args.steps * k_layers)
        achieved = bytes_alg / per_layer_s / 1e9
        line = {
            "metric": "edges propagated/sec (LightGCN d=%d, %d-layer fwd message pass)" % (d, k_layers),
            "value": nnz_all * k_layers * args.steps / elapsed, "unit": "edges/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{name} x{world} ({args.scaling}): LightGCN {k_layers}-layer d={d}, {n_u_total} users "
                                   f"(row-sharded, {n_u}/GPU) x {n_i} items / {n_e_total} interactions "
                                   f"(nnz={nnz_all}); all-gather + reduce-scatter of the item table per layer",
                       "users": n_u_total, "items": n_i, "interactions": n_e_total, "layers": k_layers, "dim": d,
                       "parallelism": f"user-row shards x{world}, items replicated for compute"},
            "infonce_pairs_per_s": None if not gcl or "error" in gcl else gcl["infonce_pairs_per_s"],
            "roofline": {"bound": "hbm", "kernel": "spmm_parts (per-layer wall time incl. collectives)",
                         "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                         "frac": round(achieved / (HBM_PEAK_GBS * world), 4), "traffic": None,
                         "frac_basis": "alg: the no-reuse byte model over the per-layer WALL time incl. collectives / (8 TB/s x N); "
                                       "no PMC capture exists for N > 1 (the 1-GPU line carries the counter-based fraction)",
                         "frac_alg": round(achieved / (HBM_PEAK_GBS * world), 4),
                         "collective_bytes_per_rank_per_layer": 2 * items_padded * d * 4 * (world - 1) // world},
            "cpu_baseline": None, "dist_backend": dist.get_backend(), "dist_world": dist.get_world_size(), "full": args.full,
            "gcl_step": gcl, "cfg4_strong": cfg4_strong,
        }
        print(json.dumps(line))
    dist.destroy_process_group()


CFG5 = dict(users=250_000, items=50_000, deg=(24, 16, 8), deg_r=10, layers=2)       # per rank (weak)


def main_cfg5(args, rank, world, dev, ra):
    line, final = cfg5_measure(args.dim, args.steps, args.warmup, rank, world, dev, ra, fwd_bwd=args.full)
    if rank == 0:
        if args.dump_outputs:                                     # rank 0's outputs
            dump_outputs(args.dump_outputs, {"user_embeddings": final[0], "item_embeddings": final[1]})
        line["full"] = args.full
        print(json.dumps(line))
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def cfg5_measure(d, steps, warmup, rank, world, dev, ra, fwd_bwd=True):
    """BASELINE config 5: MHCN's layer loop (univariate/mhcn.py:422-466) with the three U x U channel operators
    row-sharded by user: per layer three all-gathers of [U, d] channel operands, each overlapped with the
    previous channel's dual-output SpMM on its own stream, plus the R^T / R item side (all-reduce of the partial
    item sums).  Synthetic operators: `deg` random columns per row and channel, row-normalised (the motif
    adjacency of a real social graph comes from graph_ops.build_hyper_graphs).  fwd_bwd: also time forward + backward
    (extra.fwd_bwd_ms).  Returns (rank 0's line or None, what the last timed forward returned)."""
    import torch.distributed as dist
    from recommendation_amd import distributed as gdist
    from recommendation_amd.mhcn import ShardedMHCNEncoder
    if world > 1 or os.environ.get("GCR_BENCH_FORCE_COLLECTIVES") == "1":
        dist = _init_dist(dev)
        gdist.FORCE_COLLECTIVES = os.environ.get("GCR_BENCH_FORCE_COLLECTIVES") == "1"
    per_u, n_i, k_layers = CFG5["users"], CFG5["items"], CFG5["layers"]
    u_pad = per_u * world
    gen = torch.Generator(device=dev).manual_seed(SEED + rank)
    rows = torch.arange(per_u, device=dev)

    def rand_block(n_cols, deg):
        r = rows.repeat_interleave(deg)
        c = torch.randint(0, n_cols, (per_u * deg,), device=dev, generator=gen)
        return ra.CsrGraph.row_normalised(r, c, None, per_u, n_cols, dev)

    blocks = [rand_block(u_pad, k) for k in CFG5["deg"]]
    r_local = rand_block(n_i, CFG5["deg_r"])
    ch = gdist.ShardedChannels(blocks, per_u, rank, world)
    enc = ShardedMHCNEncoder(ch, r_local, d, k_layers)
    nnz_local = sum(b.nnz for b in blocks) + 2 * r_local.nnz
    torch.cuda.synchronize()

    def step():
        with torch.no_grad():
            return enc.propagate()

    def step_fb():
        enc.zero_grad(set_to_none=True)
        fu, fi = enc.propagate()
        (fu.sum() + fi.sum() / world).backward()
        enc.allreduce_grads()

    t_fb = None
    if world > 1:
        elapsed, final = _timed_ranks(dist, dev, step, warmup, steps)
        if fwd_bwd:
            t_fb = _timed_ranks(dist, dev, step_fb, 1, 3)[0] / 3
        nnz_all = torch.tensor([nnz_local], device=dev, dtype=torch.int64)
        dist.all_reduce(nnz_all)
        nnz_all = int(nnz_all.item())
    else:
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            final = None    # only the last output is kept: each earlier one is released before the next step, as if discarded
            final = step()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if fwd_bwd:
            step_fb()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                step_fb()
            torch.cuda.synchronize()
            t_fb = (time.perf_counter() - t0) / 3
        nnz_all = nnz_local
    line = None
    if rank == 0:
        n_rows = u_pad * 4 + n_i                                       # output rows of the five operators
        bytes_alg = nnz_all * (8 + 4 * d) + n_rows * (2 * 4 * d + 4)   # dual epilogue: two output rows
        achieved = bytes_alg * k_layers * steps / elapsed / 1e9
        line = {
            "metric": "edges propagated/sec (MHCN d=%d, %d-layer multi-channel message pass)" % (d, k_layers),
            "value": nnz_all * k_layers * steps / elapsed, "unit": "edges/s", "n_gpus": world,
            "steps": steps, "warmup": warmup, "ms_per_step": 1e3 * elapsed / steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"cfg5 x{world}: MHCN {k_layers}-layer d={d}, {u_pad} users ({per_u}/GPU) x {n_i} items; "
                                   f"H_s/H_j/H_p with {CFG5['deg']} nnz per row, R with {CFG5['deg_r']} (nnz={nnz_all}); "
                                   "three channel all-gathers per layer overlapped with the previous channel's SpMM",
                       "users": u_pad, "items": n_i, "layers": k_layers, "dim": d,
                       "parallelism": f"user-row shards x{world}, items replicated"},
            "roofline": {"bound": "hbm", "kernel": "spmm_parts dual epilogue (per-step wall time incl. gating / attention "
                                                   "GEMMs and collectives)",
                         "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                         "frac": round(achieved / (HBM_PEAK_GBS * world), 4), "traffic": None},
            "cpu_baseline": None, "dist_backend": dist.get_backend() if dist.is_initialized() else None, "dist_world": world,
            "extra": {} if t_fb is None else {"fwd_bwd_ms": 1e3 * t_fb, "fwd_bwd_over_fwd": round(t_fb * steps / elapsed, 3)},
        }
    return line, final


def bench_extra(ra, Fn, graph, x0, k_layers, nnz, dev, n_u, n_i):
    """Secondary rates, each timed on its own (not part of `value`)."""
    out = {}

    def timeit(fn, reps):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps

    xg = x0.clone().requires_grad_(True)

    def fwd_bwd():
        xg.grad = None
        Fn.lightgcn_propagate(graph, xg, k_layers, combine="mean").sum().backward()

    t = timeit(fwd_bwd, 5)
    out["fwd_bwd_edges_per_s"] = nnz * 2 * k_layers / t
    out["fwd_bwd_ms"] = 1e3 * t
    del xg

    # InfoNCE pairs/s at the NCL per-batch shapes: B=2048 anchors against all users
    # and all items (ncl.py:358-367) + two 2048 x 2048 prototype blocks (ncl.py:369-375)
    from recommendation_amd import losses as Ls
    d = x0.shape[1]
    gen = torch.Generator(device=dev).manual_seed(1)
    bsz = 2048
    uidx = torch.randint(0, n_u, (bsz,), device=dev, generator=gen)
    iidx = torch.randint(0, n_i, (bsz,), device=dev, generator=gen)
    ctx = x0 + 0.1 * torch.randn(x0.shape, device=dev, generator=gen)
    cent = torch.randn(2000, d, device=dev, generator=gen)
    u2c = torch.randint(0, 2000, (n_u,), device=dev, generator=gen)
    i2c = torch.randint(0, 2000, (n_i,), device=dev, generator=gen)
    pairs = bsz * (n_u + n_i) + 2 * bsz * bsz

    def ncl_contrast(x_init, x_ctx):
        return Ls.ssl_layer_loss(x_ctx, x_init, uidx, iidx, n_u, 0.1, 1e-6, 1.5) + \
            Ls.ProtoNCE_loss(x_init, uidx, iidx, n_u, cent, u2c, cent, i2c, 0.1, 8e-8, bsz)

    with torch.no_grad():
        t_f = timeit(lambda: ncl_contrast(x0, ctx), 5)
    xi, xc = x0.clone().requires_grad_(True), ctx.clone().requires_grad_(True)

    def contrast_fb():
        xi.grad = xc.grad = None
        ncl_contrast(xi, xc).backward()

    t_fb = timeit(contrast_fb, 3)
    out["infonce"] = {
        "shapes": f"{bsz} x {n_u} + {bsz} x {n_i} + 2 x {bsz} x {bsz}, d={d}",
        "pairs_per_s_fwd": pairs / t_f, "fwd_ms": 1e3 * t_f, "fwd_tflops": 2 * pairs * d / t_f / 1e12,
        "pairs_per_s_fwd_bwd": pairs / t_fb, "fwd_bwd_ms": 1e3 * t_fb,
        "engine": "split-operand 16-bit MFMA, f32 accumulate: two f16 planes / 3 terms per product (rows normalised by "
                  "the loss, d <= 64); three bf16 planes / 6 terms otherwise",
        "fwd_mfma_issued_tflops": round(3 * 2 * pairs * d / t_f / 1e12, 1),
        "fwd_frac_of_bf16_mfma_peak": round(3 * 2 * pairs * d / t_f / 1e12 / BF16_MFMA_PEAK_TF, 4),
        "note": "fwd includes gathers, row norms, positive logits and the loss reductions; fwd_tflops counts the "
                "algorithmic 2*M*N*d, the engine issues 3x that on the f16 MFMA"}
    del xi, xc, ctx

    # BPR + sampler (B = 2048 as ncl.py:293; and lightgcn.py's full batch B = E)
    ut, it = x0[:n_u], x0[n_u:]
    for name, b in (("b2048", 2048), ("full_batch", nnz // 2)):
        u = torch.randint(0, n_u, (b,), device=dev, generator=gen)
        i = torch.randint(0, n_i, (b,), device=dev, generator=gen)
        j = torch.randint(0, n_i, (b,), device=dev, generator=gen)
        with torch.no_grad():
            t_b = timeit(lambda: Fn.bpr_sums(ut, it, u, i, j, Fn.BPR_NCL), 10)
        out[f"bpr_triples_per_s_{name}"] = b / t_b
    rowptr_u = graph.rowptr[: n_u + 1].contiguous()
    items_u = (graph.col[: int(rowptr_u[-1])] - n_u).contiguous()
    ub = torch.randint(0, n_u, (1 << 20,), device=dev, generator=gen)
    t_s = timeit(lambda: Fn.neg_sample(rowptr_u, items_u, ub, 1, n_i, 7, 0, 101), 10)
    out["neg_samples_per_s"] = ub.numel() / t_s
    jn = Fn.neg_sample(rowptr_u, items_u, uidx, 1, n_i, 3, 0, 101)

    # one whole NCL training iteration at cfg3 scale (BASELINE configs[2]; the loop body ncl.py:311-329): propagate, BPR,
    # structure contrast, the PER-BATCH e_step (ncl.py:324: two k-means + assignment of every user and item), prototype
    # contrast, backward, Adam.  `ncl_train_step_full_ms` is that body as the reference defines it; `ncl_train_step_ms`
    # leaves the e_step out (round 2's number: NOT the reference's loop body, kept to show the e_step's share).
    out.update(ncl_step_legs(Fn, graph, x0, k_layers, n_u, n_i, uidx, iidx, jn, timeit))
    from recommendation_amd.optim import FusedAdam
    xp = torch.nn.Parameter(x0.clone())
    opt = FusedAdam([xp], lr=1e-3)                      # gcr_adam_step_f32 (ncl.py:305 / lightgcn.py:84 torch.optim.Adam)

    # one whole lightgcn.py training step (lightgcn.py:91-118): full batch = every training edge, fresh
    # torch.randint negatives, -log(sigmoid) BPR + L2 on the batch rows, backward, Adam
    eu = torch.repeat_interleave(torch.arange(n_u, device=dev), rowptr_u[1:] - rowptr_u[:-1])
    ei = items_u.to(torch.int64)

    def lightgcn_step():
        neg = torch.randint(0, n_i, (eu.numel(),), device=dev, generator=gen)
        final = Fn.lightgcn_propagate(graph, xp, k_layers, "sum")
        s = Fn.bpr_edge_sums(graph, final, n_u, neg, Fn.BPR_LOG_SIGMOID)       # (eu, ei) = the graph's own edge list
        loss = s[0] / eu.numel() + 1e-4 * (s[1] + s[2]) / eu.numel()
        opt.zero_grad()
        loss.backward()
        opt.step()

    out["lightgcn_full_batch_step_ms"] = 1e3 * timeit(lightgcn_step, 5)
    out["lightgcn_full_batch_edges"] = int(eu.numel())
    del xp, opt
    try:
        out["lightgcn_bce"] = bce_legs(ra, Fn, graph, x0, k_layers, n_u, n_i, dev, timeit)
    except Exception as e:      # noqa: BLE001
        out["lightgcn_bce"] = {"error": repr(e)[:300]}

    # the stages either side of the path: NCL's k-means E-step and full-ranking eval
    from recommendation_amd.evaluate import rank_topk
    from recommendation_amd.kmeans import run_kmeans
    if n_u >= 100000:
        t_k = timeit(lambda: run_kmeans(x0[:n_u], 2000, niter=20), 2)
        out["kmeans_users_k2000_20iter_ms"] = 1e3 * t_k
        q = torch.arange(0, min(n_u, 100000), device=dev)
        t_r = timeit(lambda: rank_topk(ut, it, q, rowptr_u, items_u, 50), 2)
        out["full_ranking_users_per_s"] = q.numel() / t_r
    return out


def bce_legs(ra, Fn, graph, x0, k_layers, n_u, n_i, dev, timeit):
    """The `loss_type == "bce"` branch of lightgcn.py's step (lightgcn.py:109-113): BCE-with-logits of the all-pairs scores
    [E, I] against one-hot labels.  (i) the bare all-pairs part at 2^18 user rows x all items (fused softplus row sums,
    forward, and forward + both gradients); (ii) the whole cfg1-sized training step (943 x 1682, 80 000 edges: the
    reference's own feasible size, its [E, I] matrix is 135 M logits); (iii) the whole step on the benchmark graph — the
    reference would materialise E x I = 10^12 logits; here the softplus part runs over the U distinct users weighted by
    their edge counts (U x I = 10^11 pairs), the positive logits are one SpMM."""
    from recommendation_amd.encoders import LightGCN
    from recommendation_amd.optim import FusedAdam
    out = {}
    d = x0.shape[1]
    m = min(1 << 18, n_u)
    a, b = (x0[:m] * 8).contiguous(), (x0[n_u:] * 8).contiguous()       # trained-scale rows (scores of a few tenths .. units)
    pairs = m * n_i
    legs = {}
    for eng, terms in (("auto", 3), ("b3", 6)):
        with torch.no_grad():
            t_f = _event_ms(lambda: Fn.bce_softplus_rowsum(a, b, engine=eng), 3)
        ag, bg = a.clone().requires_grad_(True), b.clone().requires_grad_(True)

        def fb():
            ag.grad = bg.grad = None
            Fn.bce_softplus_rowsum(ag, bg, engine=eng).sum().backward()

        t_fb = _event_ms(fb, 3)
        legs[eng] = {"fwd_ms": round(t_f, 3), "fwd_bwd_ms": round(t_fb, 3), "pairs_per_s_fwd": pairs / t_f * 1e3,
                     "pairs_per_s_fwd_bwd": pairs / t_fb * 1e3, "mfma_products_per_f32_product": terms,
                     "mfma_issued_frac_fwd_bwd": round(terms * 4 * 2.0 * pairs * d / t_fb / 1e9 / BF16_MFMA_PEAK_TF, 4)}
    out["all_pairs"] = {"shape": f"{m} x {n_i} x {d}", "pairs": pairs, **legs["auto"],
                        "three_bf16_planes": legs["b3"],
                        "note": "default: two f16 planes on rows scaled to unit norm inside the launch, scores un-scaled by the "
                                "norms (3 MFMA products per f32 product; DESIGN 4.7 states its range); three_bf16_planes: the raw "
                                "rows on three bf16 planes (6).  fwd (no gradient) = softplus row sums only (1 tile product), "
                                "fwd_bwd = forward with the sigmoid-weighted row sum (2) + item-side backward (2)"}
    del a, b, ag, bg

    def step_leg(model, g, reps):
        opt = FusedAdam(model.parameters(), lr=1e-3)

        def step():
            opt.zero_grad()
            model.loss(g, loss_type="bce", reg_weight=1e-4).backward()
            opt.step()
        return 1e3 * timeit(step, reps)

    w1 = WORKLOADS["cfg1"]
    u1, i1 = synth_interactions_device(w1["users"], w1["items"], w1["edges"], SEED, dev)
    ei1 = torch.stack([torch.cat([u1, i1 + w1["users"]]), torch.cat([i1 + w1["users"], u1])])    # lightgcn.py:36-39
    m1 = LightGCN(943, 1682, d, 2).to(dev)
    g1 = m1.prepare(ei1)
    out["cfg1_step_ms"] = round(step_leg(m1, g1, 10), 4)
    out["cfg1_step_logits"] = 80000 * 1682
    mb = LightGCN(n_u, n_i, d, k_layers).to(dev)
    out["full_batch_step_ms"] = round(step_leg(mb, graph, 2), 3)
    out["full_batch_step_logits_reference"] = (graph.nnz // 2) * n_i
    out["full_batch_step_pairs_computed"] = n_u * n_i
    out["note"] = "full_batch_step: propagate + BCE(all E x I logits, by distinct user) + reg + backward + Adam on the benchmark graph"
    return out


NCL_CFG3 = {"model": {"name": "NCL", "type": "graph"}, "embedding.size": 64, "batch.size": 2048, "learning.rate": 1e-3,
            "reg.lambda": 1e-4, "max.epoch": 1, "item.ranking.topN": [10, 20, 30, 50],
            "NCL": {"n_layers": 3, "tau": 0.1, "ssl_reg": 1e-6, "proto_reg": 1e-7, "alpha": 1.0, "num_clusters": 300,
                    "hyper_layers": 1}}


def ncl_step_legs(Fn, graph, x0, k_layers, n_u, n_i, uidx, iidx, jn, timeit):
    """NCLModel.train_step (recommendation_amd/ncl.py, the loop body ncl.py:311-329) on the benchmark graph: the
    hand-derived launch sequence (ncl_step.FusedNCLStep) eagerly and replayed from a hipGraph, and the autograd path,
    each WITH the per-batch e_step at num_clusters = 300 (the largest value of the reference's own grid, ncl.py:455)
    and 2000; plus the step without the e_step."""
    import copy
    from recommendation_amd.ncl import NCLModel
    from recommendation_amd.optim import FusedAdam
    out = {}
    batch = (uidx, iidx, jn)

    def model_for(k, **kw):
        conf = copy.deepcopy(NCL_CFG3)
        conf["NCL"]["n_layers"] = k_layers
        conf["NCL"]["num_clusters"] = k
        m = NCLModel.from_graph(conf, graph, n_u, n_i, **kw)
        with torch.no_grad():
            m.model.table.copy_(x0)
        return m

    def leg(k, fused, capture, e_step=True, reps=5):
        m = model_for(k, graph_capture=capture)
        opt = FusedAdam(m.model.parameters(), lr=1e-3, capturable=capture)
        m.e_step()                                                  # ncl.py:308: once before the first batch
        if not e_step:
            m.train_step(batch, opt, check_negatives=False, fused=True)
            m._fused.e_step_every_batch = False
        for _ in range(3):                                          # graph path: 2 eager warm-ups, then the capture
            m.train_step(batch, opt, check_negatives=False, fused=fused)
        t = timeit(lambda: m.train_step(batch, opt, check_negatives=False, fused=fused), reps)
        del m, opt
        torch.cuda.empty_cache()
        return 1e3 * t

    out["ncl_train_step_full_ms"] = leg(300, True, True)
    out["ncl_train_step_full"] = {
        "what": "NCLModel.train_step = the loop body ncl.py:311-329 INCLUDING the per-batch e_step (ncl.py:324,340-356: k-means "
                "of all users and of all items, faiss defaults niter 25 / 256 points per centroid / seed 1234), B = 2048, 3 "
                "layers, d = 64, 1M users x 100K items / 10M interactions, sym-normalised operator.  Assignment: the fused legs "
                "(k*_graph_ms, k*_eager_ms) search only the step's own 2 x B batch rows — the only assignments the iteration "
                "reads (ncl.py:370-373); the reference's full-table index.search (ncl.py:355) is computed lazily when "
                "user_2cluster / item_2cluster is read.  The autograd leg (k300_autograd_ms) runs the full N x k search every "
                "step, as the reference does: the legs time the same training step, not the same assignment work",
        "k300_graph_ms": out["ncl_train_step_full_ms"],
        "k300_eager_ms": leg(300, True, False),
        "k300_autograd_ms": leg(300, False, False, reps=3),
        "k2000_graph_ms": leg(2000, True, True),
        "k2000_eager_ms": leg(2000, True, False, reps=3),
        "num_clusters_note": "300 = the largest value of the reference's grid (ncl.py:455: 20 ... 300); 2000 = round 2's "
                             "k-means probe size",
    }
    out["ncl_train_step_ms"] = leg(300, True, True, e_step=False)
    out["ncl_train_step_note"] = "ncl_train_step_ms = the same iteration WITHOUT the per-batch e_step (not the reference's " \
                                 "loop body; round 2 reported this as the step); ncl_train_step_full_ms is config 3 as ncl.py runs it"
    return out


def cpu_baseline(graph, x0, k_layers, nnz, n_u, n_i):
    """The C restatement of the reference path (oracle/oracle.c, OpenMP) on this box's host cores,
    bounded to ~10-30 s: the same graph, the same K-layer propagation; plus the other §8(d) legs
    (the reference's dense contrast formulations and its Python sampler), each bounded to seconds."""
    from oracle import oracle_c
    rowptr = graph.rowptr_host
    col = graph.col.cpu().numpy()
    val = graph.val.cpu().numpy()
    xh = x0.cpu().numpy()
    threads = oracle_c.num_threads()
    oracle_c.lightgcn_propagate(rowptr, col, val, xh, 1, "sum")      # warm-up (page-in, threads)
    reps, spent = 0, 0.0
    while spent < 10.0 and reps < 5:
        t = time.perf_counter()
        oracle_c.lightgcn_propagate(rowptr, col, val, xh, k_layers, "sum")
        spent += time.perf_counter() - t
        reps += 1
    out = {"value": nnz * k_layers * reps / spent, "unit": "edges/s", "cores": threads, "kind": "port",
           "sample": f"{reps} x full {k_layers}-layer CSR propagation of the same graph (oracle/oracle.c, "
                     f"OpenMP {threads} threads, fp32)"}
    import numpy as np
    # the op the reference itself calls (stock PyTorch, ncl.py:203-209,419): torch.sparse.mm on the
    # uncoalesced COO tensor, one layer, timed on the same host cores (informative companion line)
    try:
        rows = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))
        idx = torch.from_numpy(np.stack([rows, col.astype(np.int64)]))
        a_coo = torch.sparse_coo_tensor(idx, torch.from_numpy(val), (rowptr.size - 1, rowptr.size - 1))
        xt = torch.from_numpy(xh)
        torch.sparse.mm(a_coo, xt)
        t = time.perf_counter()
        torch.sparse.mm(a_coo, xt)
        dt = time.perf_counter() - t
        out["torch_sparse_mm_coo_edges_per_s"] = nnz / dt
        out["torch_threads"] = torch.get_num_threads()
        del a_coo, idx, rows
    except Exception as e:  # informative only
        out["torch_sparse_mm_coo_error"] = str(e)[:100]
    # SURVEY §8(d) legs 3 and 4: the reference's dense contrast formulations and Python sampler
    legs = {}
    try:
        from oracle import cpu_legs
        xt = torch.from_numpy(xh)
        g = torch.Generator().manual_seed(5)
        bsz = 2048
        n_tab = min(n_u, 250_000)                 # 2048 x 250K logits = 2 GB materialised (the reference's way)
        anchors = xt[torch.randint(0, n_u, (bsz,), generator=g)]
        cpu_legs.ncl_structure_denominator(anchors[:64], xt[:n_tab], 0.1)
        t = time.perf_counter()
        cpu_legs.ncl_structure_denominator(anchors, xt[:n_tab], 0.1)
        dt = time.perf_counter() - t
        legs["ncl_structure_denominator"] = {
            "pairs_per_s": bsz * n_tab / dt, "ms": 1e3 * dt, "threads": torch.get_num_threads(),
            "sample": f"ncl.py:363-364 dense exp(A @ ALL^T / t).sum(1), {bsz} x {n_tab} (of {n_u} user rows), d={xt.shape[1]}, "
                      "torch CPU f32; the full table scales linearly (extrapolated)"}
        m = 8192
        z1, z2 = xt[:m], xt[n_u:n_u + m] if n_i >= m else xt[m:2 * m]
        cpu_legs.gcl_info_nce_loss(z1[:256], z2[:256])
        t = time.perf_counter()
        cpu_legs.gcl_info_nce_loss(z1, z2)
        dt = time.perf_counter() - t
        legs["gcl_info_nce_loss"] = {"pairs_per_s": m * m / dt, "ms": 1e3 * dt, "threads": torch.get_num_threads(),
                                     "sample": f"gcl.py:28-35 dense symmetric InfoNCE, {m} x {m}, d={xt.shape[1]}, torch CPU f32"}
        # Python rejection sampler at B = 2048 (ncl.py:91-114): one batch over this graph's users / items
        ub = torch.randint(0, n_u, (bsz,), generator=g).tolist()
        item_map = {i: i for i in range(n_i)}
        tset, pairs = {}, []
        for u in ub:
            its = (col[rowptr[u]:rowptr[u + 1]] - n_u).tolist()
            tset[u] = set(its)
            pairs.append((u, its[0] if its else 0))
        user_map = {u: u for u in tset}
        import random
        t = time.perf_counter()
        batch = next(cpu_legs.python_pairwise_sampler(pairs, user_map, item_map, tset, bsz, random.Random(3)))
        dt = time.perf_counter() - t
        legs["python_sampler"] = {"samples_per_s": len(batch[2]) / dt, "ms_per_batch": 1e3 * dt, "threads": 1,
                                  "sample": f"ncl.py:91-114 next_batch_pairwise, one batch of {bsz} over {n_i} items "
                                            "(list(item keys) rebuilt per draw, as the reference does)"}
    except Exception as e:  # noqa: BLE001
        legs["error"] = repr(e)[:200]
    out["legs"] = legs
    return out


if __name__ == "__main__":
    main()
