"""Prepared sparse operators for the LightGCN message pass (device-resident CSR + work plan).

Mirrors what the reference builds once per model and then reuses every step:
  * raw 0/1 bipartite adjacency, duplicates kept       ncl.py:74-85 (= directau.py:130-141,
                                                        sept.py:134-145, mhcn.py:245-256)   [Q1]
  * D^-1/2 (R + R^T) D^-1/2, duplicates summed          selfcf.py:291-306 + 240-255, ssl4rec.py:79-88
  * gcn_norm(add_self_loops=False) edge weights         lightgcn.py:17,25 (torch_geometric LGConv)
Layout in HBM: rowptr int64[N+1], col int32[nnz], val fp32[nnz] (absent for the all-ones raw
adjacency), plus the SpMM plan (32-byte partition descriptors) and, for split rows, an fp32
partial-sum workspace [n_slots, d].
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

# interleaved A/B on MI355X (scripts/perf_spmm_ab.py): 64 -> 0.713 ms, 128 -> 0.652, 256 -> 0.629,
# 512 -> 0.617, 1024 -> 0.631 per cfg2 layer; cfg4 7.97 / 7.22 / 6.87 / 6.70 / 6.67 ms
DEFAULT_NNZ_PER_PART = 512

# The windowed companion of the heaviest ("hub") rows (HubPlan); measurements in EXPERIMENTS.md "SpMM: hub rows by column
# window".  Fabric bytes fetched per gathered non-zero of the hub rows fall from 264 (classic plan) to 61-103 at windows of
# 2048-8192 rows, least at 64 non-zeros per partition -- but the layer is fastest at 128 (fewer, longer partitions), and
# faster still at 16384-row windows, where twice as many rows are hubs (the 8 W bound halves) and a segment is twice as
# long: interleaved A/B, ms per cfg2 layer against the parent's 0.6616: 8192:128 0.6150, 16384:128 0.6021, 16384:256
# 0.5996, 32768:128 0.5989, 65536:256 0.6303; cfg4 7.305 -> 6.681 / 6.276 / 6.223 at 8192 / 16384 / 32768.
HUB_WINDOW_ROWS = 16384
HUB_NNZ_PER_PART = 128
HUB_MIN_TABLE_BYTES = 16 << 20        # the gathered table is at least 4 x one XCD's 4 MiB L2, or the rows hit anyway
HUB_MAX_WINDOW_BYTES = 4 << 20        # one window of the table is at most one XCD's L2 (d <= 64 at the default window)
ROW_ORDER_MAX_D = 64                  # the mapped kernels (RowOrder) are the d <= 64 ones


# The order of the work inside the one grid that walks the companion and the main plan (gcr_spmm_windowed_f32); both are
# plan decisions and neither changes a word of the result.  Measurements: EXPERIMENTS.md "SpMM: one launch for both walks".
HUB_MAIN_FIRST = True                 # which range of blocks leads the grid: the main plan's (True) or the companion's
HUB_MAIN_LONG_ROWS_FIRST = False      # `HubPlan.main`'s descriptors in plan order (False) or by long_rows_first_order


def long_rows_first_order(desc):
    """A permutation of the rows of a plan's descriptors [n_parts, 4]: stable by the number of rows of a partition,
    ascending, so the chunks of split rows and the partitions of a few long rows are dispatched first and the partitions of
    many short rows last.  A partition's slot travels with its descriptor, so the split rows' tables stay as they are."""
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, 4)
    return np.argsort(desc[:, 2] >> 32, kind="stable")


def _np_i64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.int64)


class SpmmPlan:
    """Host-built partition list for gcr_spmm_csr_f32 (include/gcr.h)."""

    def __init__(self, rowptr_host: np.ndarray, device, nnz_per_part=DEFAULT_NNZ_PER_PART, row_group=None, skip=None):
        """row_group (optional int array [n_rows]): a locality group per row (reorder.locality_permutation's labels on the
        re-numbered operator).  The partitions are then laid out so that each group runs on ONE XCD, group after group
        (reorder.xcd_grouped_order), and its rows stay in that XCD's L2 between the gathers that share them; without it
        the partitions keep row order and consecutive workgroups alternate over the XCDs.
        skip (optional bool / uint8 array [n_rows]): rows that get no partition and no long-row entry (HubPlan's)."""
        rowptr_host = np.ascontiguousarray(rowptr_host, dtype=np.int64)
        n_rows = rowptr_host.size - 1
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.uint8)
            if skip.shape != (n_rows,):
                raise ValueError("skip must have one entry per row")
        sizes = np.zeros(3, np.int64)
        _lib.call("gcr_spmm_plan_size_skip_host", rowptr_host, n_rows, nnz_per_part, skip, sizes[0:1], sizes[1:2], sizes[2:3])
        self.n_parts, self.n_long, self.n_slots = int(sizes[0]), int(sizes[1]), int(sizes[2])
        desc = np.empty((max(self.n_parts, 1), 4), dtype=np.int64)
        long_row = np.zeros(max(self.n_long, 1), dtype=np.int32)
        long_slot0 = np.zeros(self.n_long + 1, dtype=np.int32)
        _lib.call("gcr_spmm_plan_fill_skip_host", rowptr_host, n_rows, nnz_per_part, skip, desc, long_row, long_slot0)
        self.nnz_per_part = nnz_per_part
        self.grouped = row_group is not None and self.n_parts > 0
        if self.grouped:
            from .reorder import xcd_grouped_order
            rg = np.asarray(row_group.detach().cpu().numpy() if isinstance(row_group, torch.Tensor) else row_group)
            if rg.shape != (n_rows,):
                raise ValueError("row_group must have one entry per row")
            order = xcd_grouped_order(desc[: self.n_parts], rg)
            pad = np.array([0, 0, 0, -1], dtype=np.int64)                 # an empty whole-row partition: writes nothing
            desc = np.where((order >= 0)[:, None], desc[np.maximum(order, 0)], pad[None, :])
            self.n_parts = int(order.size)
        self.desc_host = desc[: self.n_parts]
        self.long_row_host, self.long_slot0_host = long_row[: self.n_long], long_slot0
        self.desc = torch.from_numpy(desc).to(device)
        self.long_row = torch.from_numpy(long_row).to(device)
        self.long_slot0 = torch.from_numpy(long_slot0).to(device)

    def permuted(self, order):
        """This plan with its descriptors in another order (`order`: a permutation of range(n_parts)): the same partitions,
        one wave each, dispatched in that order.  The split rows' tables and slots are shared and unchanged."""
        import copy
        order = np.asarray(order, dtype=np.int64)
        if not np.array_equal(np.sort(order), np.arange(self.n_parts)):
            raise ValueError("order must be a permutation of the plan's partitions")
        q = copy.copy(self)
        q.desc_host = np.ascontiguousarray(self.desc_host[order])
        q.desc = torch.from_numpy(q.desc_host if self.n_parts else np.empty((1, 4), dtype=np.int64)).to(self.desc.device)
        return q


class HubPlan:
    """Windowed companion of a graph's heaviest rows: their gathers are made to hit in L2.

    A hub row (degree > max(nnz_per_part, 8 W), W = ceil(n_cols / window_rows) column windows) spans the whole gathered
    table, and so do the 512-non-zero chunks the classic plan cuts it into: nothing two chunks gather is still in an XCD's
    4 MiB L2 when the other needs it, although all hub rows share the same columns.  Here the hub rows are cut by column
    window instead.  The companion CSR `H` has W x n_hub rows; row w * n_hub + h holds the non-zeros of hub row h whose
    column lies in window w, in stored order (`col` / `val` copied window-major).  `H` gets an ordinary whole-row plan with
    small partitions whose descriptors are laid out per XCD window after window (reorder.xcd_grouped_order), so the waves
    resident on one XCD gather from two or three windows of the table at a time.  A launch is then
      1. partials[W n_hub, d] = H x            gcr_spmm_hub_parts_f32 at d <= 64 (the same partitions, one wave each, by a
                                               kernel without the epilogue that gathers the tail of a block in batches);
                                               gcr_spmm_csr_f32 on H, y only, val_scale 1 at wider d (the same bits)
      2. out[hub rows] = epilogue(sum of a row's window partials in window order)      gcr_spmm_hub_reduce_f32
      3. every other row: the classic walk with the hub rows skipped (`main`)          gcr_spmm_csr_f32
    on one stream.  At d <= 64 gcr_spmm_windowed_f32 does all of it in three launches with the same words: one grid walks
    the partitions of `main` and of `H` (`main_first`: whose blocks lead; nothing either reads is written by the other),
    one sums the split rows of both plans, the reduction of step 2 comes last.  The 8 W bound keeps the partial traffic (W x 2 x 4 d bytes per hub row) under a quarter of the row's
    gathers.  `build` returns None when the graph has no hub rows or a hub row's columns are not sorted."""

    @classmethod
    def build(cls, graph, window_rows, min_degree=None, nnz_per_part=HUB_NNZ_PER_PART, forced=False):
        window_rows = int(window_rows)
        if window_rows < 1:
            raise ValueError("hub_window_rows must be positive")
        n_win = -(-graph.n_cols // window_rows)
        thr = max(nnz_per_part, 8 * n_win) if min_degree is None else int(min_degree)
        deg_host = np.diff(graph.rowptr_host)
        hub_host = np.flatnonzero(deg_host > thr)
        n_hub = int(hub_host.size)
        if n_hub == 0 or n_win * n_hub >= (1 << 31):
            return None
        dev = graph.device
        hub = torch.from_numpy(hub_host).to(dev)
        hdeg = torch.from_numpy(deg_host[hub_host]).to(dev)
        hub_nnz = int(deg_host[hub_host].sum())
        hoff = torch.cumsum(hdeg, 0) - hdeg
        hid = torch.repeat_interleave(torch.arange(n_hub, device=dev), hdeg)            # hub index of every hub non-zero
        e = graph.rowptr[hub][hid] + (torch.arange(hub_nnz, device=dev) - hoff[hid])    # its position in col / val
        c = graph.col[e].to(torch.int64)
        if not bool(((c[1:] >= c[:-1]) | (hid[1:] != hid[:-1])).all()):
            return None                                                                  # unsorted hub row: classic plan
        # segment boundaries: a search of every hub row's sorted columns for the window edges, [n_hub, W + 1]
        pad = n_win * window_rows
        edges = (torch.arange(n_hub, device=dev)[:, None] * pad + torch.arange(n_win + 1, device=dev)[None, :] * window_rows)
        bounds = torch.searchsorted(hid * pad + c, edges.reshape(-1)).view(n_hub, n_win + 1)
        del c, edges
        seg_len = (bounds[:, 1:] - bounds[:, :-1]).t().reshape(-1)                       # of row w * n_hub + h
        rp = torch.zeros(n_win * n_hub + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(seg_len, 0)
        row_of = torch.repeat_interleave(torch.arange(n_win * n_hub, device=dev), seg_len)
        src = bounds[:, :-1].t().reshape(-1)[row_of] + (torch.arange(hub_nnz, device=dev) - rp[row_of])
        del row_of, hid
        e = e[src]
        self = cls()
        self.window_rows, self.n_windows, self.n_hub, self.min_degree, self.forced = window_rows, n_win, n_hub, thr, bool(forced)
        self.hub_nnz = hub_nnz
        self.hub_row_host = hub_host
        self.hub_row = hub.to(torch.int32)
        self.bounds = bounds
        group = np.repeat(np.arange(n_win, dtype=np.int64), n_hub)                       # window id of every row of H
        self.H = CsrGraph(rp, graph.col[e], None if graph.val is None else graph.val[e], n_win * n_hub, graph.n_cols, dev,
                          nnz_per_part=nnz_per_part, validate=False, row_group=group, hub_window_rows=0)
        skip = np.zeros(graph.n_rows, dtype=np.uint8)
        skip[hub_host] = 1
        self.main = SpmmPlan(graph.rowptr_host, dev, graph.plan.nnz_per_part, skip=skip)
        if HUB_MAIN_LONG_ROWS_FIRST:
            self.main = self.main.permuted(long_rows_first_order(self.main.desc_host))
        self.main_first = HUB_MAIN_FIRST
        self._partials = {}
        return self

    def eligible(self, d: int) -> bool:
        """Size conditions of a launch with d columns; a plan forced through the constructor keyword waives them."""
        if self.forced:
            return True
        return self.H.n_cols * 4 * d >= HUB_MIN_TABLE_BYTES and self.window_rows * 4 * d <= HUB_MAX_WINDOW_BYTES

    def partials(self, d: int):
        """fp32 [W * n_hub, d] window partial sums, one per (d, stream)."""
        key = (d, torch.cuda.current_stream(self.H.device).cuda_stream)
        ws = self._partials.get(key)
        if ws is None:
            ws = torch.empty(self.n_windows * self.n_hub, d, dtype=torch.float32, device=self.H.device)
            self._partials[key] = ws
        return ws


def coldest_column_key(rowptr, col, n_cols, lo, hi):
    """int64 [hi - lo]: the sort key of rows lo .. hi - 1 of a CSR (torch tensors, any device): degree * n_cols + id of the
    row's least-referenced column -- the degree of a column is its count in the whole `col` (bincount), ties go to the
    smaller id.  An empty row gets the largest int64, so it sorts last."""
    rowptr, col = rowptr.to(torch.int64), col.to(torch.int64)
    cnt = torch.bincount(col, minlength=n_cols)
    e0, e1 = int(rowptr[lo]), int(rowptr[hi])
    c = col[e0:e1]
    key = torch.full((hi - lo,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=col.device)
    rows = torch.repeat_interleave(torch.arange(hi - lo, device=col.device), rowptr[lo + 1: hi + 1] - rowptr[lo:hi])
    return key.scatter_reduce_(0, rows, cnt[c] * int(n_cols) + c, "amin")


def coldest_column_order(rowptr, col, n_rows, n_cols, lo, hi):
    """int64 [n_rows], a permutation of the rows: rows lo .. hi - 1 sorted stably by `coldest_column_key`, every other row
    in place.  Rows that share an unpopular column become neighbours, so one wave walks them one after another and the
    column's row of the gathered table is fetched once instead of once per row (EXPERIMENTS.md "SpMM: user rows in
    order of their coldest column")."""
    order = torch.arange(n_rows, dtype=torch.int64, device=col.device)
    if hi > lo:
        order[lo:hi] = lo + torch.argsort(coldest_column_key(rowptr, col, n_cols, lo, hi), stable=True)
    return order


class RowOrder:
    """A row-ordered plan: the rows of a graph walked in another order than they are stored in, through a row-permuted
    copy `P` of the CSR and a row map, so that nothing the caller sees is renumbered.

    `order` (int64 [n_rows], a permutation of the rows) with the rows in `skip` (the hub rows of the graph's HubPlan) left
    out gives row_id (int32 [n_p]): row r of P is row row_id[r] of the graph, with its col / val sequence copied as it
    stands (rowptr_p int64 [n_p + 1], col_p, val_p).  `plan` is an ordinary SpmmPlan over rowptr_p; its whole-row
    partitions hold consecutive rows of P, which is all `walk_partition` needs, and the mapped kernels
    (gcr_spmm_rows_mapped_f32, gcr_spmm_windowed_mapped_f32) take the row of a flush and of an acc_in load from row_id.
    Split rows keep the slots and the long_row / long_slot0 tables of `base` (the graph's classic plan, or its HubPlan's
    `main`): only the chunk descriptors of P are renumbered to those slots, so the split rows' workspace and its reducer
    see what they see without a row order.  This object is the `graph` of spmm_launch.rows_mapped: rowptr / col / val are
    P's, n_rows / n_cols the graph's.
    Memory: 8 B per non-hub non-zero (col_p, val_p) plus 12 B per row (rowptr_p, row_id) beside the graph's own CSR: about
    0.13 GB on the cfg2 benchmark graph and 1.5 GB on cfg4."""

    def __init__(self, graph, order, base, skip=None, forced=False, table_rows=None):
        dev = graph.device
        order = torch.as_tensor(order).to(device=dev, dtype=torch.int64)
        if order.shape != (graph.n_rows,) or not bool((torch.sort(order).values == torch.arange(graph.n_rows, device=dev)).all()):
            raise ValueError("row_order must be a permutation of the graph's rows")
        if skip is not None:
            order = order[~torch.as_tensor(skip, dtype=torch.bool, device=dev)[order]]
        self.forced = bool(forced)
        self.table_rows = graph.n_cols if table_rows is None else int(table_rows)
        self.n_rows, self.n_cols, self.n_p = graph.n_rows, graph.n_cols, int(order.numel())
        self.order_host = order.cpu().numpy()
        self.row_id = order.to(torch.int32)
        deg = (graph.rowptr[1:] - graph.rowptr[:-1])[order]
        self.rowptr = torch.zeros(self.n_p + 1, dtype=torch.int64, device=dev)
        self.rowptr[1:] = torch.cumsum(deg, 0)
        self.rowptr_host = self.rowptr.cpu().numpy()
        nnz_p = int(self.rowptr_host[-1])
        rid = torch.repeat_interleave(torch.arange(self.n_p, device=dev), deg)           # P row of every non-zero of P
        src = graph.rowptr[order][rid] + (torch.arange(nnz_p, device=dev) - self.rowptr[rid])
        del rid
        self.col = graph.col[src]
        self.val = None if graph.val is None else graph.val[src]
        del src
        self.plan = SpmmPlan(self.rowptr_host, dev, base.nnz_per_part)
        # split rows: base's tables (the graph's own rows) and base's slots
        p = self.plan
        if p.n_slots != base.n_slots or p.n_long != base.n_long:
            raise RuntimeError("the row-ordered plan and its base disagree on the split rows")
        if p.n_long:
            slot0_of = np.full(graph.n_rows, -1, dtype=np.int64)
            slot0_of[base.long_row_host] = base.long_slot0_host[:-1]
            own0_of = np.zeros(self.n_p, dtype=np.int64)
            own0_of[p.long_row_host] = p.long_slot0_host[:-1]
            desc = p.desc_host.copy()
            chunk = desc[:, 3] >= 0
            prow = desc[chunk, 2] & 0xFFFFFFFF
            desc[chunk, 3] += slot0_of[self.order_host[prow]] - own0_of[prow]
            if bool((desc[chunk, 3] < 0).any()):
                raise RuntimeError("a split row of the row-ordered plan is not a split row of its base")
            p.desc_host = desc
            p.desc = torch.from_numpy(desc).to(dev)
        p.long_row_host, p.long_slot0_host = base.long_row_host, base.long_slot0_host
        p.long_row, p.long_slot0 = base.long_row, base.long_slot0

    def eligible(self, d: int) -> bool:
        """The table the ordered rows gather from is large enough to miss in L2; a forced order waives it."""
        return self.forced or self.table_rows * 4 * d >= HUB_MIN_TABLE_BYTES


class CsrGraph:
    """A sparse operator A [n_rows, n_cols] resident on one GPU, ready for `functional.spmm`."""

    def __init__(self, rowptr, col, val, n_rows, n_cols, device, symmetric=False,
                 nnz_per_part=DEFAULT_NNZ_PER_PART, validate=True, transpose=None, row_group=None,
                 hub_window_rows=None, hub_min_degree=None, row_order=None, _default_row_range=None):
        """row_order: the order in which plain launches at d <= 64 walk the rows (RowOrder; results do not depend on it).
        None = the constructors of bipartite operators (`bipartite_sym_norm`, `bipartite_raw`) order the user rows by their
        coldest column (`coldest_column_order`) when the gathered table is large enough to miss in L2, every other
        constructor keeps the stored order; a (lo, hi) range = that order on rows lo .. hi - 1 at any size; an int64
        permutation of the rows = that order at any size; False = the stored order.  A graph with a `row_group` keeps its
        grouped plan.  The transpose inherits the keyword (a range or a permutation only when it has as many rows).
        hub_window_rows: None = the windowed companion of the hub rows (HubPlan) is built with HUB_WINDOW_ROWS when the
        table is large enough for it to matter and used by the launches whose sizes qualify; an int > 0 forces it with that
        window at any size; 0 disables it.  hub_min_degree: None = max(HUB_NNZ_PER_PART, 8 W); an int = rows with a larger
        degree are hubs.  A graph with a `row_group` (XCD-grouped classic plan) keeps the classic plan."""
        rowptr_host = _np_i64(rowptr)
        if rowptr_host.size != n_rows + 1:
            raise ValueError("rowptr must have n_rows + 1 entries")
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self.nnz = int(rowptr_host[-1])
        self.device = torch.device(device)
        self.symmetric = bool(symmetric)
        self.rowptr_host = rowptr_host
        self.rowptr = torch.from_numpy(rowptr_host).to(self.device)
        self.col = torch.as_tensor(col).to(device=self.device, dtype=torch.int32).contiguous()
        self.val = None if val is None else torch.as_tensor(val).to(device=self.device, dtype=torch.float32).contiguous()
        if self.col.numel() != self.nnz or (self.val is not None and self.val.numel() != self.nnz):
            raise ValueError("col / val length must equal rowptr[-1]")
        self.plan = SpmmPlan(rowptr_host, self.device, nnz_per_part, row_group=row_group)
        self._t = self if symmetric else transpose
        self._workspaces = {}
        if validate and self.device.type == "cuda":
            self.validate()
        self._hub_kw = dict(hub_window_rows=hub_window_rows, hub_min_degree=hub_min_degree)
        self.hub = None
        if hub_window_rows is None:
            # not worth a look unless some launch (d <= 256) could qualify
            if row_group is None and self.n_cols * 4 * 256 >= HUB_MIN_TABLE_BYTES:
                self.hub = HubPlan.build(self, HUB_WINDOW_ROWS, hub_min_degree)
        elif int(hub_window_rows) > 0:
            self.hub = HubPlan.build(self, hub_window_rows, hub_min_degree, forced=True)
        self._row_order_kw = row_order
        self.rows_p = None
        if row_group is None and row_order is not False:
            self.rows_p = self._build_row_order(row_order, _default_row_range)

    def _build_row_order(self, row_order, default_range):
        """The RowOrder the keyword asks for, or None (see __init__)."""
        forced = row_order is not None
        table_rows = None
        if not forced:
            if default_range is None:
                return None
            lo, hi = default_range
            table_rows = self.n_cols - (hi - lo)        # a bipartite operator: the ordered block gathers from the other one
            if table_rows * 4 * ROW_ORDER_MAX_D < HUB_MIN_TABLE_BYTES:
                return None                              # no launch the mapped kernels take (d <= 64) could qualify
            row_order = default_range
        if isinstance(row_order, tuple) and len(row_order) == 2:
            lo, hi = int(row_order[0]), int(row_order[1])
            if not 0 <= lo <= hi <= self.n_rows:
                raise ValueError("row_order range must lie inside the graph's rows")
            row_order = coldest_column_order(self.rowptr, self.col, self.n_rows, self.n_cols, lo, hi)
        skip = None
        if self.hub is not None:
            skip = torch.zeros(self.n_rows, dtype=torch.bool)
            skip[torch.from_numpy(self.hub.hub_row_host)] = True
        base = self.plan if self.hub is None else self.hub.main
        return RowOrder(self, row_order, base, skip=skip, forced=forced, table_rows=table_rows)

    # -- checks ---------------------------------------------------------------------------
    def validate(self):
        """Device-side structural check before any kernel trusts the indices."""
        errs = torch.zeros(1, dtype=torch.int64, device=self.device)
        _lib.call("gcr_csr_validate", self.rowptr, self.col, self.n_rows, self.n_cols, self.nnz, errs, on=self.device)
        n = int(errs.item())
        if n:
            raise ValueError(f"CSR graph is malformed: {n} structural errors (rowptr order / column range)")

    # -- helpers --------------------------------------------------------------------------
    def workspace(self, d: int):
        """fp32 [n_slots, d] partial-sum buffer for split rows, one per (d, stream)."""
        if self.plan.n_slots == 0:
            return None
        key = (d, torch.cuda.current_stream(self.device).cuda_stream)
        ws = self._workspaces.get(key)
        if ws is None:
            ws = torch.empty(self.plan.n_slots, d, dtype=torch.float32, device=self.device)
            self._workspaces[key] = ws
        return ws

    @property
    def t(self) -> "CsrGraph":
        """Transposed operator (for the backward pass dX = A^T dY); `self` when symmetric."""
        if self._t is None and self.device.type == "cuda":
            rows = torch.repeat_interleave(torch.arange(self.n_rows, device=self.device),
                                           self.rowptr[1:] - self.rowptr[:-1])
            rp, c, v, perm = coo_to_csr_device(self.col.to(torch.int64), rows, self.val, self.n_cols, self.n_rows,
                                               self.device, want_perm=True)
            self._t = CsrGraph(rp, c, v, self.n_cols, self.n_rows, self.device, symmetric=False,
                               nnz_per_part=self.plan.nnz_per_part, validate=False, transpose=self, **self._t_kw())
            self._t.perm_from_transpose = perm     # non-zero e of A^T is non-zero perm[e] of A (shared edge masks)
        if self._t is None:
            col_host = self.col.cpu().numpy().astype(np.int64)
            rows = np.repeat(np.arange(self.n_rows, dtype=np.int64), np.diff(self.rowptr_host))
            val_host = None if self.val is None else self.val.cpu().numpy()
            rp, c, v, _ = _coo_to_csr_host(col_host, rows, val_host, self.n_cols)
            self._t = CsrGraph(rp, c, v, self.n_cols, self.n_rows, self.device, symmetric=False,
                               nnz_per_part=self.plan.nnz_per_part, validate=False, transpose=self, **self._t_kw())
        return self._t

    def _t_kw(self):
        """Constructor keywords the transpose inherits: the hub plan's, and the row order's -- None and False as they are,
        a range or a permutation only when the transpose has as many rows as this operator."""
        ro = self._row_order_kw
        if ro is not None and ro is not False and self.n_cols != self.n_rows:
            ro = False
        return dict(self._hub_kw, row_order=ro)

    def row_degrees(self):
        """Non-zeros per row, float32 [n_rows] (cached)."""
        dg = getattr(self, "_row_deg", None)
        if dg is None:
            dg = (self.rowptr[1:] - self.rowptr[:-1]).to(torch.float32)
            self._row_deg = dg
        return dg

    def with_values(self, val):
        """A view of this operator with other per-non-zero values (float32 [nnz], same order): structure, work plan and
        workspace are shared, nothing is copied — e.g. the per-edge coefficients of `functional.bpr_edge_sums`."""
        import copy
        if tuple(val.shape) != (self.nnz,) or val.dtype != torch.float32 or val.device != self.col.device:
            raise ValueError("val must be float32 [nnz] on the graph's device")
        g = copy.copy(self)
        g.val = val.contiguous()
        g._t = None
        g.hub = None                       # the companion holds a copy of the old values: this view runs the classic plan
        g.rows_p = None                    # and so does the row-ordered copy: never walk stale values
        g._row_order_kw = False
        return g

    def user_major_edges(self, n_users):
        """Bipartite symmetric operators ([U + I] x [U + I], users first; `bipartite_sym_norm`, `from_edge_index_gcn_norm`
        of lightgcn.py:36-39's edge_index): (u_idx, i_idx) int64 [E] of the non-zeros of the user rows in CSR order — the
        training pairs when the graph was built from them — cached."""
        c = getattr(self, "_um_edges", None)
        if c is None or c[0] != int(n_users):
            n_users = int(n_users)
            rp = self.rowptr[: n_users + 1]
            e = int(rp[-1])
            if 2 * e != self.nnz:
                raise ValueError("not a symmetric bipartite operator with the users first: nnz != 2 * nnz(user rows)")
            u = torch.repeat_interleave(torch.arange(n_users, device=self.device), rp[1:] - rp[:-1])
            i = self.col[:e].to(torch.int64) - n_users
            c = (n_users, u, i)
            self._um_edges = c
        return c[1], c[2]

    def negatives_user_block(self, n_users, n_items, n_neg=1):
        """The CSR skeleton [U x I] of `n_neg` negatives per training edge in user-major order: the user rows' pointer of this
        (symmetric bipartite) operator times n_neg, with its work plan — built once, cached; the caller fills `col` / `val`
        with a step's negatives and coefficients (functional.bpr_edge_sums' backward)."""
        key = (int(n_users), int(n_items), int(n_neg))
        cache = self.__dict__.setdefault("_neg_blocks", {})
        blk = cache.get(key)
        if blk is None:
            rp = self.rowptr_host[: n_users + 1] * int(n_neg)
            nnz = int(rp[-1])
            blk = CsrGraph(rp, torch.zeros(nnz, dtype=torch.int32, device=self.device),
                           torch.zeros(nnz, dtype=torch.float32, device=self.device), n_users, n_items, self.device,
                           symmetric=False, nnz_per_part=self.plan.nnz_per_part, validate=False,
                           hub_window_rows=0)           # the caller rewrites col / val every step
            cache[key] = blk
        return blk

    def mirror_perm(self):
        """Symmetric operators only: int64 [nnz], mirror[e] = position of the non-zero (c, r) for the non-zero
        e = (r, c) — the nnz -> transpose-nnz map that lets a per-non-zero edge mask be handed to the
        backward pass in A^T's order (`functional.spmm(keep_bits_t=...)`).  Duplicate pairs (the raw
        multigraph of ncl.py:74-85) are matched copy by copy.  One-off index plumbing, cached."""
        if not self.symmetric:
            raise ValueError("mirror_perm() is for symmetric graphs; an asymmetric graph has graph.t.perm_from_transpose")
        m = getattr(self, "_mirror", None)
        if m is None:
            rows = torch.repeat_interleave(torch.arange(self.n_rows, device=self.device), self.rowptr[1:] - self.rowptr[:-1])
            cols = self.col.to(torch.int64)
            by_rc = torch.argsort(rows * self.n_cols + cols, stable=True)     # k-th copy of (r, c)
            by_cr = torch.argsort(cols * self.n_rows + rows, stable=True)     # k-th copy whose transpose is (r, c)
            m = torch.empty_like(by_rc)
            m[by_rc] = by_cr
            self._mirror = m
        return m

    # -- constructors ---------------------------------------------------------------------
    @classmethod
    def from_coo(cls, row, col, val, n_rows, n_cols, device, coalesce=False, symmetric=False, **kw):
        """Stable sort by row (COO order kept inside a row, duplicates kept — torch.sparse.mm on the
        uncoalesced COO of ncl.py:203-209 sums them), or (row, col)-sorted with duplicates summed
        when `coalesce` (scipy `tmp + tmp.T`, selfcf.py:297; `.coalesce()`, sept.py:50).
        want_perm=True (not with coalesce) keeps `coo_perm`, int64 [nnz]: non-zero e of the CSR is COO entry coo_perm[e] —
        the map that brings a per-entry mask recorded in COO order (buir.py:300-309) into non-zero order.
        On a GPU device the sort / merge runs in gcr_coo_to_csr; the numpy path only serves
        CPU-resident graphs (host logic, gloo tests)."""
        want_perm = bool(kw.pop("want_perm", False)) and not coalesce
        if torch.device(device).type == "cuda":
            rp, c, v, perm = coo_to_csr_device(row, col, val, n_rows, n_cols, device, coalesce=coalesce, want_perm=want_perm)
            g = cls(rp, c, v, n_rows, n_cols, device, symmetric=symmetric, **kw)
            g.coo_perm = perm
            return g
        row, col = _np_i64(row), _np_i64(col)
        if val is not None and isinstance(val, torch.Tensor):
            val = val.detach().cpu().numpy()
        perm = None
        if coalesce:
            rp, c, v = _coalesce_host(row, col, val, n_rows, n_cols)
        else:
            rp, c, v, perm = _coo_to_csr_host(row, col, val, n_rows)
        g = cls(rp, c, v, n_rows, n_cols, device, symmetric=symmetric, **kw)
        g.coo_perm = torch.from_numpy(perm) if want_perm else None
        return g

    @classmethod
    def bipartite_raw(cls, uid, iid, num_users, num_items, device, **kw):
        """ncl.py:74-85: rows/cols [(u, i+U), (i+U, u)] per interaction, value 1, duplicates kept (Q1)."""
        n = num_users + num_items
        kw.setdefault("_default_row_range", (0, num_users))
        if torch.device(device).type == "cuda":
            u, i = _dev_i64(uid, device), _dev_i64(iid, device) + num_users
            row = torch.stack([u, i], 1).reshape(-1)      # (u, i+U) then (i+U, u) per interaction
            col = torch.stack([i, u], 1).reshape(-1)
            return cls.from_coo(row, col, None, n, n, device, symmetric=True, **kw)
        uid, iid = _np_i64(uid), _np_i64(iid) + num_users
        row = np.empty(2 * uid.size, dtype=np.int64)
        col = np.empty_like(row)
        row[0::2], row[1::2] = uid, iid
        col[0::2], col[1::2] = iid, uid
        return cls.from_coo(row, col, None, n, n, device, symmetric=True, **kw)

    @classmethod
    def bipartite_sym_norm(cls, uid, iid, num_users, num_items, device, **kw):
        """selfcf.py:291-306 + 240-255 (ssl4rec.py:79-88): A = R~ + R~^T with duplicate interactions
        summed, then D^-1/2 A D^-1/2 with 1/sqrt(0) -> 0, float32."""
        n = num_users + num_items
        kw.setdefault("_default_row_range", (0, num_users))
        if torch.device(device).type == "cuda":
            u, i = _dev_i64(uid, device), _dev_i64(iid, device) + num_users
            rp, c, v, _ = coo_to_csr_device(torch.cat([u, i]), torch.cat([i, u]), None, n, n, device, coalesce=True)
            return cls(rp, c, sym_norm_device(rp, c, v, n), n, n, device, symmetric=True, **kw)
        uid, iid = _np_i64(uid), _np_i64(iid) + num_users
        rp, c, v = _coalesce_host(np.concatenate([uid, iid]), np.concatenate([iid, uid]), None, n, n)
        rows = np.repeat(np.arange(n), np.diff(rp))
        rowsum = np.zeros(n, dtype=np.float32)
        np.add.at(rowsum, rows, v)
        with np.errstate(divide="ignore"):
            dinv = np.power(rowsum, np.float32(-0.5), dtype=np.float32)
        dinv[np.isinf(dinv)] = 0.0
        return cls(rp, c, (dinv[rows] * v * dinv[c]).astype(np.float32), n, n, device, symmetric=True, **kw)

    @classmethod
    def row_normalised(cls, row, col, val, n_rows, n_cols, device, **kw):
        """Graph.normalize_graph_mat on a NON-square matrix (selfcf.py:250-254 = ncl.py:37-41):
        D^-1 A with 1/0 -> 0, duplicates summed first (scipy CSR) — MHCN's R and H operators
        (univariate/mhcn.py:340-368,401-402).  GPU device only."""
        rp, c, v, _ = coo_to_csr_device(row, col, val, n_rows, n_cols, device, coalesce=True)
        rinv = torch.empty(n_rows, dtype=torch.float32, device=rp.device)
        out = torch.empty_like(v)
        _lib.call("gcr_csr_row_norm_f32", rp, c, v, n_rows, rinv, out, on=rp)
        return cls(rp, c, out, n_rows, n_cols, device, symmetric=False, **kw)

    @classmethod
    def from_edge_index_gcn_norm(cls, edge_index, num_nodes, device, symmetric=False, **kw):
        """lightgcn.py:25 `LGConv()(x, edge_index)`: deg[v] = #edges with target v; w_e =
        deg^-1/2[src] deg^-1/2[dst] (inf -> 0); out[dst] += w_e x[src]  => CSR over rows = dst."""
        if torch.device(device).type == "cuda":
            ei = _dev_i64(edge_index, device)
            rp, c, _, _ = coo_to_csr_device(ei[1].contiguous(), ei[0].contiguous(), None, num_nodes, num_nodes, device)
            return cls(rp, c, sym_norm_device(rp, c, None, num_nodes), num_nodes, num_nodes, device,
                       symmetric=symmetric, **kw)
        ei = _np_i64(edge_index)
        src, dst = ei[0], ei[1]
        deg = np.bincount(dst, minlength=num_nodes).astype(np.float32)
        with np.errstate(divide="ignore"):
            dis = np.power(deg, np.float32(-0.5), dtype=np.float32)
        dis[np.isinf(dis)] = 0.0
        return cls.from_coo(dst, src, (dis[src] * dis[dst]).astype(np.float32), num_nodes, num_nodes, device,
                            symmetric=symmetric, **kw)


def _dev_i64(a, device):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return torch.as_tensor(a).to(device=device, dtype=torch.int64).contiguous()


def coo_to_csr_device(row, col, val, n_rows, n_cols, device, coalesce=False, want_perm=False):
    """gcr_coo_to_csr: returns (rowptr int64 [n_rows+1], col int32 [nnz'], val fp32 [nnz'] or None,
    perm int64 [nnz'] or None) as device tensors.  Raises on ids outside the matrix."""
    row, col = _dev_i64(row, device), _dev_i64(col, device)
    nnz = row.numel()
    if col.numel() != nnz:
        raise ValueError("row / col length mismatch")
    if val is not None:
        val = torch.as_tensor(val).to(device=device, dtype=torch.float32).contiguous()
    rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=device)
    col_out = torch.empty(max(nnz, 1), dtype=torch.int32, device=device)
    keep_val = val is not None or coalesce
    val_out = torch.empty(max(nnz, 1), dtype=torch.float32, device=device) if keep_val else None
    perm = torch.empty(max(nnz, 1), dtype=torch.int64, device=device) if (want_perm and not coalesce) else None
    meta = torch.zeros(2, dtype=torch.int64, device=device)
    ws = _lib.workspace("gcr_coo_to_csr_workspace_bytes", nnz, device=device, dtype=torch.uint8)
    _lib.call("gcr_coo_to_csr", row, col, val, nnz, n_rows, n_cols, coalesce, rowptr, col_out, val_out, perm,
              meta[0:1], meta[1:2], ws, on=device)
    n_out, n_err = (int(v) for v in meta.tolist())
    if n_err:
        raise ValueError(f"{n_err} COO entries have a row / column outside [{n_rows}, {n_cols}]")
    return (rowptr, col_out[:n_out].contiguous(), None if val_out is None else val_out[:n_out].contiguous(),
            None if perm is None else perm[:n_out].contiguous())


def sym_norm_device(rowptr, col, val, n):
    """gcr_csr_sym_norm_f32 on a square symmetric operator: D^-1/2 A D^-1/2 (val None = ones)."""
    dinv = torch.empty(n, dtype=torch.float32, device=rowptr.device)
    out = torch.empty(col.numel(), dtype=torch.float32, device=rowptr.device)
    _lib.call("gcr_csr_sym_norm_f32", rowptr, col, val, n, n, None, None, dinv, None, out, on=rowptr)
    return out


def _coo_to_csr_host(row, col, val, n_rows):
    order = np.argsort(row, kind="stable")
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n_rows), out=rowptr[1:])
    v = None if val is None else np.asarray(val, dtype=np.float32)[order]
    return rowptr, col[order].astype(np.int32), v, order


def _coalesce_host(row, col, val, n_rows, n_cols):
    key = row * np.int64(n_cols) + col
    order = np.argsort(key, kind="stable")
    key_s = key[order]
    first = np.ones(key_s.size, dtype=bool)
    first[1:] = key_s[1:] != key_s[:-1]
    seg = np.cumsum(first) - 1
    v_in = np.ones(row.size, dtype=np.float32) if val is None else np.asarray(val, dtype=np.float32)
    v = np.zeros(int(first.sum()), dtype=np.float32)
    np.add.at(v, seg, v_in[order])
    r, c = row[order][first], col[order][first]
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n_rows), out=rowptr[1:])
    return rowptr, c.astype(np.int32), v
