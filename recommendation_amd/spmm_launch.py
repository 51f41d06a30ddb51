"""The raw SpMM launches of include/gcr.h, each spelled once: for `functional`, the tests and the A/B scripts.

One function per export.  `graph` is anything with rowptr, col, val, n_rows, n_cols (a CsrGraph or a hub companion `H`) and
`plan` an SpmmPlan over it, so a caller may pass a permuted, a skipping or a companion plan; every other argument is a
keyword named as in gcr.h, workspaces included (nothing here allocates), with the defaults of `functional.spmm_into`.
Nothing is checked: a function puts its arguments in the header's order and calls.  `on` names the stream as `_lib.call`
takes it; `call` is `_lib.call` or another handle's (`_lib.call_on`).  tests/test_spmm_launch_cpu.py holds every position to
the header's parameter of that name.
"""
from . import _lib


def _plan_head(graph, plan):
    """The eight arguments every SpMM entry point of gcr.h starts with: a launch plan and the CSR it partitions."""
    return (plan.desc, plan.n_parts, plan.long_row, plan.long_slot0, plan.n_long, graph.rowptr, graph.col, graph.val)


def csr_acc2(graph, plan, *, x, d, partials, on, y=None, acc_in=None, acc_in2=None, acc_in2_scale=1.0, acc_out=None,
             acc_scale=1.0, val_scale=1.0, keep_bits=None, flags=0, inv_norm_out=None, col_active_bits=None, call=_lib.call):
    call("gcr_spmm_csr_acc2_f32", *_plan_head(graph, plan), keep_bits, val_scale, x, d, y, acc_in, acc_in2, acc_in2_scale,
         acc_out, acc_scale, flags, inv_norm_out, partials, graph.n_rows, graph.n_cols, col_active_bits, on=on)


def csr_dual(graph, plan, *, x, d, y_raw, y_norm, partials, on, inv_norm_out=None, keep_bits=None, val_scale=1.0,
             call=_lib.call):
    call("gcr_spmm_csr_dual_f32", *_plan_head(graph, plan), keep_bits, val_scale, x, d, y_raw, y_norm, inv_norm_out, partials,
         graph.n_rows, graph.n_cols, on=on)


def csr_dual_acc(graph, plan, *, x, d, y_raw, acc_in, acc_out, inv_norm_out, partials, on, y_norm=None, keep_bits=None,
                 val_scale=1.0, call=_lib.call):
    call("gcr_spmm_csr_dual_acc_f32", *_plan_head(graph, plan), keep_bits, val_scale, x, d, y_raw, y_norm, acc_in, acc_out,
         inv_norm_out, partials, graph.n_rows, graph.n_cols, on=on)


def rows(graph, plan, *, x, d, partials, on, y=None, acc_in=None, acc_out=None, acc_scale=1.0, val_scale=1.0, call=_lib.call):
    call("gcr_spmm_rows_f32", *_plan_head(graph, plan), val_scale, x, d, y, acc_in, acc_out, acc_scale, partials, graph.n_rows,
         graph.n_cols, on=on)


def rows_mapped(graph, plan, *, x, d, partials, on, y=None, acc_in=None, acc_out=None, acc_scale=1.0, val_scale=1.0,
                call=_lib.call):
    """`graph`: a row-ordered copy (graph.RowOrder: rowptr, col, val of P, row_id, and the n_rows / n_cols of the graph it
    was made from); `plan`: its plan, long_row in the graph's own rows."""
    call("gcr_spmm_rows_mapped_f32", *_plan_head(graph, plan), graph.row_id, val_scale, x, d, y, acc_in, acc_out, acc_scale,
         partials, graph.n_rows, graph.n_cols, on=on)


def hub_parts(graph, plan, *, x, d, y, partials, on, call=_lib.call):
    call("gcr_spmm_hub_parts_f32", *_plan_head(graph, plan), x, d, y, partials, graph.n_rows, graph.n_cols, on=on)


def hub_reduce(hub, *, partials, d, n_rows, on, y=None, acc_in=None, acc_out=None, acc_scale=1.0, val_scale=1.0, call=_lib.call):
    """`hub`: a HubPlan, for hub_row / n_hub / n_windows; n_rows: of the graph whose rows y and acc_out hold."""
    call("gcr_spmm_hub_reduce_f32", hub.hub_row, hub.n_hub, hub.n_windows, partials, d, val_scale, y, acc_in, acc_out, acc_scale,
         n_rows, on=on)


def windowed(hub_graph, hub_plan, graph, plan, hub, *, hub_split, partials, hub_partials, x, d, main_first, on, y=None,
             acc_in=None, acc_out=None, acc_scale=1.0, val_scale=1.0, call=_lib.call):
    """(hub_graph, hub_plan): the companion and its plan, the header's hub_* head; (graph, plan): the main pair, with the hub
    rows skipped; `hub`: the HubPlan, for hub_row / n_hub / n_windows."""
    call("gcr_spmm_windowed_f32", *_plan_head(hub_graph, hub_plan), hub_split, *_plan_head(graph, plan), partials, hub.hub_row,
         hub.n_hub, hub.n_windows, hub_partials, x, d, val_scale, y, acc_in, acc_out, acc_scale, main_first, graph.n_rows,
         graph.n_cols, on=on)


def windowed_mapped(hub_graph, hub_plan, graph, plan, hub, *, hub_split, partials, hub_partials, x, d, main_first, on, y=None,
                    acc_in=None, acc_out=None, acc_scale=1.0, val_scale=1.0, call=_lib.call):
    """`windowed` with a row-ordered main pair: (graph, plan) as `rows_mapped` takes them, over the non-hub rows."""
    call("gcr_spmm_windowed_mapped_f32", *_plan_head(hub_graph, hub_plan), hub_split, *_plan_head(graph, plan), graph.row_id,
         partials, hub.hub_row, hub.n_hub, hub.n_windows, hub_partials, x, d, val_scale, y, acc_in, acc_out, acc_scale,
         main_first, graph.n_rows, graph.n_cols, on=on)
