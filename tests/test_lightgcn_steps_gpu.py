"""LightGCN's full-batch training step (the workload bench.py times) pinned to lightgcn.py's own loop body (lightgcn.py:84-120)
run in float64: tests/golden/lightgcn_steps.npz, written by scripts/gen_golden_lightgcn_steps.py.  Six steps from the
fixture's tables through `encoders.LightGCN.loss(graph, neg_i, loss_type, reg_weight)`, `.backward()` (`_Propagate.backward`
included) and `FusedAdam(lr, weight_decay)` / `FusedSGD(lr, momentum=0, weight_decay)`, at four configurations of the
reference's grid (tests/lightgcn_steps_common.py) and, for the BPR ones, on every path that reaches other kernels:

  * sampled          `bpr_edge_sums` below BPR_SORTED_MIN_BATCH: `bpr_sums` and the atomic backward;
  * edge             BPR_SORTED_MIN_BATCH = 1: `_BprEdgeSums` (positives as one SpMM on per-edge coefficients, the negatives'
                     user side as an SpMM on `negatives_user_block`, their item side by the payload sort);
  * edge_index_sort  the same with BPR_NEG_PAYLOAD_SORT = False (an index sort and gcr_bpr_bwd_sorted_f32);
  * edge_windowed    (A) the same as `edge` on a graph whose hub rows have a forced windowed companion, so that the
                     propagation, forward and backward, is gcr_spmm_windowed_f32.

The recorded negatives are in the reference's file order; the loss wants them in the order of the operator's user rows
(`graph.user_major_edges`), which the test derives from the file by a stable sort and checks against the graph.

Everything is compared with the reference's float64 run, never with another path of ours:
  * the loss of every step at 1e-5 relative and the final tables by the rule of tests/step_pins.py (family "lightgcn":
    `atol_floor_4` of slack = the reference's own max |f32 - f64|); tests/test_lightgcn_steps_cpu.py shows that this is
    under a tenth of what a dropped regulariser or weight decay moves;
  * the step-0 gradient of each table by the rule of tests/f64_pins.py: err = max|got - f64| / max|f64| <=
    max(4 x drift, 2^-20) and <= 1e-5 (a trajectory under Adam cannot see a wrong global factor such as a missing 1 / E);
  * the isolated user's row: gradient exactly 0, the row unchanged at the end (A, C, D) or moved by weight decay alone (B).
    The isolated ITEM is no such case, in the reference either: `torch.randint` draws it as a negative and the BCE branch
    scores every item, so it has a gradient (through no edge) and is covered by the table checks.

Measured on the MI355X, worst err / bound over all parametrisations and ten further replays of each sampled case (its
atomic backward sums in another order every run; every case prints its own figures): loss 0.014 (1.4e-7 relative, B);
step-0 gradient 0.35 user table (3.3e-7, D edge), 0.43 item table (A sampled, 0.28 to 0.43 by run; 4.5e-7 of 1.15e-6 on
B sampled); final tables 0.39 user (1.6e-7 of 4.0e-7, B sampled, 0.28 to 0.39 by run), 0.40 item (2.1e-7 of 5.3e-7, C);
the isolated user's row under weight decay 0.05."""
import numpy as np
import pytest
import torch

import step_pins as sp
from lightgcn_steps_common import TABLES, adam_on_weight_decay_only, config, fixture, init_table, user_major_perm
from oracle import oracle_np as onp
from spmm_window_common import HUB_MIN_DEGREE, WINDOW_ROWS

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 2.0 ** -20
NORTH_STAR = 1e-5
CASES = [("A", "sampled"), ("A", "edge"), ("A", "edge_index_sort"), ("A", "edge_windowed"),
         ("B", "sampled"), ("B", "edge"), ("B", "edge_index_sort"),
         ("C", "bce"),
         ("D", "sampled"), ("D", "edge"), ("D", "edge_index_sort")]


def _autograd_nodes(t):
    """Names of the autograd nodes behind a tensor."""
    seen, names, stack = set(), set(), [t.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return names


def _set_path(monkeypatch, path):
    from recommendation_amd import functional as Fn
    if path.startswith("edge"):
        monkeypatch.setattr(Fn, "BPR_SORTED_MIN_BATCH", 1)
        monkeypatch.setattr(Fn, "BPR_NEG_PAYLOAD_SORT", path != "edge_index_sort")
    return dict(hub_window_rows=WINDOW_ROWS, hub_min_degree=HUB_MIN_DEGREE) if path == "edge_windowed" else {}


def _replay(g, c, path, graph_kw):
    """The fixture's steps of configuration c -> (losses [steps] float64, step-0 gradients, final tables), numpy float64."""
    from recommendation_amd import functional as Fn
    from recommendation_amd.encoders import LightGCN
    from recommendation_amd.graph import CsrGraph
    from recommendation_amd.optim import FusedAdam, FusedSGD
    cfg = config(g, c)
    nu, ni, d = int(g["num_users"]), int(g["num_items"]), cfg["embedding_dim"]
    u, i = g["train_user"].astype(np.int64), g["train_item"].astype(np.int64)
    model = LightGCN(nu, ni, embedding_dim=d, num_layers=cfg["num_layers"]).cuda()
    params = {"user": model.user_embedding.weight, "item": model.item_embedding.weight}
    with torch.no_grad():
        for k in TABLES:
            params[k].copy_(torch.from_numpy(init_table(g, c, k)))
    graph = CsrGraph.from_edge_index_gcn_norm(onp.build_edge_index(u, i, nu), nu + ni, "cuda", symmetric=True, **graph_kw)
    if path == "edge_windowed":
        assert graph.hub is not None and graph.hub.eligible(d) and d <= Fn.WINDOWED_MAX_D
        assert graph.hub.n_hub >= 3 and graph.hub.n_windows == -(-(nu + ni) // WINDOW_ROWS)
    else:
        assert graph.hub is None
    # file order -> the order of the operator's user rows
    perm = user_major_perm(g)
    eu, ei = graph.user_major_edges(nu)
    assert np.array_equal(eu.cpu().numpy(), u[perm]) and np.array_equal(ei.cpu().numpy(), i[perm])
    negs = torch.from_numpy(np.ascontiguousarray(g[f"{c}/neg_i"][:, perm]).astype(np.int64)).cuda()
    if cfg["optimizer"] == "Adam":
        opt = FusedAdam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    else:
        assert cfg["optimizer"] == "SGD"                   # torch.optim.SGD(params, lr, weight_decay): no momentum
        opt = FusedSGD(model.parameters(), lr=cfg["lr"], momentum=0, weight_decay=cfg["weight_decay"])
    losses, grad0 = [], None
    for n in range(int(g["steps"])):
        opt.zero_grad()
        loss = model.loss(graph, negs[n], cfg["loss_type"], cfg["reg_weight"])
        if n == 0:
            nodes = _autograd_nodes(loss)
            assert "_PropagateBackward" in nodes
            if path == "bce":
                assert "_BceEdgeLossBackward" in nodes
            elif path == "sampled":
                assert u.size < Fn.BPR_SORTED_MIN_BATCH and "_BprSumsBackward" in nodes
            else:
                assert "_BprEdgeSumsBackward" in nodes and "_BprSumsBackward" not in nodes
        loss.backward()
        if n == 0:
            grad0 = {k: params[k].grad.detach().cpu().double().numpy() for k in TABLES}
        opt.step()
        losses.append(loss.detach().reshape(()).clone())
    final = {k: params[k].detach().cpu().double().numpy() for k in TABLES}
    return torch.stack(losses).cpu().double().numpy(), grad0, final


@pytest.mark.parametrize("c,path", CASES, ids=[f"{c}-{p}" for c, p in CASES])
def test_trajectory_matches_reference_float64(monkeypatch, c, path):
    g = fixture()
    cfg = config(g, c)
    losses, grad0, final = _replay(g, c, path, _set_path(monkeypatch, path))
    tag = f"LGNPIN {c}:{path}"
    rec = sp.record("lightgcn", g, c, path)
    report, failures = [], []

    for k in TABLES:
        ref = g[f"{c}/f64/grad0/{k}"]
        drift = float(g[f"{c}/drift/{k}"])
        bound = min(max(4.0 * drift, GRAD_FLOOR), NORTH_STAR)
        err = float(np.abs(grad0[k] - ref).max() / np.abs(ref).max())
        report.append(f"{tag} grad0/{k} err={err:.3e} bound={bound:.3e} ratio={err / bound:.3f} (drift {drift:.3e})")
        if err > bound:
            failures.append(f"grad0/{k}: err {err:.3e} > bound {bound:.3e}")

    # the isolated user: no edge, never a negative, not among the BCE branch's users
    iso = int(g["iso_user"])
    row0 = init_table(g, c, "user")[iso].astype(np.float64)
    if grad0["user"][iso].any():
        failures.append(f"isolated user's step-0 gradient is not zero: max {np.abs(grad0['user'][iso]).max():.3e}")
    if cfg["weight_decay"]:
        want = adam_on_weight_decay_only(row0, cfg["lr"], cfg["weight_decay"], int(g["steps"]))
        err, tol = float(np.abs(final["user"][iso] - want).max()), rec.atol["user"]
        report.append(f"{tag} isolated user, weight decay alone err={err:.3e} bound={tol:.3e} ratio={err / tol:.3f}")
        if err > tol:
            failures.append(f"isolated user's row is not Adam on weight decay alone: err {err:.3e} > {tol:.3e}")
    elif not np.array_equal(final["user"][iso], row0):
        failures.append(f"isolated user's row moved by {np.abs(final['user'][iso] - row0).max():.3e}")
    print("\n".join(report))
    sp.check(rec, losses, final, failures)             # the losses and the final tables, and one message for everything


def test_edge_path_losses_are_reproducible(monkeypatch):
    """Two replays of A on the `edge` path (payload sort) give the same losses bit for bit.  The final tables are not
    asserted bitwise: the sorted scatter of the negatives' item rows adds whole rows with atomics."""
    g = fixture()
    kw = _set_path(monkeypatch, "edge")
    first, _, _ = _replay(g, "A", "edge", kw)
    second, _, _ = _replay(g, "A", "edge", kw)
    assert np.array_equal(first, second), (first.tolist(), second.tolist())
