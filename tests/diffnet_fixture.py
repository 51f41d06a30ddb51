"""tests/golden/diffnet_steps.npz (scripts/gen_golden_diffnet_steps.py): its key layout, what it regenerates instead of
storing, and its `Record`s under tests/step_pins.py's rule.  Shared by the writer, tests/test_diffnet_cpu.py and the two GPU
test files.  The family is tables by `atol_floor_1`, terms against the float64 and float32 runs: `registered()` puts it into
step_pins' two tables for as long as a `Record` is built or the writer records a table and takes it out again, because
tests/test_step_pins_cpu.py holds those tables to exactly the families it lists, in any session that imports this module.

  top level   train_user / train_item / user_ids / item_ids / social_follower / social_followee (step_golden.id_arrays),
              S_row, S_col, S_val and A_row, A_col, A_val: the reference's two COO operators in entry order,
              batch<n>_perm, batch<n>_neg (a batch is the whole training list in the sampler's shuffled order: users and
              positives are A_row[perm], A_col[perm], which `batch_arrays` rebuilds), steps, batch_size, configs, hp/lr,
              hp/reg_lambda, min_first_grad, relu_margin
  c<k>/       n_layer, d, names, table_seed, first_grad (Adam condition), min_pre and pre_err (ReLU margin),
              f64/losses and f32/losses [steps, 3], init/<name>, f64/delta/<name>, slack/<name>,
              delta_social/<name>, delta_rating/<name>, delta_reg/<name>
  comp<d>/    row, col, val (S in entry order), seed (of `component_inputs`), min_pre, pre_err,
              f64/h, f64/dx, f64/dw, scale/<k>, drift/<k>
"""
import contextlib

import numpy as np

import step_pins as sp


@contextlib.contextmanager
def registered():
    """step_pins.TABLE_FORM / TERM_FORM with the family "diffnet" in them, inside the block only."""
    forms = ((sp.TABLE_FORM, sp.atol_floor_1), (sp.TERM_FORM, "f32"))
    added = [table for table, _ in forms if "diffnet" not in table]
    for table, form in forms:
        table.setdefault("diffnet", form)
    try:
        yield
    finally:
        for table in added:
            del table["diffnet"]


TERMS = ("rec_loss", "reg_loss", "total_loss")
DROPS = ("social", "rating", "reg")
COMP_N, COMP_WIDTHS = 70, (32, 64, 128)


def load():
    return sp.load("diffnet")


def batch_perm(users, pos, a_row, a_col):
    """perm with (a_row[perm], a_col[perm]) == (users, pos): which training triple each sample of a whole-list batch is (a
    repeated triple's copies in order)."""
    slots = {}
    for t, key in enumerate(zip(a_row.tolist(), a_col.tolist())):
        slots.setdefault(key, []).append(t)
    perm = np.array([slots[key].pop(0) for key in zip(np.asarray(users).tolist(), np.asarray(pos).tolist())], dtype=np.int16)
    assert np.array_equal(a_row[perm], users) and np.array_equal(a_col[perm], pos)
    return perm


def batch_arrays(g, n):
    """(users, pos, neg) int64 of step n."""
    perm = g[f"batch{n}_perm"].astype(np.int64)
    return g["A_row"].astype(np.int64)[perm], g["A_col"].astype(np.int64)[perm], g[f"batch{n}_neg"].astype(np.int64)


def batch(g, n):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in batch_arrays(g, n))


def component_inputs(d, seed, n=COMP_N):
    """(x [n, d], w [2 d, d], g [n, d]) float32 of a component case, functions of (d, seed): x at the scale of a trained
    table, w at xavier scale, g with one element in eight and one whole row exactly zero."""
    rng = np.random.default_rng([seed, d])
    x = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    bound = np.sqrt(6.0 / (3 * d))
    w = rng.uniform(-bound, bound, (2 * d, d)).astype(np.float32)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g[rng.random((n, d)) < 0.125] = 0.0
    if n > 5:
        g[5] = 0.0
    return x, w, g


def component(g, d):
    """The component case of width d as a dict: row, col, val, x, w, g, and the float64 h, dx, dw with scale and drift."""
    pre = f"comp{d}/"
    x, w, gr = component_inputs(d, int(g[pre + "seed"]))
    out = dict(row=g[pre + "row"].astype(np.int64), col=g[pre + "col"].astype(np.int64), val=g[pre + "val"], x=x, w=w, g=gr)
    for k in ("h", "dx", "dw"):
        out[k], out[f"scale/{k}"], out[f"drift/{k}"] = g[pre + f"f64/{k}"], float(g[pre + f"scale/{k}"]), float(g[pre + f"drift/{k}"])
    return out


def names(g, c):
    return g[f"c{c}/names"].tolist()


def init(g, c):
    return {k: g[f"c{c}/init/{k}"] for k in names(g, c)}


def record(g, c):
    pre = f"c{c}/"
    ini = init(g, c)
    tables = {k: v.astype(np.float64) + g[f"{pre}f64/delta/{k}"].astype(np.float64) for k, v in ini.items()}
    with registered():                   # a Record takes its tolerances from the two tables when it is built
        return sp.Record("diffnet", f"config {c}", TERMS, g[pre + "f64/losses"], g[pre + "f32/losses"], tables,
                         {k: g[f"{pre}slack/{k}"] for k in tables},
                         dropped={k: {t: float(g[f"{pre}delta_{t}/{k}"]) for t in DROPS} for k in tables})


def conf(g, c, batch_size=None):
    return {"n_layer": int(g[f"c{c}/n_layer"]), "emb_size": int(g[f"c{c}/d"]), "lr": float(g["hp/lr"]),
            "reg_lambda": float(g["hp/reg_lambda"]), "regU": 1, "batch_size": batch_size or int(g["batch_size"]),
            "item.ranking.topN": [10, 20]}
