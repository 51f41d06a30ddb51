"""Shared by the GPU step tests, their CPU re-checks and the fixture writers (scripts/step_golden.py): the trajectory pin.

A step fixture tests/golden/<family>_steps.npz holds the reference's own training-loop body run from given tables on given
batches: in float64 (per-step loss terms, final tables), in float32 (terms; per table slack = max |f32 - f64| of its final
value) and in float64 with one loss term dropped (per table delta_<term> = max |final - f64 final|).  One rule holds a
model's `train_step` to it:

  * a loss term lies within tol = max(REL x |f64|, 4 x |f32 - f64|) of the float64 value (`term_tol`; without the float32
    run it is the pure relative form of `assert_allclose(rtol=REL)`; a term that is a difference of parts is held to the
    size of the parts, `difference_tol`).  TERM_FORM says which family uses which;
  * a final table lies within atol of the float64 final, atol built from the reference's own float32 slack and floored at
    FLOOR.  Two spellings are in use and they are NOT the same number; TABLE_FORM says which family uses which:

        family                                    form                      atol at slack = 0
        ncl, mhcn, sept, buir                     max(4 x slack, FLOOR)     1e-7     `atol_floor_1`
        gcl, lightgcn, ssl4rec, directau          4 x max(slack, FLOOR)     4e-7     `atol_floor_4`

    (tests/test_prepared_models_gpu.py takes the form of the fixture it reads.)  Unifying them at the tighter floor is
    open work: it changes what four families assert and wants GPU evidence of its own;
  * that tolerance checks something: a dropped loss term moves a table by more than DROPPED x atol (`sees_dropped`; a
    parameter no term reaches moves by exactly 0), or the table moves by more than MOVED x slack (`has_moved`); the CPU
    re-checks of lightgcn, ssl4rec and directau ask DROPPED_CPU x atol of a dropped term instead;
  * the writer asserts all of this when it stores the numbers, a CPU test re-checks it from the stored numbers
    (`Record.assert_sensitivity`), and the GPU test asserts it again before it compares (`check`).

`Record` is one configuration of one fixture as plain arrays; `record(family, g, c)` builds it from the family's own key
layout (ssl4rec and directau build theirs in tests/ssl4rec_fixture.py and tests/directau_fixture.py, which know what
those fixtures regenerate instead of storing).  Plain numpy; torch is imported only by `batch`."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-5              # a loss term, relative to |f64|
F32 = 4.0               # x the reference's own |f32 - f64|, for a term and for a table
FLOOR = 1e-7            # of a table's slack: the reference's |f32 - f64| can be at the rounding level by chance
DROPPED = 50.0          # a dropped term moves a table by more than DROPPED x atol
DROPPED_CPU = 10.0      # the variant of the lightgcn, ssl4rec and directau re-checks
MOVED = 100.0           # a table moves by more than MOVED x slack


def atol_floor_1(slack):
    return max(F32 * slack, FLOOR)


def atol_floor_4(slack):
    return F32 * max(slack, FLOOR)


TABLE_FORM = {"ncl": atol_floor_1, "mhcn": atol_floor_1, "sept": atol_floor_1, "buir": atol_floor_1,
              "gcl": atol_floor_4, "lightgcn": atol_floor_4, "ssl4rec": atol_floor_4, "directau": atol_floor_4}
TERM_FORM = {"ncl": "f32", "mhcn": "f32", "sept": "f32", "buir": "f32",
             "gcl": "rtol", "lightgcn": "rtol", "ssl4rec": "rtol", "directau": "rtol"}


def term_tol(f64, f32=None):
    """max(REL |f64|, F32 |f32 - f64|) per step; REL |f64| alone (assert_allclose's rtol) without the float32 run."""
    tol = REL * np.abs(f64)
    return tol if f32 is None else np.maximum(tol, F32 * np.abs(f32 - f64))


def difference_tol(*parts):
    """For a term that is a difference of `parts` (DirectAU's loss = pos_loss - neg_loss + ...): REL x the sum of their sizes."""
    return REL * sum(np.abs(p) for p in parts)


def sees_dropped(delta, atol, unreached=False, factor=DROPPED):
    """A tolerance that would not see a missing loss term checks nothing."""
    return delta == 0.0 if unreached else delta > factor * atol


def has_moved(moved, slack):
    return moved > MOVED * slack


class Record:
    """One configuration of a step fixture.  terms: names; f64, f32, tol: [steps, n_terms]; tables: {name: float64 final};
    slack, atol: {name: float}; dropped: {name: {term: delta}}, each held to `factor` x atol unless `factor` is None
    (ssl4rec and directau claim a term of SOME table only, in their CPU tests), unreached = {term: names};
    moved: {name: (initial table, slack unit)} (the MOVED rule), or None."""

    def __init__(self, family, tag, terms, f64, f32, tables, slack, tol=None, dropped=None, factor=DROPPED, unreached=None,
                 moved=None):
        self.family, self.tag, self.terms = family, tag, tuple(terms)
        self.f64 = np.asarray(f64, dtype=np.float64).reshape(-1, len(self.terms))
        self.f32 = np.asarray(f32, dtype=np.float64).reshape(self.f64.shape)
        self.tol = term_tol(self.f64, self.f32 if TERM_FORM[family] == "f32" else None) if tol is None else tol
        self.tables, self.slack = tables, {k: float(slack[k]) for k in tables}
        self.atol = {k: TABLE_FORM[family](self.slack[k]) for k in tables}
        self.dropped, self.factor, self.unreached, self.moved = dropped, factor, unreached or {}, moved

    def assert_sensitivity(self, finals=None):
        """The fixture's side of the rule, from stored numbers alone; with `finals` the MOVED rule is asked of them (the
        model's own tables) instead of the reference's."""
        for k in self.tables:
            for t, d in (self.dropped[k] if self.dropped and self.factor else {}).items():
                assert sees_dropped(d, self.atol[k], k in self.unreached.get(t, ()), self.factor), (self.tag, k, t, d, self.atol[k])
            if self.moved:
                init, unit = self.moved[k]
                moved = float(np.abs((finals or self.tables)[k] - init).max())
                assert has_moved(moved, unit), (self.tag, k, moved, unit)


def check(rec, terms, tables, failures=()):
    """What every trajectory test does with what the model produced, terms [steps, n_terms] and final tables by name:
    builds the report, collects every failing term and table (non-finite ones too) behind the caller's own `failures`,
    prints the report, asserts the sensitivity conditions, and fails once with the report and all failures."""
    got = np.asarray(terms, dtype=np.float64).reshape(-1, len(rec.terms))
    assert got.shape == rec.f64.shape, (rec.tag, got.shape, rec.f64.shape)
    finals = {k: np.asarray(tables[k], dtype=np.float64) for k in rec.tables}
    where = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    report, failures = [f"STEPPIN {rec.family} {rec.tag} {where}"], list(failures)
    for j, k in enumerate(rec.terms):
        ref, tol, err = rec.f64[:, j], rec.tol[:, j], np.abs(got[:, j] - rec.f64[:, j])
        report.append(f"  {k}: max err {err.max():.3g} ({(err / np.maximum(tol, 1e-300)).max():.2f} x tol), "
                      f"max tol {tol.max():.17g}")
        if not np.all(err <= tol):
            failures.append(f"{k}: got {got[:, j].tolist()} reference {ref.tolist()}")
    for k, ref in rec.tables.items():
        assert finals[k].shape == ref.shape, (rec.tag, k, finals[k].shape, ref.shape)
        err, atol = float(np.abs(finals[k] - ref).max()), rec.atol[k]
        line = f"  {k}: max err {err:.3g} ({err / atol:.2f} x atol), atol {atol:.17g}, reference f32 slack {rec.slack[k]:.17g}"
        if rec.dropped:
            line += "; a dropped term moves it by " + ", ".join(f"{t} {v:.3g}" for t, v in rec.dropped[k].items())
        if rec.moved:
            line += f"; moved {float(np.abs(finals[k] - rec.moved[k][0]).max()):.3g}"
        report.append(line)
        if not np.isfinite(finals[k]).all():
            failures.append(f"{k}: not finite")
        elif err > atol:
            failures.append(f"{k}: max |final - f64| = {err:.3g} > atol {atol:.3g}")
    print("\n".join(report))
    if all(np.isfinite(f).all() for f in finals.values()):
        rec.assert_sensitivity(finals)
    assert not failures, "\n".join(report + failures)


# ---- the families' key layouts -> Record (ssl4rec and directau: their own fixture modules) ----

NCL_TERMS = ("rec_loss", "ssl_loss", "proto_loss", "total_loss")
MHCN_TERMS = ("rec_loss", "reg_loss", "ss_loss", "total_loss")
MHCN_UNREACHED = {"ss": {"sgating_weights.4", "sgating_bias.4"}, "reg": {"sgating_bias.4"}}
SEPT_TERMS = ("rec_loss", "neighbor_dis_loss", "total_loss")
SEPT_TABLES = ("user_embeddings", "item_embeddings")
BUIR_TENSORS = ("online_encoder.embedding_dict.user_emb", "online_encoder.embedding_dict.item_emb",
                "target_encoder.embedding_dict.user_emb", "target_encoder.embedding_dict.item_emb", "predictor.weight",
                "predictor.bias")
GCL_TERMS = ("ssl_loss", "bpr_loss", "reg_loss", "total_loss")
LIGHTGCN_TABLES = ("user", "item")


def load(family):
    return np.load(os.path.join(GOLDEN, f"{family}_steps.npz"), allow_pickle=False)


def configs(family, g):
    return g["configs"].tolist() if family == "lightgcn" else [None] if family == "gcl" else list(range(int(g["configs"])))


def buir_init(g, c, k):
    return g[f"c{c}/init/" + k.replace("target_encoder", "online_encoder")]      # _init_target: the targets start as copies


def stack_terms(g, pre, terms):
    """(f64, f32) [steps, n_terms] of the layout that stores one vector per term and run."""
    return tuple(np.stack([g[f"{pre}{run}/{k}"] for k in terms], 1) for run in ("f64", "f32"))


def _with_delta(g, pre, init):
    """{name: init + f64/delta}: the float64 final stored as float32(final - init), exact to the writer's assert."""
    return {k: v.astype(np.float64) + g[f"{pre}f64/delta/{k}"].astype(np.float64) for k, v in init.items()}


def _dropped(g, pre, names, terms):
    return {k: {t: float(g[f"{pre}delta_{t}/{k}"]) for t in terms} for k in names}


def record(family, g, c=None, tag=""):
    """Configuration c of the fixture of `family` (ncl, mhcn, sept, buir, gcl, lightgcn) in its own key layout."""
    pre = "" if family == "gcl" else f"{c}/" if family == "lightgcn" else f"c{c}/"
    tag = tag if c is None else f"config {c} {tag}".strip()
    slack = lambda names: {k: g[f"{pre}slack/{k}"] for k in names}                                   # noqa: E731
    if family == "ncl":
        names = ("user_emb", "item_emb")
        return Record(family, tag, NCL_TERMS, *stack_terms(g, pre, NCL_TERMS), {k: g[f"{pre}f64/final/{k}"] for k in names},
                      slack(names), dropped=_dropped(g, pre, names, ("ssl_reg", "proto_reg", "reg")))
    if family in ("mhcn", "sept", "buir"):
        terms = {"mhcn": MHCN_TERMS, "sept": SEPT_TERMS, "buir": ("loss",)}[family]
        names = {"mhcn": lambda: g[f"{pre}names"].tolist(), "sept": lambda: SEPT_TABLES, "buir": lambda: BUIR_TENSORS}[family]()
        init = {k: buir_init(g, c, k) if family == "buir" else g[f"{pre}init/{k}"] for k in names}
        return Record(family, tag, terms, g[f"{pre}f64/losses"], g[f"{pre}f32/losses"], _with_delta(g, pre, init), slack(names),
                      dropped=_dropped(g, pre, names, ("update", "iu") if family == "buir" else ("ss", "reg")),
                      unreached=MHCN_UNREACHED if family == "mhcn" else None)
    if family == "gcl":
        names = [k[len("init/"):] for k in g.files if k.startswith("init/")]
        tables = {k: g[f"f64/final/{k}"] for k in names}
        drift = {k: float(np.abs(g[f"f32/final/{k}"] - tables[k]).max()) for k in names}    # in place of a stored slack
        return Record(family, tag, GCL_TERMS, *stack_terms(g, pre, GCL_TERMS), tables, drift,
                      moved={k: (g[f"init/{k}"], max(drift[k], FLOOR)) for k in names})
    assert family == "lightgcn", family
    init = {k: g[f"init_d{int(g[f'{c}/embedding_dim'])}/{k}"] for k in LIGHTGCN_TABLES}
    terms = ("reg", "wd") if float(g[f"{c}/weight_decay"]) else ("reg",)
    return Record(family, tag, ("loss",), g[f"{pre}f64/loss"], g[f"{pre}f32/loss"], _with_delta(g, pre, init), slack(LIGHTGCN_TABLES),
                  dropped=_dropped(g, pre, LIGHTGCN_TABLES, terms), factor=DROPPED_CPU)


# ---- the shared preamble of the GPU tests ----

def triples(g):
    return [[int(u), int(i), 1.0] for u, i in zip(g["train_user"], g["train_item"])]


def social(g):
    return [[int(a), int(b), 1.0] for a, b in zip(g["social_follower"], g["social_followee"])]


def assert_dense_id_order(m, g):
    """The fixture's batches and tables are indexed by the reference's dense ids: the model's maps must be the fixture's."""
    assert [m.data.id2user[k] for k in range(m.data.user_num)] == g["user_ids"].tolist()
    assert [m.data.id2item[k] for k in range(m.data.item_num)] == g["item_ids"].tolist()


def batch(g, n, names, prefix=""):
    import torch
    return tuple(torch.from_numpy(g[f"{prefix}batch{n}_{s}"].astype(np.int64)).cuda() for s in names)


def planted_group_lists(rng, n_u=150, n_i=200, groups=5):
    """(train, test, social) raw-id lists of the end-to-end tests: 15 items of the user's own group, 12 to train on;
    six followees of the group; 300 pairs reciprocated; one pair naming a user that never interacts."""
    train, test, soc = [], [], []
    for u in range(n_u):
        own = rng.permutation(np.arange(u % groups, n_i, groups))[:15]          # items of the user's group
        train += [[f"u{u:03d}", f"i{int(i):03d}", 1.0] for i in own[:12]]
        test += [[f"u{u:03d}", f"i{int(i):03d}", 1.0] for i in own[12:]]
        for v in rng.choice(np.arange(u % groups, n_u, groups), 6, replace=False):
            if v != u:
                soc.append([f"u{u:03d}", f"u{int(v):03d}", 1.0])
    soc += [[b, a, w] for a, b, w in soc[:300]] + [["nobody", "u001", 1.0]]
    return train, test, soc
