"""Reader of tests/golden/directau_steps.npz (written by scripts/gen_golden_directau.py, which imports this module too,
so that both sides share one definition of what is regenerated instead of stored).

Part (a), component cases: `DirectAU.alignment`, `uniformity` and `calculate_loss` of directau.py:240-251 run by the
reference itself in float64 on seeded tables and index batches, with autograd gradients with respect to the tables, and
the same in float32, kept as slack = max |f32 - f64| per output.  The tables and the index vectors are NOT stored: they
are numpy PCG64 draws from the case's seed (`Case.inputs`), CRC-checked so that a changed numpy stream fails loudly.
Gradients of more than SAMPLE entries are stored at a seeded sample of entries (`Case.at`); their slack and their
max |ref| cover the whole tensor — in a zero-row case the whole tensor but the all-zero row, whose gradient is twelve
orders larger (F.normalize's eps) and is stored, with a slack and a max of its own, by `Case.zero_grad`.

Part (b), trajectories: six bodies of the training loop directau.py:219-229 per configuration (`Config`): per-step
`pos_loss`, `neg_loss`, `l2`, `loss` and the final tables in float64, the float32 run as slack, and float64 reruns with
one term dropped (`delta`).
"""
import os
import zlib

import numpy as np

import step_pins as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "directau_steps.npz")
GRID = 2.0 ** -12
SAMPLE = 1024
TERMS = ("pos_loss", "neg_loss", "l2", "loss")
DROPPED = ("gamma", "neg", "reg")                   # gamma = 0, the negative branch dropped, reg.lambda = 0
TABLES = ("user_emb", "item_emb")
VALUES = ("sums", "align_pos", "align_neg", "unif_u", "unif_p", "unif_n", "calc_pos", "calc_neg", "train", "mix")
PRIMITIVES = ("sums", "align_pos", "align_neg", "unif_u", "unif_p", "unif_n")     # the rest are differences of these
OBJECTIVES = ("train", "mix")
# what `mix` weighs (chosen so that no coefficient of the eight sums cancels, unlike the training loss whose G_u does):
#   alignment(u, p) + MIX_NEG * alignment(u, n) + gamma * (uniformity(u, t) + MIX_P * uniformity(p, t) + MIX_N * uniformity(n, t))
MIX_NEG, MIX_P, MIX_N = 0.7, 0.5, 0.25


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def sample_index(size, seed):
    """SAMPLE distinct flat positions of a tensor of `size` entries, ascending."""
    return np.sort(np.random.default_rng(int(seed)).choice(int(size), SAMPLE, replace=False)).astype(np.int64)


def case_inputs(d, batch, n_users, n_items, zero_row, seed):
    """(user_tab [n_users, d], item_tab [n_items, d] float32; u, i, j int64 [batch]).  The tables are smaller than the
    larger batches, so ids recur; with zero_row one row of each table is all zero and is referenced by the batch."""
    rng = np.random.default_rng(int(seed))
    user_tab = (rng.standard_normal((n_users, d)) * 0.1).astype(np.float32)
    item_tab = (rng.standard_normal((n_items, d)) * 0.1).astype(np.float32)
    u = rng.integers(0, n_users, batch).astype(np.int64)
    i = rng.integers(0, n_items, batch).astype(np.int64)
    j = rng.integers(0, n_items, batch).astype(np.int64)
    if zero_row:
        user_tab[n_users // 2] = 0.0
        item_tab[n_items // 3] = 0.0
        u[batch // 4], i[batch // 2], j[batch // 5] = n_users // 2, n_items // 3, n_items // 3
    return user_tab, item_tab, u, i, j


class Case:
    """One component case of part (a)."""

    def __init__(self, g, k):
        self.g, self.pre = g, f"a{k}/"
        p = self.pre
        self.d, self.batch = int(g[p + "d"]), int(g[p + "batch"])
        self.n_users, self.n_items = int(g[p + "n_users"]), int(g[p + "n_items"])
        self.gamma, self.t, self.reg = float(g[p + "gamma"]), float(g[p + "t"]), float(g[p + "reg"])
        self.zero_row, self.seed = bool(g[p + "zero_row"]), int(g[p + "seed"])

    def __repr__(self):
        return f"d{self.d}-B{self.batch}" + ("-zero" if self.zero_row else "")

    def inputs(self):
        out = case_inputs(self.d, self.batch, self.n_users, self.n_items, self.zero_row, self.seed)
        assert crc(np.concatenate([a.reshape(-1).view(np.uint8) for a in out])) == int(self.g[self.pre + "crc"]), \
            "numpy stream changed: component inputs"
        return out

    def shape(self, table):
        return (self.n_users if table == "user_emb" else self.n_items, self.d)

    def value(self, name):
        return self.g[f"{self.pre}f64/{name}"]

    def value_slack(self, name):
        return self.g[f"{self.pre}slack/{name}"]

    def zero_index(self, table):
        """The all-zero row of `table` in a zero-row case (case_inputs), else None."""
        if not self.zero_row:
            return None
        return self.n_users // 2 if table == "user_emb" else self.n_items // 3

    def index(self, table):
        """Flat positions at which `grad` is stored: every entry, or a seeded sample of SAMPLE of them for a larger
        tensor; in a zero-row case without the zero row's entries, which `zero_grad` holds whole."""
        size = int(np.prod(self.shape(table)))
        idx = np.arange(size, dtype=np.int64) if size <= SAMPLE else sample_index(size, self.seed + (1 if table == "user_emb" else 2))
        z = self.zero_index(table)
        return idx if z is None else idx[idx // self.d != z]

    def at(self, table, full):
        return np.asarray(full).reshape(-1)[self.index(table)]

    def zero_grad(self, objective, table):
        """Gradient of the all-zero row (F.normalize divides by eps = 1e-12 there: ~1e10), its float32 slack and max."""
        p = f"{self.pre}zgrad_{objective}/{table}"
        return self.g[p], float(self.g[p + "/slack"]), float(self.g[p + "/max"])

    def grad(self, objective, table):
        return self.g[f"{self.pre}grad_{objective}/{table}"]

    def grad_slack(self, objective, table):
        return float(self.g[f"{self.pre}gslack_{objective}/{table}"])

    def grad_max(self, objective, table):
        return float(self.g[f"{self.pre}gmax_{objective}/{table}"])


class Config:
    """One trajectory configuration of part (b)."""

    def __init__(self, g, c):
        self.g, self.pre = g, f"c{c}/"
        p = self.pre
        self.n_layers, self.emb = int(g[p + "n_layers"]), int(g[p + "emb"])
        self.gamma, self.reg, self.optimizer = float(g[p + "gamma"]), float(g[p + "reg"]), str(g[p + "optimizer"])

    def __repr__(self):
        return f"L{self.n_layers}-g{self.gamma}-d{self.emb}-{self.optimizer}"

    def conf(self):
        g = self.g
        return {"model": {"name": "DirectAU", "type": "graph"}, "embedding.size": self.emb, "batch.size": int(g["batch_size"]),
                "learning.rate": float(g["learning_rate"]), "reg.lambda": self.reg, "optimizer": self.optimizer,
                "item.ranking.topN": [10, 20], "DirectAU": {"gamma": self.gamma, "n_layers": self.n_layers}}

    def init(self, table):
        return self.g[f"{self.pre}init/{table}"]

    def record(self):
        """The trajectory of this configuration as tests/step_pins.py takes it.  pos_loss, neg_loss and l2 at rtol; `loss`,
        their difference, within REL x (|pos_loss| + |neg_loss|); the MOVED rule; the deltas for the CPU test's claim."""
        g, p = self.g, self.pre
        f64, f32 = sp.stack_terms(g, p, TERMS)
        tol = sp.term_tol(f64)
        tol[:, TERMS.index("loss")] = sp.difference_tol(f64[:, TERMS.index("pos_loss")], f64[:, TERMS.index("neg_loss")])
        slack = {k: float(g[f"{p}slack/{k}"]) for k in TABLES}
        return sp.Record("directau", repr(self), TERMS, f64, f32, {k: g[f"{p}f64/final/{k}"] for k in TABLES}, slack, tol=tol,
                         dropped={k: {t: float(g[f"{p}delta_{t}/{k}"]) for t in DROPPED} for k in TABLES}, factor=None,
                         moved={k: (self.init(k), slack[k]) for k in TABLES})


def batches(g):
    """The six (user_idx, pos_idx, neg_idx) int64 triples, dense ids, as the reference's sampler drew them."""
    return [tuple(g[f"batch{n}_{k}"] for k in ("users", "pos", "neg")) for n in range(int(g["steps"]))]


def train_records(g):
    """The training records [[user, item, 1.0], ...] with their raw string ids."""
    return [[str(u), str(i), 1.0] for u, i in zip(g["train_user"], g["train_item"])]


def load():
    g = np.load(GOLDEN, allow_pickle=False)
    return g, [Case(g, k) for k in range(int(g["cases"]))], [Config(g, c) for c in range(int(g["configs"]))]
