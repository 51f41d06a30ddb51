"""Shared by tests/test_lightgcn_steps_cpu.py and tests/test_lightgcn_steps_gpu.py: tests/golden/lightgcn_steps.npz
(scripts/gen_golden_lightgcn_steps.py), six full-batch steps of lightgcn.py:84-120 run by the reference in float64 at four
configurations of its own grid (A: the default; B: d = 32, three negatives, weight decay; C: BCE at d = 128; D: plain SGD)."""
import os

import numpy as np

import step_pins as sp
from step_pins import LIGHTGCN_TABLES as TABLES  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lightgcn_steps.npz")
SIZE_CAP = 1_000_000
CONFIGS = ("A", "B", "C", "D")
HYPER = ("embedding_dim", "num_layers", "loss_type", "n_neg", "optimizer", "lr", "reg_weight", "weight_decay")
_cache = {}


def fixture():
    if "z" not in _cache:
        _cache["z"] = np.load(GOLDEN, allow_pickle=False)
    return _cache["z"]


def config(g, c):
    out = {k: g[f"{c}/{k}"].item() for k in HYPER}
    assert isinstance(out["loss_type"], str) and isinstance(out["optimizer"], str)
    return out


def init_table(g, c, k):
    return g[f"init_d{int(g[f'{c}/embedding_dim'])}/{k}"]


def final_table(g, c, k):
    """The float64 run's final table: stored as float32(final - init), exact to 4e-9 (asserted by the generator)."""
    return sp.record("lightgcn", g, c).tables[k]


def sensitivity_terms(g, c):
    return ("reg", "wd") if float(g[f"{c}/weight_decay"]) else ("reg",)


def user_major_perm(g):
    """File order -> the order of the operator's user rows: a stable sort by (user, item).  The operator keeps the file
    order inside a row (gcr_coo_to_csr sorts by row alone); the fixture's file is item-major, so that is ascending items
    (tests/test_lightgcn_steps_cpu.py checks it, the GPU test checks the result against the graph).  Copies of a pair stay
    in file order; they are interchangeable, the loss being a sum over the multiset of (user, item, negatives) triples."""
    return np.lexsort((g["train_item"], g["train_user"]))


def adam_on_weight_decay_only(p0, lr, weight_decay, steps, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's recursion in float64 on rows whose only gradient is weight_decay * p (an isolated node)."""
    p = np.asarray(p0, dtype=np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, steps + 1):
        grad = weight_decay * p
        m = betas[0] * m + (1 - betas[0]) * grad
        v = betas[1] * v + (1 - betas[1]) * grad * grad
        p = p - lr / (1 - betas[0] ** t) * m / (np.sqrt(v) / np.sqrt(1 - betas[1] ** t) + eps)
    return p
