"""What the host-side model classes (ncl, gcl, ssl4rec, directau, mhcn, sept, buir) share: the device default, the seeded
initialisation, the prepared data object of `from_graph(s)`, the batch conversion, the step body and — for the six models
that evaluate through evaluate.test / ranking_evaluation — the evaluation side (`RankingModel`).  Nothing here launches a
kernel of its own.

A new model class supplies: its config keys (`parse_config` or inline reads, `_read_topn`), its data / graphs (an
`Interaction` or a `prepared_data` object), `losses(*args)` returning a tuple whose LAST element is the total,
`_final()` returning the contiguous (query table, item table), and `train()`.
"""
from __future__ import annotations

import contextlib
import types

import torch

from .evaluate import ranking_evaluation, test as rank_test

MASK64 = 2 ** 64 - 1


def default_device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


@contextlib.contextmanager
def seeded(seed, device):
    """Initial weights drawn inside are a function of `seed`; the caller's RNG (host and `device`) stays untouched."""
    device = torch.device(device)
    with torch.random.fork_rng(devices=[device] if device.type == "cuda" else []):
        torch.manual_seed(seed)
        yield


def prepared_data(user_num, item_num, device, **fields):
    """What a training step reads from `Interaction` — sizes, device, the operators in `fields` — without the Python id
    maps (graphs too large for them): the four maps are empty."""
    return types.SimpleNamespace(user_num=int(user_num), item_num=int(item_num), device=device, **fields,
                                 test_set={}, training_set_u={}, user={}, item={})


def is_prepared(train_set, marker):
    """`train_set` is a prepared data object (any object carrying `marker`), not the list of triples."""
    return hasattr(train_set, marker)


def index_batch(batch, device):
    return tuple(torch.as_tensor(t, device=device, dtype=torch.int64).contiguous() for t in batch)


def metric_lines_to_dict(lines):
    """`ranking_evaluation`'s "Top n" / "name:value" lines -> {name: float}; lines without ':' are skipped and every
    cut-off's metrics land in one dict, so the last cut-off's four remain (as the reference returns)."""
    return {k: float(v) for m in lines if ":" in m for k, v in [m.strip().split(":", 1)]}


def optimise(self, *args):
    """The step body: zero_grad, `self.losses(*args)`, backward of the total (last element), optimizer step.  zero_grad
    comes first: it frees the old gradients before the step's peak.  Returns the detached terms."""
    self.optimizer.zero_grad(set_to_none=True)
    out = self.losses(*args)
    out[-1].backward()
    self.optimizer.step()
    return tuple(t.detach() for t in out)


class RankingModel:
    """The evaluation side of the models that rank through evaluate.test / ranking_evaluation.  A model overrides
    `_final()` -> (query table, item table), both contiguous; it has `data`, `device`, `topN`, `max_N`, `bestPerformance`."""

    _optimise = optimise

    def _read_topn(self, conf, default=(10, 20, 30, 50)):
        self.topN = [int(n) for n in conf.get("item.ranking.topN", default)]
        self.max_N = max(self.topN)

    def _final(self):
        raise NotImplementedError

    def test(self):
        query, items = self._final()
        return rank_test(self.data, query, items, self.max_N)

    def fast_evaluation(self, epoch):
        """The four metrics at max_N; bestPerformance follows Recall (strictly greater replaces it)."""
        performance = metric_lines_to_dict(ranking_evaluation(self.data.test_set, self.test(), [self.max_N], device=self.device))
        if not self.bestPerformance or performance.get("Recall", 0) > self.bestPerformance[1].get("Recall", 0):
            self.bestPerformance = [epoch + 1, performance]
        return performance

    def evaluate(self):
        """Every cut-off's metrics flattened into one dict, so the last cut-off's four remain."""
        return metric_lines_to_dict(ranking_evaluation(self.data.test_set, self.test(), self.topN, device=self.device))

    # predict in its two forms: a GEMV in the other orientation need not be bit-identical
    def predict(self, u):
        """U[u] . V^T: the scores of every item for raw user id u."""
        U, V = self._final()
        return torch.matmul(U[self.data.get_user_id(u)], V.T).cpu().numpy()

    def predict_item_major(self, u):
        """V @ U[u], as mhcn.py:546-548 and sept_social.py:479-481 write it."""
        U, V = self._final()
        return torch.matmul(V, U[self.data.get_user_id(u)]).cpu().numpy()
