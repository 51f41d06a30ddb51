"""Host-side mirror of univariate/buir.py's BUIR (bootstrapped user / item representations, the LightGCN variant
BUIR_NB) on the HIP ops.

    BUIRModel(conf, train_set, test_set).train()  ->  {'Hit Ratio': .., 'Precision': .., 'Recall': .., 'NDCG': ..}

    Interaction (sorted ids, raw `norm_adj`, Q1)              buir.py:84-126     encoders.Interaction
    LGCN_Encoder.sparse_dropout (Bernoulli keep, 1 / (1 - rate))   :300-309      functional.edge_mask_bits + `val_scale`
    LGCN_Encoder.forward: K layers on the dropped operator, mean   :311-322      functional.lightgcn_propagate(keep_bits=..)
    the batch gathers, the predictor, get_loss                :260-262, 269-277, 323-325   functional.buir_loss (gcr_buir_*)
    update_target                                             :251-257           functional.ema_rows_ (gcr_ema_rows_f32)
    the loop body: forward, loss, zero_grad, backward, Adam, update_target   :194-203   BUIRModel.train_step
    get_embedding (no dropout, online encoder)                :264-267, 328-340  BUIRModel.get_embedding
    train, save, predict                                      :149-166, 189-225  the methods of the same names
    test, fast_evaluation, evaluate                           :167-173, 227-232  model_base.RankingModel over `_final`

The reference's quirks, kept:
  * `tau` IS the momentum of the target update (:181); `lambda`, `factors` and `max.epoch` are never read, and training is
    ONE epoch (`range(1)`, :192);
  * `norm_adj` is the raw 0/1 adjacency with duplicate interactions kept (Q1), never normalised;
  * each encoder draws its own rate = uniform(0, 1) * drop_rate and its own mask per step (:312-313), every stored
    (directed) non-zero independently: the mask is not symmetric although the operator is;
  * update_target touches only the batch's rows, each once however often it recurs, and reads the online tables AFTER
    the Adam step (:202-203);
  * the negatives its sampler draws are never read (:194-195): none are drawn here.
Here the draws are functions of (seed, step, encoder) — the reference never seeds its generators.
The tuner (:343-), the prints and a sharded model are out of scope.
"""
from __future__ import annotations

import types

import numpy as np
import torch

from . import functional as Fn
from .encoders import Interaction
from .model_base import MASK64, RankingModel, default_device, index_batch, is_prepared, prepared_data, seeded
from .optim import FusedAdam
from .sampler import next_batch_pairwise

STATE_NAMES = {"online_encoder.embedding_dict.user_emb": "online_user", "online_encoder.embedding_dict.item_emb": "online_item",
               "target_encoder.embedding_dict.user_emb": "target_user", "target_encoder.embedding_dict.item_emb": "target_item",
               "predictor.weight": "weight", "predictor.bias": "bias"}


def parse_config(conf):
    """The reference's keys (buir.py:180-186) with its defaults; `tau` is the momentum."""
    args = conf["BUIR"]
    return types.SimpleNamespace(
        momentum=float(args["tau"]), n_layers=int(args["n_layer"]), drop_rate=float(args["drop_rate"]),
        emb_size=conf.get("emb_size", 64), lRate=conf.get("lr", 0.001), batch_size=conf.get("batch_size", 2048),
        topN=[int(n) for n in conf.get("item.ranking.topN", [10, 20, 30, 50])])


class BUIRModel(RankingModel):
    def __init__(self, conf, train_set, test_set, device=None, seed=0):
        """conf: conf['BUIR']['n_layer' | 'tau' | 'drop_rate'], `emb_size` (64), `lr` (1e-3), `batch_size` (2048),
        `item.ranking.topN` ([10, 20, 30, 50]).  seed: initial tables, predictor, batch order and the dropout draws are
        functions of it."""
        self.config, self.seed = conf, int(seed)
        for k, v in vars(parse_config(conf)).items():
            setattr(self, k, v)
        self.max_N = max(self.topN)
        self.device = default_device(device)
        self.data = train_set if is_prepared(train_set, "norm_adj") else Interaction(conf, train_set, test_set, device=self.device)
        n_u, n_i, d = self.data.user_num, self.data.item_num, self.emb_size
        self.norm_adj = self.data.norm_adj              # the raw adjacency, duplicates kept (Q1)
        with seeded(self.seed, self.device):
            xav = torch.nn.init.xavier_uniform_
            self.online_user = torch.nn.Parameter(xav(torch.empty(n_u, d, device=self.device)))
            self.online_item = torch.nn.Parameter(xav(torch.empty(n_i, d, device=self.device)))
            lin = torch.nn.Linear(d, d).to(self.device)             # torch's default init (:243)
        self.weight, self.bias = torch.nn.Parameter(lin.weight.detach().clone()), torch.nn.Parameter(lin.bias.detach().clone())
        # _init_target (:246-249): a copy of the online init, never in the optimiser
        self.target_user, self.target_item = self.online_user.detach().clone(), self.online_item.detach().clone()
        self.optimizer = FusedAdam(self.parameters(), lr=self.lRate)
        self.loss_fn = Fn.buir_loss                     # the fused kernels where they serve d, the composition elsewhere
        self.ema_fn = Fn.ema_rows_
        self.step_count = 0
        self.bestPerformance = []

    @classmethod
    def from_graphs(cls, conf, norm_adj, n_users, uid_dev, iid_dev, user_rowptr, user_items_sorted, **kw):
        """BUIRModel over an operator that already lives on the device: the raw bipartite adjacency [U + I, U + I], the
        training pairs' dense ids and the CSR of the distinct pairs (int64 [U + 1], int32 [nnz]) — what the training step
        reads from the data object without the Python id maps (scripts/perf_buir_step.py)."""
        data = prepared_data(n_users, norm_adj.n_rows - int(n_users), norm_adj.device, norm_adj=norm_adj, uid_dev=uid_dev,
                             iid_dev=iid_dev, user_rowptr=user_rowptr, user_items_sorted=user_items_sorted)
        return cls(conf, data, None, device=norm_adj.device, **kw)

    def parameters(self):
        return [self.online_user, self.online_item, self.weight, self.bias]

    def load_reference_state(self, state):
        """Sets the four tables and the predictor from arrays keyed by the reference's `BUIR_NB.state_dict()` names."""
        with torch.no_grad():
            for name, attr in STATE_NAMES.items():
                src = torch.as_tensor(np.asarray(state[name]), dtype=torch.float32).to(self.device)
                dst = getattr(self, attr)
                if src.shape != dst.shape:
                    raise ValueError(f"{name}: shape {tuple(src.shape)}, expected {tuple(dst.shape)}")
                dst.copy_(src)

    def reference_state(self):
        return {name: getattr(self, attr).detach().cpu().numpy().copy() for name, attr in STATE_NAMES.items()}

    # -- the dropout draws (buir.py:300-313) --------------------------------------------------------
    def draw_views(self, step):
        """((rate_o, keep_bits_o, keep_bits_t_o), (rate_t, keep_bits_t)): per encoder rate = uniform(0, 1) * drop_rate
        (host) and a keep bitmap over the operator's non-zeros (keep = u >= rate), functions of (seed, step, encoder); the
        online encoder's also in A^T's order (`mirror_perm`) for the backward."""
        nnz, out = self.norm_adj.nnz, []
        for enc in (0, 1):
            rate = float(np.random.default_rng([self.seed, int(step), enc]).random()) * self.drop_rate
            mseed = ((self.seed * 1_000_003 + int(step)) * 2 + enc) & MASK64
            bits = Fn.edge_mask_bits(nnz, rate, mseed, self.device)
            if enc == 0:
                out.append((rate, bits, Fn.edge_mask_bits(nnz, rate, mseed, self.device, edge_id=self.norm_adj.mirror_perm())))
            else:
                out.append((rate, bits))
        return tuple(out)

    # -- the loop body (buir.py:194-203) --------------------------------------------------------------
    def encode(self, user_emb, item_emb, rate=0.0, keep_bits=None, keep_bits_t=None):
        ego = torch.cat([user_emb, item_emb], 0)
        scale = 1.0 / (1.0 - rate) if keep_bits is not None else 1.0
        out = Fn.lightgcn_propagate(self.norm_adj, ego, self.n_layers, "mean", keep_bits=keep_bits, keep_bits_t=keep_bits_t,
                                    val_scale=scale)
        return Fn.split_rows(out, self.data.user_num)

    def loss(self, u, i, views):
        (rate_o, bits_o, bits_ot), (rate_t, bits_t) = views
        on_user, on_item = self.encode(self.online_user, self.online_item, rate_o, bits_o, bits_ot)
        with torch.no_grad():
            tg_user, tg_item = self.encode(self.target_user, self.target_item, rate_t, bits_t)
        return self.loss_fn(on_user, on_item, tg_user, tg_item, u, i, self.weight, self.bias)

    def update_target(self, u, i):
        self.ema_fn(self.target_user, self.online_user.detach(), u, self.momentum)
        self.ema_fn(self.target_item, self.online_item.detach(), i, self.momentum)

    def train_step(self, batch, views=None):
        """One body of :194-203 for batch = (user_idx, item_idx[, unused negatives]): the two masked propagations, the
        loss, zero_grad, backward, Adam, then the target update on the batch's rows.  views: recorded draws to replay
        (`draw_views`' layout).  Returns the detached loss."""
        u, i = index_batch(batch[:2], self.device)
        if views is None:
            views = self.draw_views(self.step_count)
        self.step_count += 1
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.loss(u, i, views)
        loss.backward()
        self.optimizer.step()
        self.update_target(u, i)
        return loss.detach()

    def train(self):
        """:189-215: one epoch, then the evaluation tables of the online encoder without dropout."""
        for epoch in range(1):
            for batch in next_batch_pairwise(self.data, self.batch_size, seed=self.seed, epoch=epoch, max_trials=0):
                self.train_step(batch)
            self.p_u_online, self.u_online, self.p_i_online, self.i_online = self.get_embedding()
            self.fast_evaluation(epoch)
            self.save()
        self.p_u_online, self.u_online, self.p_i_online, self.i_online = self.best_p_u, self.best_u, self.best_p_i, self.best_i
        return self.evaluate()

    @torch.no_grad()
    def get_embedding(self):
        """:264-267, 328-340: (predictor(u_online), u_online, predictor(i_online), i_online), no dropout."""
        u_on, i_on = self.encode(self.online_user, self.online_item)
        lin = torch.nn.functional.linear
        return lin(u_on, self.weight, self.bias), u_on.contiguous(), lin(i_on, self.weight, self.bias), i_on.contiguous()

    def save(self):
        self.best_p_u, self.best_u, self.best_p_i, self.best_i = self.get_embedding()

    def _tables(self):
        if not hasattr(self, "p_u_online"):                 # never trained: the current parameters
            self.p_u_online, self.u_online, self.p_i_online, self.i_online = self.get_embedding()
        return self.p_u_online, self.u_online, self.p_i_online, self.i_online

    def predict(self, u):
        """:220-225: p_u[u] . i_online^T + u_online[u] . p_i^T for raw user id u."""
        p_u, u_on, p_i, i_on = self._tables()
        u = self.data.get_user_id(u)
        return (torch.matmul(p_u[u], i_on.T) + torch.matmul(u_on[u], p_i.T)).cpu().numpy()

    def _final(self):
        """The same score as one product of the concatenated 2 d-wide tables [p_u | u_on] . [i_on | p_i]^T."""
        p_u, u_on, p_i, i_on = self._tables()
        return torch.cat([p_u, u_on], 1).contiguous(), torch.cat([i_on, p_i], 1).contiguous()
