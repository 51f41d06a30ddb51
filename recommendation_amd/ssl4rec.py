"""SSL4RecModel with the reference's interface (ssl4rec.py:162-266), every per-step stage but the tower GEMMs on the HIP path:

    SSL4RecModel(conf, train_set, test_set).train()  ->  {'Hit Ratio': .., 'Precision': .., 'Recall': .., 'NDCG': ..}

Stage by stage (reference line -> here):
    Interaction (first-seen ids)         ssl4rec.py:59-91     encoders.Interaction(id_order="first_seen") (gcr_dense_ids_u64)
    DNNEncoder                           ssl4rec.py:162-190   DNNEncoder (Linear / ReLU / Tanh stay torch GEMMs)
    initial_user[u]                      ssl4rec.py:190       functional.gather_rows (gcr_gather_rows_f32)
    initial_item[i] + 2 x nn.Dropout     ssl4rec.py:190-195   functional.gather_dropout_views (gcr_gather_dropout_f32): the
                                                              clean rows and both views stacked, ONE item-tower pass
    InfoNCE, batch_softmax_loss          ssl4rec.py:19-30     losses.InfoNCE / batch_softmax_loss (gcr_infonce_*, d = 128)
    l2_reg_loss                          ssl4rec.py:16-17     losses.l2_reg_loss
    torch.optim.Adam(lr)                 ssl4rec.py:212       optim.FusedAdam (gcr_adam_step_f32)
    next_batch_pairwise                  ssl4rec.py:33-50     sampler.next_batch_pairwise(max_trials=0): the loop drops the
                                                              negatives (ssl4rec.py:218), so none is rejection-sampled
    test / evaluate / predict            ssl4rec.py:143-153, 248-252   model_base.RankingModel over `_final` (evaluate.test /
                                                              ranking_evaluation: gcr_rank_*).  `self.topN` is passed as it
                                                              is: ssl4rec.py:250 wraps the list in a list, which fails inside
                                                              ranking_evaluation (univariate/ssl4rec_univariate.py has the
                                                              fix); the result is the metrics of the last cut-off
The tuner, the progress prints and the summary around it are out of scope.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import functional as Fn
from . import losses as Ls
from .encoders import Interaction
from .model_base import MASK64, RankingModel, default_device, index_batch, is_prepared, seeded
from .optim import FusedAdam
from .sampler import next_batch_pairwise

HIDDEN_DIM, OUT_DIM = 1024, 128             # ssl4rec.py:178-180
_TOWER_ROWS = 1 << 18                       # rows per tower call of the epoch-end pass (bounds the 1024-wide activations)


class DNNEncoder(nn.Module):
    """ssl4rec.py:162-196: two embedding tables and two MLP towers (hidden width 1024, output 128, ReLU between the
    layers and Tanh after the last).  Parameter names are the reference's (`initial_user`, `initial_item`,
    `user_net.{0,2,..}.{weight,bias}`, `item_net. ...`), so its `state_dict` loads directly."""

    def __init__(self, data, emb_size, drop_rate, tau, n_layers, device=None):
        super().__init__()
        self.emb_size, self.tau, self.drop_rate, self.n_layers = int(emb_size), tau, float(drop_rate), int(n_layers)
        init = nn.init.xavier_uniform_
        self.initial_user = nn.Parameter(init(torch.empty(data.user_num, self.emb_size, device=device)))
        self.initial_item = nn.Parameter(init(torch.empty(data.item_num, self.emb_size, device=device)))
        self.user_net = self.build_mlp(self.emb_size, device)
        self.item_net = self.build_mlp(self.emb_size, device)

    def build_mlp(self, input_dim, device=None):
        layers = []
        for i in range(self.n_layers):
            last = i == self.n_layers - 1
            out_dim = OUT_DIM if last else HIDDEN_DIM
            layers += [nn.Linear(input_dim, out_dim, device=device), nn.Tanh() if last else nn.ReLU()]
            input_dim = out_dim
        return nn.Sequential(*layers)

    def forward(self, u, i):
        return self.user_net(Fn.gather_rows(self.initial_user, u)), self.item_net(Fn.gather_rows(self.initial_item, i))

    def item_views(self, i, seed, keep_bits=None):
        """The item tower over the batch's rows and their two dropout views in one pass (ssl4rec.py:190 and 192-196):
        returns (i_emb, view1, view2), each [B, 128]."""
        z = self.item_net(Fn.gather_dropout_views(self.initial_item, i, self.drop_rate, seed, 2, keep_bits))
        b = z.shape[0] // 3
        return z[:b], z[b:2 * b], z[2 * b:]

    def all_rows(self):
        """`model(arange(user_num), arange(item_num))` (ssl4rec.py:232-235): both towers over every row, no gather."""
        def tower(net, table):
            return torch.cat([net(table[r:r + _TOWER_ROWS]) for r in range(0, table.shape[0], _TOWER_ROWS)])
        with torch.no_grad():
            return tower(self.user_net, self.initial_user), tower(self.item_net, self.initial_item)


class SSL4RecModel(RankingModel):
    def __init__(self, conf, train_set, test_set, device=None, seed=0):
        """conf: the reference's keys — `embedding.size`, `batch.size`, `learning.rate`, `max.epoch` (default 1),
        `item.ranking.topN` (default [10]), conf['SSL4Rec']['alpha' | 'tau' | 'drop'], top-level `n.layers` (default 1) and
        `reg.weight` (default 1e-4); `reg.lambda` is read and, as in the reference, unused.  seed: initial weights, batch
        order and dropout draws are functions of it (the reference never seeds its generators)."""
        self.config, self.seed = conf, int(seed)
        self.emb_size, self.batch_size, self.lRate = conf["embedding.size"], conf["batch.size"], conf["learning.rate"]
        self.reg = conf.get("reg.lambda")
        self.maxEpoch = conf.get("max.epoch", 1)
        self._read_topn(conf, [10])
        args = conf["SSL4Rec"]
        self.cl_rate, self.tau, self.drop = float(args["alpha"]), float(args["tau"]), float(args["drop"])
        self.n_layers = conf.get("n.layers", 1)
        self.reg_weight = conf.get("reg.weight", 0.0001)
        self.device = default_device(device)
        # `train_set` may be a prepared data object (user_num, item_num, device, ...) instead of the triple list, as for
        # NCLModel: tables too large for Python id maps (scripts/perf_ssl4rec_step.py)
        self.data = train_set if is_prepared(train_set, "user_num") else \
            Interaction(conf, train_set, test_set, device=self.device, id_order="first_seen")
        with seeded(self.seed, self.device):
            self.model = DNNEncoder(self.data, self.emb_size, self.drop, self.tau, self.n_layers, device=self.device)
        self.optimizer = FusedAdam(self.model.parameters(), lr=self.lRate)        # ssl4rec.py:212: no weight decay
        self.steps = 0
        self.best_performance = {}

    def losses(self, u, i, keep_bits=None):
        """ssl4rec.py:221-224 on the HIP path: (rec_loss, cl_loss, batch_loss), differentiable, no host sync.  Every call
        draws the step's two dropout masks from a seed of its own; keep_bits (int32 [2, ceil(B * emb / 32)]) replays
        recorded ones."""
        u, i = index_batch((u, i), self.device)
        self.steps += 1
        step_seed = (self.seed * 0x9E3779B97F4A7C15 + 2 * self.steps) & MASK64      # view v draws with step_seed + v
        u_emb = self.model.user_net(Fn.gather_rows(self.model.initial_user, u))
        i_emb, v1, v2 = self.model.item_views(i, step_seed, keep_bits)
        rec_loss = Ls.batch_softmax_loss(u_emb, i_emb, self.tau)
        cl_loss = self.cl_rate * Ls.InfoNCE(v1, v2, self.tau)
        batch_loss = rec_loss + cl_loss + Ls.l2_reg_loss(self.reg_weight, u_emb, i_emb)
        return rec_loss, cl_loss, batch_loss

    def train_step(self, u, i, keep_bits=None):
        """One body of ssl4rec.py:218-225 (zero_grad, losses, backward, Adam step).  Returns (rec_loss, cl_loss,
        batch_loss) as detached device tensors."""
        return self._optimise(u, i, keep_bits)

    def embeddings(self):
        """(query_emb [U, 128], item_emb [I, 128]): the towers over all rows under no_grad (ssl4rec.py:231-235)."""
        return self.model.all_rows()

    def train(self):
        """ssl4rec.py:211-246: per epoch the shuffled batches, the towers over all rows, evaluate(), early stopping with
        patience 3 on Recall.  Returns the best epoch's metric dict."""
        best_epoch, best_metric, patience, no_improv = 0, {}, 3, 0
        for epoch in range(self.maxEpoch):
            self.model.train()
            for u, i, _ in next_batch_pairwise(self.data, self.batch_size, seed=self.seed, epoch=epoch, max_trials=0):
                self.train_step(u, i)
            self.model.eval()
            self.query_emb, self.item_emb = self.embeddings()
            current = self.evaluate()
            if not best_metric or self.is_better(current, best_metric):
                best_metric, best_epoch = current, epoch
                self.save()
                no_improv = 0
            else:
                no_improv += 1
            if no_improv >= patience:
                break
        self.best_epoch, self.best_performance = best_epoch, best_metric
        return best_metric

    def _final(self):
        return self.query_emb.contiguous(), self.item_emb.contiguous()

    def is_better(self, current, best):
        return current.get("Recall", 0) > best.get("Recall", 0)

    def save(self):
        """ssl4rec.py:257-262 runs the towers again on unchanged parameters; the epoch's own outputs are those values."""
        self.best_query_emb, self.best_item_emb = self.query_emb, self.item_emb
