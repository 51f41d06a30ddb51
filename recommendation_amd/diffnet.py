"""Host-side mirror of univariate/diffnet.py's DiffNet (social diffusion over the follower graph) on the HIP ops.

  DiffNet.forward            diffnet.py:1124-1132  per layer sparse.mm(S, X), cat, matmul with W [2d, d], relu over ALL users on
                                                   every batch: one fused launch per layer forward and one backward
                                                   (functional.diffuse_layer: gcr_diffuse_fwd_f32 / gcr_diffuse_bwd_f32);
                                                   final = H_K + A item_embeddings as one SpMM launch with a fused addend
  buildSparseRelationMatrix  diffnet.py:1070-1077  after the cleaning of SocialRecommender.__init__ (:873-908): `social_coo`
  create_sparse_rating_matrix diffnet.py:1030-1037 `rating_coo`
  the loop body              diffnet.py:1103-1119  DiffNetModel.train_step: functional.bpr_sums' five sums, optim.FusedAdam

Quirks kept (each pinned by tests/golden/diffnet_steps.npz, which the reference itself wrote):
  * dense ids follow first appearance in the training list (Rating.__generateSet, :57-65);
  * S has one entry per kept relation pair in list order (a repeated pair twice: the entries sum), valued
    1 / (number of DISTINCT kept followees of the follower); A has one entry per training triple, valued 1 / (number of
    distinct items of the user).  Neither is a row normalisation: a row with a repeated entry sums to more than 1;
  * trainModel re-draws both tables as randn * 0.005 (initModel, :935-938), then draws the layers' xavier-uniform weights
    (:1087-1090): that order, under `seeded`;
  * the loss and `predict` use the RAW item table; only the user side is propagated;
  * loss = -sum log sigmoid(y) (a sum, no eps; here the softplus form, finite for any y) + regU * (|u| + |v| + |n|), the
    Frobenius norms of the gathered blocks, not squared;
  * regU is conf['reg_lambda'] only when the KEY 'regU' is in conf, 1e-4 otherwise (:1064);
  * one Adam over tables and weights; `range(1)` epochs whatever the conf says (:1101); the ranking after training
    re-encodes with the updated parameters (predictForRanking calls forward, :1139).
The tuner (diffnet.py:1152-), the prints and the rating-prediction side are out of scope.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import functional as Fn
from .encoders import Interaction
from .graph import CsrGraph
from .mhcn import social_pairs
from .model_base import RankingModel, default_device, index_batch, is_prepared, prepared_data, seeded
from .optim import FusedAdam
from .sampler import MAX_TRIALS, next_batch_pairwise

DEFAULT_REG_U = 1e-4


def diffusion_values(row, col, n_cols):
    """Per COO entry 1 / (number of distinct columns in the entry's row), float32 of the double quotient: the values of
    diffnet.py:1035 and :1075, where `len(dict)` counts a repeated pair once."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    if row.size == 0:
        return np.zeros(0, dtype=np.float32)
    distinct = np.unique(row * int(n_cols) + col) // int(n_cols)
    count = np.bincount(distinct, minlength=int(row.max()) + 1)
    return (1.0 / count[row]).astype(np.float32)


def social_coo(social_data, user):
    """(follower ids, followee ids, values) of S in the reference's entry order (diffnet.py:1070-1077 after :873-908): the
    pairs whose two users both occur in the training set, a repeated pair repeated."""
    row, col = social_pairs(social_data, user)
    row, col = row.numpy(), col.numpy()
    return row, col, diffusion_values(row, col, max(len(user), 1))


def rating_coo(uid, iid, n_items):
    """(user ids, item ids, values) of A, one entry per training triple (diffnet.py:1030-1037)."""
    uid, iid = np.asarray(uid, dtype=np.int64), np.asarray(iid, dtype=np.int64)
    return uid, iid, diffusion_values(uid, iid, max(int(n_items), 1))


def reg_u(conf):
    """diffnet.py:1064: conf['reg_lambda'] when the key 'regU' is present (its own value is never read), else 1e-4."""
    return float(conf["reg_lambda"]) if "regU" in conf else DEFAULT_REG_U


def diffnet_loss(final_user, item_embeddings, u, i, j, reg):
    """(rec_loss, reg_loss, total) of diffnet.py:1106-1115 from `functional.bpr_sums`' sums: the loss sum and the three
    squared Frobenius norms of the gathered blocks come out of one fused forward."""
    s = Fn.bpr_sums(final_user, item_embeddings, u, i, j, Fn.BPR_LOGSIGMOID)
    rec = s[0]
    # |x|_F = sqrt(Q); the clamp gives an all-zero block the zero gradient torch.norm has there
    reg_loss = reg * torch.sqrt(s[1:4].clamp_min(1e-30)).sum()
    return rec, reg_loss, rec + reg_loss


class DiffNetEncoder(nn.Module):
    """Parameters and forward of DiffNet (:935-938, :1087-1090, :1124-1132) with the reference's attribute names.
    s: CsrGraph [U, U] (S), a: CsrGraph [U, I] (A).  gather: `functional.diffuse_layer`'s switch; fused=False runs the
    layers as the reference composes them (`functional.diffuse_layer_composed`)."""

    def __init__(self, s: CsrGraph, a: CsrGraph, emb_size=64, n_layers=2, gather=None, fused=True):
        super().__init__()
        self.S, self.A = s, a
        self.user_num, self.item_num = a.n_rows, a.n_cols
        self.emb_size, self.n_layers, self.gather, self.fused = emb_size, n_layers, gather, fused
        dev = a.device
        self.user_embeddings = nn.Parameter(torch.randn(self.user_num, emb_size, device=dev) * 0.005)
        self.item_embeddings = nn.Parameter(torch.randn(self.item_num, emb_size, device=dev) * 0.005)
        self.weights = nn.ParameterList([nn.Parameter(nn.init.xavier_uniform_(torch.empty(2 * emb_size, emb_size, device=dev)))
                                         for _ in range(n_layers)])

    def diffuse(self):
        """H_K: the user table after the n_layers diffusion layers."""
        h = self.user_embeddings
        for w in self.weights:
            h = Fn.diffuse_layer(self.S, h, w, self.gather) if self.fused else Fn.diffuse_layer_composed(self.S, h, w)
        return h

    def forward(self):
        """final_user_embeddings [U, d] = H_K + A item_embeddings (:1131)."""
        return Fn.spmm_add(self.A, self.item_embeddings, self.diffuse())


class DiffNetModel(RankingModel):
    def __init__(self, conf, train_set, test_set, social_data=None, device=None, seed=0, gather=None, fused=True):
        """conf: the reference's keys (diffnet.py:1054-1065) — `n_layer`, `emb_size` (64), `batch_size`, `lr`, `reg_lambda`
        (read only when the key `regU` is present), `item.ranking.topN` ([10, 20, 30, 50]).  social_data: [follower,
        followee, weight] triples.  seed: initial weights, batch order and negatives are functions of it."""
        self.config, self.seed = conf, int(seed)
        self.n_layers = int(conf["n_layer"])
        self.emb_size = int(conf["emb_size"]) if "emb_size" in conf else 64
        self.batch_size = conf.get("batch_size", 2048)
        self.lRate = conf.get("lr", 0.001)
        self.regU = reg_u(conf)
        self.maxEpoch = 1                                       # :1101 `for epoch in range(1)`
        self._read_topn(conf)
        self.device = default_device(device)
        if is_prepared(train_set, "graphs"):                    # prepared operators (`from_graphs`)
            self.data = train_set
            s, a = train_set.graphs
        else:
            self.data = Interaction(conf, train_set, test_set, device=self.device, id_order="first_seen")
            n_u, n_i = self.data.user_num, self.data.item_num
            self.social_coo = social_coo(social_data or [], self.data.user)
            self.rating_coo = rating_coo(self.data.uid, self.data.iid, n_i)
            s = CsrGraph.from_coo(*self.social_coo, n_u, n_u, self.device)
            a = CsrGraph.from_coo(*self.rating_coo, n_u, n_i, self.device)
        with seeded(self.seed, self.device):
            self.model = DiffNetEncoder(s, a, emb_size=self.emb_size, n_layers=self.n_layers, gather=gather, fused=fused)
        self.optimizer = FusedAdam(list(self.model.parameters()), lr=self.lRate)
        self.bestPerformance = []

    @classmethod
    def from_graphs(cls, conf, s, a, **kw):
        """DiffNetModel over operators that already live on the device (S [U, U], A [U, I] with the reference's values):
        what the training step reads from the data object without the Python id maps (scripts/perf_diffnet_step.py)."""
        data = prepared_data(a.n_rows, a.n_cols, a.device, graphs=(s, a))
        return cls(conf, data, None, None, device=a.device, **kw)

    def losses(self, u, i, j):
        """diffnet.py:1105-1115 on the HIP path: (rec_loss, reg_loss, total_loss), differentiable, no host sync."""
        final_user = self.model()
        return diffnet_loss(final_user, self.model.item_embeddings, u, i, j, self.regU)

    def train_step(self, batch):
        """One body of diffnet.py:1103-1119 for batch = (user_idx, pos_idx, neg_idx): losses, zero_grad, backward, Adam
        step.  Returns the detached (rec_loss, reg_loss, total_loss)."""
        self.__dict__.pop("U", None)                            # the tables `_final` cached are stale from here on
        return self._optimise(*index_batch(batch, self.device))

    def train_epoch(self, epoch):
        self.model.train()
        for batch in next_batch_pairwise(self.data, self.batch_size, seed=self.seed, epoch=epoch, max_trials=MAX_TRIALS):
            self.train_step(batch)

    def train(self):
        """trainModel (:1092-1122): one epoch, then the ranking metrics of the updated parameters' forward."""
        for epoch in range(self.maxEpoch):
            self.train_epoch(epoch)
        return self.evaluate()

    def _final(self):
        if not hasattr(self, "U"):                              # :1138-1141: the current parameters' forward, raw items
            with torch.no_grad():
                fu = self.model()
            self.U, self.V = fu.contiguous(), self.model.item_embeddings.detach().contiguous()
        return self.U, self.V
