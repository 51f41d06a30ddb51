"""Host-side mirror of univariate/sept_social.py's SEPT (socially-aware tri-training) on the HIP ops.

    SEPTModel(conf, train_set, test_set, social_data).train()  ->  {'Hit Ratio': .., 'Precision': .., 'Recall': .., 'NDCG': ..}

    Interaction (sorted ids, raw `norm_adj`, Q1)      sept_social.py:236-286   encoders.Interaction
    Relation.__initialize (pair filter)               sept_social.py:119-130   mhcn.social_pairs
    get_birectional_social_mat, get_social_related_views  :141-144, 361-368    graph_ops.social_related_views
    encoder / social_encoder (sum of normalised layers)   :370-385             encoders.sept_encoder(combine="sum")
    label_prediction, generate_pesudo_labels, neighbor_discrimination  :394-420  functional.tri_training_loss (gcr_tri_*)
    the loop body: four encoders, bpr_loss + reg, the tri-training terms, Adam   :432-465   SEPTModel.losses / train_step
    GraphAugmentor.edge_dropout                       sept_social.py:72-78     SEPTModel.augmented_graph (gcr_edge_mask_exact_bits)
    next_batch_pairwise                               sept_social.py:15-33     sampler.next_batch_pairwise (gcr_neg_sample)
    train, save                                       sept_social.py:422-473   SEPTModel.train / save
    fast_evaluation, predict, evaluate                :323-329, 479-488        model_base.RankingModel over `_final`

sept_social.py:427 calls `self.data.convert_to_laplacian_mat`, which `Interaction` does not have: the reference
cannot run an epoch of its tri-training branch.  The choice made here: the augmented operator is the
UN-normalised bipartite adjacency [[0, D], [D^T, 0]] of the dropped interaction matrix D — the same form as the `norm_adj`
(raw, Q1) that the early epochs pass as `aug_mat` (:429) — built once per epoch.
The tuner (:492-), the prints, univariate/sept.py's stale-graph loop and a sharded model are out of scope.
"""
from __future__ import annotations

import types

import torch

from . import functional as Fn
from . import losses as Ls
from .encoders import Interaction, sept_encoder
from .graph import CsrGraph
from .graph_ops import social_related_views
from .mhcn import MAX_TRIALS, social_pairs
from .model_base import RankingModel, default_device, index_batch, is_prepared, prepared_data, seeded
from .optim import FusedAdam
from .sampler import next_batch_pairwise


def parse_config(conf):
    """The reference's keys (sept_social.py:336-345) with its defaults."""
    args = conf["SEPT"]
    return types.SimpleNamespace(
        n_layers=int(args["n_layer"]), ss_rate=float(args["ss_rate"]), drop_rate=float(args["drop_rate"]),
        instance_cnt=int(args["ins_cnt"]), emb_size=conf.get("emb_size", 64), batch_size=conf.get("batch_size", 2048),
        lRate=conf.get("lr", 0.001), reg=conf.get("reg_lambda", 0.0001), maxEpoch=int(conf["max.epoch"]),
        topN=[int(n) for n in conf.get("item.ranking.topN", [10, 20, 30, 50])])


def is_tri_training_epoch(epoch, max_epoch):
    """sept_social.py:425,446: the tri-training branch runs in the epochs after the first third."""
    return epoch > max_epoch // 3


class SEPTModel(RankingModel):
    def __init__(self, conf, train_set, test_set, social_data=None, device=None, seed=0):
        """conf: conf['SEPT']['n_layer' | 'ss_rate' | 'drop_rate' | 'ins_cnt'], `emb_size` (64), `batch_size` (2048), `lr`
        (1e-3), `reg_lambda` (1e-4), `max.epoch`, `item.ranking.topN` ([10, 20, 30, 50]).  social_data: [follower, followee,
        weight] triples.  seed: initial tables, batch order, negatives and the edge dropout are functions of it."""
        self.config, self.seed = conf, int(seed)
        for k, v in vars(parse_config(conf)).items():
            setattr(self, k, v)
        self.max_N = max(self.topN)
        self.device = default_device(device)
        if is_prepared(train_set, "graphs"):                   # prepared operators (`from_graphs`)
            self.data = train_set
            self.social_mat, self.sharing_mat = train_set.graphs
        else:
            self.data = Interaction(conf, train_set, test_set, device=self.device)
            s_row, s_col = social_pairs(social_data or [], self.data.user)
            self.social_pairs = (s_row, s_col)
            self.social_mat, self.sharing_mat = social_related_views(s_row, s_col, self.data.uid_dev, self.data.iid_dev,
                                                                     self.data.user_num, self.data.item_num, self.device)
        n_u, n_i = self.data.user_num, self.data.item_num
        self.norm_adj = self.data.norm_adj              # the raw adjacency, duplicates kept (Q1)
        # interaction_mat.nonzero(): the distinct (user, item) pairs in row-major order
        rp = self.data.user_rowptr
        self.pair_user = torch.repeat_interleave(torch.arange(n_u, device=self.device), rp[1:] - rp[:-1])
        self.pair_item = self.data.user_items_sorted.to(torch.int64)
        self.tri_loss = Fn.tri_training_loss            # the fused kernels where they serve (d, k), the composition elsewhere
        with seeded(self.seed, self.device):
            xav = torch.nn.init.xavier_uniform_
            self.user_embeddings = torch.nn.Parameter(xav(torch.empty(n_u, self.emb_size, device=self.device)))
            self.item_embeddings = torch.nn.Parameter(xav(torch.empty(n_i, self.emb_size, device=self.device)))
        self.optimizer = FusedAdam([self.user_embeddings, self.item_embeddings], lr=self.lRate)
        self.bestPerformance = []
        self.last_positives = None

    @classmethod
    def from_graphs(cls, conf, norm_adj, social_mat, sharing_mat, user_rowptr, user_items_sorted, **kw):
        """SEPTModel over operators that already live on the device: the raw bipartite adjacency [U + I, U + I], the two
        normalised social views [U, U] and the CSR of the distinct training pairs (int64 [U + 1], int32 [nnz]) — what the
        training step reads from the data object without the Python id maps (scripts/perf_sept_step.py)."""
        n_u = social_mat.n_rows
        data = prepared_data(n_u, norm_adj.n_rows - n_u, norm_adj.device, norm_adj=norm_adj, graphs=(social_mat, sharing_mat),
                             user_rowptr=user_rowptr, user_items_sorted=user_items_sorted)
        return cls(conf, data, None, None, device=norm_adj.device, **kw)

    def parameters(self):
        return [self.user_embeddings, self.item_embeddings]

    # -- the augmented operator (sept_social.py:426-427, Q10) --------------------------------------
    def graph_from_kept_pairs(self, u, i):
        """[[0, D], [D^T, 0]], un-normalised, for the kept (user, item) pairs of a dropped interaction matrix D."""
        return CsrGraph.bipartite_raw(torch.as_tensor(u, device=self.device, dtype=torch.int64),
                                      torch.as_tensor(i, device=self.device, dtype=torch.int64),
                                      self.data.user_num, self.data.item_num, self.device)

    def kept_pairs(self, epoch):
        """`GraphAugmentor.edge_dropout(interaction_mat, drop_rate)` (:72-78): exactly int(nnz (1 - drop_rate)) of the
        distinct pairs, a uniform subset without replacement, a function of (seed, epoch)."""
        nnz = self.pair_user.numel()
        n_keep = int(nnz * (1 - self.drop_rate))
        bits = Fn.edge_mask_exact_bits(nnz, n_keep, self.seed * 1_000_003 + int(epoch), self.device)
        e = torch.arange(nnz, device=self.device)
        keep = ((bits[e >> 5] >> (e & 31)) & 1).to(torch.bool)
        return self.pair_user[keep], self.pair_item[keep]

    def augmented_graph(self, epoch):
        return self.graph_from_kept_pairs(*self.kept_pairs(epoch))

    # -- the loop body (sept_social.py:432-465) ------------------------------------------------------
    def encode(self, adj):
        ego = torch.cat([self.user_embeddings, self.item_embeddings], 0)
        out = sept_encoder(ego, adj, self.n_layers, combine="sum")
        return Fn.split_rows(out, self.data.user_num)

    def losses(self, u, i, j, tri_training, aug_graph=None, positives=None):
        """(rec_loss, neighbor_dis_loss, total_loss), differentiable; the one host read-back is the size of
        `torch.unique(u)`.  rec_loss includes reg (|U|_F^2 + |V|_F^2) over the whole tables (:444).  Outside the tri-training branch the augmented and the two social encoders
        are skipped (nothing reads them: the results are identical) and neighbor_dis_loss is 0.  positives: [3, M, k]
        label sets to replay; the sets used are kept in `last_positives`."""
        rec_user, rec_item = self.encode(self.norm_adj)
        rec_loss = Ls.bpr_gather_loss(rec_user, rec_item, u, i, j, Fn.BPR_LOGSIGMOID)[0]
        rec_loss = rec_loss + self.reg * ((self.user_embeddings ** 2).sum() + (self.item_embeddings ** 2).sum())
        self.rec_user_embeddings, self.rec_item_embeddings = rec_user.detach(), rec_item.detach()
        if not tri_training:
            return rec_loss, torch.zeros((), device=self.device), rec_loss
        aug_user, _ = self.encode(aug_graph if aug_graph is not None else self.norm_adj)
        sharing = sept_encoder(self.user_embeddings, self.sharing_mat, self.n_layers, combine="sum")
        friend = sept_encoder(self.user_embeddings, self.social_mat, self.n_layers, combine="sum")
        loss3, self.last_positives = self.tri_loss(friend, sharing, rec_user, aug_user, torch.unique(u), self.instance_cnt,
                                                   0.1, positives)
        nd = loss3.sum()
        return rec_loss, nd, rec_loss + self.ss_rate * nd

    def train_step(self, batch, tri_training, aug_graph=None, positives=None):
        """One body of :432-465 for batch = (user_idx, pos_idx, neg_idx): losses, zero_grad, backward, Adam step.  Returns
        the detached (rec_loss, neighbor_dis_loss, total_loss)."""
        return self._optimise(*index_batch(batch, self.device), tri_training, aug_graph, positives)

    def train_epoch(self, epoch):
        tri = is_tri_training_epoch(epoch, self.maxEpoch)
        aug = self.augmented_graph(epoch) if tri else None
        for batch in next_batch_pairwise(self.data, self.batch_size, seed=self.seed, epoch=epoch, max_trials=MAX_TRIALS):
            self.train_step(batch, tri, aug)

    def train(self):
        """:422-473 with its quirks: the tables evaluated after an epoch are the ones the LAST batch's forward produced,
        before that batch's update, and `save()` runs once after the loop."""
        for epoch in range(self.maxEpoch):
            self.train_epoch(epoch)
            self.U, self.V = self.rec_user_embeddings.contiguous(), self.rec_item_embeddings.contiguous()
            self.fast_evaluation(epoch)
        self.save()
        self.U, self.V = self.best_user_emb, self.best_item_emb
        return self.evaluate()

    def save(self):
        self.best_user_emb = self.rec_user_embeddings.contiguous()
        self.best_item_emb = self.rec_item_embeddings.contiguous()

    def _final(self):
        if not hasattr(self, "U"):                          # never trained: the current parameters' forward
            with torch.no_grad():
                fu, fi = self.encode(self.norm_adj)
            self.U, self.V = fu.contiguous(), fi.contiguous()
        return self.U, self.V

    predict = RankingModel.predict_item_major             # :479-481: V @ U[u]
