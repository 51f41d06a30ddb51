"""DirectAUModel with the reference's interface (directau.py:196-266), every per-step stage on the HIP path:

    DirectAUModel(conf, train_set, test_set).train()  ->  {'Hit Ratio': .., 'Precision': .., 'Recall': .., 'NDCG': ..}

Stage by stage (reference line -> here):
    Interaction (sorted ids, raw adjacency)   directau.py:102-144   encoders.Interaction (gcr_dense_ids_u64, gcr_coo_to_csr)
    LGCNEncoder                               directau.py:269-293   encoders.LGCNEncoder's stacked table through
                                                                    functional.lightgcn_propagate (gcr_spmm_csr_acc2_f32)
    user_emb[user_idx], item_emb[pos / neg]   directau.py:222       inside functional.au_sums (gcr_directau_fwd_f32): no
                                                                    gathered copy is formed
    alignment, uniformity, calculate_loss     directau.py:240-251   losses.directau_loss: the eight sums of one fused
                                                                    forward; uniformity(u_emb), which the reference computes
                                                                    for pos_loss and again for neg_loss, is computed once
    l2_reg_loss / batch_size                  directau.py:35-36,226 the Q sums of the same forward
    loss.backward()                           directau.py:228       gcr_directau_bwd_f32 (rows added straight into the table
                                                                    gradient), then the propagation's transposed recurrence
    torch.optim.Adam(lr) | SGD(lr, 0.9)       directau.py:211-216   optim.FusedAdam | optim.FusedSGD (gcr_adam_step_f32 |
                                                                    gcr_sgd_momentum_step_f32)
    next_batch_pairwise                       directau.py:14-32     sampler.next_batch_pairwise (gcr_neg_sample)
    test / evaluate / predict                 directau.py:167-178, 253-266   model_base.RankingModel over `_final`
                                                                    (evaluate.test / ranking_evaluation: gcr_rank_*)
The tuner (directau.py:296-358), the print every 100 batches (directau.py:230-233) and the result files are out of
scope.
"""
from __future__ import annotations

import torch

from . import functional as Fn
from . import losses as Ls
from .encoders import Interaction, LGCNEncoder
from .model_base import RankingModel, default_device, index_batch, is_prepared, prepared_data, seeded
from .optim import FusedAdam, FusedSGD
from .sampler import MAX_TRIALS, next_batch_pairwise          # directau.py:27-31 retries until a negative is found


class DirectAUModel(RankingModel):
    def __init__(self, conf, train_set, test_set, device=None, seed=0):
        """conf: the reference's keys (directau.py:197-207) — conf['DirectAU']['gamma' | 'n_layers'], `reg.lambda` (1e-4),
        `batch.size` (512), `embedding.size` (64), `learning.rate` (1e-3), `optimizer` ('adam' | 'sgd'),
        `item.ranking.topN` ([10, 20, 30, 50]).  seed: initial weights, batch order and negatives are functions of it
        (the reference never seeds its generators)."""
        self.config, self.seed = conf, int(seed)
        args = conf["DirectAU"]
        self.gamma, self.n_layers = float(args["gamma"]), int(args["n_layers"])
        self.reg = conf.get("reg.lambda", 0.0001)
        self.batch_size = conf.get("batch.size", 512)
        self.emb_size = conf.get("embedding.size", 64)
        self.lRate = conf.get("learning.rate", 0.001)
        self.optimizer_type = str(conf.get("optimizer", "adam")).lower()
        if self.optimizer_type not in ("adam", "sgd"):
            raise ValueError(f"Unsupported optimizer: {self.optimizer_type}")          # directau.py:216
        self._read_topn(conf)
        self.device = default_device(device)
        # `train_set` may be a prepared data object (`from_graph`): graphs too large for Python id maps
        self.data = train_set if is_prepared(train_set, "norm_adj") else Interaction(conf, train_set, test_set, device=self.device)
        with seeded(self.seed, self.device):
            self.model = LGCNEncoder(self.data, self.emb_size, self.n_layers)
        params = list(self.model.parameters())
        self.optimizer = FusedAdam(params, lr=self.lRate) if self.optimizer_type == "adam" else \
            FusedSGD(params, lr=self.lRate, momentum=0.9)
        self.bestPerformance = []

    @classmethod
    def from_graph(cls, conf, norm_adj, user_num, item_num, **kw):
        """DirectAUModel over an operator that already lives on the device: what the training step reads from
        `Interaction` — sizes, the operator, the device — without the Python id maps (scripts/perf_directau_step.py)."""
        data = prepared_data(user_num, item_num, norm_adj.device, norm_adj=norm_adj)
        return cls(conf, data, None, device=norm_adj.device, **kw)

    def encode(self):
        """(user_emb [U, d], item_emb [I, d]) of directau.py:220: the mean of the K + 1 layer outputs, as the two halves of
        one table (their gradients then share one buffer)."""
        final = Fn.lightgcn_propagate(self.data.norm_adj, self.model.stacked(), self.n_layers, combine="mean")
        return Fn.split_rows(final, self.data.user_num)

    def losses(self, u, i, j):
        """directau.py:220-226 on the HIP path: (pos_loss, neg_loss, l2, loss), differentiable, no host sync."""
        u, i, j = index_batch((u, i, j), self.device)
        user_emb, item_emb = self.encode()
        return Ls.directau_loss(user_emb, item_emb, u, i, j, self.gamma, self.reg, self.batch_size)

    def train_step(self, batch):
        """One body of directau.py:219-229 for batch = (user_idx, pos_idx, neg_idx): zero_grad, losses, backward, optimizer
        step.  Returns the detached terms (pos_loss, neg_loss, l2, loss); l2 is l2_reg_loss before the division by the
        configured batch size that `loss` applies."""
        return self._optimise(*batch)

    def embeddings(self):
        with torch.no_grad():
            user_emb, item_emb = self.encode()
        return user_emb.contiguous(), item_emb.contiguous()

    def train(self):
        """directau.py:209-238: ONE epoch (`for epoch in range(1)`) of shuffled batches, the final embeddings, evaluate()."""
        self.model.train()
        for epoch in range(1):
            for batch in next_batch_pairwise(self.data, self.batch_size, seed=self.seed, epoch=epoch, max_trials=MAX_TRIALS):
                self.train_step(batch)
        self.user_emb, self.item_emb = self.embeddings()
        return self.evaluate()

    def calculate_loss(self, user_emb, item_emb):
        """directau.py:240-243 on two already-gathered [B, d] tensors: one fused forward."""
        s = Fn.au_sums(user_emb, item_emb, None, None)
        rows = user_emb.shape[0]
        unif = Ls._log_mean_pairs(s[2:4], rows) if rows >= 2 else torch.zeros(2, device=s.device)
        return s[0] / rows + self.gamma * (unif[0] + unif[1]) / 2

    def alignment(self, x, y):
        return Ls.alignment(x, y)

    def uniformity(self, x, t=2):
        return Ls.uniformity(x, t)

    def _final(self):
        if not hasattr(self, "user_emb"):                                               # directau.py:255-258
            self.user_emb, self.item_emb = self.embeddings()
        return self.user_emb, self.item_emb
