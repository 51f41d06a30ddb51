"""GCLModel with the reference's interface (gcl.py:38-64, 180-236), every per-step stage but the Linear layers on the HIP path:

    GCLModel(config, train, test).train()  ->  {10: {"HR": .., "P": .., "R": .., "NDCG": ..}, 20: {...}, 30: ..., 50: ...}

Stage by stage (reference line -> here):
    GRACEModel                           gcl.py:38-64     GRACEModel (convs / proj_head stay torch GEMMs)
    EdgeRemoving                         gcl.py:18-25     sampler.EdgeRemoving (gcr_edge_mask_bits)
    info_nce_loss                        gcl.py:28-35     losses.info_nce_loss (gcr_infonce_*: row + column logsumexp)
    gathers, BPR, regulariser            gcl.py:216-223   functional.bpr_sums(..., BPR_LOGSIGMOID) (gcr_bpr_*)
    torch.optim.Adam(lr, weight_decay)   gcl.py:201       optim.FusedAdam (gcr_adam_step_f32)
    next_batch_pairwise                  gcl.py:111-125   sampler.next_batch_pairwise (gcr_neg_sample)
    evaluate                             gcl.py:87-108    evaluate.rank_topk + rank_metric_terms (gcr_rank_*)
The hyper-parameter grid, logging and summary printer around it are out of scope.

encoder="linear" is the faithful form: `encode` ignores the edges, so both views are the same tensor and the
two EdgeRemoving draws have no effect on any output.  encoder="lightgcn" is the form BASELINE config 4 names (bench.py's
GCL leg): each view is a K-layer mean propagation of the stacked table over the symmetric-normalised bipartite operator with
that view's stored non-zeros dropped, then the projection head.

ShardedGCLStep is the same step row-sharded over the GPUs of one node (distributed.py).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import distributed as gd
from . import functional as Fn
from . import losses as Ls
from .encoders import load_data
from .evaluate import rank_metric_terms, rank_topk
from .graph import CsrGraph
from .model_base import MASK64, default_device, index_batch, optimise, seeded
from .optim import FusedAdam
from .sampler import MAX_TRIALS, EdgeRemoving, next_batch_pairwise      # gcl.py:120-124 retries forever: a large max_trials

ENCODERS = ("linear", "lightgcn")
KS = (10, 20, 30, 50)                       # gcl.py:232


class GraphView:
    """One edge-dropped view of a symmetric operator: every stored non-zero is kept independently with probability
    1 - pe (gcl.py:22-24 over the directed edges), `keep_bits` in the operator's non-zero order and `keep_bits_t` the same
    draws in its transpose's order (the backward pass).  pe == 0 keeps every edge and carries no bitmap."""

    def __init__(self, graph: CsrGraph, pe: float, seed: int):
        self.graph, self.pe = graph, float(pe)
        self.keep_bits = self.keep_bits_t = None
        if self.pe > 0:
            self.keep_bits = Fn.edge_mask_bits(graph.nnz, self.pe, seed, graph.device)
            self.keep_bits_t = Fn.edge_mask_bits(graph.nnz, self.pe, seed, graph.device, edge_id=graph.mirror_perm())


class GRACEModel(nn.Module):
    """gcl.py:38-64.  encoder="lightgcn" needs `graph`, the [U + I] x [U + I] operator the views are drawn from."""

    def __init__(self, num_users, num_items, emb_size=64, num_layers=2, proj_dim=64, encoder="linear", graph=None,
                 device=None):
        super().__init__()
        if encoder not in ENCODERS:
            raise ValueError(f"encoder must be one of {ENCODERS}")
        if encoder == "lightgcn" and graph is None:
            raise ValueError("encoder='lightgcn' needs the graph to propagate over")
        self.num_users, self.num_items, self.num_layers, self.encoder, self.graph = \
            int(num_users), int(num_items), int(num_layers), encoder, graph
        self.user_emb = nn.Embedding(num_users, emb_size, device=device)
        self.item_emb = nn.Embedding(num_items, emb_size, device=device)
        # the reference's Linear stack; the lightgcn form propagates instead and leaves it untouched (no gradient)
        self.convs = nn.ModuleList([nn.Linear(emb_size, emb_size, device=device) for _ in range(num_layers)])
        self.proj_head = nn.Sequential(nn.Linear(emb_size, proj_dim, device=device), nn.ReLU(),
                                       nn.Linear(proj_dim, proj_dim, device=device))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.user_emb.weight)
        nn.init.xavier_uniform_(self.item_emb.weight)

    def encode(self, edge_index=None):
        """linear: gcl.py:53-57 (edges ignored).  lightgcn: mean of the K + 1 layer outputs over `edge_index`, a GraphView
        (None: the whole operator)."""
        x = torch.cat([self.user_emb.weight, self.item_emb.weight], dim=0)
        if self.encoder == "linear":
            for conv in self.convs:
                x = conv(x)
            return x
        view = edge_index
        if view is None or view.keep_bits is None:
            return Fn.lightgcn_propagate(self.graph, x, self.num_layers, combine="mean")
        acc, h = x, x
        for _ in range(self.num_layers):
            h = Fn.spmm(self.graph, h, keep_bits=view.keep_bits, keep_bits_t=view.keep_bits_t)
            acc = acc + h
        return acc * (1.0 / (self.num_layers + 1))

    def project(self, x):
        return self.proj_head(x)

    def forward(self, edge_index1, edge_index2):
        if self.encoder == "linear":
            z = self.project(self.encode(edge_index1))      # encode ignores the edges: z1 == z2, computed once
            return z, z
        return self.project(self.encode(edge_index1)), self.project(self.encode(edge_index2))


def _positives_csr(users, items, n_users, device):
    """Sorted, de-duplicated items per user: (rowptr int64 [n_users + 1], items int32) on the device."""
    users = torch.as_tensor(np.asarray(users), dtype=torch.int64, device=device)
    items = torch.as_tensor(np.asarray(items), dtype=torch.int64, device=device)
    n_items = int(items.max()) + 1 if items.numel() else 1
    keys = torch.unique(users * n_items + items)
    u, i = keys // n_items, keys % n_items
    rowptr = torch.zeros(n_users + 1, dtype=torch.int64, device=device)
    rowptr[1:] = torch.cumsum(torch.bincount(u, minlength=n_users), 0)
    return rowptr, i.to(torch.int32).contiguous()


class _GCLData:
    """What the device sampler and the evaluation read, for integer ids that are already dense (gcl.py:67-78)."""

    def __init__(self, train, test, num_users, num_items, device):
        self.device = device
        self.user_num, self.item_num = int(num_users), int(num_items)
        tu, ti = (np.asarray(a, dtype=np.int64) for a in train)
        su, si = (np.asarray(a, dtype=np.int64) for a in test)
        self.uid_dev = torch.from_numpy(tu).to(device)
        self.iid_dev = torch.from_numpy(ti).to(device)
        self.user_rowptr, self.user_items_sorted = _positives_csr(tu, ti, self.user_num, device)
        # test users in order of first appearance (test_df['user'].unique(), gcl.py:90) and their test-item sets
        self.test_users = np.asarray(list(dict.fromkeys(su.tolist())), dtype=np.int64)
        rank = np.full(self.user_num, -1, dtype=np.int64)
        rank[self.test_users] = np.arange(self.test_users.size)
        self.test_rowptr, self.test_items_sorted = _positives_csr(rank[su], si, self.test_users.size, device)


class GCLModel:
    def __init__(self, config, train, test, device=None, seed=0, encoder="linear", num_users=None, num_items=None):
        """config: the keys of gcl.py:180-192 (embedding_size, num_layers, lr, weight_decay, ssl_temp, drop_edge,
        reg_weight, batch_size, max_epoch) plus an optional ssl_weight (univariate/gcl_univariate.py:202; the default 1.0
        is gcl.py's total).  train / test: (users, items) integer arrays as `encoders.load_data` returns them; raw ids
        are the dense ids and num_users / num_items default to max id + 1 over both (gcl.py:72-73)."""
        self.config, self.seed, self.encoder = dict(config), int(seed), encoder
        c = self.config
        self.emb_size, self.num_layers = int(c["embedding_size"]), int(c["num_layers"])
        self.lr, self.weight_decay = float(c["lr"]), float(c["weight_decay"])
        self.ssl_temp, self.drop_edge, self.reg_weight = float(c["ssl_temp"]), float(c["drop_edge"]), float(c["reg_weight"])
        self.ssl_weight = float(c.get("ssl_weight", 1.0))
        self.batch_size, self.max_epoch = int(c["batch_size"]), int(c["max_epoch"])
        self.device = default_device(device)
        tu, ti = (np.asarray(a, dtype=np.int64) for a in train)
        su, si = (np.asarray(a, dtype=np.int64) for a in test)
        if num_users is None:
            num_users = int(max(tu.max(), su.max(initial=-1))) + 1
        if num_items is None:
            num_items = int(max(ti.max(), si.max(initial=-1))) + 1
        self.num_users, self.num_items = int(num_users), int(num_items)
        self.data = _GCLData((tu, ti), (su, si), self.num_users, self.num_items, self.device)
        # gcl.py:75-77: [[u; i + U], [i + U; u]]; the linear form's EdgeRemoving views are drawn over it
        u = self.data.uid_dev
        i = self.data.iid_dev + self.num_users
        self.edge_index = torch.stack([torch.cat([u, i]), torch.cat([i, u])])
        graph = None
        if encoder == "lightgcn":
            graph = CsrGraph.bipartite_sym_norm(self.data.uid_dev, self.data.iid_dev, self.num_users, self.num_items,
                                                self.device)
        with seeded(self.seed, self.device):
            self.model = GRACEModel(self.num_users, self.num_items, self.emb_size, self.num_layers, encoder=encoder,
                                    graph=graph, device=self.device)
        self.aug = EdgeRemoving(pe=self.drop_edge, seed=self.seed)
        self.optimizer = FusedAdam(self.model.parameters(), lr=self.lr, weight_decay=self.weight_decay)

    @classmethod
    def from_files(cls, config, train_path, test_path, **kw):
        """gcl.py's data in: the `user item rating` files of load_data (gcl.py:67-78)."""
        _, train, test, num_users, num_items = load_data(train_path, test_path)
        return cls(config, train, test, num_users=num_users, num_items=num_items, **kw)

    def views(self):
        """The two augmented views of one step (gcl.py:209-210)."""
        if self.encoder == "linear":
            return self.aug(self.edge_index), self.aug(self.edge_index)
        out = []
        for _ in range(2):
            self.aug.calls += 1              # EdgeRemoving's counter: every view its own draws
            seed = (self.aug.seed * 0x9E3779B97F4A7C15 + self.aug.calls) & MASK64
            out.append(GraphView(self.model.graph, self.drop_edge, seed))
        return tuple(out)

    def losses(self, users, pos, neg, views=None):
        """gcl.py:211-224 on the HIP path: (ssl_loss, bpr_loss, reg_loss, total_loss), differentiable, no host sync."""
        users, pos, neg = index_batch((users, pos, neg), self.device)
        v1, v2 = self.views() if views is None else views
        z1, z2 = self.model(v1, v2)
        n_u = self.num_users
        user_z1, item_z1 = Fn.split_rows(z1, n_u)
        user_z2, item_z2 = (user_z1, item_z1) if z2 is z1 else Fn.split_rows(z2, n_u)
        ssl_loss = Ls.info_nce_loss(user_z1, user_z2, self.ssl_temp) + Ls.info_nce_loss(item_z1, item_z2, self.ssl_temp)
        # the three gathers, both scores, the BPR term and the three squared Frobenius norms in one kernel
        sums = Fn.bpr_sums(user_z1, item_z1, users, pos, neg, Fn.BPR_LOGSIGMOID)
        b = float(users.numel())
        bpr_loss = sums[0] / b
        reg_loss = (sums[1] + sums[2] + sums[3]) / b
        total_loss = self.ssl_weight * ssl_loss + bpr_loss + self.reg_weight * reg_loss
        return ssl_loss, bpr_loss, reg_loss, total_loss

    def train_step(self, users, pos, neg, views=None):
        """One body of gcl.py:208-225 (zero_grad, two views, losses, backward, Adam step).  Returns the four loss terms
        as device tensors.  views: the step's two views when the caller drew them (default: `views()`)."""
        return optimise(self, users, pos, neg, views)

    def train(self):
        self.model.train()
        for epoch in range(self.max_epoch):
            batches = next_batch_pairwise(self.data, self.batch_size, seed=self.seed, epoch=epoch, max_trials=MAX_TRIALS)
            for n, (users, pos, neg) in enumerate(batches):
                out = self.train_step(users, pos, neg)
                if (n + 1) % 100 == 0:
                    print(f"Batch {n + 1}, SSL loss: {float(out[0]):.4f}, BPR loss: {float(out[1]):.4f}, "
                          f"Reg loss: {float(out[2]):.4f}, Total loss: {float(out[3]):.4f}")
        self.model.eval()
        return self.evaluate()

    def embeddings(self):
        """gcl.py:229-232: the encoder output over the whole graph (no projection head)."""
        with torch.no_grad():
            final_z = self.model.encode(None)
        return final_z[:self.num_users].contiguous(), final_z[self.num_users:].contiguous()

    def evaluate(self, ks=KS):
        """gcl.py:87-108 with its own metric definitions (not ncl.py's): over every test user, HR = share of users with at
        least one hit, P = hits / k, R = hits / |test items of the user|, NDCG = the un-normalised DCG; all averaged over
        the test users.  Training positives are excluded from the ranking (gcl.py:94)."""
        user_emb, item_emb = self.embeddings()
        data = self.data
        ks = [int(k) for k in ks]
        q = data.test_users.size
        if q == 0:
            return {k: {"HR": 0.0, "P": 0.0, "R": 0.0, "NDCG": 0.0} for k in ks}
        ids = torch.from_numpy(data.test_users).to(self.device)
        top, _ = rank_topk(user_emb, item_emb, ids, data.user_rowptr, data.user_items_sorted, min(max(ks), self.num_items))
        cut, hits, dcg, _ = rank_metric_terms(top, data.test_rowptr, data.test_items_sorted, ks)
        n_test = (data.test_rowptr[1:] - data.test_rowptr[:-1]).to(torch.float64).unsqueeze(1)
        h = hits.to(torch.float64)
        # per-cut-off sums over the test users on the device, one read-back: [4, C]
        sums = torch.stack([(hits > 0).to(torch.float64).sum(0), h.sum(0), (h / n_test).sum(0), dcg.sum(0)]).cpu().numpy()
        out = {}
        for c, k in enumerate(cut.tolist()):
            out[k] = {"HR": sums[0, c] / q, "P": sums[1, c] / k / q, "R": sums[2, c] / q, "NDCG": sums[3, c] / q}
        return {k: {m: float(v) for m, v in out[k].items()} for k in ks}


class HipGCLOps:
    """The primitives of ShardedGCLStep on the HIP path (the product default).  The gloo choreography tests inject CPU
    stand-ins with the same members."""
    spmm = staticmethod(gd._hip_spmm)
    infonce_stats = None                      # None: distributed._ShardedSymInfoNCE
    bpr_sums = staticmethod(Fn.bpr_sums)
    edge_drop = gd.ShardedEdgeDrop


class ShardedGCLStep(nn.Module):
    """One GCL training step (gcl.py:208-225) row-sharded over the ranks of `g.group` (BASELINE config 4):
      * rank r owns the embedding rows of its users (`user_emb`, [U / world, d]) and an equal shard of the item rows
        (`item_emb`, [I / world, d]); convs / proj_head are replicated;
      * lightgcn form: two ShardedEdgeDrop views, each propagated by `sharded_lightgcn_propagate` (item shards all-gathered
        and partial item sums reduce-scattered every layer); linear form: the row-wise Linear stack on the local rows;
      * symmetric InfoNCE over all users and over all items (`sharded_info_nce_loss`: local anchors against the
        all-gathered other view), BPR + regulariser on this rank's triples against the all-gathered item rows;
      * backward (item gradients reduce-scattered to their owner shard), then the all-reduce of the replicated
        parameters' partial gradients.
    Every rank's returned loss terms are its share: summed over the ranks they are the one-process values, and after
    `step` the gradients of every local row and every replicated parameter are the one-process gradients.
    Padding rows would enter the all-pairs softmax as extra negatives, so the user and item counts must divide by the
    world size."""

    def __init__(self, g: gd.ShardedBipartiteGraph, num_users, emb_size=64, num_layers=2, proj_dim=64, encoder="lightgcn",
                 ssl_temp=0.2, drop_edge=0.2, reg_weight=1e-4, ssl_weight=1.0, seed=0, ops=HipGCLOps, device=None):
        super().__init__()
        if encoder not in ENCODERS:
            raise ValueError(f"encoder must be one of {ENCODERS}")
        if num_users % g.world or g.num_items % g.world or g.n_local_users * g.world != num_users:
            raise ValueError("ShardedGCLStep needs users and items divisible by the world size (equal row blocks)")
        self.g, self.ops, self.encoder = g, ops, encoder
        self.num_users, self.num_items, self.num_layers = int(num_users), int(g.num_items), int(num_layers)
        self.ssl_temp, self.drop_edge, self.reg_weight, self.ssl_weight = float(ssl_temp), float(drop_edge), \
            float(reg_weight), float(ssl_weight)
        self.seed, self.steps = int(seed), 0
        dev = device if device is not None else g.r_ui.device
        # xavier-uniform rows of the GLOBAL [U, d] / [I, d] tables (GRACEModel.reset_parameters); `load_global` replaces them
        bu, bi = (6.0 / (self.num_users + emb_size)) ** 0.5, (6.0 / (self.num_items + emb_size)) ** 0.5
        self.user_emb = nn.Parameter((torch.rand(g.n_local_users, emb_size, device=dev) * 2 - 1) * bu)
        self.item_emb = nn.Parameter((torch.rand(g.items_per_rank, emb_size, device=dev) * 2 - 1) * bi)
        self.convs = nn.ModuleList([nn.Linear(emb_size, emb_size, device=dev) for _ in range(num_layers)])
        self.proj_head = nn.Sequential(nn.Linear(emb_size, proj_dim, device=dev), nn.ReLU(),
                                       nn.Linear(proj_dim, proj_dim, device=dev))

    def load_global(self, state):
        """This rank's rows of a GRACEModel state dict (user_emb.weight / item_emb.weight [global rows, d]) and the
        replicated layers."""
        g = self.g
        lo_u, lo_i = g.rank * g.n_local_users, g.rank * g.items_per_rank
        with torch.no_grad():
            self.user_emb.copy_(torch.as_tensor(state["user_emb.weight"])[lo_u:lo_u + g.n_local_users])
            self.item_emb.copy_(torch.as_tensor(state["item_emb.weight"])[lo_i:lo_i + g.items_per_rank])
            for name, p in self.named_parameters():
                if name.startswith(("convs.", "proj_head.")):
                    p.copy_(torch.as_tensor(state[name]))
        return self

    def replicated_parameters(self):
        return [p for n, p in self.named_parameters() if n not in ("user_emb", "item_emb")]

    def _encode(self, view):
        if self.encoder == "linear":
            hu, hi = self.user_emb, self.item_emb
            for conv in self.convs:
                hu, hi = conv(hu), conv(hi)
            return hu, hi
        return gd.sharded_lightgcn_propagate(self.g, self.user_emb, self.item_emb, self.num_layers, "mean",
                                             spmm=self.ops.spmm, view=view)

    def losses(self, users, pos, neg, batch_size):
        """This rank's share of (ssl_loss, bpr_loss, reg_loss, total_loss).  users: LOCAL user rows of this rank's
        triples; pos / neg: global item ids; batch_size: the global batch (the BPR / regulariser denominator)."""
        g, ops = self.g, self.ops
        self.steps += 1
        v1 = v2 = None
        if self.encoder == "lightgcn" and self.drop_edge > 0:
            base = (self.seed * 0x9E3779B97F4A7C15 + 2 * self.steps) & MASK64
            v1, v2 = ops.edge_drop(g, self.drop_edge, base + 1), ops.edge_drop(g, self.drop_edge, base + 2)
        hu1, hi1 = self._encode(v1)
        zu1, zi1 = self.proj_head(hu1), self.proj_head(hi1)
        if self.encoder == "linear":                      # the edges do not reach the encoder: one view
            zu2, zi2 = zu1, zi1
        else:
            hu2, hi2 = self._encode(v2)
            zu2, zi2 = self.proj_head(hu2), self.proj_head(hi2)
        nce = gd.sharded_info_nce_loss
        ssl_loss = nce(zu1, zu2, self.ssl_temp, g.group, ops.infonce_stats) + \
            nce(zi1, zi2, self.ssl_temp, g.group, ops.infonce_stats)
        items_full = gd.gather_items(zi1, g.group)[:self.num_items]
        sums = ops.bpr_sums(zu1, items_full, users, pos, neg, Fn.BPR_LOGSIGMOID)
        b = float(batch_size)
        bpr_loss = sums[0] / b
        reg_loss = (sums[1] + sums[2] + sums[3]) / b
        return ssl_loss, bpr_loss, reg_loss, self.ssl_weight * ssl_loss + bpr_loss + self.reg_weight * reg_loss

    def step(self, users, pos, neg, batch_size, optimizer=None):
        """losses + backward + all-reduce of the replicated gradients (+ optimizer.step() when given).  Returns this
        rank's share of the four loss terms (detached)."""
        if optimizer is not None:
            optimizer.zero_grad(set_to_none=True)
        out = self.losses(users, pos, neg, batch_size)
        out[3].backward()
        gd.allreduce_replicated_grads(self.replicated_parameters(), self.g.group)
        if optimizer is not None:
            optimizer.step()
        return tuple(t.detach() for t in out)
