"""Host-side mirror of gat.py's GATRec (two torch_geometric GATConv layers over the user-item graph) on the HIP ops.

  GATConv (torch_geometric)   gat.py:20-23, 34, 37   `GATConv` below: h = x W^T and the two logit tables stay torch (hipBLASLt
                                                     serves the product); the edge softmax, its dropout and the weighted
                                                     gather-sum are ONE autograd node (functional.gat_aggregate:
                                                     gcr_gat_fwd_f32 / gcr_gat_bwd_f32), which writes nothing per edge
  GATRec                      gat.py:14-40           `GATRec`: same constructor, `forward(edge_index)`; the graph is prepared
                                                     once per edge_index tensor and cached
  the loop body               gat.py:104-120         `GATRec.loss` (functional.bpr_sums' loss sum / E) + optim.FusedAdam
  train_model                 gat.py:90-126          `GATRecModel.train`: 30 full-batch epochs, then the eval-mode forward and
                                                     the fused full-ranking evaluation at N = 10

torch_geometric is not a dependency: `GATConv` is written from PyG's documented semantics with the defaults gat.py leaves
in place (concat=True, add_self_loops=True, bias=True; `functional.gat_aggregate_composed` is the statement-by-statement
form).  Parity with PyG's own GATConv is therefore unpinned, as it is for LGConv (README).
Quirks kept: negatives are `randint` draws with no rejection; the loss is a mean over the training pairs with no
regulariser; weight decay is Adam's (L2 added to the gradient).  The tuner (gat.py:129-164) and the CSV writer stay out.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as Fn
from .encoders import Interaction
from .graph import CsrGraph
from .model_base import MASK64, RankingModel, default_device, seeded
from .optim import FusedAdam

N_EPOCHS = 30                       # gat.py:103


def glorot_(t):
    """torch_geometric.nn.inits.glorot: uniform(-a, a), a = sqrt(6 / (size(-2) + size(-1)))."""
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        return t.uniform_(-a, a)


class _Lin(nn.Module):
    """PyG's bias-free Linear: `weight` [out, in] only, so the parameter is named `lin.weight`."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))

    def forward(self, x):
        return F.linear(x, self.weight)


class GATConv(nn.Module):
    """torch_geometric.nn.GATConv(in_channels, out_channels, heads, dropout=, negative_slope=) with its other defaults,
    over a prepared graph (`GATRec.prepare`: rows = targets, no diagonal).  Parameters under PyG's names: `lin.weight`
    [heads * out, in], `att_src`, `att_dst` [1, heads, out], `bias` [heads * out]; a state dict of an older PyG with
    `lin_src.weight` loads too."""

    def __init__(self, in_channels, out_channels, heads=1, dropout=0.0, negative_slope=0.2, seed=0):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.dropout, self.negative_slope = float(dropout), float(negative_slope)
        self.lin = _Lin(in_channels, heads * out_channels)
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.empty(heads * out_channels))
        self.seed, self.calls = int(seed), 0
        self.fused = True               # False: functional.gat_aggregate_composed (the A/B baseline)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.lin.weight)
        glorot_(self.att_src)
        glorot_(self.att_dst)
        nn.init.zeros_(self.bias)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        old = prefix + "lin_src.weight"
        if old in state_dict:
            state_dict[prefix + "lin.weight"] = state_dict.pop(old)
            state_dict.pop(prefix + "lin_dst.weight", None)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def draw_keep_bits(self, graph, device):
        """The attention dropout's draw of this call (training, dropout > 0): `rand >= p` per (term, head) from the counter
        RNG, a function of (seed, number of draws so far)."""
        self.calls += 1
        return Fn.edge_mask_bits((graph.nnz + graph.n_rows) * self.heads, self.dropout,
                                 (self.seed * 0x9E3779B97F4A7C15 + self.calls) & MASK64, device)

    def forward(self, x, graph, keep_bits=None):
        """keep_bits: a recorded attention keep bitmap (`functional.gat_aggregate`'s order) instead of a draw."""
        h = self.lin(x)
        hv = h.view(-1, self.heads, self.out_channels)
        a_src = (hv * self.att_src).sum(-1)
        a_dst = (hv * self.att_dst).sum(-1)
        p = self.dropout if self.training else 0.0
        if p == 0.0:
            keep_bits = None
        elif keep_bits is None:
            keep_bits = self.draw_keep_bits(graph, x.device)
        aggregate = Fn.gat_aggregate if self.fused else Fn.gat_aggregate_composed
        return aggregate(graph, h, a_src, a_dst, self.heads, self.negative_slope, keep_bits, p, self.bias)


def gat_graph(edge_index, num_nodes, device):
    """The operator of GATConv's message passing for `edge_index` int64 [2, E] (edge j -> i = (edge_index[0],
    edge_index[1])): CSR [n, n] without values, rows = edge_index[1], cols = edge_index[0], a row's entries in
    edge_index order, duplicates kept, the diagonal removed (PyG removes the self loops and adds one per node, which the
    kernel does implicitly).  `coo_perm`: entry e of the CSR is the coo_perm[e]-th of the kept edges."""
    ei = torch.as_tensor(edge_index).detach().to(torch.int64).cpu().numpy()
    off = ei[0] != ei[1]
    return CsrGraph.from_coo(ei[1][off], ei[0][off], None, num_nodes, num_nodes, device, want_perm=True, hub_window_rows=0)


class GATRec(nn.Module):
    """gat.py:14-40 with the reference's constructor; `forward(edge_index)` -> (user_emb, item_emb)."""

    def __init__(self, num_users, num_items, in_channels, hidden_channels, out_channels, num_heads, dropout, edge_dropout,
                 neg_slope, seed=0):
        super().__init__()
        self.user_embedding = nn.Embedding(num_users, in_channels)
        self.item_embedding = nn.Embedding(num_items, in_channels)
        self.gat1 = GATConv(in_channels, hidden_channels, heads=num_heads, dropout=edge_dropout, negative_slope=neg_slope,
                            seed=2 * seed + 1)
        self.gat2 = GATConv(hidden_channels * num_heads, out_channels, heads=1, dropout=edge_dropout,
                            negative_slope=neg_slope, seed=2 * seed + 2)
        self.dropout = dropout
        self.init_weights()
        self._graph_key, self._graph, self._graph_src = None, None, None

    def init_weights(self):
        nn.init.xavier_uniform_(self.user_embedding.weight)
        nn.init.xavier_uniform_(self.item_embedding.weight)

    def prepare(self, edge_index):
        """Builds (or returns the cached) `gat_graph` of `edge_index` int64 [2, E].  The cache is keyed on the tensor's
        address, shape and version counter and holds the tensor, so a new tensor or an in-place edit rebuilds the graph.
        An edit through `.data` or a numpy alias moves neither the address nor the version and is NOT seen: pass a new
        tensor (or edit in place through torch) instead."""
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version)
        if self._graph_key != key:
            n = self.user_embedding.num_embeddings + self.item_embedding.num_embeddings
            self._graph = gat_graph(edge_index, n, self.user_embedding.weight.device)
            self._graph_key = key
            self._graph_src = edge_index            # holding edge_index keeps the pointer from being recycled
        return self._graph

    def _feature_dropout(self, x, keep):
        """F.dropout(x, p, training) (gat.py:33, 36): drawn on x's device, or the recorded keep mask `keep` [n, d]."""
        if not self.training or self.dropout == 0.0:
            return x
        if keep is None:
            return F.dropout(x, p=self.dropout, training=True)
        return x * (keep.to(device=x.device, dtype=x.dtype) * (1.0 / (1.0 - self.dropout)))

    def forward(self, edge_index, masks=None):
        """masks (the pins' recorded draws): {"feat": (keep [n, in], keep [n, hidden * heads]), "att": (bitmap, bitmap)},
        either key optional; the bitmaps in `functional.gat_aggregate`'s order."""
        graph = edge_index if isinstance(edge_index, CsrGraph) else self.prepare(edge_index)
        feat = (masks or {}).get("feat", (None, None))
        att = (masks or {}).get("att", (None, None))
        x = torch.cat([self.user_embedding.weight, self.item_embedding.weight], dim=0)
        x = self._feature_dropout(x, feat[0])
        x = self.gat1(x, graph, att[0])
        x = F.elu(x)
        x = self._feature_dropout(x, feat[1])
        x = self.gat2(x, graph, att[1])
        nu = self.user_embedding.num_embeddings
        return x[:nu], x[nu:]

    def loss(self, edge_index, neg_i, masks=None):
        """gat.py:105-117 on the full batch: the training pairs are the first half of gat.py:51-52's edge_index
        ([[u; i + U], [i + U; u]]), neg_i int64 [E] their negatives; -log(sigmoid(pos - neg)).mean()."""
        nu = self.user_embedding.num_embeddings
        e = edge_index.shape[1] // 2
        pos_u = edge_index[0, :e]
        pos_i = edge_index[1, :e] - nu
        user_emb, item_emb = self(edge_index, masks=masks)
        s = Fn.bpr_sums(user_emb.contiguous(), item_emb.contiguous(), pos_u, pos_i, neg_i, Fn.BPR_LOG_SIGMOID)
        return s[0] / e


def bipartite_edge_index(uid, iid, num_users):
    """gat.py:49-52: [[u; i + U], [i + U; u]] int64 [2, 2 E]."""
    u, i = torch.as_tensor(uid, dtype=torch.int64), torch.as_tensor(iid, dtype=torch.int64) + num_users
    return torch.stack([torch.cat([u, i]), torch.cat([i, u])])


class GATRecModel(RankingModel):
    DEFAULTS = dict(in_channels=64, hidden_channels=64, out_channels=64, num_heads=2, dropout=0.2, edge_dropout=0.2,
                    neg_slope=0.2, lr=0.005, weight_decay=0.0)         # gat.py:130-141

    def __init__(self, config, train_set, test_set, device=None, seed=0):
        """config: gat.py:130-141's keys (missing ones take its defaults) and `item.ranking.topN` ([10]).  seed: initial
        weights, negatives and dropout draws are functions of it."""
        self.config, self.seed = {**self.DEFAULTS, **config}, int(seed)
        c = self.config
        self._read_topn(c, default=(10,))
        self.device = default_device(device)
        self.data = Interaction(c, train_set, test_set, device=self.device)
        nu, ni = self.data.user_num, self.data.item_num
        self.edge_index = bipartite_edge_index(self.data.uid, self.data.iid, nu).to(self.device)
        with seeded(self.seed, self.device):
            self.model = GATRec(nu, ni, c["in_channels"], c["hidden_channels"], c["out_channels"], c["num_heads"],
                                c["dropout"], c["edge_dropout"], c["neg_slope"], seed=self.seed).to(self.device)
        self.optimizer = FusedAdam(list(self.model.parameters()), lr=c["lr"], weight_decay=c["weight_decay"])
        self.maxEpoch = N_EPOCHS
        self.bestPerformance = []
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self.seed)

    def losses(self, neg_i):
        return (self.model.loss(self.edge_index, neg_i),)

    def train_step(self, neg_i=None):
        """One body of gat.py:104-120; neg_i: the step's negatives, drawn like gat.py:109 (no rejection) when None."""
        self.__dict__.pop("U", None)
        if neg_i is None:
            neg_i = torch.randint(0, self.data.item_num, (self.edge_index.shape[1] // 2,), device=self.device,
                                  generator=self._gen)
        return self._optimise(torch.as_tensor(neg_i, device=self.device, dtype=torch.int64))

    def train(self):
        """train_model (gat.py:100-126): 30 full-batch epochs in training mode, then the metrics of the eval-mode forward."""
        self.model.train()
        for _ in range(self.maxEpoch):
            self.train_step()
        return self.evaluate()

    def _final(self):
        if not hasattr(self, "U"):
            self.model.eval()
            with torch.no_grad():
                u, v = self.model(self.edge_index)
            self.U, self.V = u.contiguous(), v.contiguous()
        return self.U, self.V
