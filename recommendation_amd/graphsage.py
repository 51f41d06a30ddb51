"""Host-side mirror of graphsage.py's GraphSAGE (torch_geometric SAGEConv layers over the user-item graph) on the HIP ops.

  SAGEConv (torch_geometric)  graphsage.py:21-24, 28   `SAGEConv` below: the mean aggregation is the tuned SpMM on
                                                       `functional.sage_mean_graph`; lin_l, lin_r, the bias, the
  self.activation, F.dropout  graphsage.py:29-30       activation and the dropout of a hidden layer are ONE autograd node
                                                       (functional.sage_layer: gcr_sage_fwd_f32 / gcr_sage_bwd_f32)
  GraphSAGE                   graphsage.py:15-32       `GraphSAGE`: same constructor, `forward(x, edge_index)`; the graph is
                                                       prepared once per edge_index tensor and cached
  the loop body               graphsage.py:99-126      `GraphSAGEModel.train_step`: 'bpr' = functional.bpr_sums' loss sum / E,
                                                       'bce' = functional.bce_edge_loss (graphsage.py:117-121 is
                                                       lightgcn.py:109-113); Adam -> optim.FusedAdam, SGD ->
                                                       optim.FusedSGD(momentum=0), AdamW -> torch.optim.AdamW
  train_model                 graphsage.py:85-134      `GraphSAGEModel.train`: 30 full-batch epochs, then the eval-mode forward
                                                       and the fused full-ranking evaluation at N = 10, 20, 30, 50

torch_geometric is not a dependency: `SAGEConv` is written from PyG's documented semantics with the defaults graphsage.py
leaves in place (aggr='mean', root_weight=True, bias=True, normalize=False, project=False;
`functional.sage_layer_composed` is the statement-by-statement form).  Parity with PyG's own SAGEConv is therefore
unpinned, as it is for GATConv and LGConv (README).
Quirks kept: n_layers = 1 and n_layers = 2 build the same two layers; the node features are a fixed randn draw, not a
parameter; negatives are `randint` draws with no rejection; the loss is a mean over the training pairs with no regulariser;
weight decay is the optimiser's.  A fused decoupled-decay Adam (AdamW) is out of scope: that choice runs torch's own
optimiser on the same gradients.  The tuner (graphsage.py:137-179) and the CSV writer stay out.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as Fn
from .encoders import Interaction
from .graph import CsrGraph
from .model_base import MASK64, RankingModel, default_device, is_prepared, seeded
from .optim import FusedAdam, FusedSGD

N_EPOCHS = 30                       # graphsage.py:98
IN_CHANNELS = OUT_CHANNELS = 64     # graphsage.py:46, 88, 90


class _Lin(nn.Module):
    """torch_geometric's Linear under PyG's parameter names (`weight` [out, in], `bias` [out] or absent) with
    torch.nn.Linear's default initialisation: kaiming-uniform with a = sqrt(5), bias uniform in +-1 / sqrt(in)."""

    def __init__(self, in_channels, out_channels, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.weight.shape[1])
            nn.init.uniform_(self.bias, -bound, bound)


class SAGEConv(nn.Module):
    """torch_geometric.nn.SAGEConv(in_channels, out_channels) with its defaults, over a prepared graph
    (`functional.sage_mean_graph`): lin_l(mean_j x_j) + lin_r(x).  Parameters under PyG's names: `lin_l.weight`
    [out, in], `lin_l.bias` [out], `lin_r.weight` [out, in] (no bias).  `forward` also takes the activation and the
    dropout that follow the layer in GraphSAGE.forward, so that they run in the layer's kernel."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_l = _Lin(in_channels, out_channels, bias=True)
        self.lin_r = _Lin(in_channels, out_channels, bias=False)
        self.fused = True               # False: functional.sage_layer_composed (the A/B baseline)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()

    def forward(self, x, graph, act="none", keep_bits=None, p=0.0):
        layer = Fn.sage_layer if self.fused else Fn.sage_layer_composed
        return layer(graph, x, self.lin_l.weight, self.lin_r.weight, self.lin_l.bias, act, keep_bits, p)


class GraphSAGE(nn.Module):
    """graphsage.py:15-32 with the reference's constructor; `forward(x, edge_index)` -> [n, out_channels]."""

    def __init__(self, in_channels, hidden_channels, out_channels, n_layers, dropout=0.2, activation="relu", seed=0):
        super().__init__()
        self.layers = nn.ModuleList()
        self.dropout = dropout
        # 'relu' and 'gelu' run inside the layer kernel; any other F name runs the composed layer with that function
        self.activation = activation if activation in ("relu", "gelu") else getattr(F, activation)
        self.layers.append(SAGEConv(in_channels, hidden_channels))
        for _ in range(n_layers - 2):               # empty for n_layers 1 and 2 alike: both build two layers
            self.layers.append(SAGEConv(hidden_channels, hidden_channels))
        self.layers.append(SAGEConv(hidden_channels, out_channels))
        self.seed, self.calls = int(seed), 0
        self._graph_key, self._graph, self._graph_src = None, None, None

    def prepare(self, edge_index, num_nodes):
        """Builds (or returns the cached) `functional.sage_mean_graph` of `edge_index` int64 [2, E].  The cache is keyed
        on the tensor's address, shape and version counter (and num_nodes) and holds the tensor, so a new tensor or an
        in-place edit rebuilds the graph.  An edit through `.data` or a numpy alias moves neither the address nor the
        version and is NOT seen: pass a new tensor (or edit in place through torch) instead."""
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, int(num_nodes))
        if self._graph_key != key:
            self._graph = Fn.sage_mean_graph(edge_index, num_nodes, self.layers[0].lin_l.weight.device)
            self._graph_key = key
            self._graph_src = edge_index            # holding edge_index keeps the pointer from being recycled
        return self._graph

    def draw_keep_bits(self, count, device):
        """One F.dropout draw (training, dropout > 0): `rand >= p` for `count` elements from the counter RNG, a function
        of (seed, number of draws so far)."""
        self.calls += 1
        return Fn.edge_mask_bits(count, self.dropout, (self.seed * 0x9E3779B97F4A7C15 + self.calls) & MASK64, device)

    def forward(self, x, edge_index, masks=None):
        """masks (the pins' recorded draws): one keep mask per hidden layer, bool [n, hidden] or a packed bitmap in
        `functional.sage_layer`'s order, instead of a draw."""
        graph = edge_index if isinstance(edge_index, CsrGraph) else self.prepare(edge_index, x.shape[0])
        p = float(self.dropout) if self.training else 0.0
        for k, conv in enumerate(self.layers[:-1]):
            keep = None
            if p > 0.0:
                keep = masks[k] if masks is not None else self.draw_keep_bits(x.shape[0] * conv.out_channels, x.device)
                if keep.dtype == torch.bool:
                    keep = Fn.pack_bits(keep.reshape(-1)).to(x.device)
            x = conv(x, graph, self.activation, keep, p)
        return self.layers[-1](x, graph)


def bipartite_edge_index(uid, iid, num_users):
    """graphsage.py:41-44: [[u; i + U], [i + U; u]] int64 [2, 2 E]."""
    u, i = torch.as_tensor(uid, dtype=torch.int64), torch.as_tensor(iid, dtype=torch.int64) + num_users
    return torch.stack([torch.cat([u, i]), torch.cat([i, u])])


class GraphSAGEModel(RankingModel):
    DEFAULTS = dict(hidden_channels=64, n_layers=2, dropout=0.2, activation="relu", lr=0.01, weight_decay=1e-4,
                    optimizer="Adam", loss_type="bpr")                  # graphsage.py:138-147

    def __init__(self, config, train_set, test_set, x=None, device=None, seed=0):
        """config: graphsage.py:138-147's keys (missing ones take its defaults) and `item.ranking.topN` ([10, 20, 30, 50]).
        x: the node features [U + I, 64] (graphsage.py:46), a randn draw from the seed when None; not a parameter.
        seed: features, initial weights, negatives and dropout draws are functions of it.  train_set: the list of
        triples, or a prepared data object carrying `uid`, `iid` (dense ids of the training pairs), `user_num`,
        `item_num` and, for 'bce', `norm_adj` (CsrGraph.bipartite_raw)."""
        self.config, self.seed = {**self.DEFAULTS, **config}, int(seed)
        c = self.config
        if c["loss_type"] not in ("bpr", "bce"):
            raise ValueError("Invalid loss_type")                       # graphsage.py:123
        self._read_topn(c)
        self.device = default_device(device)
        self.data = train_set if is_prepared(train_set, "uid") else Interaction(c, train_set, test_set, device=self.device)
        nu, ni = self.data.user_num, self.data.item_num
        self.edge_index = bipartite_edge_index(self.data.uid, self.data.iid, nu).to(self.device)
        self.pos_u, self.pos_i = self.edge_index[0, :len(self.data.uid)], self.edge_index[1, :len(self.data.uid)] - nu
        with seeded(self.seed, self.device):
            if x is None:
                x = torch.randn(nu + ni, IN_CHANNELS)
            self.model = GraphSAGE(IN_CHANNELS, c["hidden_channels"], OUT_CHANNELS, c["n_layers"], c["dropout"],
                                   c["activation"], seed=self.seed).to(self.device)
        self.x = torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous()
        params = list(self.model.parameters())
        if c["optimizer"] == "Adam":
            self.optimizer = FusedAdam(params, lr=c["lr"], weight_decay=c["weight_decay"])
        elif c["optimizer"] == "SGD":                                   # torch.optim.SGD's default momentum, as the reference gets
            self.optimizer = FusedSGD(params, lr=c["lr"], momentum=0.0, weight_decay=c["weight_decay"])
        elif c["optimizer"] == "AdamW":                                 # no fused decoupled-decay Adam (module docstring)
            self.optimizer = torch.optim.AdamW(params, lr=c["lr"], weight_decay=c["weight_decay"])
        else:
            raise ValueError("optimizer must be 'Adam', 'AdamW' or 'SGD'")
        self.maxEpoch = N_EPOCHS
        self.bestPerformance = []
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self.seed)

    def losses(self, neg_i, masks=None):
        """graphsage.py:101-121 on the full batch."""
        nu = self.data.user_num
        out = self.model(self.x, self.edge_index, masks=masks)
        if self.config["loss_type"] == "bce":
            return (Fn.bce_edge_loss(self.data.norm_adj, out, nu),)
        s = Fn.bpr_sums(out[:nu], out[nu:], self.pos_u, self.pos_i, neg_i, Fn.BPR_LOG_SIGMOID)
        return (s[0] / self.pos_u.numel(),)

    def train_step(self, neg_i=None, masks=None):
        """One body of graphsage.py:99-126; neg_i: the step's negatives, drawn like graphsage.py:107 (no rejection) when
        None ('bce' draws them too and leaves them unused, as the reference does); masks: `GraphSAGE.forward`'s."""
        self.__dict__.pop("U", None)
        self.model.train()                                              # graphsage.py:99
        if neg_i is None:
            neg_i = torch.randint(0, self.data.item_num, (self.pos_u.numel(),), device=self.device, generator=self._gen)
        return self._optimise(torch.as_tensor(neg_i, device=self.device, dtype=torch.int64), masks)

    def train(self):
        """train_model (graphsage.py:98-134): 30 full-batch epochs in training mode, then the metrics of the eval-mode
        forward."""
        for _ in range(self.maxEpoch):
            self.train_step()
        return self.evaluate()

    def _final(self):
        if not hasattr(self, "U"):
            self.model.eval()
            with torch.no_grad():
                out = self.model(self.x, self.edge_index)
            nu = self.data.user_num
            self.U, self.V = out[:nu].contiguous(), out[nu:].contiguous()
        return self.U, self.V
