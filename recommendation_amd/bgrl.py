"""Host-side mirror of univariate/bgrl_g2l.py (BGRL, the bootstrapped global-to-local objective, over GIN layers) on the HIP
ops.

  GINConv, make_gin_conv      bgrl_g2l.py:20, 500-505  `GINConv` below: the sum aggregation (1 + eps) x_i + sum_j x_j is the
  self.activation, F.dropout  bgrl_g2l.py:526-529      tuned SpMM on `functional.gin_sum_graph` with x as its `acc_in`;
                                                       Linear, ReLU, Linear, the ReLU and the dropout behind them are ONE
                                                       autograd node (functional.gin_layer: gcr_gin_fwd_f32 / _bwd_f32)
  Normalize, GConv            bgrl_g2l.py:486-531      `Normalize`, `GConv`: BatchNorm1d, the projection head's Linear,
                                                       BatchNorm1d, PReLU and Dropout stay torch ops (library GEMMs)
  EdgeRemoving                bgrl_g2l.py:448-456      a keep bitmap over the graph's entries (the SpMM's keep_bits /
                                                       keep_bits_t), one draw per edge shared by A and A^T
  FeatureMasking              bgrl_g2l.py:409-425      functional.feature_masking
  Encoder                     bgrl_g2l.py:534-572      `Encoder`: same constructor (the augmentor is a pair of (edge_p, feat_p)),
                                                       get_target_encoder, update_target_encoder, forward
  global_add_pool             bgrl_g2l.py:563-571      a column sum (one graph)
  BootstrapLatent / Contrast  bgrl_g2l.py:277-308, 436-446   the same classes; torch ops on [n, hidden]
  train                       bgrl_g2l.py:575-583      `BGRLModel.train_step`; Adam (coupled weight decay) -> optim.FusedAdam
  main's loop body            bgrl_g2l.py:646-673      `BGRLModel.train`: ONE epoch of one full-batch step, then the eval-mode
                                                       online encoder and the fused full-ranking evaluation at N = 10 .. 50

torch_geometric is not a dependency: `GINConv` is written from PyG's documented semantics (out = nn((1 + eps) x_i +
sum_j x_j), eps = 0 and not trained; `functional.gin_layer_composed` is the statement-by-statement form).  Parity with PyG's
own GINConv is therefore unpinned, as it is for SAGEConv, GATConv and LGConv (README).

Quirks kept:
  * `GConv.forward` overwrites `self.activation` with ReLU in every layer (:526): the configured activation has no effect;
  * `conv(z, edge_index, edge_weight)` passes the weight as GINConv's `size`: there are no edge weights;
  * eps = 0, not trained;
  * `data.x` is an nn.Embedding(num_nodes, hidden_dim).weight that is not in `encoder.parameters()`: a fixed N(0, 1) table
    drawn from the seed and never updated, so the first layer takes no input gradient;
  * the target encoder is a deep copy made at the first forward, after the optimiser exists; it is never optimised, runs
    in train mode (batch statistics, its own dropout draws), only its PARAMETERS are EMA-updated, in `zip` order, and its
    BatchNorm buffers follow their own running updates;
  * `train()` ignores its `momentum` argument and calls `update_target_encoder()` with the default 0.99 (:582):
    config['momentum'] and config['batch_size'] have no effect;
  * the loss takes the single-graph branch (:297-300): 0.5 (L(g1_target, h2_pred) + L(g2_target, h1_pred)),
    L = mean_n (2 - 2 cos(h_n, g)), g the column sum of the target's projected output; g1 and g2 of the online side are
    computed and unused;
  * `Encoder` is built without a `dropout` argument (:656-659), so the predictor's Dropout keeps the default 0.2 whatever
    config['dropout'] says;
  * the optimiser is Adam with coupled weight_decay over the online encoder and the predictor (:661); training is one
    epoch of one full-batch step (:664);
  * `Interaction` uses sorted ids and an adjacency with both directions, (u, i) and (i, u) interleaved, duplicates kept
    (:85-115);
  * `predict` runs the online encoder in eval mode, so BatchNorm uses its running statistics after however many steps
    were taken, and scores z[items] @ z[user] with z the FIRST output (:157-164).  The reference's evaluator builds a new
    random table for this (:151); here the training table is used.
The tuner's grid (bgrl_g2l.py:610-645) and the SVM evaluator stay out.
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as Fn
from .encoders import Interaction
from .graph import CsrGraph
from .model_base import MASK64, RankingModel, default_device, is_prepared, seeded
from .optim import FusedAdam

N_EPOCHS = 1                        # bgrl_g2l.py:664
TARGET_MOMENTUM = 0.99              # bgrl_g2l.py:553, 582: the default, whatever the configuration says


class Normalize(nn.Module):
    """bgrl_g2l.py:486-497."""

    def __init__(self, dim=None, norm="batch"):
        super().__init__()
        if norm == "none" or dim is None:
            self.norm = lambda x: x
        elif norm == "batch":
            self.norm = nn.BatchNorm1d(dim)
        elif norm == "layer":
            self.norm = nn.LayerNorm(dim)

    def forward(self, x):
        return self.norm(x)


class GINConv(nn.Module):
    """torch_geometric.nn.GINConv(nn) with its defaults (eps = 0, train_eps = False: `eps` is a buffer, as PyG registers it)
    over a prepared graph (`functional.gin_sum_graph`), for nn = Sequential(Linear, ReLU, Linear).  `forward` also takes the
    ReLU and the dropout that follow the layer in GConv.forward, so that they run in the layer's kernel."""

    def __init__(self, nn_, eps=0.0):
        super().__init__()
        self.nn = nn_
        self.initial_eps = float(eps)
        self.register_buffer("eps", torch.tensor([float(eps)]))
        self.fused = True               # False: functional.gin_layer_composed (the A/B baseline)

    def forward(self, x, graph, keep_bits=None, p=0.0, edge_keep_bits=None, edge_keep_bits_t=None):
        layer = Fn.gin_layer if self.fused else Fn.gin_layer_composed
        lin1, lin2 = self.nn[0], self.nn[2]
        return layer(graph, x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, self.initial_eps, keep_bits, p, edge_keep_bits,
                     edge_keep_bits_t)


def make_gin_conv(input_dim, out_dim):
    """bgrl_g2l.py:500-505."""
    return GINConv(nn.Sequential(nn.Linear(input_dim, out_dim), nn.ReLU(), nn.Linear(out_dim, out_dim)))


def _draw_bits(module, count, p, device):
    """One dropout draw of `module` (it carries `seed` and `calls`) as a packed keep bitmap over `count` elements,
    `rand >= p`, a function of (seed, number of draws so far): the counter RNG on the device, a seeded torch generator on the
    host."""
    module.calls += 1
    key = (module.seed * 0x9E3779B97F4A7C15 + module.calls) & MASK64
    if torch.device(device).type == "cuda":
        return Fn.edge_mask_bits(count, p, key, device)
    return Fn.pack_bits(torch.rand(count, generator=torch.Generator().manual_seed(key & (2 ** 63 - 1))) >= p)


def _draw_keep(module, count, p, device):
    """`_draw_bits` unpacked: bool [count] (bit e of word e // 32, 32 shifts per word)."""
    bits = _draw_bits(module, count, p, device)
    return ((bits[:, None] >> torch.arange(32, dtype=torch.int32, device=bits.device)) & 1).reshape(-1)[:count].bool()


def _as_bits(keep, device):
    """A keep mask (bool, any shape) or a packed bitmap -> the packed bitmap on `device`."""
    keep = torch.as_tensor(keep)
    return (Fn.pack_bits(keep.reshape(-1)) if keep.dtype == torch.bool else keep).to(device)


def _head(seq, z, masks, owner):
    """Sequential(Linear, Normalize, PReLU, Dropout) with the dropout's mask, when it is active, taken from the front of
    `masks` (bool [n, hidden]) or, without masks, drawn from `owner`'s counter."""
    z = seq[2](seq[1](seq[0](z)))
    p = float(seq[3].p)
    if not seq[3].training or p == 0.0:
        return z
    keep = masks.pop(0) if masks is not None else _draw_keep(owner, z.numel(), p, z.device)
    return z * torch.as_tensor(keep).to(z.device).reshape(z.shape).to(z.dtype) / (1.0 - p)


class GConv(nn.Module):
    """bgrl_g2l.py:508-531 with the reference's constructor; `forward(x, edge_index)` -> (z, projection_head(z))."""

    def __init__(self, input_dim, hidden_dim, num_layers, dropout, activation, encoder_norm="batch", projector_norm="batch",
                 seed=0):
        super().__init__()
        self.activation = activation
        self.dropout = dropout
        self.layers = nn.ModuleList([make_gin_conv(input_dim, hidden_dim)] +
                                    [make_gin_conv(hidden_dim, hidden_dim) for _ in range(num_layers - 1)])
        self.batch_norm = Normalize(hidden_dim, encoder_norm)
        self.projection_head = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), Normalize(hidden_dim, projector_norm), nn.PReLU(),
                                             nn.Dropout(dropout))
        self.seed, self.calls = int(seed), 0
        self._graph_key, self._graph, self._graph_src = None, None, None

    def prepare(self, edge_index, num_nodes):
        """Builds (or returns the cached) `functional.gin_sum_graph` of `edge_index` int64 [2, E].  The cache is keyed on
        the tensor's address, shape and version counter (and num_nodes) and holds the tensor, so a new tensor or an in-place
        edit rebuilds the graph.  An edit through `.data` or a numpy alias moves neither the address nor the version and is
        NOT seen: pass a new tensor (or edit in place through torch) instead."""
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, int(num_nodes))
        if self._graph_key != key:
            self._graph = Fn.gin_sum_graph(edge_index, num_nodes, self.layers[0].nn[0].weight.device)
            self._graph_key = key
            self._graph_src = edge_index            # holding edge_index keeps the pointer from being recycled
        return self._graph

    def __deepcopy__(self, memo):
        """The target encoder's copy (Encoder.get_target_encoder) shares no graph: the cache stays with the original."""
        cache = self._graph_key, self._graph, self._graph_src
        self._graph_key, self._graph, self._graph_src = None, None, None
        try:
            new = self.__class__.__new__(self.__class__)
            memo[id(self)] = new
            new.__dict__ = copy.deepcopy(self.__dict__, memo)
        finally:
            self._graph_key, self._graph, self._graph_src = cache
        return new

    def forward(self, x, edge_index, edge_weight=None, masks=None, edge_keep=(None, None)):
        """edge_weight is ignored (the reference hands it to GINConv as `size`).  masks (the pins' recorded draws): a list
        that is consumed from the front, one keep mask per dropout that is active (training, p > 0) in call order -- the
        layers', then the projection head's -- each bool [n, hidden] or (layers only) a packed bitmap in
        `functional.gin_layer`'s order, instead of a draw.  edge_keep: EdgeRemoving's (keep_bits, keep_bits_t)."""
        graph = edge_index if isinstance(edge_index, CsrGraph) else self.prepare(edge_index, x.shape[0])
        p = float(self.dropout) if self.training else 0.0
        z = x
        for conv in self.layers:
            self.activation = nn.ReLU()             # bgrl_g2l.py:526: whatever was configured, the layer's kernel applies ReLU
            keep = None
            if p > 0.0:
                count = x.shape[0] * conv.nn[2].out_features
                keep = _as_bits(masks.pop(0), z.device) if masks is not None else _draw_bits(self, count, p, z.device)
            z = conv(z, graph, keep, p, *edge_keep)
        z = self.batch_norm(z)
        return z, _head(self.projection_head, z, masks, self)


class Encoder(nn.Module):
    """bgrl_g2l.py:534-572.  augmentor: ((edge_p, feat_p), (edge_p, feat_p)), the two views' Compose([EdgeRemoving(pe),
    FeatureMasking(pf)])."""

    def __init__(self, encoder, augmentor, hidden_dim, dropout=0.2, predictor_norm="batch", seed=0):
        super().__init__()
        self.online_encoder = encoder
        self.augmentor = augmentor
        self.target_encoder = None
        self.predictor = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), Normalize(hidden_dim, predictor_norm), nn.PReLU(),
                                       nn.Dropout(dropout))
        self.seed, self.calls = int(seed) + 0x5851F42D, 0

    def get_target_encoder(self):
        if self.target_encoder is None:
            self.target_encoder = copy.deepcopy(self.online_encoder)
            self.target_encoder.seed = self.online_encoder.seed + 0x2545F491       # its own dropout draws
            for p in self.target_encoder.parameters():
                p.requires_grad = False
        return self.target_encoder

    def update_target_encoder(self, momentum=0.99):
        for p, new_p in zip(self.get_target_encoder().parameters(), self.online_encoder.parameters()):
            p.data = momentum * p.data + (1 - momentum) * new_p.data

    def _augment(self, x, graph, view, masks):
        """(x_v, (keep_bits, keep_bits_t)) of one view: EdgeRemoving's mask, one draw per edge of edge_index shared by the
        entry orders of A and A^T, and FeatureMasking's column mask."""
        pe, pf = self.augmentor[view]
        edge_keep = (None, None)
        if masks is not None and masks.get("edge") is not None:
            edge_keep = Fn.gin_edge_keep_bits(graph, masks["edge"][view])
        elif pe > 0.0:
            if graph.device.type == "cuda":
                self.calls += 1
                key = (self.seed * 0x9E3779B97F4A7C15 + self.calls) & MASK64
                edge_keep = tuple(Fn.edge_mask_bits(g.nnz, pe, key, g.device, edge_id=g.edge_of_entry) for g in (graph, graph.t))
            else:
                edge_keep = Fn.gin_edge_keep_bits(graph, _draw_keep(self, graph.nnz, pe, "cpu"))
        if masks is not None and masks.get("feat") is not None:
            keep = torch.as_tensor(masks["feat"][view]).to(x.device)
        elif pf > 0.0:
            keep = _draw_keep(self, x.shape[1], pf, x.device)
        else:
            return x, edge_keep
        if x.is_cuda and x.dtype == torch.float32:
            return Fn.feature_masking(x, pf, 0, keep_bits=_as_bits(keep, x.device))[0], edge_keep
        return x * keep.to(x.dtype), edge_keep

    def forward(self, x, edge_index, edge_weight=None, batch=None, masks=None):
        """masks (the pins' recorded draws), a dict: edge [2] bool [E] in edge_index order, feat [2] bool [hidden] (either may be None: drawn), node: the
        keep masks bool [n, hidden] of the dropouts that are active, in the order they are used below (online view 1: the
        layers then the head; online view 2; predictor view 1, view 2; target view 1; target view 2)."""
        online = self.online_encoder
        graph = edge_index if isinstance(edge_index, CsrGraph) else online.prepare(edge_index, x.shape[0])
        (x1, ek1), (x2, ek2) = self._augment(x, graph, 0, masks), self._augment(x, graph, 1, masks)
        node = None if masks is None or masks.get("node") is None else list(masks["node"])
        h1, h1_online = online(x1, graph, None, node, ek1)
        h2, h2_online = online(x2, graph, None, node, ek2)
        g1 = h1.sum(dim=0, keepdim=True)            # global_add_pool over one graph; unused, as in the reference
        g2 = h2.sum(dim=0, keepdim=True)
        h1_pred = _head(self.predictor, h1_online, node, self)
        h2_pred = _head(self.predictor, h2_online, node, self)
        with torch.no_grad():
            target = self.get_target_encoder()
            _, h1_target = target(x1, graph, None, node, ek1)
            _, h2_target = target(x2, graph, None, node, ek2)
            g1_target = h1_target.sum(dim=0, keepdim=True)
            g2_target = h2_target.sum(dim=0, keepdim=True)
        assert not node, "more recorded masks than active dropouts"
        return g1, g2, h1_pred, h2_pred, g1_target, g2_target


class BootstrapLatent:
    """bgrl_g2l.py:436-446."""

    def compute(self, anchor, sample, pos_mask=None, neg_mask=None, *args, **kwargs):
        anchor = F.normalize(anchor, dim=-1)
        sample = F.normalize(sample, dim=-1)
        loss = 2 - 2 * (sample * anchor).sum(dim=-1)
        return loss.mean()

    __call__ = compute


class BootstrapContrast(nn.Module):
    """bgrl_g2l.py:277-308: 'L2L', 'G2G' (same-scale pairs) and 'G2L' for a single graph (:297-300); the multi-graph G2L
    sampler is out of scope (the reference's data is one graph)."""

    def __init__(self, loss, mode="L2L"):
        super().__init__()
        if mode not in ("L2L", "G2G", "G2L"):
            raise RuntimeError(f"unsupported mode: {mode}")
        self.loss, self.mode = loss, mode

    def forward(self, h1_pred=None, h2_pred=None, h1_target=None, h2_target=None, g1_pred=None, g2_pred=None, g1_target=None,
                g2_target=None, batch=None, extra_pos_mask=None):
        if extra_pos_mask is not None:
            raise NotImplementedError("extra_pos_mask: BootstrapLatent does not read its masks")
        if self.mode == "L2L":
            pairs = ((h1_target, h2_pred), (h2_target, h1_pred))
        elif self.mode == "G2G":
            pairs = ((g1_target, g2_pred), (g2_target, g1_pred))
        else:
            if batch is not None and int(batch.max().item()) + 1 > 1:
                raise NotImplementedError("G2L over several graphs")
            pairs = ((g1_target, h2_pred), (g2_target, h1_pred))
        assert all(v is not None for pair in pairs for v in pair)
        l1, l2 = (self.loss(anchor=a, sample=s) for a, s in pairs)
        return (l1 + l2) * 0.5


def bipartite_edge_index(uid, iid, num_users):
    """bgrl_g2l.py:106-123: (u, i + U) and (i + U, u) of every training pair, interleaved in the pairs' order; int64 [2, 2 E]."""
    u, i = torch.as_tensor(uid, dtype=torch.int64), torch.as_tensor(iid, dtype=torch.int64) + num_users
    return torch.stack([torch.stack([u, i], 1).reshape(-1), torch.stack([i, u], 1).reshape(-1)])


class BGRLModel(RankingModel):
    DEFAULTS = dict(hidden_dim=32, num_layers=2, dropout=0.2, lr=1e-2, batch_size=128, edge_p=0.2, feat_p=0.1, momentum=0.99,
                    weight_decay=1e-5, activation=nn.ReLU)                # bgrl_g2l.py:622-633

    def __init__(self, config, train_set, test_set, x=None, device=None, seed=0, dtype=torch.float32):
        """config: bgrl_g2l.py:622-633's keys (missing ones take its defaults) and `item.ranking.topN` ([10, 20, 30, 50]).
        x: the node table [U + I, hidden_dim] (bgrl_g2l.py:125-126), a randn draw from the seed when None; not a parameter.
        seed: the table, initial weights and every mask draw are functions of it.  train_set: the list of triples, or a
        prepared data object carrying `uid`, `iid` (dense ids of the training pairs), `user_num` and `item_num`.  dtype and a
        CPU device select the composed layer and torch's Adam (the float64 pins); the HIP path is float32 on the GPU."""
        self.config, self.seed = {**self.DEFAULTS, **config}, int(seed)
        c = self.config
        self._read_topn(c)
        self.device = default_device(device)
        self.data = train_set if is_prepared(train_set, "uid") else Interaction(c, train_set, test_set, device=self.device)
        nu, ni, hid = self.data.user_num, self.data.item_num, int(c["hidden_dim"])
        self.edge_index = bipartite_edge_index(self.data.uid, self.data.iid, nu).to(self.device)
        with seeded(self.seed, self.device):
            if x is None:
                x = torch.randn(nu + ni, hid)
            gconv = GConv(hid, hid, int(c["num_layers"]), c["dropout"], c["activation"], seed=self.seed)
            aug = ((c["edge_p"], c["feat_p"]), (c["edge_p"], c["feat_p"]))
            self.encoder = Encoder(gconv, aug, hid, seed=self.seed).to(device=self.device, dtype=dtype)
        self.contrast = BootstrapContrast(BootstrapLatent(), mode="G2L")
        self.x = torch.as_tensor(x).to(device=self.device, dtype=dtype).contiguous()
        params = list(self.encoder.parameters())    # the online encoder and the predictor: the target does not exist yet
        hip = self.device.type == "cuda" and dtype == torch.float32
        self.optimizer = (FusedAdam if hip else torch.optim.Adam)(params, lr=c["lr"], weight_decay=c["weight_decay"])
        self.maxEpoch = N_EPOCHS
        self.bestPerformance = []

    def losses(self, masks=None):
        """bgrl_g2l.py:578-579 on the full batch."""
        _, _, h1_pred, h2_pred, g1_target, g2_target = self.encoder(self.x, self.edge_index, masks=masks)
        return (self.contrast(h1_pred=h1_pred, h2_pred=h2_pred, g1_target=g1_target.detach(), g2_target=g2_target.detach()),)

    def train_step(self, masks=None):
        """One call of bgrl_g2l.py:575-583; masks: `Encoder.forward`'s."""
        self.__dict__.pop("Z", None)
        self.encoder.train()
        out = self._optimise(masks)
        self.encoder.update_target_encoder()        # the default momentum, not the configuration's (bgrl_g2l.py:582)
        return out

    def train(self):
        """main's loop body (bgrl_g2l.py:664-673): one epoch of one full-batch step, then the metrics of the eval-mode online
        encoder."""
        for _ in range(self.maxEpoch):
            self.train_step()
        return self.evaluate()

    def _final(self):
        if not hasattr(self, "Z"):
            self.encoder.eval()                     # bgrl_g2l.py:157-159
            with torch.no_grad():
                self.Z, _ = self.encoder.online_encoder(self.x, self.edge_index)
        nu = self.data.user_num
        return self.Z[:nu].contiguous(), self.Z[nu:].contiguous()

    def predict(self, raw_user_id):
        """bgrl_g2l.py:160-164: item_embs @ user_emb."""
        return self.predict_item_major(raw_user_id)

    def load_reference_state(self, state):
        """Loads a reference `Encoder.state_dict()` (names as bgrl_g2l.py builds them; PyG's `eps` buffers and BatchNorm's
        `num_batches_tracked` counters may be present or absent).  A state with `target_encoder.*` entries creates the target encoder first."""
        state = {k: torch.as_tensor(v) for k, v in state.items()}
        if any(k.startswith("target_encoder.") for k in state):
            self.encoder.get_target_encoder()
        own = self.encoder.state_dict()
        optional = (".eps", ".num_batches_tracked")                     # PyG's buffer; BatchNorm's counter (momentum is fixed)
        state = {k: v for k, v in state.items() if k in own or not k.endswith(optional)}
        missing = [k for k in own if k not in state and not k.endswith(optional)]
        unexpected = [k for k in state if k not in own]
        if missing or unexpected:
            raise KeyError(f"reference state: missing {missing}, unexpected {unexpected}")
        self.encoder.load_state_dict(state, strict=False)
        self.__dict__.pop("Z", None)
