"""What the BGRL / GIN tests and the writer of tests/golden/bgrl_steps.npz (scripts/gen_golden_bgrl_steps.py) share: the
comparison rule, the float64 restatement of one layer, the case builders, the tile and cap constants of csrc/gcr_gin.hip
and the fixture's key layout.

The rule, the project's (tests/sage_rules.py `check`):  err / S <= max(4 x drift, 2^-20)  and  err / S <= 1e-5,
S = max |f64|, drift = the float32 error of the SAME float64 source.  Training steps are held to tests/step_pins.py's rules
(`check_steps`: `term_tol` with the float32 run for the loss, `atol_floor_1` for a final parameter or BatchNorm buffer,
`has_moved` and `sees_dropped` for what the tolerance sees).

The layer, bgrl_g2l.py:525-529 over torch_geometric's GINConv(Sequential(Linear, ReLU, Linear)) with eps = 0, for edges
j -> i (src, dst), duplicates and self loops counted as they come, an edge kept where `edge_keep` says so:
    s_i = (1 + eps) x_i + sum over the kept edges into i of x_j;   pre1 = s w1^T + b1;   t = relu(pre1);
    pre2 = t w2^T + b2;   h = relu(pre2) * keep / (1 - p).
`restatement` runs these in a given dtype under autograd.  ReLU has a kink at zero, so a margin case is drawn until every
float64 pre-activation of BOTH ReLUs keeps 8 x the float32 error from zero (`margin_case`, sage_rules.has_margin).  A
launch with millions of pre-activations has no such seed, and zeroing g where the outer mask is ambiguous
(sage_rules.large_case) cannot reach the inner ReLU; the large cases are therefore `exact_case`s: small integers, where
every product and every partial sum in any order is a float32, both kinks are unambiguous (an argument of exactly 0 has
gradient 0, as torch's ReLU gives it) and the kernels owe float64's every bit.  `exact_bounds` is the proof, from sums of
absolute values.  tests/test_gin_cpu.py asserts each builder's conditions."""
import functools
import os

import numpy as np
import torch

import sage_rules as sr
import step_pins as sp

FLOOR, NORTH_STAR = sr.FLOOR, sr.NORTH_STAR
KEYS = ("h", "dx", "dw1", "db1", "dw2", "db2")
WIDTHS = (32, 64, 128)
PAIRS = tuple((a, b) for a in WIDTHS for b in WIDTHS)          # every (din, dout) the kernels serve
DEGREES = sr.DEGREES                                           # a node's in-degree cycle: none, one, a few, many
SENTINEL = sr.SENTINEL
EXACT_LIMIT = 2.0 ** 24                                        # integers below it are float32s
STORED_F32 = 2.0 ** -23                                        # a float64 result stored as float32: 2^-24 of its scale, twice over

# ---- csrc/gcr_gin.hip's launch shapes ----
FWD_CAP, BWD_CAP, BWD_ROWS = 1024, 512, 32


def fwd_rows(dout):
    return 64 if dout <= 64 else 32


def w_in_lds(din, dout):
    return (din + dout) * dout <= 8192


def fwd_class(din, dout):
    return fwd_rows(dout), w_in_lds(din, dout)


def bwd_class(din, dout):
    return BWD_ROWS, w_in_lds(din, dout)


def workspace_words(n, din, dout):
    w = (din + dout) * dout
    return w + min(-(-n // BWD_ROWS), BWD_CAP) * (w + 2 * dout)


# One pair per distinct (tile rows, weights in LDS) class of the forward: (64, yes) (32, 32); (64, no) (128, 64);
# (32, no) (32, 128) -- there is no (32, yes): dout = 128 never fits.  The backward's classes (32, yes) and (32, no) are both
# among them.  n = cap x tile rows + 1 is the smallest n at which workgroup 0 takes a second trip (its tile holds one row);
# n - 1 gives exactly one tile per workgroup.  The forward's n is past the backward's 512 x 32 + 1 = 16385 for every class,
# so each case is multi-trip in both launches; BWD_TRIP_SHAPES adds the backward's own threshold.
FWD_TRIP_PAIRS = ((32, 32), (128, 64), (32, 128))
FWD_TRIP_SHAPES = tuple((FWD_CAP * fwd_rows(b) + 1, a, b) for a, b in FWD_TRIP_PAIRS)
BWD_TRIP_PAIRS = ((64, 64), (64, 128))
BWD_TRIP_SHAPES = tuple((BWD_CAP * BWD_ROWS + 1, a, b) for a, b in BWD_TRIP_PAIRS)
# Hub rows (sage_rules.HUB_N's reasoning): the SpMM's windowed plan exists and is used at d = 64 for a table of 65537 rows
HUB_N, HUB_PAIRS = sr.HUB_N, ((64, 32), (64, 128))
COMP_N, COMP_P, COMP_EDGE_P = 12, 0.5, 0.3                     # the fixture's layer cases
COMP_CASES = ((32, 64), (64, 32), (128, 128))
STEP_CASES = ("A", "B", "C")
GOLDEN = os.path.join(sp.GOLDEN, "bgrl_steps.npz")


def check(got, ref, drift, tag):
    """drift: relative to the scale, per key."""
    lines, bad = [], []
    for k, want in ref.items():
        scale = float(np.abs(want).max()) or 1.0
        err = float(np.abs(np.asarray(got[k], dtype=np.float64) - want).max()) / scale
        bound = max(4.0 * drift[k], FLOOR)
        lines.append(f"GIN {tag} {k}: err/S {err:.3g} bound {bound:.3g} (drift {drift[k]:.3g}, S {scale:.3g})")
        if not (np.isfinite(got[k]).all() and err <= bound and err <= NORTH_STAR):
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


drift_of, has_margin, margin_of, checksum = sr.drift_of, sr.has_margin, sr.margin_of, sr.checksum


def relu(v):
    return torch.where(v > 0, v, torch.zeros_like(v))


def sum_rows(src, dst, n, xt, edge_keep=None):
    """sum over the (kept) edges into each node of x_j, in xt's dtype."""
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    msg = xt[s]
    if edge_keep is not None:
        msg = msg * torch.from_numpy(edge_keep).to(xt.dtype)[:, None]
    return torch.zeros(n, xt.shape[1], dtype=xt.dtype).index_add_(0, d, msg)


def restatement(src, dst, n, x, w1, b1, w2, b2, g, dtype, keep=None, p=0.0, edge_keep=None, eps=0.0, root=True):
    """(dict of h, dx, dw1, db1, dw2, db2; (pre1, pre2)), float64 arrays computed in `dtype`.  keep: bool [n, dout] or
    None; edge_keep: bool [E] or None.  root=False drops the (1 + eps) x term (what the step fixture's sensitivity run
    drops)."""
    xt, t1, c1, t2, c2 = (torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (x, w1, b1, w2, b2))
    s = sum_rows(src, dst, n, xt, edge_keep)
    if root:
        s = s + (1.0 + eps) * xt
    pre1 = s @ t1.T + c1
    pre2 = relu(pre1) @ t2.T + c2
    h = relu(pre2)
    if keep is not None:
        h = h * torch.from_numpy(keep).to(dtype) / (1.0 - p)
    h.backward(torch.from_numpy(g).to(dtype))
    res = dict(h=h.detach(), dx=xt.grad, dw1=t1.grad, db1=c1.grad, dw2=t2.grad, db2=c2.grad)
    return {k: v.double().numpy() for k, v in res.items()}, (pre1.detach().double().numpy(), pre2.detach().double().numpy())


sweep_graph, hub_graph, hub_nodes, out_isolated, keep_mask = sr.sweep_graph, sr.hub_graph, sr.hub_nodes, sr.out_isolated, sr.keep_mask


def edge_mask(n_edges, p, seed):
    """bool [E], `rand >= p` as dropout_adj keeps; None at p = 0."""
    return None if p == 0.0 else np.random.default_rng([n_edges, seed, 55]).random(n_edges) >= p


def inputs(n, din, dout, seed):
    """x ~ N(0, 1) [n, din], w1, b1 ~ U(+-1 / sqrt(din)), w2, b2 ~ U(+-1 / sqrt(dout)), g ~ N(0, 1) [n, dout]."""
    rng = np.random.default_rng([n, din, dout, seed, 9])
    a, b = 1.0 / np.sqrt(din), 1.0 / np.sqrt(dout)
    x = rng.standard_normal((n, din)).astype(np.float32)
    w1, b1 = rng.uniform(-a, a, (dout, din)).astype(np.float32), rng.uniform(-a, a, dout).astype(np.float32)
    w2, b2 = rng.uniform(-b, b, (dout, dout)).astype(np.float32), rng.uniform(-b, b, dout).astype(np.float32)
    g = rng.standard_normal((n, dout)).astype(np.float32)
    return x, w1, b1, w2, b2, g


def _case(src, dst, n, din, dout, p, seed, x, w1, b1, w2, b2, g, keep, edge_keep):
    args = (src, dst, n, x, w1, b1, w2, b2, g)
    ref, pre = restatement(*args, torch.float64, keep, p, edge_keep)
    f32, pre32 = restatement(*args, torch.float32, keep, p, edge_keep)
    return dict(src=src, dst=dst, n=n, din=din, dout=dout, p=p, seed=seed, x=x, w1=w1, b1=b1, w2=w2, b2=b2, g=g, keep=keep,
                edge_keep=edge_keep, ref=ref, f32=f32, pre=pre, pre32=pre32, drift=drift_of(f32, ref))


@functools.lru_cache(maxsize=None)
def margin_case(n, din, dout, p=0.0, edge_p=0.0, seeds=200):
    """A case on `sweep_graph(n)`: the first seed's inputs whose pre-activations of both ReLUs keep the margin, with ref
    (float64) and drift; shared among the tests that need it and never written to."""
    src, dst = sweep_graph(n)
    for seed in range(seeds):
        case = _case(src, dst, n, din, dout, p, seed, *inputs(n, din, dout, seed), keep_mask(n, dout, p, seed),
                     edge_mask(src.size, edge_p, seed))
        if all(has_margin(a, b) for a, b in zip(case["pre"], case["pre32"])):
            return case
    raise AssertionError("no seed with a margin at both ReLUs")


def _banded(rng, rows, cols):
    """[rows, cols] with entries +-1 at (k, k % cols) and (k, (k + 1) % cols), zero elsewhere: two non-zeros per row and at
    most 2 ceil(rows / cols) per column, so that no sum of a product grows with the width."""
    w = np.zeros((rows, cols), dtype=np.float32)
    k = np.arange(rows)
    w[k, k % cols] = rng.choice(np.float32([-1, 1]), rows)
    w[k, (k + 1) % cols] = rng.choice(np.float32([-1, 1]), rows)
    return w


def exact_bounds(case):
    """{name: the largest sum of absolute values behind any element of that intermediate or output}: below EXACT_LIMIT
    every partial sum, in any order, is an integer that float32 holds (the inputs are integers, the keep scale a power of
    two)."""
    n, src, dst = case["n"], case["src"], case["dst"]
    a = {k: np.abs(case[k]).astype(np.float64) for k in ("x", "w1", "b1", "w2", "b2", "g")}
    ek = np.ones(src.size) if case["edge_keep"] is None else case["edge_keep"].astype(np.float64)
    scale = 1.0 if case["keep"] is None else 1.0 / (1.0 - case["p"])
    s = a["x"].copy()
    np.add.at(s, dst, a["x"][src] * ek[:, None])
    t = s @ a["w1"].T + a["b1"]
    h = (t @ a["w2"].T + a["b2"]) * scale
    m = a["g"] * scale
    u = m @ a["w2"]
    ds = u @ a["w1"]
    dx = ds.copy()
    np.add.at(dx, src, ds[dst] * ek[:, None])
    out = dict(s=s, t=t, h=h, u=u, ds=ds, dx=dx, dw2=m.T @ t, db2=m.sum(0), dw1=u.T @ s, db1=u.sum(0))
    return {k: float(v.max()) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def exact_case(n, din, dout, dense=False, graph=sweep_graph, edge_p=0.5):
    """A case in which float32 is exact (`exact_bounds` < EXACT_LIMIT, asserted): x in {-1, 0, 1} (dense: -2 .. 2), w1 and w2
    banded +-1 (`_banded`; dense: every entry in {-1, 0, 1}), biases in {-1, 0, 1}, g in {-1, 1} (dense: {-2, -1, 1, 2}; never
    zero), a dropout mask with p = 0.5 (scale 2) and an edge mask with p = edge_p.  Row `zero_col` of w1 and its bias entry are
    zero, so column zero_col of pre1 is exactly 0 under a non-zero upstream gradient, and so is column zero_col + 1 of pre2
    (w2's row and b2's entry zero): torch's ReLU gives such an element gradient 0.  dense is for small n only."""
    rng = np.random.default_rng([n, din, dout, int(dense)])
    src, dst = graph(n)
    if dense:
        x = rng.integers(-2, 3, (n, din)).astype(np.float32)
        w1, w2 = rng.integers(-1, 2, (dout, din)).astype(np.float32), rng.integers(-1, 2, (dout, dout)).astype(np.float32)
        g = rng.choice(np.float32([-2, -1, 1, 2]), (n, dout))
    else:
        x = rng.integers(-1, 2, (n, din)).astype(np.float32)
        w1, w2 = _banded(rng, dout, din), _banded(rng, dout, dout)
        g = rng.choice(np.float32([-1, 1]), (n, dout))
    b1, b2 = (rng.integers(-1, 2, dout).astype(np.float32) for _ in range(2))
    zero_col = dout // 2 + 1
    w1[zero_col], b1[zero_col] = 0.0, 0.0
    w2[zero_col + 1], b2[zero_col + 1] = 0.0, 0.0
    case = _case(src, dst, n, din, dout, 0.5, 0, x, w1, b1, w2, b2, g, keep_mask(n, dout, 0.5, 0), edge_mask(src.size, edge_p, 0))
    case["zero_col"], case["bounds"] = zero_col, exact_bounds(case)
    worst = max(case["bounds"].values())
    assert worst < EXACT_LIMIT, f"exact_case({n}, {din}, {dout}): a sum may reach {worst:.3g}"
    return case


def assert_exact(got, ref, tag):
    """Every element equal; the first differing index otherwise."""
    for k, want in ref.items():
        have = np.asarray(got[k], dtype=np.float64)
        assert have.shape == want.shape, (tag, k, have.shape, want.shape)
        if not np.array_equal(have, want):
            at = tuple(int(v) for v in np.argwhere(have != want)[0])
            raise AssertionError(f"GIN exact {tag} {k}: {int((have != want).sum())} of {want.size} elements differ, the first "
                                 f"at {at}: got {have[at]!r}, float64 {want[at]!r}")


# ---- the device side ----

def device_graph(src, dst, n, device="cuda"):
    from recommendation_amd import functional as Fn
    return Fn.gin_sum_graph(torch.from_numpy(np.stack([src, dst])), n, device)


def packed(keep, device="cuda"):
    from recommendation_amd import functional as Fn
    return None if keep is None else Fn.pack_bits(torch.from_numpy(keep.reshape(-1))).to(device)


def edge_bits(graph, edge_keep):
    from recommendation_amd import functional as Fn
    return (None, None) if edge_keep is None else Fn.gin_edge_keep_bits(graph, torch.from_numpy(edge_keep))


def is_fused(h):
    return h.grad_fn is not None and type(h.grad_fn).__name__.startswith("_GinLayer")


def no_fused_node_below(h):
    """Walks the autograd graph under h: the fused node is nowhere in it."""
    todo, seen = [h.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is not None and f not in seen:
            seen.add(f)
            if type(f).__name__.startswith("_GinLayer"):
                return False
            todo += [nf for nf, _ in f.next_functions]
    return h.grad_fn is not None


PARAMS = ("w1", "b1", "w2", "b2")


def layer(graph, case, device="cuda", fused=True, fn=None, dtype=torch.float32, want_dx=True, tensors=None):
    """h, dx, dw1, db1, dw2, db2 of functional.gin_layer (or `fn`) for a case, as arrays; with `fused` the node must be the
    fused one, without it the node must be nowhere below h.  tensors: given in place of the case's (x, w1, b1, w2, b2, g)."""
    from recommendation_amd import functional as Fn
    t = {k: torch.from_numpy(case[k]).to(device=device, dtype=dtype).requires_grad_(k != "x" or want_dx) for k in ("x",) + PARAMS}
    t["g"] = torch.from_numpy(case["g"]).to(device=device, dtype=dtype)
    t.update(tensors or {})
    bits, bits_t = edge_bits(graph, case["edge_keep"])
    h = (fn or Fn.gin_layer)(graph, t["x"], t["w1"], t["b1"], t["w2"], t["b2"], 0.0, packed(case["keep"], device), case["p"],
                             bits, bits_t)
    if fused:
        assert is_fused(h), "the fused node must run"
    else:
        assert no_fused_node_below(h), "the composed layer must run"
    h.backward(t["g"])
    res = dict(h=h.detach(), **{"d" + k: t[k].grad for k in PARAMS})
    if want_dx:
        res["dx"] = t["x"].grad
    return {k: v.cpu().numpy() for k, v in res.items()}


class Raw:
    """The arguments of gcr_gin_fwd_f32 / gcr_gin_bwd_f32 for n rows of (din, dout), every buffer its own, the workspace of
    the size gcr_gin_workspace_bytes gives.  fill (the bounds tests): every output and the workspace hold that value, h and
    ds over pad_rows more rows and the workspace over pad_words more words than the call is told of."""

    def __init__(self, n=40, din=64, dout=64, fill=None, pad_rows=0, pad_words=0):
        from recommendation_amd import _lib
        self.lib, self.n, self.din, self.dout = _lib, n, din, dout
        f = functools.partial(torch.randn, device="cuda")
        self.s, self.g = f(n, din), f(n, dout)
        self.w1, self.b1, self.w2, self.b2 = f(dout, din), f(dout), f(dout, dout), f(dout)
        out = functools.partial(torch.full, fill_value=0.0 if fill is None else fill, device="cuda")
        self.h, self.ds = out((n + pad_rows, dout)), out((n + pad_rows, din))
        grad = functools.partial(torch.full, fill_value=1.0 if fill is None else fill, device="cuda")
        self.dw1, self.db1, self.dw2, self.db2 = grad((dout, din)), grad((dout,)), grad((dout, dout)), grad((dout,))
        self.ws_words = int(_lib.call("gcr_gin_workspace_bytes", max(n, 1), din, dout)) // 4
        self.ws = torch.empty(max(self.ws_words, 1) + pad_words, device="cuda")
        if fill is not None:
            self.ws.fill_(fill)

    def fwd(self, **kw):
        a = dict(n=self.n, s=self.s, w1=self.w1, b1=self.b1, w2=self.w2, b2=self.b2, din=self.din, dout=self.dout, keep=None,
                 scale=1.0, h=self.h, ws=self.ws)
        a.update(kw)
        self.lib.call("gcr_gin_fwd_f32", a["n"], a["s"], a["w1"], a["b1"], a["w2"], a["b2"], a["din"], a["dout"], a["keep"],
                      a["scale"], a["h"], a["ws"], on=self.g)

    def bwd(self, **kw):
        a = dict(n=self.n, s=self.s, w1=self.w1, b1=self.b1, w2=self.w2, h=self.h, g=self.g, din=self.din, dout=self.dout,
                 scale=1.0, ds=self.ds, dw1=self.dw1, db1=self.db1, dw2=self.dw2, db2=self.db2, ws=self.ws)
        a.update(kw)
        self.lib.call("gcr_gin_bwd_f32", a["n"], a["s"], a["w1"], a["b1"], a["w2"], a["h"], a["g"], a["din"], a["dout"],
                      a["scale"], a["ds"], a["dw1"], a["db1"], a["dw2"], a["db2"], a["ws"], on=self.g)


# ---- the fixture's layout ----

def load():
    return np.load(GOLDEN, allow_pickle=False)


def comp_prefix(din, dout):
    return f"comp/{din}x{dout}/"


def component(g, din, dout):
    """One layer case of the fixture as `margin_case`'s dict: the inputs redrawn from the stored seed (and checked against
    the writer's checksum), ref = the reference stand-in's float64 run (stored as float32 of it) and the float32 run's
    drift."""
    pre = comp_prefix(din, dout)
    src, dst = g["comp/src"].astype(np.int64), g["comp/dst"].astype(np.int64)
    seed = int(g[pre + "seed"])
    x, w1, b1, w2, b2, gr = inputs(COMP_N, din, dout, seed)
    keep, ek = keep_mask(COMP_N, dout, COMP_P, seed), edge_mask(src.size, COMP_EDGE_P, seed)
    assert abs(checksum(x, w1, b1, w2, b2, gr, keep, ek) - float(g[pre + "checksum"])) < 1e-6, "the inputs' streams changed"
    return dict(src=src, dst=dst, n=COMP_N, din=din, dout=dout, p=COMP_P, seed=seed, x=x, w1=w1, b1=b1, w2=w2, b2=b2, g=gr,
                keep=keep, edge_keep=ek, ref={k: g[pre + k].astype(np.float64) for k in KEYS},
                drift={k: float(g[pre + "drift/" + k]) for k in KEYS})


# ---- training steps: step_pins' rules on the fixture's step cases ----

CONFIG_INTS, CONFIG_FLOATS = ("hidden_dim", "num_layers"), ("dropout", "lr", "edge_p", "feat_p", "weight_decay")
# What the loss does not reach: a constant column shift in front of a BatchNorm is removed by it, so the bias of a Linear
# that feeds one (the head's and the predictor's first), and the encoder BatchNorm's own bias (a constant shift of z, which
# only the head's Linear -> BatchNorm reads: the pooled g1, g2 of the online side are unused), have gradient zero in exact
# arithmetic.  What they get is rounding noise, which Adam's normalisation turns into steps of its own size in float32 and
# into nothing in float64; neither `has_moved` nor `sees_dropped` can be asked of them.  They are still compared, under the
# same atol from the reference's own float32 slack.  The running mean of the BatchNorm behind such a Linear carries its bias
# and with it the noise, so it is treated alike.
UNREACHED = ("projection_head.0.bias", "predictor.0.bias", "batch_norm.norm.bias", "projection_head.1.norm.running_mean",
             "predictor.1.norm.running_mean")


def step_config(g, case):
    pre = f"{case}/"
    cfg = {k: int(g[pre + k]) for k in CONFIG_INTS}
    cfg.update({k: float(g[pre + k]) for k in CONFIG_FLOATS})
    return cfg


def _gconv_shapes(cfg, prefix, buffers):
    hid, out = int(cfg["hidden_dim"]), {}
    for k in range(int(cfg["num_layers"])):
        for j in (0, 2):
            out[f"{prefix}layers.{k}.nn.{j}.weight"], out[f"{prefix}layers.{k}.nn.{j}.bias"] = (hid, hid), (hid,)
    out.update(_norm_shapes(f"{prefix}batch_norm.norm.", hid, buffers))
    out.update(_head_shapes(f"{prefix}projection_head.", hid, buffers))
    return out


def _norm_shapes(prefix, hid, buffers):
    names = ("weight", "bias") + (("running_mean", "running_var") if buffers else ())
    return {prefix + k: (hid,) for k in names}


def _head_shapes(prefix, hid, buffers):
    out = {prefix + "0.weight": (hid, hid), prefix + "0.bias": (hid,)}
    out.update(_norm_shapes(prefix + "1.norm.", hid, buffers))
    out[prefix + "2.weight"] = (1,)
    return out


def tensor_shapes(cfg, buffers=True):
    """{name: shape} of what a step case pins, under the reference Encoder's state_dict names: the online encoder's and the
    predictor's parameters (what the optimiser holds), the target encoder's (the EMA's), and with `buffers` the five
    BatchNorms' running statistics."""
    out = _gconv_shapes(cfg, "online_encoder.", buffers)
    out.update(_head_shapes("predictor.", int(cfg["hidden_dim"]), buffers))
    out.update(_gconv_shapes(cfg, "target_encoder.", buffers))
    return out


def is_unreached(name):
    return name.endswith(UNREACHED)


PREDICTOR_DROPOUT = 0.2             # Encoder's default: main() builds it without the argument (bgrl_g2l.py:656-659)


def n_node_masks(cfg):
    """The dropouts that draw in one training step: the layers' and the head's of four encoder passes when the
    configuration's dropout is positive, and the predictor's two."""
    return (4 * (int(cfg["num_layers"]) + 1) if cfg["dropout"] > 0 else 0) + 2


def init_arrays(cfg, n_nodes, seed):
    """The step cases' node table x ~ N(0, 1) [n, hidden] (nn.Embedding's default; bgrl_g2l.py:125-126) and the initial Linear
    parameters of the online encoder and the predictor, float32, functions of the seed (numpy's PCG64): torch.nn.Linear's
    default bounds, uniform(+-1 / sqrt(in)) for weights and biases alike.  The reference's own draws are overwritten with
    these; BatchNorm (1, 0) and PReLU (0.25) keep their constant defaults; the target encoder starts as the online one's
    copy."""
    hid = int(cfg["hidden_dim"])
    rng = np.random.default_rng([int(seed), n_nodes, hid])
    out = {"x": rng.standard_normal((n_nodes, hid)).astype(np.float32)}
    b = 1.0 / np.sqrt(hid)
    for k, shape in tensor_shapes(cfg, buffers=False).items():
        if not k.startswith("target_encoder.") and ".norm." not in k and shape != (1,):
            out[k] = rng.uniform(-b, b, shape).astype(np.float32)
    return out


def initial_tensors(cfg, init):
    """{name: float64 initial value} of every pinned tensor."""
    out = {}
    for k, shape in tensor_shapes(cfg).items():
        src = k.replace("target_encoder.", "online_encoder.")
        if src in init:
            out[k] = init[src].astype(np.float64)
        elif k.endswith(("running_mean", ".norm.bias")):
            out[k] = np.zeros(shape)
        elif k.endswith(("running_var", ".norm.weight")):
            out[k] = np.ones(shape)
        else:
            out[k] = np.full(shape, 0.25)                       # PReLU
    return out


def step_triples(g, case):
    """The case's training triples: the first `<case>/n_pairs` of the file's pairs (the writer shrinks a case until a seed
    keeps the kink margin over all its steps)."""
    k = int(g[f"{case}/n_pairs"])
    return [[int(u), int(i), 1.0] for u, i in zip(g["train_user"][:k], g["train_item"][:k])]


def n_nodes(g, case):
    return int(g[f"{case}/num_users"]) + int(g[f"{case}/num_items"])


def step_init(g, case):
    cfg = step_config(g, case)
    init = init_arrays(cfg, n_nodes(g, case), int(g[f"{case}/init_seed"]))
    assert abs(checksum(*init.values()) - float(g[f"{case}/init_checksum"])) < 1e-6, "the initial parameters' stream changed"
    return init


def step_masks(g, case, step, cfg):
    """The recorded draws of one step as `Encoder.forward(masks=)` takes them: edge [2] bool [E] in edge_index order and
    feat [2] bool [hidden] (None where the probability is 0: nothing was drawn), node: the n_node_masks(cfg) dropout keep
    masks bool [n, hidden] in the reference's call order (online view 1: L layers then the head; online view 2; predictor
    view 1, view 2; target view 1; target view 2)."""
    n, hid, n_edges = n_nodes(g, case), int(cfg["hidden_dim"]), 2 * int(g[f"{case}/n_pairs"])
    unpack = lambda a, count: np.unpackbits(a, count=count).astype(bool)                  # noqa: E731
    node = [unpack(m, n * hid).reshape(n, hid) for m in g[f"{case}/node"][step]]
    assert len(node) == n_node_masks(cfg)
    return dict(edge=[unpack(g[f"{case}/edge"][step, v], n_edges) for v in range(2)] if cfg["edge_p"] > 0 else None,
                feat=[unpack(g[f"{case}/feat"][step, v], hid) for v in range(2)] if cfg["feat_p"] > 0 else None, node=node)


def step_tables(g, case):
    """(init, {tensor: (float64 final, slack, atol, what dropping the root term moves it by)}) of a step case."""
    cfg, init, pre = step_config(g, case), step_init(g, case), f"{case}/"
    first = initial_tensors(cfg, init)
    out = {}
    for k in tensor_shapes(cfg):
        slack = float(g[f"{pre}slack/{k}"])
        out[k] = (first[k] + g[f"{pre}f64/delta/{k}"].astype(np.float64), slack, sp.atol_floor_1(slack), float(g[f"{pre}delta_root/{k}"]))
    return first, out


def assert_sensitivity(g, case):
    """The fixture's side of step_pins' rule, from stored numbers alone: the float64 run without the root term
    ((1 + eps) x_i dropped in every layer) ends more than DROPPED x atol away in every tensor the loss reaches (`UNREACHED`
    says which it does not), and every tensor moved by more than MOVED x max(slack, FLOOR)."""
    first, tables = step_tables(g, case)
    for k, (ref, slack, atol, d_root) in tables.items():
        if is_unreached(k):
            continue
        assert sp.sees_dropped(d_root, atol), (case, k, d_root, atol)
        moved = float(np.abs(ref - first[k]).max())
        assert sp.has_moved(moved, max(slack, sp.FLOOR)), (case, k, moved, slack)


def check_steps(g, case, losses, finals):
    """losses [steps]; finals: {tensor: array}.  Loss: `term_tol` with the float32 run; a final parameter or buffer:
    `atol_floor_1` of the stored float32 slack; and the tolerance sees the training (`assert_sensitivity` first, and
    `has_moved` of the model's own finals)."""
    pre = f"{case}/"
    assert_sensitivity(g, case)
    l64, l32 = g[pre + "f64/loss"], g[pre + "f32/loss"]
    tol = sp.term_tol(l64, l32)
    err = np.abs(np.asarray(losses, dtype=np.float64) - l64)
    report = [f"STEPPIN bgrl case {case}", f"  loss: max err {err.max():.3g} ({(err / tol).max():.2f} x tol)"]
    failures = [] if np.all(err <= tol) else [f"loss: got {list(losses)} reference {l64.tolist()}"]
    first, tables = step_tables(g, case)
    for k, (ref, slack, atol, d_root) in tables.items():
        got = np.asarray(finals[k], dtype=np.float64).reshape(ref.shape)
        e = float(np.abs(got - ref).max())
        moved = float(np.abs(got - first[k]).max())
        report.append(f"  {k}: max err {e:.3g} ({e / atol:.2f} x atol), atol {atol:.3g}, reference f32 slack {slack:.3g}, "
                      f"moved {moved:.3g}; dropping the root term moves it by {d_root:.3g}")
        if not (np.isfinite(got).all() and e <= atol):
            failures.append(f"{k}: max |final - f64| = {e:.3g} > atol {atol:.3g}")
        if not is_unreached(k) and not sp.has_moved(moved, max(slack, sp.FLOOR)):
            failures.append(f"{k}: moved {moved:.3g}, which the tolerance does not see")
    print("\n".join(report))
    assert not failures, "\n".join(report + failures)


def run_steps(g, case, device, dtype):
    """BGRLModel from the case's initial arrays over its recorded steps with its recorded masks -> (model, losses).  The
    configuration carries a momentum, a batch size and an activation of its own: none of them has an effect (the module
    docstring's quirks)."""
    from recommendation_amd.bgrl import BGRLModel
    cfg, init = step_config(g, case), step_init(g, case)
    model = BGRLModel(dict(cfg, momentum=0.5, batch_size=7, activation=torch.nn.PReLU), step_triples(g, case), [], x=init["x"],
                      device=device, dtype=dtype)
    assert (model.data.user_num, model.data.item_num) == (int(g[f"{case}/num_users"]), int(g[f"{case}/num_items"]))
    model.load_reference_state({k: torch.from_numpy(v) for k, v in initial_tensors(cfg, init).items()
                                if not k.startswith("target_encoder.")})
    assert model.encoder.target_encoder is None
    losses = [float(model.train_step(step_masks(g, case, step, cfg))[0]) for step in range(int(g[f"{case}/steps"]))]
    return model, losses


def finals_of(model, cfg):
    state = model.encoder.state_dict()
    return {k: state[k].detach().double().cpu().numpy() for k in tensor_shapes(cfg)}


def check_scores(g, case, got):
    """`predict` after the case's steps against the stored float64 scores.  The scores are a function of the final
    parameters, so they are held as a final table is: atol = `atol_floor_1` of the reference's own float32 slack,
    max |f32 scores - f64 scores| (stored relative to the largest float64 score).  The layer rule's 1e-5 cap cannot be asked
    here: the reference's own float32 run ends 2e-5 to 3e-4 of the scale away (the Adam steps in between)."""
    want = g[f"{case}/f64/scores"].astype(np.float64)
    slack = float(g[f"{case}/drift/scores"]) * float(np.abs(want).max())
    atol = max(sp.atol_floor_1(slack), STORED_F32 * float(np.abs(want).max()))
    err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    print(f"STEPPIN bgrl case {case} scores: max err {err:.3g} ({err / atol:.2f} x atol), atol {atol:.3g}, reference f32 slack "
          f"{slack:.3g}, largest score {np.abs(want).max():.3g}")
    assert np.shape(got) == want.shape and np.isfinite(got).all() and err <= atol, (case, err, atol)
