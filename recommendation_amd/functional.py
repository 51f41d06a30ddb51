"""Differentiable ops over libgcr (HIP kernels behind the C ABI of include/gcr.h).

Each op names the reference expression it stands in for.  Tensors must live on the GPU; a
missing/failed HIP library raises (there is deliberately no eager PyTorch fallback here).
"""
from __future__ import annotations

import torch

from . import _lib, spmm_launch
from .graph import CsrGraph

SPMM_ROW_L2NORM = 1
ROWS_MAX_D = 64            # gcr_spmm_rows_f32, the plain launch's own kernel, holds one register per lane and row; wider
                           # launches keep gcr_spmm_csr_acc2_f32
WINDOWED_MAX_D = 64        # gcr_spmm_windowed_f32, a whole windowed launch, likewise; wider ones keep spmm_parts on both plans

# bench.py sets this to a list to receive a (start, end) HIP event pair per gcr_spmm_csr_f32
# launch, recorded on the stream the kernel is launched on
EVENT_SINK = None


def _check_dense(x, n_rows, name):
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != n_rows:
        raise ValueError(f"{name} must be float32 [{n_rows}, d], got {tuple(x.shape)} {x.dtype}")
    if not (1 <= x.shape[1] <= 256):
        raise ValueError("embedding dim must be in [1, 256]")


def _check_spmm_outputs(graph, d, keep_bits, inv_norm_out, **outputs):
    """What every raw SpMM launch asks of its caller-allocated buffers: each output that is given contiguous float32
    [n_rows, d], keep_bits an int32 bitmap over the non-zeros, inv_norm_out float32 [n_rows]."""
    for nm, t in outputs.items():
        if t is not None:
            _check_dense(t, graph.n_rows, nm)
            if t.shape[1] != d or not t.is_contiguous():
                raise ValueError(f"{nm} must be contiguous [{graph.n_rows}, {d}]")
    if keep_bits is not None and (keep_bits.dtype != torch.int32 or keep_bits.numel() * 32 < graph.nnz):
        raise ValueError("keep_bits must be an int32 bitmap with >= nnz bits")
    if inv_norm_out is not None and (inv_norm_out.dtype != torch.float32 or inv_norm_out.numel() != graph.n_rows):
        raise ValueError("inv_norm_out must be float32 [n_rows]")


def spmm_into(graph: CsrGraph, x, *, y=None, acc_in=None, acc_out=None, acc_scale=1.0, val_scale=1.0,
              keep_bits=None, l2norm=False, inv_norm_out=None, acc_in2=None, acc_in2_scale=1.0, col_active_bits=None):
    """Raw launch of gcr_spmm_csr_acc2_f32: y = epilogue(val_scale * A[keep] x); optional fused layer
    combine acc_out = (acc_in + acc_in2_scale * acc_in2 + y) * acc_scale (lightgcn.py:26, ncl.py:421) and row L2
    normalise (sept.py:224).  col_active_bits: an int32 bitmap over the rows of x, clear = that row is zero (its
    non-zeros are skipped; `active_rows_bitmap`).  Outputs are caller-allocated; nothing is recorded for autograd."""
    _lib.require_cuda(x, y, acc_in, acc_out, keep_bits, inv_norm_out, acc_in2, col_active_bits)
    if col_active_bits is not None and (col_active_bits.dtype != torch.int32 or col_active_bits.numel() * 32 < graph.n_cols
                                        or keep_bits is not None):
        raise ValueError("col_active_bits must be an int32 bitmap with >= n_cols bits (and excludes keep_bits)")
    x = x.contiguous()
    _check_dense(x, graph.n_cols, "x")
    d = x.shape[1]
    if y is None and acc_out is None:
        raise ValueError("need y and/or acc_out")
    if acc_in2 is not None and acc_out is None:
        raise ValueError("acc_in2 needs acc_out")
    _check_spmm_outputs(graph, d, keep_bits, inv_norm_out, y=y, acc_in=acc_in, acc_out=acc_out, acc_in2=acc_in2)
    p = graph.plan
    ws = graph.workspace(d)
    sink = EVENT_SINK
    if sink is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    # plain launches: no mask (a predicate per stored non-zero of the classic order), no second addend, no row normalise
    plain = keep_bits is None and col_active_bits is None and acc_in2 is None and not l2norm and inv_norm_out is None
    stream = _lib.cur_stream(x.device)
    # the heaviest rows by column window (graph.HubPlan): plain launches only
    hub = graph.hub if plain and graph.hub is not None and graph.hub.eligible(d) else None
    out = dict(y=y, acc_in=acc_in, acc_out=acc_out, acc_scale=acc_scale, val_scale=val_scale)    # every route's epilogue
    # a row order (graph.RowOrder) stands in for the plan it was built beside: the hub plan's `main`, or the classic plan
    # when the graph has no hub plan.  Plain launches at d <= 64 only; the same words in another order of the rows
    rp = graph.rows_p if plain and d <= ROWS_MAX_D and (hub is not None or graph.hub is None) else None
    if rp is not None and not rp.eligible(d):
        rp = None
    if hub is not None and d <= WINDOWED_MAX_D:
        # both walks in one grid, both plans' split rows in another, then the hub reduction: the words of the branch below
        H = hub.H
        win = dict(hub_split=H.workspace(d), partials=ws, hub_partials=hub.partials(d), x=x, d=d, main_first=hub.main_first,
                   on=stream, **out)
        if rp is not None:
            spmm_launch.windowed_mapped(H, H.plan, rp, rp.plan, hub, **win)
        else:
            spmm_launch.windowed(H, H.plan, graph, hub.main, hub, **win)
    elif rp is not None:
        spmm_launch.rows_mapped(rp, rp.plan, x=x, d=d, partials=ws, on=stream, **out)
    else:
        if hub is not None:               # d > 64: the companion through the generic kernel, the reduction, then `main`
            H, part = hub.H, hub.partials(d)
            spmm_launch.csr_acc2(H, H.plan, x=x, d=d, y=part, acc_in2_scale=0.0, partials=H.workspace(d), on=stream)
            spmm_launch.hub_reduce(hub, partials=part, d=d, n_rows=graph.n_rows, on=stream, **out)
            p = hub.main                  # every other row: the classic walk with the hub rows skipped
        if plain and d <= ROWS_MAX_D:     # the plain launch's own kernel: the same words on another schedule
            spmm_launch.rows(graph, p, x=x, d=d, partials=ws, on=stream, **out)
        else:
            spmm_launch.csr_acc2(graph, p, x=x, d=d, partials=ws, keep_bits=keep_bits, acc_in2=acc_in2, acc_in2_scale=acc_in2_scale,
                                 flags=SPMM_ROW_L2NORM if l2norm else 0, inv_norm_out=inv_norm_out,
                                 col_active_bits=col_active_bits, on=stream, **out)
    if sink is not None:
        ev1.record()
        sink.append((ev0, ev1))
    return y if y is not None else acc_out


def active_rows_bitmap(idx, n_rows):
    """int32 bitmap with bit r set for every r in `idx` (int64 ids; out-of-range ids ignored): the `col_active_bits` of a
    launch whose input is zero outside those rows (gcr_bitmap_set)."""
    idx = _as_index(idx, idx.device if isinstance(idx, torch.Tensor) else None).reshape(-1)
    _lib.require_cuda(idx)
    bits = torch.zeros((int(n_rows) + 31) // 32, dtype=torch.int32, device=idx.device)
    _lib.call("gcr_bitmap_set", idx, idx.numel(), n_rows, bits, on=idx)
    return bits


def _spmm_t(graph, dz, **mask):
    """A^T dz into a fresh [n_cols, d] tensor: the product every SpMM backward ends with (`mask`: the launch's keep_bits in
    A^T's non-zero order and val_scale)."""
    gt = graph.t
    dx = torch.empty(gt.n_rows, dz.shape[1], dtype=torch.float32, device=dz.device)
    return spmm_into(gt, dz.contiguous(), y=dx, **mask)


def _need_mask_t(x, or_else=""):
    """The rule of every masked product: a gradient through it needs the mask in A^T's non-zero order."""
    if x.requires_grad and torch.is_grad_enabled():
        raise ValueError("backward through a masked graph needs keep_bits_t (the mask in A^T's non-zero order); "
                         "for a symmetric graph build it with graph.mirror_perm()" + or_else)


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, keep_bits, keep_bits_t, val_scale):
        ctx.graph, ctx.keep_bits_t, ctx.val_scale = graph, keep_bits_t, val_scale
        y = torch.empty(graph.n_rows, x.shape[1], dtype=torch.float32, device=x.device)
        return spmm_into(graph, x, y=y, keep_bits=keep_bits, val_scale=val_scale)

    @staticmethod
    def backward(ctx, dy):
        return _spmm_t(ctx.graph, dy, keep_bits=ctx.keep_bits_t, val_scale=ctx.val_scale), None, None, None, None


def spmm(graph: CsrGraph, x, keep_bits=None, keep_bits_t=None, val_scale=1.0, mask_symmetric=False):
    """Drop-in for `torch.sparse.mm(A, x)` (ncl.py:419 and the 13 other call sites of SURVEY §2.3
    S1), differentiable w.r.t. x: backward is the same kernel on A^T.  `keep_bits` is an edge-
    dropout bitmap in A's non-zero order, `keep_bits_t` the SAME mask in A^T's non-zero order.

    The backward computes (A o M)^T dy, so it needs the transposed mask even when A itself is
    symmetric: gcl.py:22-25 / buir.py:300-309 draw every stored (directed) non-zero independently, so
    M is not symmetric although A is.  For a symmetric graph `graph.mirror_perm()` maps each
    non-zero (r, c) to the position of (c, r): `edge_mask_bits(nnz, pe, seed, dev, edge_id=mirror)`
    (or `mirror_bits`) is the transposed mask.  Pass mask_symmetric=True only when (r, c) and (c, r)
    really share one draw (an undirected-edge mask); then keep_bits serves both directions."""
    if keep_bits is not None and keep_bits_t is None:
        if mask_symmetric and graph.symmetric:
            keep_bits_t = keep_bits
        else:
            _need_mask_t(x, ", or pass mask_symmetric=True if the mask itself is symmetric")
    return _SpMM.apply(x, graph, keep_bits, keep_bits_t, float(val_scale))


def mirror_bits(keep_bits, mirror, nnz):
    """The bitmap `keep_bits` re-ordered by `mirror` (int64 [nnz]): bit e of the result = bit mirror[e] of
    the input — the transposed mask of a symmetric graph for masks that are not functions of a counter
    (e.g. a recorded draw).  Small one-off index plumbing (torch)."""
    shifts = torch.arange(32, device=keep_bits.device, dtype=torch.int32)
    flat = ((keep_bits.unsqueeze(1) >> shifts) & 1).reshape(-1)[:nnz]
    return pack_bits(flat[mirror].bool())


def pack_bits(keep_bool):
    """bool [nnz] -> little-endian int32 bitmap (bit e of word e // 32)."""
    n = keep_bool.numel()
    pad = (-n) % 32
    b = torch.cat([keep_bool.to(torch.int64), torch.zeros(pad, dtype=torch.int64, device=keep_bool.device)]).view(-1, 32)
    w = (b << torch.arange(32, device=b.device, dtype=torch.int64)).sum(1)
    return (w & 0xFFFFFFFF).to(torch.int64).where(w < 2 ** 31, w - 2 ** 32).to(torch.int32)


class _Propagate(torch.autograd.Function):
    """final = c * sum_{k=0..K} A^k x0 (c = 1 or 1/(K+1)), optionally also every layer output.
    Linear in x0, so backward is the same recurrence on A^T (Horner form):
        h_K = g_K + c g_final ; h_k = g_k + c g_final + A^T h_{k+1} ; dx0 = h_0."""

    @staticmethod
    def forward(ctx, x0, graph, n_layers, scale, want_layers, keep_bits=None, keep_bits_t=None, val_scale=1.0):
        ctx.graph, ctx.n_layers, ctx.scale, ctx.want_layers = graph, n_layers, scale, want_layers
        ctx.mask_t = mk_t = dict(keep_bits=keep_bits_t, val_scale=val_scale)      # the backward's launches: A^T's order
        mk = dict(keep_bits=keep_bits, val_scale=val_scale)
        x0 = x0.contiguous()
        if not want_layers and n_layers > 0:
            # Horner form  sum_k A^k x0 = x0 + A (x0 + A (x0 + ...)): every layer reads x0 and writes ONE
            # [N, d] array (no separate layer output + running sum): one N x d write less per layer
            z = x0
            for k in range(n_layers):
                nxt = torch.empty_like(x0)
                spmm_into(graph, z, acc_in=x0, acc_out=nxt, acc_scale=scale if k == n_layers - 1 else 1.0, **mk)
                z = nxt
            return z
        cur, acc = x0, x0
        layers = []
        for k in range(n_layers):
            last = k == n_layers - 1
            need_y = want_layers or not last
            y = torch.empty_like(x0) if need_y else None
            acc_out = torch.empty_like(x0) if k == 0 else acc  # in place after the first layer
            spmm_into(graph, cur, y=y, acc_in=acc, acc_out=acc_out, acc_scale=scale if last else 1.0, **mk)
            acc = acc_out
            if need_y:
                cur = y
                layers.append(y)
        if n_layers == 0:
            acc = x0 * scale
        return (acc, *layers) if want_layers else acc

    @staticmethod
    def backward(ctx, g_final, *g_layers):
        gt, K, c, mk_t = ctx.graph.t, ctx.n_layers, ctx.scale, ctx.mask_t
        g = g_final.contiguous()
        if K == 0:
            return g * c, None, None, None, None, None, None, None
        # the recurrence on h' = h / c: h'_K = g + g_K / c, h'_k = g + g_k / c + A^T h'_{k+1}, dx0 = c h'_0 — the scale
        # rides on the last launch's epilogue instead of a pass over g_final
        gl = [x.contiguous() if x is not None else None for x in g_layers] if ctx.want_layers else [None] * K
        inv_c = 1.0 / c
        # the last layer's own gradient is part of the first launch's INPUT, so it is the one addend that needs a pass;
        # every other g_k rides on an epilogue as the second addend (gcr_spmm_csr_acc2_f32)
        h = g if gl[K - 1] is None else torch.add(g, gl[K - 1], alpha=inv_c)
        for k in range(K - 1, 0, -1):
            out = torch.empty_like(g)
            spmm_into(gt, h, acc_in=g, acc_in2=gl[k - 1], acc_in2_scale=inv_c, acc_out=out, **mk_t)
            h = out
        dx0 = torch.empty_like(g)
        spmm_into(gt, h, acc_in=g, acc_out=dx0, acc_scale=c, **mk_t)
        return dx0, None, None, None, None, None, None, None


def lightgcn_propagate(graph: CsrGraph, x0, n_layers: int, combine: str = "mean", return_layers: bool = False,
                       keep_bits=None, keep_bits_t=None, val_scale=1.0):
    """K-layer LightGCN message pass with the layer combine fused into the SpMM epilogue.
    combine='mean' -> ncl.py:415-422 / selfcf.py:475-485 (mean of the K+1 layer outputs);
    combine='sum'  -> lightgcn.py:21-27 (x += out, no division, Q3).
    Returns final [N, d] (and the list [x0, A x0, ..., A^K x0] when return_layers).
    keep_bits / keep_bits_t / val_scale: every layer runs on the dropped, rescaled operator val_scale * A[keep]
    (buir.py:300-320), the mask in A's non-zero order and, for the backward, in A^T's — `functional.spmm`'s arguments and
    its rule: a gradient through a masked graph without keep_bits_t raises.  Without them nothing changes."""
    if combine not in ("mean", "sum"):
        raise ValueError("combine must be 'mean' or 'sum'")
    _lib.require_cuda(x0)
    _check_dense(x0, graph.n_cols, "x0")
    if graph.n_rows != graph.n_cols:
        raise ValueError("propagation needs a square operator")
    scale = 1.0 / (n_layers + 1) if combine == "mean" else 1.0
    if keep_bits is None:
        if keep_bits_t is not None:
            raise ValueError("keep_bits_t without keep_bits")
    elif keep_bits_t is None:
        _need_mask_t(x0)
    out = _Propagate.apply(x0, graph, int(n_layers), scale, bool(return_layers), keep_bits, keep_bits_t, float(val_scale))
    if return_layers:
        return out[0], [x0, *out[1:]]
    return out


def normalize_bwd_n(nrm, inv, g_n, g_raw=None, out=None, from_raw=False):
    """d(A x) of `F.normalize(A x)` from the saved normalised rows: (g_n - nrm <nrm, g_n>) * inv (+ g_raw) in ONE pass
    (gcr_normalize_bwd_n_f32; sept.py:223-224, mhcn.py:440-457).  Rows clamped by eps have inv = 1e12 and nrm = 0.
    `out` may be g_n or g_raw themselves (in place).  from_raw: `nrm` holds the RAW rows A x (n = raw * inv on the fly,
    gcr_normalize_bwd_raw_f32) — the forward of `spmm_dual_acc_into` keeps no normalised copy."""
    _lib.require_cuda(nrm, inv, g_n, g_raw, out)
    g_n = g_n.contiguous()
    g_raw = None if g_raw is None else g_raw.contiguous()
    if out is None:
        out = torch.empty_like(g_n)
    rows, d = nrm.shape
    if g_n.shape != nrm.shape or out.shape != nrm.shape or (g_raw is not None and g_raw.shape != nrm.shape) or d % 4 or d > 256:
        raise ValueError("normalize_bwd_n: [rows, d] float32 tensors of one shape, d a multiple of 4 and <= 256")
    _lib.call("gcr_normalize_bwd_raw_f32" if from_raw else "gcr_normalize_bwd_n_f32", nrm, inv, g_n, g_raw, rows, d, out, on=nrm)
    return out


_GRAM_DIMS = (32, 64, 96, 128)


def gram_tn(x, g):
    """x^T g ([dx, dg]) for tall x [n, dx], g [n, dg] with the rows split over the whole chip (gcr_gram_tn_f32): the weight
    gradient of `em @ W` (mhcn.py:404-420).  Widths outside {32, 64, 96, 128} go to the library GEMM."""
    _lib.require_cuda(x, g)
    x, g = x.contiguous(), g.contiguous()
    n, dx = x.shape
    dg = g.shape[1]
    if dx not in _GRAM_DIMS or dg not in _GRAM_DIMS or g.shape[0] != n:
        return x.t() @ g
    out = torch.empty(dx, dg, dtype=torch.float32, device=x.device)
    ws = _lib.workspace("gcr_gram_tn_workspace_bytes", n, dx, dg, device=x.device)
    _lib.call("gcr_gram_tn_f32", x, g, n, dx, dg, out, ws, on=x)
    return out


class _DenseProj(torch.autograd.Function):
    """em @ W for a tall em [n, d] and a small square-ish W (MHCN's gating / attention, mhcn.py:404-420): forward and
    d em stay library GEMMs (n is the large dimension: they tile well); dW = em^T g is `gram_tn`."""

    @staticmethod
    def forward(ctx, em, w):
        ctx.save_for_backward(em, w)
        return em @ w

    @staticmethod
    def backward(ctx, g):
        em, w = ctx.saved_tensors
        g = g.contiguous()
        gem = g @ w.t() if ctx.needs_input_grad[0] else None
        gw = gram_tn(em, g) if ctx.needs_input_grad[1] else None
        return gem, gw


def dense_proj(em, w):
    """`torch.matmul(em, W)` of mhcn.py:405,409,414 with the weight gradient computed by a row-split kernel."""
    if not em.is_cuda or em.dim() != 2 or w.dim() != 2 or em.dtype != torch.float32:
        return em @ w
    return _DenseProj.apply(em, w)


class _RowsDotVec(torch.autograd.Function):
    """em @ v for tall em [n, d] and v [d]: d em = g v^T (one write pass), d v = sum_r g_r em_r (gcr_weighted_colsum_f32:
    the library's transposed GEMV of this shape ran 1.1 ms at n = 250K)."""

    @staticmethod
    def forward(ctx, em, v):
        ctx.save_for_backward(em, v)
        v = v.contiguous()
        out = torch.empty(em.shape[0], dtype=torch.float32, device=em.device)
        _lib.call("gcr_rows_dot_vec_f32", em, v, em.shape[0], em.shape[1], out, on=em)
        return out

    @staticmethod
    def backward(ctx, g):
        em, v = ctx.saved_tensors
        g = g.contiguous()
        gem = torch.outer(g, v) if ctx.needs_input_grad[0] else None
        gv = None
        if ctx.needs_input_grad[1]:
            n, d = em.shape
            gv = torch.empty(d, dtype=torch.float32, device=em.device)
            ws = _lib.workspace("gcr_weighted_colsum_workspace_bytes", n, d, device=em.device)
            _lib.call("gcr_weighted_colsum_f32", em, g, n, d, gv, ws, on=em)
        return gem, gv


def rows_dot_vec(em, v):
    """`em @ v` ([n, d] x [d] -> [n]) with the row-split weighted column sum as the gradient of v."""
    if not em.is_cuda or em.dim() != 2 or v.dim() != 1 or em.dtype != torch.float32 or em.shape[1] > 256:
        return em @ v
    return _RowsDotVec.apply(em.contiguous(), v)


class _Gate(torch.autograd.Function):
    """em * sigmoid(z + bias) (mhcn.py:404-411 around the GEMM z = em W) as one pass forward (gcr_gate_fwd_f32) and one
    backward (gcr_gate_bwd_f32: d em, d z and the bias gradient; the sigmoid is recomputed from the saved z)."""

    @staticmethod
    def forward(ctx, em, z, bias):
        em, z = em.contiguous(), z.contiguous()
        b = None if bias is None else bias.reshape(-1).contiguous()
        out = torch.empty_like(em)
        n, d = em.shape
        _lib.call("gcr_gate_fwd_f32", em, z, b, n, d, out, on=em)
        ctx.save_for_backward(em, z, b)
        ctx.bias_shape = None if bias is None else bias.shape
        return out

    @staticmethod
    def backward(ctx, g):
        em, z, b = ctx.saved_tensors
        n, d = em.shape
        g = g.contiguous()
        d_em, d_z = torch.empty_like(em), torch.empty_like(z)
        d_b = torch.empty(d, dtype=torch.float32, device=em.device)
        ws = _lib.workspace("gcr_gate_bwd_workspace_bytes", n, d, device=em.device)
        _lib.call("gcr_gate_bwd_f32", g, em, z, b, n, d, d_em, d_z, d_b, ws, on=em)
        return d_em, d_z, (None if ctx.bias_shape is None else d_b.reshape(ctx.bias_shape))


def gate(em, z, bias=None):
    """`em * torch.sigmoid(z + bias)` — mhcn.py:405-406 / 409-410 with z = em @ W; em, z float32 [n, d], bias [1, d] or [d]."""
    if not em.is_cuda or em.dim() != 2 or z.shape != em.shape or em.dtype != torch.float32 or z.dtype != torch.float32 \
            or em.shape[1] > 256 or (bias is not None and bias.numel() != em.shape[1]):
        return em * torch.sigmoid(z if bias is None else z + bias)
    return _Gate.apply(em, z, bias)


class _ChannelMix(torch.autograd.Function):
    """mhcn.py:413-420 on the logits e_k . v: (mixed, score) in one pass, the backward in one pass + the partial-sum
    reduction of d v (gcr_channel_mix_fwd_f32 / gcr_channel_mix_bwd_f32)."""

    @staticmethod
    def forward(ctx, e1, e2, e3, v, extra, extra_scale):
        e1, e2, e3, v = e1.contiguous(), e2.contiguous(), e3.contiguous(), v.contiguous()
        ex = None if extra is None else extra.contiguous()
        n, d = e1.shape
        mixed = torch.empty_like(e1)
        score = torch.empty(3, n, dtype=torch.float32, device=e1.device)
        _lib.call("gcr_channel_mix_fwd_f32", e1, e2, e3, v, ex, extra_scale, n, d, mixed, score, on=e1)
        ctx.save_for_backward(e1, e2, e3, v, score)
        ctx.extra_scale, ctx.has_extra = float(extra_scale), extra is not None
        ctx.mark_non_differentiable(score)
        return mixed, score

    @staticmethod
    def backward(ctx, g, _g_score):
        e1, e2, e3, v, score = ctx.saved_tensors
        n, d = e1.shape
        g = g.contiguous()
        d1, d2, d3 = torch.empty_like(e1), torch.empty_like(e1), torch.empty_like(e1)
        dx = torch.empty_like(e1) if ctx.has_extra else None
        dv = torch.empty(d, dtype=torch.float32, device=e1.device)
        ws = _lib.workspace("gcr_channel_mix_bwd_workspace_bytes", n, d, device=e1.device)
        _lib.call("gcr_channel_mix_bwd_f32", g, e1, e2, e3, v, score, ctx.extra_scale, n, d, d1, d2, d3, dx, dv, ws, on=e1)
        return d1, d2, d3, dv, dx, None


def channel_mix(e1, e2, e3, v, extra=None, extra_scale=0.0):
    """(mixed, score) of mhcn.py:413-420 for three channel tables [n, d] and the logit vector v [d]:
    score = softmax over the channels of e_k @ v ([3, n], not differentiable on this path), mixed = sum_k score_k e_k
    (+ extra_scale * extra).  Widths other than 32 / 64 / 128 / 256 and CPU tensors take the torch expression."""
    fused = e1.is_cuda and e1.dim() == 2 and e1.dtype == torch.float32 and e2.shape == e1.shape and e3.shape == e1.shape \
        and v.dim() == 1 and v.numel() == e1.shape[1] and (extra is None or extra.shape == e1.shape) \
        and bool(_lib.call("gcr_channel_mix_supported", e1.shape[1]))
    if not fused:
        logits = torch.stack([rows_dot_vec(e, v) for e in (e1, e2, e3)])
        score = torch.softmax(logits, dim=0)
        mixed = score[0].unsqueeze(1) * e1 + score[1].unsqueeze(1) * e2 + score[2].unsqueeze(1) * e3
        return (mixed if extra is None else mixed + extra_scale * extra), score
    return _ChannelMix.apply(e1, e2, e3, v, extra, float(extra_scale))


class _MimLoss(torch.autograd.Function):
    """mhcn.py:496-505 from em, edge = H em and three row permutations: two launches forward (gcr_mim_fwd_f32), two
    backward (gcr_mim_bwd_f32); saves the [3, n] sigmoid coefficients and (g, dg), never a gathered copy."""

    @staticmethod
    def forward(ctx, em, edge, p0, p1, p2):
        em, edge = em.contiguous(), edge.contiguous()
        n, d = em.shape
        dev = em.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(3, n, dtype=torch.float32, device=dev)
        gvec = torch.empty(2, d, dtype=torch.float32, device=dev)
        ws = _lib.workspace("gcr_mim_workspace_bytes", n, d, device=dev, dtype=torch.float64)
        _lib.call("gcr_mim_fwd_f32", em, edge, p0, p1, p2, n, d, loss, coef, gvec, ws, on=dev)
        ctx.save_for_backward(em, edge, p0, p1, p2, coef, gvec)
        return loss

    @staticmethod
    def backward(ctx, g):
        em, edge, p0, p1, p2, coef, gvec = ctx.saved_tensors
        n, d = em.shape
        g = g.to(torch.float32).contiguous()
        d_em, d_edge = torch.empty_like(em), torch.empty_like(edge)
        ws = _lib.workspace("gcr_mim_workspace_bytes", n, d, device=em.device, dtype=torch.float64)
        _lib.call("gcr_mim_bwd_f32", em, edge, p0, p1, p2, n, d, coef, gvec, g, d_em, d_edge, ws, on=em)
        return d_em, d_edge, None, None, None


def mim_supported(em):
    """True when `mim_loss` runs these rows: float32 [n, d] on the GPU with d in {32, 64, 128, 256}."""
    return bool(em.is_cuda and em.dim() == 2 and em.dtype == torch.float32 and _lib.call("gcr_mim_supported", em.shape[1]))


def mim_loss(em, edge, perms=None):
    """The hierarchical mutual-information loss of mhcn.py:496-505 (local + global) for em [n, d] and edge = H em [n, d]
    (the caller's `spmm`; the gradient reaches em through it a second time): `-log(sigmoid(x))` as a softplus that is
    finite at any x, the loss and both gradients bitwise reproducible.  perms: the three row permutations of
    row_shuffle / row_column_shuffle x 2 (int64 [n]); given ones are checked to be permutations on the host before any
    launch (ValueError), None draws them on the device.  Widths other than 32 / 64 / 128 / 256 raise (`mim_supported`)."""
    _lib.require_cuda(em, edge)
    if em.dim() != 2 or edge.shape != em.shape or em.dtype != torch.float32 or edge.dtype != torch.float32:
        raise ValueError("em and edge must be float32 [n, d] of the same shape")
    n, dev = em.shape[0], em.device
    if perms is None:
        perms = [torch.randperm(n, device=dev) for _ in range(3)]
    else:
        if len(perms) != 3:
            raise ValueError("perms must hold three row permutations")
        perms = [torch.as_tensor(p).to(device=dev, dtype=torch.int64).contiguous() for p in perms]
        rows = torch.arange(n, device=dev)
        for k, p in enumerate(perms):
            if p.shape != (n,) or not torch.equal(torch.sort(p).values, rows):
                raise ValueError(f"perms[{k}] is not a permutation of the {n} rows")
    if not _lib.call("gcr_mim_supported", em.shape[1]):
        raise _lib.GcrError(f"mim_loss: unsupported width {em.shape[1]} (32, 64, 128 or 256)")
    if n == 0:
        return (em.sum() + edge.sum()) * 0.0
    return _MimLoss.apply(em, edge, *perms)


class _NormProp(torch.autograd.Function):
    """One SEPT layer: y = normalize(A x) row-wise (sept.py:223-224); saves y and 1/||Ax||."""

    @staticmethod
    def forward(ctx, x, graph):
        y = torch.empty(graph.n_rows, x.shape[1], dtype=torch.float32, device=x.device)
        inv = torch.empty(graph.n_rows, dtype=torch.float32, device=x.device)
        spmm_into(graph, x.contiguous(), y=y, l2norm=True, inv_norm_out=inv)
        ctx.graph = graph
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        # d(Ax) = (dy - y <y, dy>) / max(||Ax||, eps); rows clamped by eps have inv = 1e12 and y = 0
        return _spmm_t(ctx.graph, normalize_bwd_n(y, inv, dy)), None


def spmm_l2norm(graph: CsrGraph, x):
    """`F.normalize(torch.sparse.mm(adj, emb), dim=1)` in one kernel, for encoders that feed the NORMALISED
    rows to the next layer (sept.py:223-224, sept_social.py:373-374,382-383).  MHCN feeds the raw product
    forward and only keeps the normalised copy: use `spmm_l2norm_dual` there."""
    _lib.require_cuda(x)
    return _NormProp.apply(x, graph)


def spmm_dual_into(graph: CsrGraph, x, y_raw, y_norm, inv_norm_out=None, keep_bits=None, val_scale=1.0):
    """Raw launch of gcr_spmm_csr_dual_f32: y_raw = A x and y_norm = normalize(A x) from one pass."""
    _lib.require_cuda(x, y_raw, y_norm, inv_norm_out, keep_bits)
    x = x.contiguous()
    _check_dense(x, graph.n_cols, "x")
    d = x.shape[1]
    _check_spmm_outputs(graph, d, keep_bits, inv_norm_out, y_raw=y_raw, y_norm=y_norm)
    if y_raw.data_ptr() == y_norm.data_ptr():
        raise ValueError("y_raw and y_norm must be different buffers")
    spmm_launch.csr_dual(graph, graph.plan, x=x, d=d, y_raw=y_raw, y_norm=y_norm, inv_norm_out=inv_norm_out, keep_bits=keep_bits,
                         val_scale=val_scale, partials=graph.workspace(d), on=x)
    return y_raw, y_norm


def spmm_dual_acc_into(graph: CsrGraph, x, y_raw, acc_in, acc_out, inv_norm_out, y_norm=None, keep_bits=None, val_scale=1.0):
    """Raw launch of gcr_spmm_csr_dual_acc_f32: y_raw = A x, acc_out = acc_in + normalize(A x), inv_norm_out = 1 / |A x| per row
    from one pass (mhcn.py:440-457: the normalised product joins a layer list that is summed); y_norm optional."""
    _lib.require_cuda(x, y_raw, acc_in, acc_out, inv_norm_out, y_norm, keep_bits)
    x = x.contiguous()
    _check_dense(x, graph.n_cols, "x")
    d = x.shape[1]
    if inv_norm_out is None:
        raise ValueError("inv_norm_out must be float32 [n_rows]")
    _check_spmm_outputs(graph, d, keep_bits, inv_norm_out, y_raw=y_raw, acc_out=acc_out, acc_in=acc_in, y_norm=y_norm)
    if y_raw.data_ptr() == acc_out.data_ptr() or (y_norm is not None and y_norm.data_ptr() == y_raw.data_ptr()):
        raise ValueError("y_raw, y_norm and acc_out must be different buffers")
    spmm_launch.csr_dual_acc(graph, graph.plan, x=x, d=d, y_raw=y_raw, y_norm=y_norm, acc_in=acc_in, acc_out=acc_out,
                             inv_norm_out=inv_norm_out, keep_bits=keep_bits, val_scale=val_scale, partials=graph.workspace(d),
                             on=x)
    return y_raw, acc_out


class _NormPropDual(torch.autograd.Function):
    """One MHCN channel layer: (z, n) = (A x, normalize(A x)) from one launch (univariate/mhcn.py:440-442:
    the RAW product feeds the next layer, the normalised copy joins the layer list)."""

    @staticmethod
    def forward(ctx, x, graph):
        z = torch.empty(graph.n_rows, x.shape[1], dtype=torch.float32, device=x.device)
        n = torch.empty_like(z)
        inv = torch.empty(graph.n_rows, dtype=torch.float32, device=x.device)
        spmm_dual_into(graph, x, z, n, inv)
        ctx.graph = graph
        ctx.save_for_backward(n, inv)
        # an unused output (the raw rows of the last MHCN layer) arrives as None instead of a materialised [U, d] zero
        ctx.set_materialize_grads(False)
        return z, n

    @staticmethod
    def backward(ctx, gz, gn):
        n, inv = ctx.saved_tensors
        if gz is None and gn is None:
            return None, None
        # dz = gz + (gn - n <n, gn>) / max(||z||, eps); rows clamped by eps have inv = 1e12 and n = 0
        dz = normalize_bwd_n(n, inv, gn, gz) if gn is not None else gz
        return _spmm_t(ctx.graph, dz), None


def spmm_l2norm_dual(graph: CsrGraph, x):
    """(torch.sparse.mm(adj, emb), F.normalize(torch.sparse.mm(adj, emb), p=2, dim=1)) in one kernel —
    the MHCN layer step (univariate/mhcn.py:440-457), differentiable w.r.t. x through both outputs."""
    _lib.require_cuda(x)
    return _NormPropDual.apply(x, graph)


class _NormPropDualAcc(torch.autograd.Function):
    """(z, acc + normalize(z)), z = A x, from one launch (gcr_spmm_csr_dual_acc_f32): the layer-list accumulation of
    mhcn.py:440-457 folded into the product; saves z and 1 / |z| (no normalised copy)."""

    @staticmethod
    def forward(ctx, x, acc, graph):
        z = torch.empty(graph.n_rows, x.shape[1], dtype=torch.float32, device=x.device)
        out = torch.empty_like(z)
        inv = torch.empty(graph.n_rows, dtype=torch.float32, device=x.device)
        spmm_dual_acc_into(graph, x, z, acc.contiguous(), out, inv)
        ctx.graph = graph
        ctx.save_for_backward(z, inv)
        ctx.set_materialize_grads(False)
        return z, out

    @staticmethod
    def backward(ctx, gz, gs):
        z, inv = ctx.saved_tensors
        if gz is None and gs is None:
            return None, None, None
        dz = normalize_bwd_n(z, inv, gs, gz, from_raw=True) if gs is not None else gz
        return _spmm_t(ctx.graph, dz), gs, None


def spmm_l2norm_dual_acc(graph: CsrGraph, x, acc):
    """(A x, acc + F.normalize(A x, p=2, dim=1)) in one kernel: `spmm_l2norm_dual` with the running layer sum folded in."""
    _lib.require_cuda(x, acc)
    return _NormPropDualAcc.apply(x, acc, graph)


class _SplitRows(torch.autograd.Function):
    """(x[:n], x[n:]) of the stacked [users; items] table (ncl.py:422-423 `torch.split`).  Plain
    slicing back-propagates each half as zeros(N, d) + copy and then adds the two: three extra
    passes over the 280 MB table per use.  Here the backward is one concatenation."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.rows = n, x.shape[0]
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, g_top, g_bot):
        ref = g_top if g_top is not None else g_bot
        d = ref.shape[1]
        # a producer that wrote both halves into ONE [rows, d] buffer (bpr_sums on the two halves of a split table):
        # hand that buffer back instead of copying the halves together
        if g_top is not None and g_bot is not None:
            base = g_top._base
            if base is not None and base is g_bot._base and tuple(base.shape) == (ctx.rows, d) and base.is_contiguous() \
                    and g_top.data_ptr() == base.data_ptr() and tuple(g_top.shape) == (ctx.n, d) \
                    and g_bot.data_ptr() == base.data_ptr() + ctx.n * d * base.element_size() \
                    and g_top.is_contiguous() and g_bot.is_contiguous():
                return base, None
        if g_top is None:
            g_top = ref.new_zeros(ctx.n, d)
        if g_bot is None:
            g_bot = ref.new_zeros(ctx.rows - ctx.n, d)
        return torch.cat([g_top, g_bot], 0), None


def split_rows(x, n):
    """User / item halves of a stacked embedding table with a single-pass backward."""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return x[:n], x[n:]
    return _SplitRows.apply(x, int(n))


# ---------------------------------------------------------------------------------------------
# BPR pairwise loss (P1/P2)
# ---------------------------------------------------------------------------------------------
BPR_NCL, BPR_LOGSIGMOID, BPR_LOG_SIGMOID = 0, 1, 2


def _as_index(t, device):
    t = torch.as_tensor(t, device=device)
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return t.contiguous()


# batches at least this large take the sorted backward (gcr_bpr_bwd_sorted_f32); below it the three
# row atomics per sample are cheaper than the sorts
BPR_SORTED_MIN_BATCH = 1 << 18
# full-batch edge-list BPR: order the negatives by item together with their (user, coefficient) payload (one 12-byte
# sort) instead of sorting an index and gathering through it
BPR_NEG_PAYLOAD_SORT = True
_ORDER_CACHE = {}


def _sorted_order(idx, n_keys, cache=False):
    """(keys_sorted uint32 as int32 tensor, perm int32) of a flat int64 index vector (gcr_sort_index).
    cache=True keeps the order of an index tensor that is reused step after step (lightgcn.py trains
    on the same edge arrays every step), keyed by storage pointer / length / version."""
    key = (idx.data_ptr(), idx.numel(), idx._version, int(n_keys))
    if cache and key in _ORDER_CACHE:
        return _ORDER_CACHE[key]
    n = idx.numel()
    keys = torch.empty(n, dtype=torch.int32, device=idx.device)
    perm = torch.empty(n, dtype=torch.int32, device=idx.device)
    ws = _lib.workspace("gcr_sort_index_workspace_bytes", n, device=idx.device, dtype=torch.uint8)
    _lib.call("gcr_sort_index", idx, n, n_keys, keys, perm, ws, on=idx)
    if cache:
        if len(_ORDER_CACHE) >= 8:
            _ORDER_CACHE.pop(next(iter(_ORDER_CACHE)))
        _ORDER_CACHE[key] = (keys, perm, idx)       # holding idx keeps the pointer from being recycled
    return keys, perm, idx


def _halves_of_one_table(top, bot):
    """True when `top` / `bot` are the two row blocks of ONE contiguous [rows, d] tensor (split_rows' outputs): decided
    from the views themselves — same base, shapes adding up to it — not from address adjacency, which two unrelated
    allocations can show by accident."""
    base = top._base
    return base is not None and base is bot._base and base.dim() == 2 and base.is_contiguous() \
        and top.is_contiguous() and bot.is_contiguous() and top.shape[1] == base.shape[1] == bot.shape[1] \
        and top.shape[0] + bot.shape[0] == base.shape[0] and top.data_ptr() == base.data_ptr() \
        and bot.data_ptr() == base.data_ptr() + top.numel() * base.element_size()


def _table_grads(user_tab, item_tab, stacked):
    """Zeroed gradients (gu, gi) of two tables: for the halves of one stacked table (`_halves_of_one_table`) the two row
    blocks of ONE [U + I, d] buffer, which _SplitRows.backward hands on without a copy; else one tensor each (gi None for an
    absent item table)."""
    if stacked:
        n_users = user_tab.shape[0]
        gfull = torch.zeros(n_users + item_tab.shape[0], user_tab.shape[1], dtype=torch.float32, device=user_tab.device)
        return gfull[:n_users], gfull[n_users:]
    return torch.zeros_like(user_tab), None if item_tab is None else torch.zeros_like(item_tab)


def _bpr_forward(user_tab, item_tab, u_idx, i_idx, j_idx, variant):
    """The forward launch of both BPR nodes (gcr_bpr_fwd_f32) -> (sums [5], dL/dx per sample, n_neg)."""
    batch, dev = u_idx.numel(), user_tab.device
    n_neg = 1 if j_idx.dim() == 1 else j_idx.shape[1]
    dldx = torch.empty(max(batch, 1), dtype=torch.float32, device=dev)
    sums = torch.zeros(5, dtype=torch.float32, device=dev)
    ws = _lib.workspace("gcr_bpr_workspace_floats", batch, device=dev)
    _lib.call("gcr_bpr_fwd_f32", user_tab, item_tab, user_tab.shape[1], u_idx, i_idx, j_idx, batch, n_neg, variant,
              user_tab.shape[0], item_tab.shape[0], dldx, sums, ws, on=dev)
    return sums, dldx, n_neg


def _bpr_neg_items(user_tab, item_tab, skey, spay, gs, gi):
    """The negatives' item rows from the (key j, payload (user, coefficient)) pairs gcr_bpr_neg_block_f32 wrote.  They are
    fresh every step, so their sort carries the payload with the key (gcr_sort_pairs_u64) and the scatter into gi streams
    sorted arrays (gcr_bpr_neg_items_sorted_f32) instead of chasing perm -> sample -> (u_idx, dloss_dx)."""
    slots, n_items = skey.numel(), item_tab.shape[0]
    ks, ps = torch.empty_like(skey), torch.empty_like(spay)
    ws = _lib.workspace("gcr_sort_pairs_u64_workspace_bytes", slots, device=skey.device, dtype=torch.uint8)
    stream = _lib.cur_stream(skey.device)
    _lib.call("gcr_sort_pairs_u64", skey, spay, slots, n_items, ks, ps, ws, on=stream)
    _lib.call("gcr_bpr_neg_items_sorted_f32", user_tab, item_tab, user_tab.shape[1], ks, ps, slots, user_tab.shape[0], n_items,
              gs, gi, on=stream)


class _BprSums(torch.autograd.Function):
    """sums = [sum_b loss_b, sum|U[u]|^2, sum|I[i]|^2, sum|I[j]|^2] through gcr_bpr_fwd/bwd_f32."""

    @staticmethod
    def forward(ctx, user_tab, item_tab, u_idx, i_idx, j_idx, variant):
        user_tab, item_tab = user_tab.contiguous(), item_tab.contiguous()
        sums, dldx, ctx.n_neg = _bpr_forward(user_tab, item_tab, u_idx, i_idx, j_idx, variant)
        ctx.save_for_backward(user_tab, item_tab, u_idx, i_idx, j_idx, dldx)
        # the two tables are the halves of one stacked [N, d] table (split_rows): the backward then writes both
        # gradients into one buffer, which _SplitRows.backward hands on without a copy
        ctx.stacked = _halves_of_one_table(user_tab, item_tab)
        ctx.mark_non_differentiable(u_idx, i_idx, j_idx)
        return sums

    @staticmethod
    def backward(ctx, g_sums):
        user_tab, item_tab, u_idx, i_idx, j_idx, dldx = ctx.saved_tensors
        gs = g_sums.contiguous().to(torch.float32)
        gu, gi = _table_grads(user_tab, item_tab, ctx.stacked)
        batch, d, n_users, n_items = u_idx.numel(), user_tab.shape[1], user_tab.shape[0], item_tab.shape[0]
        if batch >= BPR_SORTED_MIN_BATCH and batch * ctx.n_neg < 2 ** 31:
            ku, pu, _ = _sorted_order(u_idx, n_users, cache=True)
            ki, pi, _ = _sorted_order(i_idx, n_items, cache=True)
            dev, stream = user_tab.device, _lib.cur_stream(user_tab.device)
            kj = pj = None
            if not BPR_NEG_PAYLOAD_SORT:
                kj, pj, _ = _sorted_order(j_idx.reshape(-1), n_items)             # fresh negatives every step
            _lib.call("gcr_bpr_bwd_sorted_f32", user_tab, item_tab, d, u_idx, i_idx, j_idx, batch, ctx.n_neg, n_users, n_items,
                      dldx, gs, ku, pu, ki, pi, kj, pj, gu, gi, on=stream)
            if BPR_NEG_PAYLOAD_SORT:
                skey = torch.empty(batch * ctx.n_neg, dtype=torch.int32, device=dev)
                spay = torch.empty(batch * ctx.n_neg, dtype=torch.int64, device=dev)
                _lib.call("gcr_bpr_neg_block_f32", dldx, j_idx, u_idx, batch, ctx.n_neg, n_items, gs, None, None, None, skey, spay,
                          on=stream)
                _bpr_neg_items(user_tab, item_tab, skey, spay, gs, gi)
            return gu, gi, None, None, None, None
        _lib.call("gcr_bpr_bwd_f32", user_tab, item_tab, d, u_idx, i_idx, j_idx, batch, ctx.n_neg, n_users, n_items, dldx, gs,
                  gu, gi, on=user_tab)
        return gu, gi, None, None, None, None


class _BprEdgeSums(torch.autograd.Function):
    """`bpr_sums` for the batch that IS the training graph's edge list (lightgcn.py:91-118 trains on every edge at once).
    Same forward launch; in the backward the positive-pair parts of both gradients,
        dU[u] += sum_{i in N(u)} c_ui I[i],   dI[i] += sum_{u in N(i)} c_ui U[u],   c_ui = dL/dx of the pair (u, i),
    are ONE launch of the SpMM kernel on the graph's own structure with the coefficients as values (the item-major half
    through `CsrGraph.mirror_perm`) instead of two sorted scatters over E samples; the negatives keep their sorted scatter."""

    @staticmethod
    def forward(ctx, table, graph, n_users, j_idx, variant):
        table = table.contiguous()
        u_idx, i_idx = graph.user_major_edges(n_users)
        sums, dldx, n_neg = _bpr_forward(table[:n_users], table[n_users:], u_idx, i_idx, j_idx, variant)
        ctx.save_for_backward(table, j_idx, dldx)
        ctx.graph, ctx.n_users, ctx.n_neg = graph, n_users, n_neg
        ctx.mark_non_differentiable(j_idx)
        return sums

    @staticmethod
    def backward(ctx, g_sums):
        table, j_idx, dldx = ctx.saved_tensors
        graph, n_users = ctx.graph, ctx.n_users
        n_items = table.shape[0] - n_users
        gs = g_sums.contiguous().to(torch.float32)
        u_idx, i_idx = graph.user_major_edges(n_users)
        batch = u_idx.numel()
        # positive pairs: G = C_sym [U; I], C_sym = the graph's pattern with c_ui at (u, i) and (i, u)
        val = torch.empty(2 * batch, dtype=torch.float32, device=table.device)
        dropped = torch.zeros(n_items, dtype=torch.float32, device=table.device)   # samples the forward dropped, per positive item
        _lib.call("gcr_bpr_edge_values_f32", dldx, graph.mirror_perm(), graph.col, n_users, batch, gs, val, dropped, on=table)
        gfull = torch.empty_like(table)
        spmm_into(graph.with_values(val), table, y=gfull)
        gu, gi = gfull[:n_users], gfull[n_users:]
        # ... and the |I[i]|^2 term of the positives: 2 g_2 (number of live samples with item i) I[i]  (the users' |U[u]|^2
        # term rides in the launch below, which walks the samples user by user)
        live = graph.row_degrees()[n_users:] - dropped
        gi.addcmul_(table[n_users:], (2.0 * gs[2] * live).unsqueeze(1))
        # the negatives' USER side: the edges are in user-major order, so this step's negatives are a CSR block [U x I] on the
        # graph's own user row pointer (x n_neg) — one more SpMM on a cached work plan instead of a sorted scatter over E
        # samples (0.84 -> ~0.4 ms at cfg2); its |U[u]|^2 term counts the live samples of every user
        n_neg = ctx.n_neg
        nb = graph.negatives_user_block(n_users, n_items, n_neg)
        ncol = torch.empty(batch * n_neg, dtype=torch.int32, device=table.device)
        nval = torch.empty(batch * n_neg, dtype=torch.float32, device=table.device)
        dropped_u = torch.zeros(n_users, dtype=torch.float32, device=table.device)
        payload_sort = BPR_NEG_PAYLOAD_SORT and batch * n_neg < 2 ** 31
        skey = spay = None
        if payload_sort:                     # the same walk also writes the item side's (key j, payload (u, value)) pairs
            skey = torch.empty(batch * n_neg, dtype=torch.int32, device=table.device)
            spay = torch.empty(batch * n_neg, dtype=torch.int64, device=table.device)
        _lib.call("gcr_bpr_neg_block_f32", dldx, j_idx, u_idx, batch, n_neg, n_items, gs, ncol, nval, dropped_u, skey, spay,
                  on=table)
        nb.col, nb.val = ncol, nval
        spmm_into(nb, table[n_users:], acc_in=gu, acc_out=gu)
        gu.addcmul_(table[:n_users], (2.0 * gs[1] * (graph.row_degrees()[:n_users] - dropped_u)).unsqueeze(1))
        # the negatives' item rows
        if payload_sort:
            _bpr_neg_items(table[:n_users], table[n_users:], skey, spay, gs, gi)
            return gfull, None, None, None, None
        kj, pj, _ = _sorted_order(j_idx.reshape(-1), n_items)
        _lib.call("gcr_bpr_bwd_sorted_f32", table[:n_users], table[n_users:], table.shape[1], u_idx, None, j_idx, batch, n_neg,
                  n_users, n_items, dldx, gs, None, None, None, None, kj, pj, gu, gi, on=table)
        return gfull, None, None, None, None


def bpr_edge_sums(graph, table, n_users, j_idx, variant=BPR_LOG_SIGMOID):
    """`bpr_sums(table[:U], table[U:], u_idx, i_idx, j_idx, variant)` for (u_idx, i_idx) = the non-zeros of the user rows
    of `graph` in CSR order (`graph.user_major_edges`), i.e. a full batch over the training edges the graph was built from
    (lightgcn.py:91-118).  `table`: the stacked [U + I, d] encoder output; j_idx: [E] or [E, n_neg] negatives in that
    order.  Same sums, same gradients (the sums in another order: ~1e-6 relative); the backward's positive-pair parts are
    one SpMM launch.  The graph must be a symmetric bipartite operator with the users first."""
    _lib.require_cuda(table)
    if not graph.symmetric:
        raise ValueError("bpr_edge_sums needs a symmetric bipartite operator (users first)")
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[0] != graph.n_rows:
        raise ValueError("table must be float32 [n_rows, d]")
    j_idx = _as_index(j_idx, table.device)
    e = graph.user_major_edges(n_users)[0].numel()
    if j_idx.shape[0] != e or j_idx.dim() > 2:
        raise ValueError("j_idx: [E] or [E, n_neg] with E = the number of training edges")
    if e < BPR_SORTED_MIN_BATCH or e * (1 if j_idx.dim() == 1 else j_idx.shape[1]) >= 2 ** 31:
        u_idx, i_idx = graph.user_major_edges(n_users)
        ue, ie = split_rows(table, n_users)
        return bpr_sums(ue, ie, u_idx, i_idx, j_idx, variant)
    return _BprEdgeSums.apply(table, graph, int(n_users), j_idx, int(variant))


def bpr_sums(user_tab, item_tab, u_idx, i_idx, j_idx, variant=BPR_NCL):
    """Fused gather + BPR + squared norms.  Returns a differentiable float32[5]:
    [sum_b loss_b, sum_b |U[u_b]|^2, sum_b |I[i_b]|^2, sum_bk |I[j_bk]|^2, #samples with a bad id].
    j_idx may be [B] or [B, n_neg] (lightgcn.py:93: negatives' scores are averaged)."""
    _lib.require_cuda(user_tab, item_tab)
    if user_tab.dtype != torch.float32 or item_tab.dtype != torch.float32 or user_tab.shape[1] != item_tab.shape[1]:
        raise ValueError("user_tab / item_tab must be float32 [*, d] with the same d")
    dev = user_tab.device
    u_idx, i_idx, j_idx = _as_index(u_idx, dev), _as_index(i_idx, dev), _as_index(j_idx, dev)
    if u_idx.dim() != 1 or i_idx.shape != u_idx.shape or j_idx.shape[0] != u_idx.shape[0] or j_idx.dim() > 2:
        raise ValueError("u_idx, i_idx: [B]; j_idx: [B] or [B, n_neg]")
    return _BprSums.apply(user_tab, item_tab, u_idx, i_idx, j_idx, int(variant))


# ---------------------------------------------------------------------------------------------
# DirectAU: alignment + uniformity sums (directau.py:240-251)
# ---------------------------------------------------------------------------------------------
AU_NATIVE_MAX_DIM = 512          # gcr_directau_fwd_f32 runs any multiple of 16 up to here as it is


class _AuSums(torch.autograd.Function):
    """sums = [A_pos, A_neg, G_u, G_p, G_n, Q_u, Q_p, Q_n] through gcr_directau_fwd/bwd_f32 (include/gcr.h); n_sets
    1 / 2 / 3 takes the row sets u / u, p / u, p, n.  The forward keeps 1 / |x|, r and o, so the backward is one launch
    that adds the row gradients straight into the table gradients."""

    @staticmethod
    def forward(ctx, user_tab, item_tab, u_idx, i_idx, j_idx, n_sets, t):
        user_tab = user_tab.contiguous()
        item_tab = None if item_tab is None else item_tab.contiguous()
        batch = u_idx.numel() if u_idx is not None else user_tab.shape[0]
        d, dev = user_tab.shape[1], user_tab.device
        n_items = 0 if item_tab is None else item_tab.shape[0]
        want_grad = ctx.needs_input_grad[0] or (item_tab is not None and ctx.needs_input_grad[1])
        sums = torch.empty(8, dtype=torch.float32, device=dev)
        inv = torch.empty(3 * batch, dtype=torch.float32, device=dev)
        r = torch.empty(3 * batch, dtype=torch.float32, device=dev) if want_grad else None
        o = torch.empty(3 * batch, d, dtype=torch.float32, device=dev) if want_grad else None
        ws = _lib.workspace("gcr_directau_workspace_bytes", batch, d, device=dev)
        _lib.call("gcr_directau_fwd_f32", user_tab, item_tab, d, u_idx, i_idx, j_idx, batch, n_sets, user_tab.shape[0], n_items, t,
                  sums, inv, r, o, ws, on=dev)
        if want_grad:
            ctx.save_for_backward(user_tab, item_tab, u_idx, i_idx, j_idx, inv, r, o)
            ctx.n_sets, ctx.t, ctx.batch = n_sets, float(t), batch
            ctx.stacked = item_tab is not None and _halves_of_one_table(user_tab, item_tab)
        ctx.mark_non_differentiable(*[k for k in (u_idx, i_idx, j_idx) if k is not None])
        return sums

    @staticmethod
    def backward(ctx, g_sums):
        user_tab, item_tab, u_idx, i_idx, j_idx, inv, r, o = ctx.saved_tensors
        gs = g_sums.contiguous().to(torch.float32)
        gu, gi = _table_grads(user_tab, item_tab, ctx.stacked)
        _lib.call("gcr_directau_bwd_f32", user_tab, item_tab, user_tab.shape[1], u_idx, i_idx, j_idx, ctx.batch, ctx.n_sets,
                  user_tab.shape[0], 0 if item_tab is None else item_tab.shape[0], ctx.t, inv, r, o, gs, gu, gi, on=user_tab)
        return gu, gi, None, None, None, None, None


def _au_sums(user_tab, item_tab, u_idx, i_idx, j_idx, n_sets, t):
    _lib.require_cuda(user_tab, item_tab)
    tabs = [x for x in (user_tab, item_tab) if x is not None]
    if any(x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] != user_tab.shape[1] for x in tabs):
        raise ValueError("user_tab / item_tab must be float32 [*, d] with the same d")
    dev = user_tab.device
    idx = [None if k is None else _as_index(k, dev).reshape(-1) for k in (u_idx, i_idx, j_idx)]
    sizes = [user_tab.shape[0], None if item_tab is None else item_tab.shape[0], None if item_tab is None else item_tab.shape[0]]
    lens = {k.numel() if k is not None else sizes[s] for s, k in enumerate(idx[:n_sets])}
    if len(lens) != 1 or min(lens) < 1:
        raise ValueError("the row sets must have one common length >= 1 (an absent index vector stands for all rows of its table)")
    d = user_tab.shape[1]
    if d > AU_NATIVE_MAX_DIM:
        raise ValueError(f"embedding dim must be <= {AU_NATIVE_MAX_DIM}")
    if d % 16:
        # other widths: zero columns up to the next multiple of 16 change neither a norm nor a distance.  This copies the
        # WHOLE tables (and their gradients on the way back) every call and gives up the shared gradient buffer of a
        # stacked table: fine for [B, d] inputs, a full-table pass per step for a large embedding table
        pad = (0, 16 - d % 16)
        user_tab = torch.nn.functional.pad(user_tab, pad)
        item_tab = None if item_tab is None else torch.nn.functional.pad(item_tab, pad)
    return _AuSums.apply(user_tab, item_tab, idx[0], idx[1], idx[2], int(n_sets), float(t))


def au_sums(user_tab, item_tab, u_idx, i_idx, j_idx=None, t=2.0):
    """The sums DirectAU's losses are made of (directau.py:222-226, 240-251), for the row sets u = user_tab[u_idx],
    p = item_tab[i_idx] and — with j_idx — n = item_tab[j_idx], x^ = F.normalize(x, dim=-1).  Differentiable float32 [8]:
        [A_pos = sum_b |u^_b - p^_b|^2, A_neg = sum_b |u^_b - n^_b|^2, G_u, G_p, G_n, Q_u, Q_p, Q_n],
        G_s = sum over the pairs a < b of batch positions of exp(-t |x^_a - x^_b|^2),  Q_s = sum_b |x_b|^2
    (entries of an absent set are 0).  An index vector may be None: all rows of the table, in order.  Gathers, normalise,
    the all-pairs reduction and the norms are two launches, the backward one (gcr_directau_fwd_f32 / _bwd_f32); ids out
    of range give zero rows and no gradient.  Widths that are a multiple of 16 up to 512 run as they are; any other
    width up to 512 is zero-padded to the next multiple of 16, which copies both tables in full on every call (use a
    multiple of 16 for a large embedding table)."""
    return _au_sums(user_tab, item_tab, u_idx, i_idx, j_idx, 3 if j_idx is not None else 2, t)


# ---------------------------------------------------------------------------------------------
# negative sampler (N1) and edge-dropout bitmaps (A1)
# ---------------------------------------------------------------------------------------------
def neg_sample(user_rowptr, user_items_sorted, u_idx, n_negs, num_items, seed, offset=0, max_trials=101):
    """Uniform negatives with rejection against the user's sorted training row (device Philox).
    max_trials=0: no rejection (lightgcn.py:92); slots that exhaust max_trials come back as -1
    (ncl.py:110-112).  Returns int64 [B * n_negs]."""
    _lib.require_cuda(user_rowptr, u_idx)
    dev = u_idx.device
    u_idx = _as_index(u_idx, dev)
    out = torch.empty(u_idx.numel() * n_negs, dtype=torch.int64, device=dev)
    _lib.call("gcr_neg_sample", user_rowptr, user_items_sorted, u_idx, u_idx.numel(), n_negs, user_rowptr.numel() - 1, num_items,
              int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), max_trials, out, on=dev)
    return out


def edge_mask_bits(nnz, pe, seed, device, edge_id=None):
    """Bernoulli keep bitmap (`rand >= pe`, gcl.py:22-25) as int32 words, bit e <-> non-zero e.
    edge_id (int64 [nnz]) gives every non-zero a canonical id so that A and A^T share one mask."""
    bits = torch.zeros((nnz + 31) // 32, dtype=torch.int32, device=device)
    if edge_id is not None:
        edge_id = _as_index(edge_id, device)
    _lib.call("gcr_edge_mask_bits", nnz, pe, int(seed) & (2 ** 64 - 1), edge_id, bits, on=device)
    return bits


# ---------------------------------------------------------------------------------------------
# InfoNCE family (C1-C4): row logsumexp of the all-pairs logits on the fp32 MFMA
# ---------------------------------------------------------------------------------------------
_MFMA_DIMS = (32, 64, 128, 256)

# True: the column logsumexp of the symmetric loss (gcl.py:34) is computed by a second, bitwise
# reproducible pass instead of float atomics in the first one
COL_DETERMINISTIC = False


def _pad_dim(x):
    """Zero-pad the feature dim to the next width the MFMA kernels are built for (dot products
    and norms are unchanged by zero columns)."""
    d = x.shape[1]
    for w in _MFMA_DIMS:
        if d == w:
            return x
        if d < w:
            return torch.nn.functional.pad(x, (0, w - d))
    raise ValueError("embedding dim must be <= 256")


def _unpad(g, d):
    """The first d columns of a gradient computed on `_pad_dim`'s width (None stays None)."""
    return g if g is None or g.shape[1] == d else g[:, :d].contiguous()


def row_inv_norm(x, eps=1e-12, out=None):
    """1 / max(||x_r||, eps) per row — F.normalize's denominator (ncl.py:127, gcl.py:29-30)."""
    _lib.require_cuda(x)
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    elif out.shape != (x.shape[0],) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("row_inv_norm: out must be a contiguous float32 [rows] tensor on x's device")
    _lib.call("gcr_row_inv_norm_f32", x, x.shape[0], x.shape[1], eps, out, on=x)
    return out


INFONCE_EXCLUDE_DIAGONAL = 1
INFONCE_UNIT_ROWS = 2
INFONCE_ENGINE_F32 = 4

# "auto": the library default — split-operand engine for d <= 128 (its two-product launches on two f16 planes when
# the rows are normalised by the op itself, d <= 64 — flash forward and backward also d = 128: the
# GCR_INFONCE_UNIT_ROWS promise), f32 MFMA for d = 256;
# "b3": withhold the unit-rows promise (three bf16 planes everywhere); "f32": force the f32 MFMA.
# Read ONCE per forward (`_resolve_engine`); the backward reuses what the forward ran on.
INFONCE_ENGINE = "auto"


def _resolve_engine(engine=None, unit_rows=False):
    e = INFONCE_ENGINE if engine is None else engine
    if e not in ("auto", "b3", "f32"):
        raise ValueError("InfoNCE engine must be 'auto', 'b3' or 'f32'")
    if e == "f32":
        return INFONCE_ENGINE_F32
    return INFONCE_UNIT_ROWS if (unit_rows and e == "auto") else 0


def _infonce_flags(exclude_diagonal, engine_flag):
    """The flag word of an InfoNCE launch: the diagonal's bit and the engine (None: `_resolve_engine()`'s)."""
    return (INFONCE_EXCLUDE_DIAGONAL if exclude_diagonal else 0) | (_resolve_engine() if engine_flag is None else engine_flag)


def infonce_lse_raw(a, a_scale, b, b_scale, inv_tau, col_bound=None, exclude_diagonal=False, engine_flag=None):
    """lse[i] = log sum_j exp(inv_tau * a_scale[i] b_scale[j] <a_i, b_j>) (no autograd).
    col_bound (an upper bound of every logit, e.g. inv_tau for unit rows): also return the column
    logsumexp over the anchors [N] from the same pass (float atomics) as a second value.
    exclude_diagonal: the sum runs over j != i (grace.py:396-404, intra-view negatives)."""
    m, d = a.shape
    n = b.shape[0]
    lse = torch.empty(m, dtype=torch.float32, device=a.device)
    col_sum = torch.empty(n, dtype=torch.float32, device=a.device) if col_bound is not None else None
    ws = _lib.workspace("gcr_infonce_fwd_workspace_bytes", m, n, d, device=a.device)
    _lib.call("gcr_infonce_fwd_ex_f32", a, a_scale, m, b, b_scale, n, d, inv_tau, lse, col_sum,
              0.0 if col_bound is None else col_bound, ws, _infonce_flags(exclude_diagonal, engine_flag), on=a)
    if col_bound is None:
        return lse
    return lse, torch.log(col_sum) + float(col_bound)


# True: a row-softmax problem whose anchors need a gradient runs the flash-style forward (lse AND the
# softmax-weighted row sum o in one pass, gcr_infonce_fwd_o_f32): the anchor-side gradient is then
# dL/dlse * inv_tau * o and the backward recomputes the score tile once (table side) instead of twice.
FWD_O = True


def infonce_fwd_o_supported(d, engine_flag=0):
    return bool(_lib.call("gcr_infonce_fwd_o_supported", d, engine_flag))


def infonce_fwd_o_raw(a, a_scale, b, b_scale, inv_tau, exclude_diagonal=False, engine_flag=None, lse_out=None, o_out=None):
    """(lse [M], o [M, d]): lse[i] = log sum_j exp(s_ij), o[i] = sum_j softmax(s_i.)_j * (b_scale[j] b_j)
    (no autograd).  lse_out / o_out: caller-owned contiguous outputs (e.g. slices of one stacked buffer)."""
    m, d = a.shape
    n = b.shape[0]
    lse = torch.empty(m, dtype=torch.float32, device=a.device) if lse_out is None else lse_out
    o = torch.empty(m, d, dtype=torch.float32, device=a.device) if o_out is None else o_out
    if lse.shape != (m,) or o.shape != (m, d) or lse.dtype != torch.float32 or o.dtype != torch.float32:
        raise ValueError("lse_out [M] / o_out [M, d] must be float32")
    ws = _lib.workspace("gcr_infonce_fwd_o_workspace_bytes", m, n, d, device=a.device)
    _lib.call("gcr_infonce_fwd_o_f32", a, a_scale, m, b, b_scale, n, d, inv_tau, lse, o, ws,
              _infonce_flags(exclude_diagonal, engine_flag), on=a)
    return lse, o


def pos_logit_raw(a, a_scale, b, b_scale, pos, scale, out=None):
    m, d = a.shape
    out = torch.empty(m, dtype=torch.float32, device=a.device) if out is None else out
    _lib.call("gcr_pos_logit_f32", a, a_scale, b, b_scale, pos, m, b.shape[0], d, scale, out, on=a)
    return out


def _infonce_bwd_raw(x, x_scale, y, y_scale, inv_tau, lse_x, w_x, lse_y, w_y, exclude_diagonal=False, engine_flag=None,
                     out=None):
    """g = inv_tau * sum_j P_ij yhat_j (see gcr_infonce_bwd_f32): gradient w.r.t. the scaled rows of x.
    out: caller-owned contiguous [Mx, d] (e.g. one half of a stacked gradient table)."""
    mx, d = x.shape
    g = torch.empty_like(x) if out is None else out
    if g.shape != x.shape or g.dtype != torch.float32:
        raise ValueError("out must be float32 with x's shape")
    ws = _lib.workspace("gcr_infonce_bwd_workspace_bytes", mx, y.shape[0], d, device=x.device)
    _lib.call("gcr_infonce_bwd_ex_f32", x, x_scale, mx, y, y_scale, y.shape[0], d, inv_tau, lse_x, w_x, lse_y, w_y, g, ws,
              _infonce_flags(exclude_diagonal, engine_flag), on=x)
    return g


class _InfoNCEStats(torch.autograd.Function):
    """(a, b) -> row_lse [M], pos_logit [M] (and col_lse [N]) of S = inv_tau * ahat bhat^T, with the
    flash-style HIP backward.  Every loss of the InfoNCE family is a few [M]-vector ops on top.

    Diagonal positives (pos None, M = N >= 2, nothing excluded): the kernels run with the diagonal left out and the
    positive's share is carried as q_i = 1 - p_ii = sigmoid(lse_ex_i - s_ii), which fp32 holds to its own relative
    precision; lse = logaddexp(lse_ex, s_ii).  The backward then forms the diagonal's coefficient as a scalar,
    (g_lse + g_col + g_pos) - g_lse q - g_col q_col, as autograd's (softmax - one-hot) does.  exp(s_ii - lse_i) - 1
    from an lse stored in fp32 would carry an absolute error of ~ulp(lse) into p_ii - 1, which at p_ii -> 1 is all of
    it (gcl.py:28-35 at small batches, ncl.py:125-130 with b_cos=False; tests/golden/contrast_f64.npz)."""

    @staticmethod
    def forward(ctx, a, b, pos, inv_tau, normalize, want_col, exd=False, grad_a=False):
        a_p, b_p = _pad_dim(a).contiguous(), _pad_dim(b).contiguous()
        sa = row_inv_norm(a_p) if normalize else None
        sb = row_inv_norm(b_p) if normalize else None
        # unit-norm rows bound every logit by 1/tau: on the f32-MFMA engine row and column LSE come out
        # of ONE pass (the column sums by float atomics: 15.9 vs 21.0 ms at 100K x 100K);
        # COL_DETERMINISTIC forces the bitwise-reproducible second pass with the roles swapped, which
        # is also the path for un-normalised inputs — and for the split-operand engine, whose MFMA
        # work is cheap enough that the second pass costs no more than the column-sum epilogue
        # (two passes vs one: 11.5 vs 11.2 ms on three bf16 planes, 8.2 vs 13.6 ms on two f16 planes at 100K x 100K;
        # 0.34-0.49 vs 0.62-0.89 ms at 20K x 20K; scripts/perf_infonce_sym.py)
        eng = _resolve_engine(unit_rows=normalize)   # once per problem: the backward runs on the same engine
        on_f32 = bool(eng & INFONCE_ENGINE_F32) or _lib.call("gcr_infonce_engine", a_p.shape[1]) == 0
        diag = pos is None and not exd and a_p.shape[0] == b_p.shape[0] >= 2
        kex = exd or diag                            # the kernels leave the diagonal out
        one_pass = want_col and normalize and inv_tau <= 40.0 and not COL_DETERMINISTIC and not kex and on_f32
        o = None
        if FWD_O and not want_col and grad_a and a_p.shape[0] > 0 and \
                infonce_fwd_o_supported(a_p.shape[1], eng):
            lse, o = infonce_fwd_o_raw(a_p, sa, b_p, sb, inv_tau, exclude_diagonal=kex, engine_flag=eng)
            col = None
        elif one_pass:
            lse, col = infonce_lse_raw(a_p, sa, b_p, sb, inv_tau, col_bound=inv_tau * 1.0001, engine_flag=eng)
        else:
            lse = infonce_lse_raw(a_p, sa, b_p, sb, inv_tau, exclude_diagonal=kex, engine_flag=eng)
            col = infonce_lse_raw(b_p, sb, a_p, sa, inv_tau, exclude_diagonal=kex, engine_flag=eng) if want_col else None
        pl = pos_logit_raw(a_p, sa, b_p, sb, pos, inv_tau)
        q = q_col = None
        if diag:                                     # lse / col above leave out s_ii: put it back, keep 1 - p_ii
            q = torch.sigmoid(lse - pl)
            lse = torch.logaddexp(lse, pl)
            if col is not None:
                q_col = torch.sigmoid(col - pl)
                col = torch.logaddexp(col, pl)
        ctx.save_for_backward(a_p, b_p, pos, sa, sb, lse, col, o, q, q_col)
        ctx.inv_tau, ctx.d, ctx.exd, ctx.eng, ctx.diag = inv_tau, a.shape[1], exd, eng, diag
        if want_col:
            return lse, pl, col
        return lse, pl

    @staticmethod
    def backward(ctx, g_lse, g_pos, g_col=None):
        a, b, pos, sa, sb, lse, col, o, q, q_col = ctx.saved_tensors
        inv_tau = ctx.inv_tau
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_lse = g_lse.contiguous().float() if g_lse is not None else None
        g_col = g_col.contiguous().float() if (g_col is not None and col is not None) else None
        lse_r = lse if g_lse is not None else None
        col_r = col if g_col is not None else None
        kex = ctx.exd or ctx.diag
        ga = gb = None
        stream = _lib.cur_stream(a.device)
        if need_a and o is not None:
            # flash-style forward kept o[i] = sum_j softmax_ij bhat_j: the softmax part of dL/dahat_i is one scale
            # (diagonal positives: o is the softmax over j != i, whose share of the full row is q)
            w = g_lse * q if ctx.diag and g_lse is not None else g_lse
            ga = o * (w * inv_tau).unsqueeze(1) if g_lse is not None else torch.zeros_like(o)
        elif need_a:
            ga = _infonce_bwd_raw(a, sa, b, sb, inv_tau, lse_r, g_lse, col_r, g_col, kex, ctx.eng)
        if need_b:
            gb = _infonce_bwd_raw(b, sb, a, sa, inv_tau, col_r, g_col, lse_r, g_lse, kex, ctx.eng)
        if ctx.diag and (need_a or need_b):
            # the diagonal, left out above: g_lse p_ii + g_col p^col_ii + g_pos with p_ii = 1 - q, the weights summed
            # first (they cancel exactly where g_pos = -(g_lse + g_col): gcl.py:28-35, ncl.py:125-130)
            total = torch.zeros_like(q) if g_pos is None else g_pos.contiguous().float()
            corr = torch.zeros_like(q)
            if g_lse is not None:
                total, corr = total + g_lse, corr + g_lse * q
            if g_col is not None:
                total, corr = total + g_col, corr + g_col * q_col
            g_pos = total - corr
        if g_pos is not None and (need_a or need_b):
            _lib.call("gcr_infonce_pos_bwd_f32", a, sa, b, sb, pos, g_pos.contiguous().float(), a.shape[0], b.shape[0], a.shape[1],
                      inv_tau, ga, gb, on=stream)
        if sa is not None:
            for x, s, g in ((a, sa, ga), (b, sb, gb)):
                if g is not None:
                    _lib.call("gcr_normalize_bwd_f32", x, s, g, x.shape[0], x.shape[1], g, on=stream)
        return _unpad(ga, ctx.d), _unpad(gb, ctx.d), None, None, None, None, None, None


def infonce_stats(a, b, pos=None, temperature=0.2, normalize=True, want_col=False, exclude_diagonal=False):
    """Row logsumexp and positive logit of S = (ahat @ bhat.T) / temperature without materialising S.
    a: [M, d] anchors, b: [N, d] candidates, pos: int64 [M] index of each anchor's positive row in b
    (None: the diagonal, requires N >= M).  Returns (lse [M], pos_logit [M]) and, with want_col,
    also the column logsumexp [N] (gcl.py:34 `cross_entropy(sim.T, labels)`).  exclude_diagonal: the
    sums leave out the pair (i, j = i) (grace.py:396-404).  Differentiable w.r.t. a and b."""
    _lib.require_cuda(a, b)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("a [M, d] and b [N, d] must be float32 with the same d")
    if b.shape[0] == 0:
        raise ValueError("empty candidate table")
    if pos is None:
        if b.shape[0] < a.shape[0]:
            raise ValueError("diagonal positives need N >= M")
    else:
        pos = _as_index(pos, a.device)
        if pos.shape != (a.shape[0],):
            raise ValueError("pos must be [M]")
    # the flash-style forward (lse + weighted row sum) only pays off when the anchors will get a gradient: decided
    # here, where the caller's grad mode is still visible (inside Function.forward it is always off)
    grad_a = torch.is_grad_enabled() and a.requires_grad
    return _InfoNCEStats.apply(a, b, pos, 1.0 / float(temperature), bool(normalize), bool(want_col), bool(exclude_diagonal),
                               grad_a)


# ---------------------------------------------------------------------------------------------
# BCE-with-logits over all pairs (lightgcn.py:109-113, `loss_type == "bce"`)
# ---------------------------------------------------------------------------------------------
BCE_TWO_PLANES = 8          # include/gcr.h GCR_BCE_TWO_PLANES


def _bce_flags(engine=None):
    """'auto': two f16 planes on rows scaled to unit norm inside the launch (scores un-scaled by the norms); 'b3': three bf16
    planes on the raw rows; 'f32': the f32 MFMA."""
    e = INFONCE_ENGINE if engine is None else engine
    if e not in ("auto", "b3", "f32"):
        raise ValueError("BCE engine must be 'auto', 'b3' or 'f32'")
    return {"auto": BCE_TWO_PLANES, "b3": 0, "f32": INFONCE_ENGINE_F32}[e]


def bce_fwd_raw(a, b, want_o=False, engine_flag=0):
    """(rowsum [M], o [M, d] or None): rowsum[i] = sum_j softplus(<a_i, b_j>), o[i] = sum_j sigmoid(<a_i, b_j>) b_j (no autograd)."""
    m, d = a.shape
    n = b.shape[0]
    rows = torch.empty(m, dtype=torch.float32, device=a.device)
    o = torch.empty(m, d, dtype=torch.float32, device=a.device) if want_o else None
    ws = _lib.workspace("gcr_bce_fwd_workspace_bytes", m, n, d, device=a.device)
    _lib.call("gcr_bce_fwd_f32", a, m, b, n, d, rows, o, ws, engine_flag, on=a)
    return rows, o


def bce_bwd_raw(x, y, w_x=None, w_y=None, engine_flag=0, out=None):
    """g[i] = sum_j (w_x[i] | w_y[j]) sigmoid(<x_i, y_j>) y_j (exactly one of the weight vectors; gcr_bce_bwd_f32)."""
    mx, d = x.shape
    g = torch.empty_like(x) if out is None else out
    ws = _lib.workspace("gcr_bce_bwd_workspace_bytes", mx, y.shape[0], d, device=x.device)
    _lib.call("gcr_bce_bwd_f32", x, mx, y, y.shape[0], d, w_x, w_y, g, ws, engine_flag, on=x)
    return g


class _BceRows(torch.autograd.Function):
    """(a, b) -> rowsum [M] of softplus(a b^T); the backward is sigmoid-weighted operand sums (no M x N matrix)."""

    @staticmethod
    def forward(ctx, a, b, eng, grad_a):
        a_p, b_p = _pad_dim(a).contiguous(), _pad_dim(b).contiguous()
        want_o = bool(grad_a and a_p.shape[0] > 0 and _lib.call("gcr_bce_fwd_o_supported", a_p.shape[1], eng))
        rows, o = bce_fwd_raw(a_p, b_p, want_o, eng)
        ctx.save_for_backward(a_p, b_p, o)
        ctx.eng, ctx.d = eng, a.shape[1]
        return rows

    @staticmethod
    def backward(ctx, g):
        a, b, o = ctx.saved_tensors
        g = g.contiguous().float()
        ga = gb = None
        if ctx.needs_input_grad[0]:
            ga = o * g.unsqueeze(1) if o is not None else bce_bwd_raw(a, b, w_x=g, engine_flag=ctx.eng)
        if ctx.needs_input_grad[1]:
            gb = bce_bwd_raw(b, a, w_y=g, engine_flag=ctx.eng)
        return _unpad(ga, ctx.d), _unpad(gb, ctx.d), None, None


def bce_softplus_rowsum(a, b, engine=None):
    """rowsum[i] = sum_j softplus(<a_i, b_j>) = sum_j BCE-with-logits(s_ij, label 0) without materialising the [M, N]
    scores of lightgcn.py:110; differentiable w.r.t. a and b.  With a one-hot label per row the loss of lightgcn.py:113
    is (rowsum.sum() - sum_i s_{i, pos_i}) / (M N)  (`losses.lightgcn_bce_loss`)."""
    _lib.require_cuda(a, b)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("a [M, d] and b [N, d] must be float32 with the same d")
    if b.shape[0] == 0:
        raise ValueError("empty item table")
    return _BceRows.apply(a, b, _bce_flags(engine), torch.is_grad_enabled() and a.requires_grad)


class _BceEdgeLoss(torch.autograd.Function):
    """lightgcn.py:109-113 for the batch that IS the training graph's edge list (the full batch of lightgcn.py:86-87):
        loss = ( sum_u deg(u) rowsum_u  -  sum_{(u,i) in E} <U_u, I_i> ) / (E * I)
    * rows of the [E, I] score matrix that belong to the same user are equal: the softplus part runs over the U distinct
      users, weighted by their number of training edges (E / U times fewer pairs than the reference's matmul);
    * the positive-logit sum is 1/2 <T, A1 T> with A1 the graph's pattern with unit values (duplicate edges counted), and
      its gradient w.r.t. the stacked table T is A1 T itself: ONE SpMM launch gives the value and both gradients."""

    @staticmethod
    def forward(ctx, table, graph, n_users, eng):
        table = table.contiguous()
        ue, ie = table[:n_users], table[n_users:]
        n_edges = graph.user_major_edges(n_users)[0].numel()
        deg = graph.row_degrees()[:n_users].contiguous()
        want_o = bool(_lib.call("gcr_bce_fwd_o_supported", table.shape[1], eng))
        rows, o = bce_fwd_raw(ue, ie, want_o, eng)
        ones = getattr(graph, "_unit_values", None)
        if ones is None:
            ones = graph if graph.val is None else \
                graph.with_values(torch.ones(graph.nnz, dtype=torch.float32, device=table.device))
            graph._unit_values = ones
        y = torch.empty_like(table)
        spmm_into(ones, table, y=y)
        scale = 1.0 / (float(n_edges) * float(ie.shape[0]))
        ctx.save_for_backward(table, o, y, deg)
        ctx.n_users, ctx.eng, ctx.scale = n_users, eng, scale
        return (torch.dot(deg, rows) - 0.5 * torch.dot(table.reshape(-1), y.reshape(-1))) * scale

    @staticmethod
    def backward(ctx, g):
        table, o, y, deg = ctx.saved_tensors
        n_users = ctx.n_users
        ue, ie = table[:n_users], table[n_users:]
        c = g * ctx.scale
        gt = torch.empty_like(table)
        w = (deg * c).contiguous()
        if o is not None:
            torch.mul(o, w.unsqueeze(1), out=gt[:n_users])
        else:
            bce_bwd_raw(ue, ie, w_x=w, engine_flag=ctx.eng, out=gt[:n_users])
        bce_bwd_raw(ie, ue, w_y=w, engine_flag=ctx.eng, out=gt[n_users:])
        torch.addcmul(gt, y, (-c).reshape(1, 1), out=gt)          # (c stays on the device: no host read-back)
        return gt, None, None, None


def bce_edge_loss(graph, table, n_users, engine=None):
    """`F.binary_cross_entropy_with_logits(user_emb[pos_u] @ item_emb.T, one_hot(pos_i))` (lightgcn.py:109-113) for
    (pos_u, pos_i) = the training edges `graph` was built from (`graph.user_major_edges`); `table` = the stacked [U + I, d]
    encoder output.  d must be one of the MFMA widths (32 / 64 / 128 / 256)."""
    _lib.require_cuda(table)
    if not graph.symmetric:
        raise ValueError("bce_edge_loss needs a symmetric bipartite operator (users first)")
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[0] != graph.n_rows:
        raise ValueError("table must be float32 [n_rows, d]")
    if table.shape[1] not in _MFMA_DIMS:
        raise ValueError("bce_edge_loss: embedding dim must be 32, 64, 128 or 256 (use losses.lightgcn_bce_loss otherwise)")
    return _BceEdgeLoss.apply(table, graph, int(n_users), _bce_flags(engine))


def edge_mask_exact_bits(nnz, n_keep, seed, device):
    """Keep bitmap with exactly n_keep of nnz bits set, a uniformly random subset without replacement
    (univariate/sept.py:55-61: `np.random.choice(idx, int(len(idx) * (1 - drop_rate)), replace=False)`)."""
    bits = torch.empty((nnz + 31) // 32, dtype=torch.int32, device=device)
    ws = _lib.workspace("gcr_edge_mask_exact_workspace_bytes", nnz, device=device, dtype=torch.uint8)
    _lib.call("gcr_edge_mask_exact_bits", nnz, n_keep, int(seed) & (2 ** 64 - 1), bits, ws, on=device)
    return bits


# ---------------------------------------------------------------------------------------------
# PyGCL feature masking (univariate/grace.py:261-278)
# ---------------------------------------------------------------------------------------------
class _MaskColumns(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep_bits):
        ctx.save_for_backward(keep_bits)
        return mask_columns_raw(x, keep_bits)

    @staticmethod
    def backward(ctx, g):
        (keep_bits,) = ctx.saved_tensors
        return mask_columns_raw(g, keep_bits), None


def mask_columns_raw(x, keep_bits):
    _lib.require_cuda(x, keep_bits)
    x = x.contiguous()
    if x.dim() != 2 or x.dtype != torch.float32 or keep_bits.dtype != torch.int32 or keep_bits.numel() * 32 < x.shape[1]:
        raise ValueError("x float32 [n, d]; keep_bits int32 bitmap with >= d bits")
    out = torch.empty_like(x)
    _lib.call("gcr_mask_columns_f32", x, x.shape[0], x.shape[1], keep_bits, out, on=x)
    return out


def feature_masking(x, pf, seed, keep_bits=None):
    """`drop_feature(x, pf)` / FeatureMasking(pf) (univariate/grace.py:261-278): every feature COLUMN is zeroed with
    probability pf (one draw per column: `uniform_(0, 1) < drop_prob` drops), x itself untouched; differentiable.
    The d draws come from the counter RNG (gcr_edge_mask_bits over the d column ids: keep = u_c >= pf); pass
    `keep_bits` to replay a recorded mask.  Returns (masked x, keep_bits)."""
    if keep_bits is None:
        keep_bits = edge_mask_bits(x.shape[1], pf, seed, x.device)
    return _MaskColumns.apply(x, keep_bits), keep_bits


# ---------------------------------------------------------------------------------------------
# batch-row gathers of the loss functions
# ---------------------------------------------------------------------------------------------
class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, idx):
        table = table.contiguous()
        out = torch.empty(idx.numel(), table.shape[1], dtype=torch.float32, device=table.device)
        _lib.call("gcr_gather_rows_f32", table, idx, idx.numel(), table.shape[1], table.shape[0], out, on=table)
        ctx.save_for_backward(idx)
        ctx.shape = table.shape
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        gt = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        g = g.contiguous()
        _lib.call("gcr_scatter_add_rows_f32", g, idx, idx.numel(), g.shape[1], ctx.shape[0], gt, on=g)
        return gt, None


# True: gather_rows checks its ids on the host (one min / max read-back per call) and raises IndexError like `table[idx]`
# does; off by default because the read-back stalls the stream (and forbids hipGraph capture)
CHECK_INDEX = False


def gather_rows(table, idx):
    """`table[idx]` for a float32 [N, d] table and int64 ids in [0, N) — NOT torch's full indexing contract: negative
    ids do not wrap, and an id outside [0, N) yields a zero row and is skipped by the backward instead of raising (set
    `functional.CHECK_INDEX = True` to get torch's IndexError, at the price of a host read-back).  The backward adds
    duplicate ids with float atomics: their order, hence the last bits of such rows, can differ from run to run.

    `table[idx]` for a float32 [N, d] table and int64 ids (`rec_user_emb[user_idx]`, `context[user]` ...; ncl.py:314-316,
    360-361,370-373) whose backward scatters the row gradients with float atomics (gcr_scatter_add_rows_f32) instead of
    the sort + segmented reduction of a generic index_put(accumulate=True) (which grows with the batch; at B = 2048
    the two cost the same within noise, profiles/r02_ncl_step_kernel_stats.csv)."""
    _lib.require_cuda(table)
    if table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError("table must be float32 [N, d]")
    idx = _as_index(idx, table.device).reshape(-1)
    if CHECK_INDEX and idx.numel() > 0:
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= table.shape[0]:
            raise IndexError(f"gather_rows: index {lo if lo < 0 else hi} is out of bounds for a table of {table.shape[0]} rows")
    return _GatherRows.apply(table, idx)


class _GatherDropoutViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, idx, p, seed, n_views, keep_bits):
        table = table.contiguous()
        n, d = idx.numel(), table.shape[1]
        out = torch.empty((1 + n_views) * n, d, dtype=torch.float32, device=table.device)
        _lib.call("gcr_gather_dropout_f32", table, idx, n, d, table.shape[0], p, seed, n_views, keep_bits, out, on=table)
        ctx.save_for_backward(idx, *(() if keep_bits is None else (keep_bits,)))      # no mask of its own: (p, seed)
        ctx.args = (table.shape, p, seed, n_views)
        return out

    @staticmethod
    def backward(ctx, g):
        idx, *bits = ctx.saved_tensors
        shape, p, seed, n_views = ctx.args
        gt = torch.zeros(shape, dtype=torch.float32, device=g.device)
        g = g.contiguous()
        _lib.call("gcr_gather_dropout_bwd_f32", g, idx, idx.numel(), shape[1], shape[0], p, seed, n_views,
                  bits[0] if bits else None, gt, on=g)
        return gt, None, None, None, None, None


def gather_dropout_views(table, idx, p, seed, n_views=2, keep_bits=None):
    """`emb = table[idx]` and `n_views` training-mode `nn.Dropout(p)` draws of it (ssl4rec.py:192-196), stacked
    [(1 + n_views) * n, d] in one kernel: rows [0, n) are `gather_rows(table, idx)` (same contract for ids outside the
    table), rows [(1 + v) n, (2 + v) n) are view v, `keep_v ? emb * (1 / (1 - p)) : 0`.  Bit i * d + c of view v's mask is
    that bit of `edge_mask_bits(n * d, p, seed + v)`; the kernel recomputes it and stores no mask, and the backward
    regenerates it: one float atomic per table element for all 1 + n_views gradient blocks.  keep_bits (int32
    [n_views, ceil(n * d / 32)], p < 1) replays recorded masks instead of drawing."""
    _lib.require_cuda(table, keep_bits)
    if table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError("table must be float32 [N, d]")
    p, n_views = float(p), int(n_views)
    if not (0.0 <= p <= 1.0) or not (1 <= n_views <= 4):
        raise ValueError("p in [0, 1] and n_views in 1..4")
    idx = _as_index(idx, table.device).reshape(-1)
    if keep_bits is not None:
        n_words = (idx.numel() * table.shape[1] + 31) // 32
        if keep_bits.dtype != torch.int32 or tuple(keep_bits.shape) != (n_views, n_words) or p >= 1.0:
            raise ValueError(f"keep_bits must be int32 [{n_views}, {n_words}] (and p < 1)")
        keep_bits = keep_bits.contiguous()
    return _GatherDropoutViews.apply(table, idx, p, int(seed) & (2 ** 64 - 1), n_views, keep_bits)


# ---------------------------------------------------------------------------------------------
# SEPT's tri-training block (univariate/sept_social.py:394-420, 447-457)
# ---------------------------------------------------------------------------------------------
class _TriTraining(torch.autograd.Function):
    """gcr_tri_fwd_f32 / gcr_tri_bwd_f32: saves the four tables, uniq, the [2, 3, M] reciprocal sums (1 / all and
    1 / all - 1 / positives) and the membership bitmap (3 M^2 bits), never an M x M matrix."""

    @staticmethod
    def forward(ctx, x_f, x_s, x_r, aug, uniq, k, inv_t, positives):
        tabs = [t.contiguous() for t in (x_f, x_s, x_r, aug)]
        n_rows, d = tabs[0].shape
        m, dev = uniq.numel(), tabs[0].device
        loss = torch.empty(3, dtype=torch.float32, device=dev)
        replay = positives is not None
        pos = positives if replay else torch.empty(3, m, k, dtype=torch.int64, device=dev)
        rsum = torch.empty(2, 3, m, dtype=torch.float32, device=dev)
        inv_norm = torch.empty(4, m, dtype=torch.float32, device=dev)
        member = _lib.workspace("gcr_tri_member_words", m, device=dev, dtype=torch.int32)
        ws = _lib.workspace("gcr_tri_workspace_bytes", m, d, k, device=dev)
        _lib.call("gcr_tri_fwd_f32", *tabs, n_rows, d, uniq, m, k, inv_t, replay, loss, pos, rsum, inv_norm, member, ws, on=dev)
        ctx.save_for_backward(*tabs, uniq, rsum, member)
        ctx.args = (k, inv_t)
        ctx.mark_non_differentiable(pos)
        return loss, pos

    @staticmethod
    def backward(ctx, g, _g_pos):
        *tabs, uniq, rsum, member = ctx.saved_tensors
        k, inv_t = ctx.args
        n_rows, d = tabs[0].shape
        m, dev = uniq.numel(), tabs[0].device
        g = g.to(torch.float32).contiguous()
        grads = [torch.zeros_like(t) for t in tabs]
        ws = _lib.workspace("gcr_tri_workspace_bytes", m, d, k, device=dev)
        _lib.call("gcr_tri_bwd_f32", *tabs, n_rows, d, uniq, m, k, inv_t, rsum, member, g, *grads, ws, on=dev)
        return (*grads, None, None, None, None)


def tri_training_supported(d, k):
    """True when the fused kernels (gcr_tri_*) serve rows of width d with k pseudo-labels: d in {32, 64, 128}, 1 <= k <= 32."""
    return bool(_lib.call("gcr_tri_supported", d, k))


def tri_training_loss_composed(x_f, x_s, x_r, aug, uniq, k, temperature=0.1, positives=None):
    """`tri_training_loss` as the reference writes it, from the ops that were there before the fused kernel: torch's
    label_prediction (sept_social.py:394-399), `torch.topk` (:401-406) and `losses.neighbor_discrimination` (:408-420)."""
    import torch.nn.functional as F
    from . import losses as Ls
    a = aug[uniq]
    views = [x[uniq] for x in (x_f, x_s, x_r)]
    if positives is None:
        with torch.no_grad():                        # nothing flows through the probabilities or the indices
            an = F.normalize(a)
            p_f, p_s, p_r = (F.softmax(torch.matmul(F.normalize(e), an.T), dim=1) for e in views)
            positives = torch.stack([torch.topk((p1 + p2) / 2, k, dim=1).indices
                                     for p1, p2 in ((p_s, p_r), (p_f, p_r), (p_f, p_s))])
    loss = torch.stack([Ls.neighbor_discrimination(positives[v], views[v], a, temperature) for v in range(3)])
    return loss, positives


def tri_training_loss(x_f, x_s, x_r, aug, uniq, k, temperature=0.1, positives=None):
    """The tri-training block of univariate/sept_social.py:447-457 for the friend, sharing and rec view tables and the
    augmented table (all float32 [U, d]) over the distinct batch users `uniq` = torch.unique(user_idx) (int64 [M], strictly
    ascending — computed once here where the reference computes it six times):
        P_v = label_prediction(x_v)                                     :394-399
        pos_f = topk(P_s + P_r), pos_s = topk(P_f + P_r), pos_r = topk(P_f + P_s)      :401-406, 451-453
        loss[v] = neighbor_discrimination(pos_v, x_v)  at temperature `temperature` (the reference hard-codes 0.1)  :408-420
    Returns (loss [3] in the order friend, sharing, rec; positives int64 [3, M, k], every row in descending order of the
    combined probability, ties to the smaller column).  One autograd node, differentiable in the four tables; nothing flows
    through the probabilities or the indices.  positives=: replays given label sets (rows of distinct columns in [0, M))
    instead of selecting.  Shapes outside `tri_training_supported(d, k)`, and temperatures below 1 / 40, run
    `tri_training_loss_composed`.  M < k raises
    (the reference's topk does); M = 0 gives zeros."""
    _lib.require_cuda(x_f, x_s, x_r, aug)
    tabs = (x_f, x_s, x_r, aug)
    if any(t.dim() != 2 or t.dtype != torch.float32 or t.shape != x_f.shape for t in tabs):
        raise ValueError("the four tables must be float32 [U, d] of one shape")
    k = int(k)
    uniq = _as_index(uniq, x_f.device).reshape(-1)
    m = uniq.numel()
    if k < 1:
        raise ValueError("k must be at least 1")
    if m == 0:
        return sum(t.sum() for t in tabs) * torch.zeros(3, device=x_f.device), torch.zeros(3, 0, k, dtype=torch.int64, device=x_f.device)
    if m < k:
        raise ValueError(f"tri_training_loss: {m} distinct users cannot give {k} pseudo-labels each")
    if positives is not None:
        positives = torch.as_tensor(positives).to(device=x_f.device, dtype=torch.int64).contiguous()
        if tuple(positives.shape) != (3, m, k):
            raise ValueError(f"positives must be int64 [3, {m}, {k}]")
    if not tri_training_supported(x_f.shape[1], k) or not (0.025 <= float(temperature)):
        return tri_training_loss_composed(x_f, x_s, x_r, aug, uniq, k, temperature, positives)
    if positives is not None:
        positives = positives.clone()                # the node returns the tensor it was given: keep the caller's apart
    return _TriTraining.apply(x_f, x_s, x_r, aug, uniq, k, 1.0 / float(temperature), positives)


# ---------------------------------------------------------------------------------------------
# BUIR's bootstrap loss and target update (univariate/buir.py:251-277)
# ---------------------------------------------------------------------------------------------
class _BuirLoss(torch.autograd.Function):
    """gcr_buir_fwd_f32 / gcr_buir_bwd_f32: saves the inputs and stats [2, 3, B] = (|p|, |t|, cosine) per side; the
    backward recomputes the predictions.  No gradient to the target tables."""

    @staticmethod
    def forward(ctx, on_user, on_item, tg_user, tg_item, u_idx, i_idx, weight, bias):
        tabs = [t.contiguous() for t in (on_user, on_item, tg_user, tg_item)]
        weight, bias = weight.contiguous(), bias.contiguous()
        d, batch, dev = weight.shape[0], u_idx.numel(), weight.device
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        stats = torch.empty(2, 3, batch, dtype=torch.float32, device=dev)
        _lib.call("gcr_buir_fwd_f32", *tabs, tabs[0].shape[0], tabs[1].shape[0], d, u_idx, i_idx, batch, weight, bias, loss, stats,
                  on=dev)
        ctx.save_for_backward(*tabs, u_idx, i_idx, weight, bias, stats)
        ctx.stacked = _halves_of_one_table(tabs[0], tabs[1])
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        on_user, on_item, tg_user, tg_item, u_idx, i_idx, weight, bias, stats = ctx.saved_tensors
        d, batch, dev = weight.shape[0], u_idx.numel(), weight.device
        n_users, n_items = on_user.shape[0], on_item.shape[0]
        gu, gi = _table_grads(on_user, on_item, ctx.stacked)
        gw, gb = torch.zeros_like(weight), torch.zeros_like(bias)
        if batch:
            ku, pu, _ = _sorted_order(u_idx, n_users)
            ki, pi, _ = _sorted_order(i_idx, n_items)
            ws = _lib.workspace("gcr_buir_workspace_bytes", batch, d, device=dev)
            g = g.to(torch.float32).reshape(1).contiguous()
            _lib.call("gcr_buir_bwd_f32", on_user, on_item, tg_user, tg_item, n_users, n_items, d, u_idx, i_idx, batch, weight,
                      bias, stats, g, ku, pu, ki, pi, gu, gi, gw, gb, ws, on=dev)
        return gu, gi, None, None, None, None, gw, gb


def buir_supported(d):
    """True when the fused kernels (gcr_buir_*) serve rows of width d: a multiple of 16 in [16, 512]."""
    return bool(_lib.call("gcr_buir_supported", d))


def _buir_args(on_user, on_item, tg_user, tg_item, u_idx, i_idx, weight, bias):
    _lib.require_cuda(on_user, on_item, tg_user, tg_item, weight, bias)
    d = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != d or tuple(bias.shape) != (d,) or weight.dtype != torch.float32 \
            or bias.dtype != torch.float32:
        raise ValueError("weight must be float32 [d, d] and bias float32 [d]")
    for t, o in ((on_user, tg_user), (on_item, tg_item)):
        if t.dim() != 2 or t.dtype != torch.float32 or t.shape[1] != d or o.shape != t.shape or o.dtype != torch.float32:
            raise ValueError("the online and target tables must be float32 [n, d] of one shape per side")
    u_idx, i_idx = _as_index(u_idx, weight.device).reshape(-1), _as_index(i_idx, weight.device).reshape(-1)
    if u_idx.numel() != i_idx.numel():
        raise ValueError("u_idx and i_idx must have one length")
    return u_idx, i_idx


def buir_loss_composed(on_user, on_item, tg_user, tg_item, u_idx, i_idx, weight, bias):
    """`buir_loss` as the reference writes it, from the ops that were there before the fused kernels: `gather_rows`
    (buir.py:323-325), torch's linear (:262) and F.normalize, the products, the sums and the mean (:269-277)."""
    import torch.nn.functional as F
    u_idx, i_idx = _buir_args(on_user, on_item, tg_user, tg_item, u_idx, i_idx, weight, bias)
    p_u = F.normalize(F.linear(gather_rows(on_user, u_idx), weight, bias), dim=-1)
    p_i = F.normalize(F.linear(gather_rows(on_item, i_idx), weight, bias), dim=-1)
    with torch.no_grad():
        t_u, t_i = F.normalize(gather_rows(tg_user, u_idx), dim=-1), F.normalize(gather_rows(tg_item, i_idx), dim=-1)
    loss_ui = 2 - 2 * (p_u * t_i).sum(dim=-1)
    loss_iu = 2 - 2 * (p_i * t_u).sum(dim=-1)
    return (loss_ui + loss_iu).mean()


def buir_loss(on_user, on_item, tg_user, tg_item, u_idx, i_idx, weight, bias):
    """BUIR's batch loss, univariate/buir.py:260-262, 269-277, 323-325, for the propagated online and target tables
    (float32 [U, d] / [I, d]), the batch ids and the predictor `nn.Linear(d, d)`'s weight and bias:
        p_u = W on_user[u] + b,  p_i = W on_item[i] + b
        loss = mean_b (2 - 2 <n(p_u), n(tg_item[i])>) + (2 - 2 <n(p_i), n(tg_user[u])>),   n = F.normalize
    One autograd node (two launches forward, three backward and the two id sorts), differentiable in on_user, on_item,
    weight and bias; the targets get no gradient.  An id outside its table reads as a zero row (`gather_rows`' contract).
    Every output is bitwise reproducible.  Widths outside `buir_supported(d)` run `buir_loss_composed`.  An empty batch
    launches nothing and gives 0 with zero gradients."""
    u_idx, i_idx = _buir_args(on_user, on_item, tg_user, tg_item, u_idx, i_idx, weight, bias)
    if not buir_supported(weight.shape[0]):
        return buir_loss_composed(on_user, on_item, tg_user, tg_item, u_idx, i_idx, weight, bias)
    if u_idx.numel() == 0:
        return (on_user.sum() + on_item.sum() + weight.sum() + bias.sum()) * 0.0
    return _BuirLoss.apply(on_user, on_item, tg_user.detach(), tg_item.detach(), u_idx, i_idx, weight, bias)


def ema_rows_(target, online, idx, momentum):
    """In place `target[idx] = target[idx] * momentum + online[idx] * (1 - momentum)` (buir.py:254-257) for float32
    [N, d] tables: every distinct row of idx is updated exactly once however often it recurs, ids outside [0, N) are
    skipped, the other rows are not touched (gcr_ema_rows_f32; no host read-back, bitwise reproducible).  Returns target."""
    _lib.require_cuda(target, online)
    if target.dim() != 2 or target.dtype != torch.float32 or online.shape != target.shape or online.dtype != torch.float32 \
            or not target.is_contiguous():
        raise ValueError("target (contiguous) and online must be float32 [N, d] of one shape")
    if target.requires_grad and torch.is_grad_enabled():
        raise ValueError("ema_rows_ writes in place: call it on a tensor outside autograd (or under no_grad)")
    idx = _as_index(idx, target.device).reshape(-1)
    n_rows, d = target.shape
    claim = torch.empty((n_rows + 31) // 32, dtype=torch.int32, device=target.device)
    _lib.call("gcr_ema_rows_f32", target, online.detach().contiguous(), idx, idx.numel(), d, n_rows, momentum, claim, on=target)
    return target


# ---------------------------------------------------------------------------------------------
# DiffNet's social-diffusion layer (univariate/diffnet.py:1127-1130)
# ---------------------------------------------------------------------------------------------
# `diffuse_layer(gather=None)` sums S x inside the layer kernel only when no row of S has more entries than this.  Measured
# (scripts/perf_diffnet_step.py; EXPERIMENTS.md, "DiffNet: the fused social-diffusion layer"): at 1M users the in-kernel gather
# loses to the tuned SpMM + scratch z already at ten entries per row (4.03 against 2.69 ms per layer, forward + backward),
# and by more with a 20 000-entry row (8.69 against 2.51), so the rule keeps it for a graph without entries.
DIFFUSE_GATHER_MAX_DEGREE = 0


def diffuse_supported(d):
    """True when the fused kernels (gcr_diffuse_*) serve rows of width d: 32, 64 or 128."""
    return bool(_lib.call("gcr_diffuse_supported", int(d)))


def _diffuse_args(graph, x, w):
    if x.dim() != 2 or w.dim() != 2 or tuple(w.shape) != (2 * x.shape[1], x.shape[1]) or w.dtype != x.dtype:
        raise ValueError("x must be [n, d] and w [2 d, d] of one dtype")
    if graph.n_rows != x.shape[0] or graph.n_cols != x.shape[0]:
        raise ValueError("the graph must be [n, n] for x [n, d]")


def _sparse_mm_torch(graph, x):
    """S x where libgcr has no kernel (a CPU tensor, or a dtype other than float32): torch's own sparse product on the
    graph's entries (duplicates sum), on x's device and in its dtype."""
    rowptr = graph.rowptr.to(x.device)
    rows = torch.repeat_interleave(torch.arange(graph.n_rows, device=x.device), rowptr[1:] - rowptr[:-1])
    val = torch.ones(graph.nnz, device=x.device) if graph.val is None else graph.val.to(x.device)
    s = torch.sparse_coo_tensor(torch.stack([rows, graph.col.to(device=x.device, dtype=torch.int64)]), val.to(x.dtype),
                                (graph.n_rows, graph.n_cols))
    return torch.sparse.mm(s, x)


def diffuse_layer_composed(graph, x, w):
    """One DiffNet layer as the reference writes it (diffnet.py:1127-1130): sparse.mm, cat, matmul, relu, the product
    through `spmm` for float32 on the device; a CPU tensor and any other dtype (float64 on either side) take torch's
    sparse product, as the reference does."""
    _diffuse_args(graph, x, w)
    z = spmm(graph, x) if x.is_cuda and x.dtype == torch.float32 else _sparse_mm_torch(graph, x)
    return torch.relu(torch.matmul(torch.cat([z, x], dim=1), w))


class _DiffuseLayer(torch.autograd.Function):
    """gcr_diffuse_fwd_f32 / gcr_diffuse_bwd_f32: saves x, w and h only; the backward rebuilds S x (inside the kernel, or
    by the SpMM into a scratch z when not `gather`) and finishes dx = S^T p + q with the SpMM on S^T."""

    @staticmethod
    def _z(graph, x, gather):
        return None if gather else spmm_into(graph, x, y=torch.empty_like(x))

    @staticmethod
    def _col(graph):
        """graph.col, or a one-element stand-in for a graph without entries: an empty tensor's pointer is NULL, which the
        kernels refuse when they gather (gcr.h), and no row reads it."""
        return graph.col if graph.nnz else torch.zeros(1, dtype=torch.int32, device=graph.col.device)

    @staticmethod
    def forward(ctx, x, w, graph, gather):
        x, w = x.contiguous(), w.contiguous()
        n, d = x.shape
        h = torch.empty_like(x)
        _lib.call("gcr_diffuse_fwd_f32", graph.rowptr, _DiffuseLayer._col(graph), graph.val, n, x,
                  _DiffuseLayer._z(graph, x, gather), w, d, h, on=x)
        ctx.save_for_backward(x, w, h)
        ctx.graph, ctx.gather = graph, gather
        return h

    @staticmethod
    def backward(ctx, g):
        x, w, h = ctx.saved_tensors
        graph = ctx.graph
        n, d = x.shape
        p, q, dw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(w)
        ws = _lib.workspace("gcr_diffuse_workspace_bytes", n, d, device=x.device)
        _lib.call("gcr_diffuse_bwd_f32", graph.rowptr, _DiffuseLayer._col(graph), graph.val, n, x,
                  _DiffuseLayer._z(graph, x, ctx.gather), w, h, g.contiguous(), d, p, q, dw, ws, on=x)
        dx = spmm_into(graph.t, p, acc_in=q, acc_out=torch.empty_like(x)) if ctx.needs_input_grad[0] else None
        return dx, dw, None, None


class _SpmmAdd(torch.autograd.Function):
    """acc + A x as one launch (the SpMM's fused addend); backward: g to acc, A^T g to x."""

    @staticmethod
    def forward(ctx, x, acc, graph):
        ctx.graph = graph
        acc = acc.contiguous()
        return spmm_into(graph, x, acc_in=acc, acc_out=torch.empty_like(acc))

    @staticmethod
    def backward(ctx, g):
        return (_spmm_t(ctx.graph, g) if ctx.needs_input_grad[0] else None), (g if ctx.needs_input_grad[1] else None), None


def spmm_add(graph: CsrGraph, x, acc):
    """`acc + torch.sparse.mm(A, x)` (diffnet.py:1131) in one launch, differentiable in x and acc."""
    return _SpmmAdd.apply(x, acc, graph)


def diffuse_max_degree(graph):
    """The largest number of entries in a row of the graph (cached on it)."""
    m = getattr(graph, "_max_degree", None)
    if m is None:
        rp = graph.rowptr_host
        m = graph._max_degree = int((rp[1:] - rp[:-1]).max()) if graph.n_rows else 0
    return m


def diffuse_layer(graph, x, w, gather=None):
    """relu([S x | x] w), one layer of DiffNet.forward (diffnet.py:1127-1130), for S = `graph` [n, n], x [n, d], w [2 d, d]:
    one autograd node over the fused kernels, differentiable in x and w, which keeps x, w and the output only (the
    composition keeps S x and the [n, 2 d] concatenation as well).  gather=True sums S x inside the kernel (a row's entries
    in stored order); gather=False runs the tuned SpMM into a scratch z first, forward and backward; None takes the first
    when no row has more than DIFFUSE_GATHER_MAX_DEGREE entries (measured: SpMM + z wins on every graph with an entry).  Bitwise reproducible.  Widths outside
    `diffuse_supported(d)`, other dtypes than float32, CPU tensors and n = 0 run `diffuse_layer_composed`."""
    _diffuse_args(graph, x, w)
    if not (x.is_cuda and x.dtype == torch.float32 and x.shape[0] > 0 and diffuse_supported(x.shape[1])):
        return diffuse_layer_composed(graph, x, w)
    if gather is None:
        gather = diffuse_max_degree(graph) <= DIFFUSE_GATHER_MAX_DEGREE
    return _DiffuseLayer.apply(x, w, graph, bool(gather))


# ---------------------------------------------------------------------------------------------
# GAT: the attention aggregation of torch_geometric's GATConv (gat.py:20-23, 34, 37)
# ---------------------------------------------------------------------------------------------
def gat_supported(heads, c):
    """True when the fused kernels (gcr_gat_*) serve `heads` heads of `c` columns: c in {32, 64, 128}, heads in {1, 2, 4},
    heads * c <= 256."""
    return bool(_lib.call("gcr_gat_supported", int(heads), int(c)))


def _gat_args(graph, h, a_src, a_dst, heads, keep_bits, p, bias):
    n = graph.n_rows
    if graph.n_cols != n or h.dim() != 2 or h.shape[0] != n or h.shape[1] % heads:
        raise ValueError("the graph must be [n, n] and h [n, heads * c]")
    if tuple(a_src.shape) != (n, heads) or tuple(a_dst.shape) != (n, heads):
        raise ValueError("a_src and a_dst must be [n, heads]")
    if bias is not None and tuple(bias.shape) != (h.shape[1],):
        raise ValueError("bias must be [heads * c]")
    if not 0.0 <= p < 1.0:
        raise ValueError("p must be in [0, 1)")
    if keep_bits is not None and (keep_bits.dtype != torch.int32 or keep_bits.numel() < ((graph.nnz + n) * heads + 31) // 32):
        raise ValueError("keep_bits must be int32 words covering (nnz + n) * heads bits")


def unpack_bits(bits, count):
    """bool [count] of an int32 little-endian bitmap (`pack_bits`' inverse), on the bitmap's device."""
    idx = torch.arange(count, device=bits.device)
    return ((bits[idx >> 5] >> (idx & 31)) & 1).bool()


def gat_edges(graph, device):
    """(src, dst) int64 [nnz + n] of the aggregation's terms in the bitmap's order: the graph's entries (rows = targets,
    cols = sources) in CSR order, then one self loop per node."""
    rowptr = graph.rowptr.to(device)
    loops = torch.arange(graph.n_rows, device=device)
    dst = torch.repeat_interleave(loops, rowptr[1:] - rowptr[:-1])
    return torch.cat([graph.col.to(device=device, dtype=torch.int64), loops]), torch.cat([dst, loops])


def gat_aggregate_composed(graph, h, a_src, a_dst, heads, negative_slope=0.2, keep_bits=None, p=0.0, bias=None):
    """`gat_aggregate` as torch_geometric's GATConv composes it, statement by statement in torch (alpha [E, heads] and the
    messages [E, heads, c] are materialised), on any device and dtype: the path of shapes outside `gat_supported`, the
    baseline of scripts/perf_gat_layer.py, and the float64 reference on CPU tensors."""
    _gat_args(graph, h, a_src, a_dst, heads, keep_bits, p, bias)
    n, c = h.shape[0], h.shape[1] // heads
    src, dst = gat_edges(graph, h.device)
    alpha = torch.nn.functional.leaky_relu(a_src[src] + a_dst[dst], negative_slope)
    index = dst[:, None].expand(-1, heads)
    amax = torch.zeros_like(a_dst).scatter_reduce(0, index, alpha.detach(), "amax", include_self=False)
    alpha = (alpha - amax[dst]).exp()
    alpha = alpha / (torch.zeros_like(a_dst).index_add_(0, dst, alpha) + 1e-16)[dst]
    if keep_bits is not None:
        keep = unpack_bits(keep_bits.to(h.device), src.numel() * heads).view(-1, heads)
        alpha = alpha * keep.to(h.dtype) * (1.0 / (1.0 - p))
    out = torch.zeros(n, heads, c, dtype=h.dtype, device=h.device).index_add_(0, dst, h.view(n, heads, c)[src] * alpha[:, :, None])
    out = out.view(n, heads * c)
    return out if bias is None else out + bias


class _GatAggregate(torch.autograd.Function):
    """gcr_gat_fwd_f32 / gcr_gat_bwd_f32: beside the inputs and the bitmap only lse [n, heads] is saved."""

    @staticmethod
    def _col(graph):
        return graph.col if graph.nnz else torch.zeros(4, dtype=torch.int32, device=graph.col.device)

    @staticmethod
    def forward(ctx, h, a_src, a_dst, bias, graph, heads, slope, keep_bits, keep_scale):
        h, a_src, a_dst = h.contiguous(), a_src.contiguous(), a_dst.contiguous()
        n, c = h.shape[0], h.shape[1] // heads
        out = torch.empty_like(h)
        lse = torch.empty_like(a_src)
        _lib.call("gcr_gat_fwd_f32", graph.rowptr, _GatAggregate._col(graph), n, h, a_src, a_dst, heads, c, slope, keep_bits,
                  keep_scale, None if bias is None else bias.contiguous(), out, lse, None, on=h)
        ctx.save_for_backward(h, a_src, a_dst, lse)
        ctx.graph, ctx.hp, ctx.keep_bits = graph, (heads, c, slope, keep_scale), keep_bits
        return out

    @staticmethod
    def backward(ctx, g):
        h, a_src, a_dst, lse = ctx.saved_tensors
        graph, keep_bits = ctx.graph, ctx.keep_bits
        heads, c, slope, keep_scale = ctx.hp
        n = h.shape[0]
        g = g.contiguous()
        gt = graph.t
        perm = None
        if keep_bits is not None:
            perm = graph.mirror_perm() if graph.symmetric else gt.perm_from_transpose
            if perm.numel() == 0:             # no entries: never read, but not NULL beside a bitmap (gcr.h)
                perm = torch.zeros(2, dtype=torch.int64, device=h.device)
        dh, da_src, da_dst = torch.empty_like(h), torch.empty_like(a_src), torch.empty_like(a_dst)
        ws = _lib.workspace("gcr_gat_workspace_bytes", n, graph.nnz, heads, c, device=h.device)
        _lib.call("gcr_gat_bwd_f32", graph.rowptr, _GatAggregate._col(graph), gt.rowptr, _GatAggregate._col(gt), perm, n, h,
                  a_src, a_dst, lse, g, heads, c, slope, keep_bits, keep_scale, dh, da_src, da_dst, ws, on=h)
        dbias = g.sum(dim=0) if ctx.needs_input_grad[3] else None
        return dh, da_src, da_dst, dbias, None, None, None, None, None


def gat_aggregate(graph, h, a_src, a_dst, heads, negative_slope=0.2, keep_bits=None, p=0.0, bias=None):
    """The message passing of GATConv (concat=True, add_self_loops=True) for `graph` [n, n] WITHOUT values and WITHOUT
    diagonal entries (rows = targets, cols = sources; duplicates are separate terms), h [n, heads * c], a_src / a_dst
    [n, heads]: per head, alpha = softmax over {i} + row i of leaky_relu(a_src[j] + a_dst[i]), dropped by `keep_bits`
    (bit (e * heads + head) of `edge_mask_bits((nnz + n) * heads, p, seed, device)`, e in CSR order, the self loop of node
    i at nnz + i) and scaled by 1 / (1 - p), out_i = sum_j alpha_ij h_j + bias.  One autograd node over gcr_gat_fwd_f32 /
    gcr_gat_bwd_f32 (include/gcr.h), differentiable in h, a_src, a_dst and bias, which writes nothing per edge and saves
    lse [n, heads] only; bitwise reproducible.  Shapes outside `gat_supported`, other dtypes than float32, CPU tensors
    and n = 0 run `gat_aggregate_composed`."""
    _gat_args(graph, h, a_src, a_dst, heads, keep_bits, p, bias)
    c = h.shape[1] // heads
    if not (h.is_cuda and h.dtype == torch.float32 and h.shape[0] > 0 and gat_supported(heads, c)):
        return gat_aggregate_composed(graph, h, a_src, a_dst, heads, negative_slope, keep_bits, p, bias)
    keep_bits = None if keep_bits is None else keep_bits.contiguous()
    return _GatAggregate.apply(h, a_src, a_dst, bias, graph, int(heads), float(negative_slope), keep_bits, 1.0 / (1.0 - p))


# ---------------------------------------------------------------------------------------------
# GraphSAGE: one SAGEConv layer with its activation and dropout (graphsage.py:28-30)
# ---------------------------------------------------------------------------------------------
SAGE_ACTS = {"none": 0, "relu": 1, "gelu": 2}          # gcr_sage_*'s `act`; gelu is the exact (erf) form, F.gelu's default

# (din, dout) pairs that `sage_layer` hands to `sage_layer_composed` although the kernels serve them: a pair belongs here
# when scripts/perf_sage_layer.py does not show the fused layer's p10 - p90 band disjoint from, and below, the composed
# one's.  Measured (EXPERIMENTS.md, "GraphSAGE: the fused SAGEConv layer"; 1.1M nodes, 20M entries, forward + backward): the
# bands are disjoint in the fused layer's favour at all nine pairs, from 2.18 against 5.81 ms at (32, 32) to 7.14 against
# 9.96 ms at (128, 128), so the set is empty.  It was not always: with one backward workgroup per CU (64, 128) under gelu took
# 6.74 against 6.58 ms and would have been listed here.
SAGE_COMPOSED_PAIRS = frozenset()


def sage_supported(din, dout):
    """True when the fused kernels (gcr_sage_*) serve a layer [n, din] -> [n, dout]: each width 32, 64 or 128."""
    return bool(_lib.call("gcr_sage_supported", int(din), int(dout)))


def sage_mean_graph(edge_index, num_nodes, device):
    """The [n, n] operator of torch_geometric's mean aggregation for `edge_index` int64 [2, E] (edge j -> i =
    (edge_index[0], edge_index[1])): CSR with rows = edge_index[1], cols = edge_index[0], a row's entries in edge_index
    order, duplicates kept (a duplicated edge counts twice in the mean), self loops kept (SAGEConv adds or removes none),
    val = 1 / (entries of the row); a node without in-edges has an empty row, so its mean is 0.  The transpose is built
    with it (`graph.t`, which the backward's dx = A^T p + q walks)."""
    import numpy as np
    ei = torch.as_tensor(edge_index).detach().to(torch.int64).cpu().numpy()
    deg = np.bincount(ei[1], minlength=num_nodes)
    val = (1.0 / deg[ei[1]]).astype(np.float32)
    graph = CsrGraph.from_coo(ei[1], ei[0], val, num_nodes, num_nodes, device)
    graph.t                                       # noqa: B018  (built now, not inside the first backward)
    graph.mean_counts = torch.from_numpy(deg)     # the rows' entry counts: `_sage_mean_torch` divides by them exactly
    return graph


def _sage_mean_torch(graph, x):
    """The mean aggregation where libgcr has no kernel (a CPU tensor, or a dtype other than float32), in x's dtype: the
    rows' sums divided by their counts (the stored float32 reciprocals would put 2^-24 on a float64 run)."""
    counts = getattr(graph, "mean_counts", None)
    if counts is None:
        return _sparse_mm_torch(graph, x)
    rowptr = graph.rowptr.to(x.device)
    rows = torch.repeat_interleave(torch.arange(graph.n_rows, device=x.device), rowptr[1:] - rowptr[:-1])
    sums = torch.zeros_like(x).index_add_(0, rows, x[graph.col.to(device=x.device, dtype=torch.int64)])
    return sums / counts.to(device=x.device, dtype=x.dtype).clamp(min=1)[:, None]


def _sage_args(graph, x, wl, wr, bias, keep_bits, p):
    if x.dim() != 2 or wl.dim() != 2 or wl.shape[1] != x.shape[1] or wr.shape != wl.shape:
        raise ValueError("x must be [n, din] and wl, wr [dout, din]")
    if graph.n_rows != x.shape[0] or graph.n_cols != x.shape[0]:
        raise ValueError("the graph must be [n, n] for x [n, din]")
    if bias is not None and tuple(bias.shape) != (wl.shape[0],):
        raise ValueError("bias must be [dout]")
    if not 0.0 <= p < 1.0:
        raise ValueError("p must be in [0, 1)")
    if keep_bits is not None and (keep_bits.dtype != torch.int32 or keep_bits.numel() < (x.shape[0] * wl.shape[0] + 31) // 32):
        raise ValueError("keep_bits must be int32 words covering n * dout bits")


def sage_layer_composed(graph, x, wl, wr, bias, act, keep_bits=None, p=0.0):
    """`sage_layer` as torch_geometric and graphsage.py:28-30 compose it, statement by statement in torch: the mean
    aggregation (through `spmm` for float32 on the device, torch's sparse product otherwise), lin_l(z) + lin_r(x), the
    activation, the dropout.  Any dtype, CPU tensors, any widths; `act` may also be a callable (another F function)."""
    _sage_args(graph, x, wl, wr, bias, keep_bits, p)
    z = spmm(graph, x) if x.is_cuda and x.dtype == torch.float32 else _sage_mean_torch(graph, x)
    out = torch.nn.functional.linear(z, wl, bias) + torch.nn.functional.linear(x, wr)
    if callable(act):
        out = act(out)
    elif SAGE_ACTS[act] == 1:
        out = torch.relu(out)
    elif SAGE_ACTS[act] == 2:
        out = torch.nn.functional.gelu(out)
    if keep_bits is not None:
        keep = unpack_bits(keep_bits.to(out.device), out.numel()).view_as(out)
        out = out * keep.to(out.dtype) * (1.0 / (1.0 - p))
    return out


class _SageLayer(torch.autograd.Function):
    """gcr_sage_fwd_f32 / gcr_sage_bwd_f32: saves x, wl, wr, h, and the pre-activation only under gelu; the backward re-runs
    the SpMM for z and finishes dx = A^T p + q with the SpMM on A^T."""

    @staticmethod
    def forward(ctx, x, wl, wr, bias, graph, act, keep_bits, keep_scale):
        x, wl, wr = x.contiguous(), wl.contiguous(), wr.contiguous()
        n, din = x.shape
        dout = wl.shape[0]
        z = spmm_into(graph, x, y=torch.empty_like(x))
        h = torch.empty(n, dout, dtype=x.dtype, device=x.device)
        pre = torch.empty_like(h) if act == 2 else None
        ws = _lib.workspace("gcr_sage_workspace_bytes", n, din, dout, device=x.device)
        _lib.call("gcr_sage_fwd_f32", n, x, z, wl, wr, None if bias is None else bias.contiguous(), din, dout, act, keep_bits,
                  keep_scale, h, pre, ws, on=x)
        ctx.save_for_backward(*((x, wl, wr, h) + (() if pre is None else (pre,))))
        ctx.graph, ctx.hp, ctx.keep_bits, ctx.has_bias = graph, (act, keep_scale), keep_bits, bias is not None
        return h

    @staticmethod
    def backward(ctx, g):
        x, wl, wr, h = ctx.saved_tensors[:4]
        pre = ctx.saved_tensors[4] if len(ctx.saved_tensors) == 5 else None
        graph = ctx.graph
        act, keep_scale = ctx.hp
        n, din = x.shape
        dout = wl.shape[0]
        z = spmm_into(graph, x, y=torch.empty_like(x))
        want_dx = ctx.needs_input_grad[0]
        p, q = (torch.empty_like(x), torch.empty_like(x)) if want_dx else (None, None)
        dwl, dwr = torch.empty_like(wl), torch.empty_like(wr)
        dbias = torch.empty(dout, dtype=x.dtype, device=x.device) if ctx.has_bias else None
        ws = _lib.workspace("gcr_sage_workspace_bytes", n, din, dout, device=x.device)
        _lib.call("gcr_sage_bwd_f32", n, x, z, wl, wr, h, pre, g.contiguous(), din, dout, act, ctx.keep_bits, keep_scale, p, q,
                  dwl, dwr, dbias, ws, on=x)
        dx = spmm_into(graph.t, p, acc_in=q, acc_out=torch.empty_like(x)) if want_dx else None
        return dx, dwl, dwr, dbias, None, None, None, None


def sage_layer(graph, x, wl, wr, bias=None, act="relu", keep_bits=None, p=0.0):
    """One hidden layer of GraphSAGE.forward (graphsage.py:28-30) behind one autograd node:
    keep / (1 - p) * act(lin_l(mean_j x_j) + lin_r(x)) for `graph` = `sage_mean_graph(...)` [n, n], x [n, din], wl
    (lin_l.weight), wr (lin_r.weight) [dout, din], bias (lin_l.bias) [dout] or None, act 'none', 'relu' or 'gelu' (exact).
    keep_bits: the dropout's keep bitmap, bit r * dout + c (`pack_bits` / `edge_mask_bits(n * dout, p, seed, device)`
    order); None = no dropout, whatever p.  Differentiable in x, wl, wr and bias; the mean runs as the tuned SpMM into a
    scratch z, forward and again in the backward; x, wl, wr, the output and (gelu only) the pre-activation are kept, where
    the composition keeps z, the pre-activation, the activation's output and a mask.  Bitwise reproducible.  Widths
    outside `sage_supported`, pairs in SAGE_COMPOSED_PAIRS, a callable act, other dtypes than float32, CPU tensors and
    n = 0 run `sage_layer_composed`."""
    _sage_args(graph, x, wl, wr, bias, keep_bits, p)
    pair = (x.shape[1], wl.shape[0])
    if not (x.is_cuda and x.dtype == torch.float32 and x.shape[0] > 0 and not callable(act) and sage_supported(*pair)
            and pair not in SAGE_COMPOSED_PAIRS):
        return sage_layer_composed(graph, x, wl, wr, bias, act, keep_bits, p)
    keep_bits = None if keep_bits is None else keep_bits.contiguous()
    return _SageLayer.apply(x, wl, wr, bias, graph, SAGE_ACTS[act], keep_bits, 1.0 / (1.0 - p) if keep_bits is not None else 1.0)


# ---------------------------------------------------------------------------------------------
# BGRL: one GINConv layer (Linear, ReLU, Linear) with the ReLU and dropout behind it (bgrl_g2l.py:500-505, 525-529)
# ---------------------------------------------------------------------------------------------
# (din, dout) pairs that `gin_layer` hands to `gin_layer_composed` although the kernels serve them: a pair belongs here
# when scripts/perf_gin_layer.py does not show the fused layer's p10 - p90 band disjoint from, and below, the composed
# one's.  Measured (EXPERIMENTS.md, "BGRL: the fused GINConv layer"; 1.1M nodes, 20M entries, forward + backward): the bands
# are disjoint in the fused layer's favour at all nine pairs, from 1.51 against 5.32 ms at (32, 32) to 6.44 against 10.87 ms
# at (128, 128), so the set is empty.
GIN_COMPOSED_PAIRS = frozenset()


def gin_supported(din, dout):
    """True when the fused kernels (gcr_gin_*) serve a layer [n, din] -> [n, dout]: each width 32, 64 or 128."""
    return bool(_lib.call("gcr_gin_supported", int(din), int(dout)))


def gin_sum_graph(edge_index, num_nodes, device):
    """The [n, n] operator of torch_geometric's sum aggregation for `edge_index` int64 [2, E] (edge j -> i =
    (edge_index[0], edge_index[1])): CSR WITHOUT values, rows = edge_index[1], cols = edge_index[0], a row's entries in
    edge_index order, duplicates kept (a duplicated edge counts twice), self loops kept (GINConv adds or removes none).
    The transpose is built with it (`graph.t`, which the backward's dx walks), and so are `graph.edge_of_entry` and
    `graph.t.edge_of_entry` (int64 [E] on the graph's device: entry e of the CSR is edge edge_of_entry[e]), with which
    `gin_edge_keep_bits` brings a per-edge mask in edge_index order into both entry orders."""
    import numpy as np
    ei = torch.as_tensor(edge_index).detach().to(torch.int64).cpu().numpy()
    graph = CsrGraph.from_coo(ei[1], ei[0], None, num_nodes, num_nodes, device, want_perm=True)
    gt = graph.t
    perm = graph.coo_perm.to(graph.device)
    graph.edge_of_entry = perm
    perm_t = getattr(gt, "perm_from_transpose", None)          # the device build keeps it; the host build sorts stably by column
    if perm_t is None:
        perm_t = torch.from_numpy(np.argsort(graph.col.cpu().numpy(), kind="stable"))
    gt.edge_of_entry = perm[perm_t.to(graph.device)]
    return graph


def gin_edge_keep_bits(graph, keep_edges):
    """(keep_bits, keep_bits_t) of `gin_layer` for a per-edge keep mask, bool [E] in the order of the edge_index that
    `gin_sum_graph` was built from (dropout_adj's `rand >= p` mask: EdgeRemoving, bgrl_g2l.py:448-456)."""
    keep_edges = torch.as_tensor(keep_edges).reshape(-1).to(graph.device)
    return tuple(pack_bits(keep_edges[g.edge_of_entry]) for g in (graph, graph.t))


def _gin_sum_torch(graph, x, edge_keep_bits):
    """sum_j x_j over the (kept) entries where libgcr has no kernel (a CPU tensor, or a dtype other than float32)."""
    rowptr = graph.rowptr.to(x.device)
    rows = torch.repeat_interleave(torch.arange(graph.n_rows, device=x.device), rowptr[1:] - rowptr[:-1])
    msg = x[graph.col.to(device=x.device, dtype=torch.int64)]
    if edge_keep_bits is not None:
        msg = msg * unpack_bits(edge_keep_bits.to(x.device), graph.nnz).to(x.dtype)[:, None]
    return torch.zeros_like(x).index_add_(0, rows, msg)


def _gin_args(graph, x, w1, b1, w2, b2, keep_bits, p, edge_keep_bits):
    if x.dim() != 2 or w1.dim() != 2 or w1.shape[1] != x.shape[1] or tuple(w2.shape) != (w1.shape[0], w1.shape[0]):
        raise ValueError("x must be [n, din], w1 [dout, din] and w2 [dout, dout]")
    if tuple(b1.shape) != (w1.shape[0],) or tuple(b2.shape) != (w1.shape[0],):
        raise ValueError("b1 and b2 must be [dout]")
    if graph.n_rows != x.shape[0] or graph.n_cols != x.shape[0]:
        raise ValueError("the graph must be [n, n] for x [n, din]")
    if not 0.0 <= p < 1.0:
        raise ValueError("p must be in [0, 1)")
    if keep_bits is not None and (keep_bits.dtype != torch.int32 or keep_bits.numel() < (x.shape[0] * w1.shape[0] + 31) // 32):
        raise ValueError("keep_bits must be int32 words covering n * dout bits")
    if edge_keep_bits is not None and (edge_keep_bits.dtype != torch.int32 or edge_keep_bits.numel() * 32 < graph.nnz):
        raise ValueError("edge_keep_bits must be int32 words covering the graph's entries")


def gin_layer_composed(graph, x, w1, b1, w2, b2, eps=0.0, keep_bits=None, p=0.0, edge_keep_bits=None, edge_keep_bits_t=None):
    """`gin_layer` as torch_geometric and bgrl_g2l.py:525-529 compose it, statement by statement in torch: the sum
    aggregation over the kept edges (through `spmm` for float32 on the device, an index_add otherwise), out + (1 + eps) x,
    Linear, ReLU, Linear, the ReLU, the dropout.  Any dtype, CPU tensors, any widths."""
    _gin_args(graph, x, w1, b1, w2, b2, keep_bits, p, edge_keep_bits)
    if x.is_cuda and x.dtype == torch.float32 and x.shape[0] > 0:
        out = spmm(graph, x, keep_bits=edge_keep_bits, keep_bits_t=edge_keep_bits_t)
    else:
        out = _gin_sum_torch(graph, x, edge_keep_bits)
    out = out + (1.0 + eps) * x
    out = torch.nn.functional.linear(out, w1, b1)
    out = torch.relu(out)
    out = torch.nn.functional.linear(out, w2, b2)
    out = torch.relu(out)
    if keep_bits is not None:
        keep = unpack_bits(keep_bits.to(out.device), out.numel()).view_as(out)
        out = out * keep.to(out.dtype) * (1.0 / (1.0 - p))
    return out


class _GinLayer(torch.autograd.Function):
    """gcr_gin_fwd_f32 / gcr_gin_bwd_f32: saves s = (1 + eps) x + A x, h and the weights (w1, b1, w2: the backward
    recomputes the hidden activation from them), nothing else; the backward finishes dx = (1 + eps) ds + A^T ds with the
    SpMM on A^T."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, graph, eps, keep_bits, keep_scale, edge_keep_bits, edge_keep_bits_t):
        x, w1, b1, w2, b2 = (t.contiguous() for t in (x, w1, b1, w2, b2))
        n, din = x.shape
        dout = w1.shape[0]
        root = x if eps == 0.0 else x * (1.0 + eps)
        s = spmm_into(graph, x, acc_in=root, acc_out=torch.empty_like(x), keep_bits=edge_keep_bits)
        h = torch.empty(n, dout, dtype=x.dtype, device=x.device)
        ws = _lib.workspace("gcr_gin_workspace_bytes", n, din, dout, device=x.device)
        _lib.call("gcr_gin_fwd_f32", n, s, w1, b1, w2, b2, din, dout, keep_bits, keep_scale, h, ws, on=x)
        ctx.save_for_backward(s, h, w1, b1, w2)
        ctx.graph, ctx.hp, ctx.edge_keep_bits_t = graph, (eps, keep_scale), edge_keep_bits_t
        return h

    @staticmethod
    def backward(ctx, g):
        s, h, w1, b1, w2 = ctx.saved_tensors
        eps, keep_scale = ctx.hp
        n, din = s.shape
        dout = w1.shape[0]
        want_dx = ctx.needs_input_grad[0]
        ds = torch.empty_like(s) if want_dx else None
        dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
        db1, db2 = torch.empty_like(b1), torch.empty_like(b1)
        ws = _lib.workspace("gcr_gin_workspace_bytes", n, din, dout, device=s.device)
        _lib.call("gcr_gin_bwd_f32", n, s, w1, b1, w2, h, g.contiguous(), din, dout, keep_scale, ds, dw1, db1, dw2, db2, ws,
                  on=s)
        dx = None
        if want_dx:
            root = ds if eps == 0.0 else ds * (1.0 + eps)
            dx = spmm_into(ctx.graph.t, ds, acc_in=root, acc_out=torch.empty_like(ds), keep_bits=ctx.edge_keep_bits_t)
        return dx, dw1, db1, dw2, db2, None, None, None, None, None, None


def gin_layer(graph, x, w1, b1, w2, b2, eps=0.0, keep_bits=None, p=0.0, edge_keep_bits=None, edge_keep_bits_t=None):
    """One layer of BGRL's GConv.forward (bgrl_g2l.py:525-529) behind one autograd node:
    keep / (1 - p) * relu(relu(s w1^T + b1) w2^T + b2),  s = (1 + eps) x + sum over the kept edges into i of x_j,
    for `graph` = `gin_sum_graph(...)` [n, n], x [n, din], w1 / b1 (nn.0) [dout, din] / [dout], w2 / b2 (nn.2)
    [dout, dout] / [dout].  keep_bits: the dropout's keep bitmap, bit r * dout + c (`pack_bits` /
    `edge_mask_bits(n * dout, p, seed, device)` order); None = no dropout, whatever p.  edge_keep_bits / edge_keep_bits_t:
    EdgeRemoving's mask in the entry order of `graph` and of `graph.t` (`gin_edge_keep_bits`); the second is needed when x
    takes a gradient.  Differentiable in x and the four parameters; s runs as the tuned SpMM with x as its `acc_in`; s, the
    output and the weights are kept, where the composition keeps the aggregate, s, both pre-activations, the hidden
    activation, the output before the dropout and a mask.  Bitwise reproducible.  Widths outside `gin_supported`, pairs in
    GIN_COMPOSED_PAIRS, other dtypes than float32, CPU tensors and n = 0 run `gin_layer_composed`."""
    _gin_args(graph, x, w1, b1, w2, b2, keep_bits, p, edge_keep_bits)
    pair = (x.shape[1], w1.shape[0])
    if not (x.is_cuda and x.dtype == torch.float32 and x.shape[0] > 0 and gin_supported(*pair) and pair not in GIN_COMPOSED_PAIRS):
        return gin_layer_composed(graph, x, w1, b1, w2, b2, eps, keep_bits, p, edge_keep_bits, edge_keep_bits_t)
    if edge_keep_bits is not None and edge_keep_bits_t is None:
        _need_mask_t(x)
    keep_bits = None if keep_bits is None else keep_bits.contiguous()
    return _GinLayer.apply(x, w1, b1, w2, b2, graph, float(eps), keep_bits, 1.0 / (1.0 - p) if keep_bits is not None else 1.0,
                           edge_keep_bits, edge_keep_bits_t)


# ---------------------------------------------------------------------------------------------
# Barlow Twins: redundancy reduction over two full-batch views (univariate/gbt.py:203-228, 386-395)
# ---------------------------------------------------------------------------------------------
BT_WIDTHS = (32, 64, 96, 128, 256)


def column_stats(x):
    """(mean, std) of the columns of a float32 [n, d] device tensor, std unbiased (`x.mean(dim=0)`, `x.std(dim=0)`, gbt.py:
    209-210) from one pass over the rows (gcr_col_stats_f32: Welford on shifted values per thread, Chan merges in a fixed order;
    bitwise reproducible).  n >= 2, d % 4 == 0, d <= 1024.  Not differentiable."""
    _lib.require_cuda(x)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 2:
        raise ValueError("column_stats needs a float32 [n, d] tensor with n >= 2")
    x = x.detach().contiguous()
    n, d = x.shape
    out = torch.empty(2, d, dtype=torch.float32, device=x.device)
    ws = _lib.workspace("gcr_col_stats_workspace_bytes", n, d, device=x.device)
    _lib.call("gcr_col_stats_f32", x, n, d, out[0], out[1], ws, on=x)
    return out[0], out[1]


def bt_supported(d):
    """True when the fused kernels (gcr_bt_*) serve views of width d: 32, 64, 96, 128 or 256."""
    return int(d) in BT_WIDTHS


def _bt_args(h1, h2, lambda_, batch_norm):
    if h1.dim() != 2 or h1.shape != h2.shape or h1.dtype != h2.dtype or h1.device != h2.device:
        raise ValueError("bt_loss needs two [n, d] views of one shape, dtype and device")
    if h1.shape[0] < (2 if batch_norm else 1):
        raise ValueError("bt_loss needs n >= 2 rows (n >= 1 without batch_norm)")
    return 1.0 / h1.shape[1] if lambda_ is None else float(lambda_)


def bt_cross_correlation_composed(h1, h2, batch_norm=True, eps=1e-15):
    """c [d, d] of gbt.py:208-213 as the reference writes it: the standardised views' (or the raw views') product over n."""
    batch_size = h1.size(0)
    if batch_norm:
        z1_norm = (h1 - h1.mean(dim=0)) / (h1.std(dim=0) + eps)
        z2_norm = (h2 - h2.mean(dim=0)) / (h2.std(dim=0) + eps)
        return (z1_norm.T @ z2_norm) / batch_size
    return h1.T @ h2 / batch_size


def bt_loss_composed(h1, h2, lambda_=None, batch_norm=True, eps=1e-15):
    """`bt_loss` as the reference writes it (gbt.py:203-217), statement by statement in torch, on any device and dtype: the
    path of widths outside `bt_supported` and the baseline of scripts/perf_bt_loss.py."""
    lambda_ = _bt_args(h1, h2, lambda_, batch_norm)
    feature_dim = h1.size(1)
    c = bt_cross_correlation_composed(h1, h2, batch_norm, eps)
    off_diagonal_mask = ~torch.eye(feature_dim, device=h1.device).bool()
    loss = (1 - c.diagonal()).pow(2).sum()
    return loss + lambda_ * c[off_diagonal_mask].pow(2).sum()


def bt_forward_raw(h1, h2, lambda_, batch_norm=True, eps=1e-15):
    """gcr_bt_fwd_f32 on contiguous float32 device views -> (loss [1], c [d, d], stats [4, d]: mean1, std1, mean2, std2;
    not written without batch_norm)."""
    n, d = h1.shape
    dev = h1.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    c = torch.empty(d, d, dtype=torch.float32, device=dev)
    stats = torch.zeros(4, d, dtype=torch.float32, device=dev)
    ws = _lib.workspace("gcr_bt_workspace_bytes", n, d, device=dev)
    _lib.call("gcr_bt_fwd_f32", h1, h2, n, d, lambda_, eps, bool(batch_norm), stats, c, loss, ws, on=dev)
    return loss, c, stats


def bt_backward_raw(h1, h2, lambda_, batch_norm, eps, stats, c, g, want1=True, want2=True):
    """gcr_bt_bwd_f32 -> (g_h1 or None, g_h2 or None) for the upstream device scalar g (float32 [1])."""
    n, d = h1.shape
    dev = h1.device
    g1 = torch.empty_like(h1) if want1 else None
    g2 = torch.empty_like(h2) if want2 else None
    ws = _lib.workspace("gcr_bt_workspace_bytes", n, d, device=dev)
    _lib.call("gcr_bt_bwd_f32", h1, h2, n, d, lambda_, eps, bool(batch_norm), stats, c, g, g1, g2, ws, on=dev)
    return g1, g2


class _BtLoss(torch.autograd.Function):
    """gcr_bt_fwd_f32 / gcr_bt_bwd_f32: beside the two inputs only stats [4, d] and c [d, d] are saved."""

    @staticmethod
    def forward(ctx, h1, h2, lambda_, batch_norm, eps):
        h1, h2 = h1.contiguous(), h2.contiguous()
        loss, c, stats = bt_forward_raw(h1, h2, lambda_, batch_norm, eps)
        ctx.save_for_backward(h1, h2, stats, c)
        ctx.hp = (lambda_, batch_norm, eps)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        h1, h2, stats, c = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).contiguous()
        g1, g2 = bt_backward_raw(h1, h2, *ctx.hp, stats, c, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return g1, g2, None, None, None


def bt_loss(h1, h2, lambda_=None, batch_norm=True, eps=1e-15):
    """The Barlow Twins loss of two float32 [n, d] device views, univariate/gbt.py:203-217:
        z = (h - h.mean(0)) / (h.std(0) + eps)   (batch_norm; otherwise z = h),   c = z1^T z2 / n,
        loss = sum_j (1 - c_jj)^2 + lambda_ sum_{j != k} c_jk^2,   lambda_ = None: 1 / d
    as ONE autograd node over gcr_bt_fwd_f32 / gcr_bt_bwd_f32 (include/gcr.h has the backward's formulas): five launches
    forward and two backward, three of them over the rows; z is never written and only the statistics and c are saved.
    Returns a 0-d device tensor; every output is bitwise reproducible.  The loss of (h2, h1) is the same number (c^T has c's
    diagonal and off-diagonal sum of squares), so `WithinEmbedContrast` needs one evaluation.  A column of exactly zero
    std gets a zero gradient column where the reference's autograd gives one of magnitude 1 / eps (or NaN, by the torch
    version's std backward); `bt_loss_composed` keeps the reference's behaviour.  Widths
    outside `bt_supported(d)` run `bt_loss_composed`."""
    _lib.require_cuda(h1, h2)
    lam = _bt_args(h1, h2, lambda_, batch_norm)
    if h1.dtype != torch.float32:
        raise ValueError("bt_loss needs float32 views")
    if not bt_supported(h1.shape[1]):
        return bt_loss_composed(h1, h2, lam, batch_norm, eps)
    return _BtLoss.apply(h1, h2, lam, bool(batch_norm), float(eps))
