"""What the row-op and optimiser path tests share (tests/test_rowops_paths_gpu.py, tests/test_optim_paths_gpu.py and
tests/test_rowops_rules_cpu.py): the comparison rule, the float64 restatements and the case builders.  numpy / torch on
the CPU only; nothing here touches a device.

The rule, the project's (restated from tests/diffuse_rules.py because f64_pins.FAMILIES is fixed):
    err / S <= max(4 x drift, 2^-20)  and  err / S <= 1e-5,
S = max |f64| of the output, drift = the float32 error of the SAME restatement on the SAME inputs, on the CPU.  Two outputs
span twelve decades (1 / eps next to 1 / norm) and are compared row by row, each row against its own scale, with the
drift per row too: `row_inv_norm` (`check_rows`) and the eps-clamped row of `normalize_bwd*` (`check(apart=...)`: that row
is inv * g (+ g_raw) with inv = 1e12; it is compared against its own scale and left out of the others' S).

Every restatement takes the arrays the kernel is handed (float32) and a dtype; the float64 run is the reference, the
float32 run the drift.  tests/test_rowops_rules_cpu.py holds each against plain float64 autograd.

The shapes are chosen against the launch constants below; each names the source line it restates, and the CPU test
checks the arithmetic (that n gives a second grid-stride trip, which remainder of an unrolled loop a case lands in ...)."""
import functools

import numpy as np
import torch

FLOOR, NORTH_STAR = 2.0 ** -20, 1e-5
EPS = 1e-12

# gcr_infonce.hip, gcr_row_inv_norm_f32 / gcr_pos_logit_f32 / gcr_normalize_bwd_f32: `want = (n + 15) / 16`, grid
# `want > 8192 ? 8192 : want`, 16 rows per workgroup (`blockIdx.x * 16 + (threadIdx.x >> 4)`)
INFONCE_WGS, INFONCE_ROWS = 8192, 16
# gcr_infonce_pos_bwd_f32: `want = (mx + 3) / 4`, the same cap, one wave per anchor (`blockIdx.x * 4 + (threadIdx.x >> 6)`)
POS_BWD_ROWS = 4
# gcr_dense.hip, row_grid(n, 16): `gcr_grid((n + rows - 1) / rows, 16384)` (normalize_bwd_n / _raw, rows_dot_vec)
ROW_GRID_WGS, ROW_GRID_ROWS = 16384, 16
# gcr_dense.hip, gram_blocks(n): `gcr_grid((n + 255) / 256, 1024)` (gram_tn, weighted_colsum)
GRAM_WGS, GRAM_MIN_ROWS = 1024, 256
# gcr_ops.hip, ops_grid(n, 4): `g > 65536 ? 65536 : g`, one wave per id (gather_rows / scatter_add_rows)
OPS_WGS, GATHER_ROWS = 65536, 4

SECOND_TRIP_INFONCE = INFONCE_WGS * INFONCE_ROWS + 5          # 131077 rows: the first 5 workgroups' waves go round twice
SECOND_TRIP_POS_BWD = INFONCE_WGS * POS_BWD_ROWS + 5          # 32773
SECOND_TRIP_ROW_GRID = ROW_GRID_WGS * ROW_GRID_ROWS + 5       # 262149
OVER_CAP_GRAM = GRAM_WGS * GRAM_MIN_ROWS + 3                  # 262147: 1024 workgroups of 258 (gram) / 257 (colsum) rows
SECOND_TRIP_GATHER = OPS_WGS * GATHER_ROWS + 5                # 262149 ids

GRAM_DIMS = (32, 64, 96, 128)
GRAM_PAIRS = tuple((dx, dg) for dx in GRAM_DIMS for dg in GRAM_DIMS)
GRAM_SMALL_N = (1, 2, 15, 16, 17, 257, 513)                   # around the 8-pair (16-row) unroll; two and three workgroups


def trips(n, rows_per_wg, cap):
    """Grid-stride trips of the busiest workgroup: ceil(n / (workgroups x rows per workgroup))."""
    wgs = min(-(-n // rows_per_wg), cap)
    return -(-n // (wgs * rows_per_wg))


def gram_launch(n):
    """(workgroups, rows per workgroup) of gcr_gram_tn_f32: `per = ((n + nb - 1) / nb + 1) & ~1`."""
    nb = max(1, min(-(-n // GRAM_MIN_ROWS), GRAM_WGS))
    return nb, ((-(-n // nb)) + 1) & ~1


def gram_masked_tiles(dx, dg):
    """gram_tn_kernel<TX, TG>: NTILE = TX TG tiles over four waves, PER_WAVE = (NTILE + 3) / 4 each.  Returns (per_wave,
    the waves whose LAST tile slot is masked by `tile < NTILE`)."""
    ntile = (dx // 32) * (dg // 32)
    per_wave = (ntile + 3) // 4
    return per_wave, tuple(w for w in range(4) if w + 4 * (per_wave - 1) >= ntile)


def colsum_launch(n, d):
    """(workgroups, rows per workgroup, dp, step) of gcr_weighted_colsum_f32: `per = (n + nb - 1) / nb`, dp = d rounded up
    to a power of two, step = 256 / dp rows abreast."""
    nb = max(1, min(-(-n // GRAM_MIN_ROWS), GRAM_WGS))
    dp = 1
    while dp < d:
        dp <<= 1
    return nb, -(-n // nb), dp, 256 // dp


def colsum_remainders(n, d):
    """The set of (rows one thread sums) % 4 over every workgroup and lane row: what is left to the loop after
    weighted_colsum_kernel's unrolled-by-four one (`for (; r + 3 * step < r1; r += 4 * step)`)."""
    nb, per, _, step = colsum_launch(n, d)
    out = set()
    for b in range(nb):
        r0, r1 = b * per, min(n, (b + 1) * per)
        for lane_row in range(step):
            out.add(max(0, -(-(r1 - r0 - lane_row) // step)) % 4)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).astype(np.float64)


def check(got, ref, f32, tag, apart=None, scale=None):
    """The rule with one scale S = max |ref| (or `scale`, for a declared ill-conditioned case).  apart: a boolean row mask;
    those rows are compared by `check_rows` and left out of S.  Prints every figure before asserting."""
    got, ref, f32 = _f64(got), _f64(ref), _f64(f32)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    if apart is not None and apart.any():
        check_rows(got[apart], ref[apart], f32[apart], tag + " clamped rows")
        got, ref, f32 = got[~apart], ref[~apart], f32[~apart]
    s = float(np.abs(ref).max()) if scale is None else float(scale)
    if s == 0.0:
        print(f"ROWOPS {tag}: the reference is all zeros; max |got| {float(np.abs(got).max()) if got.size else 0.0:.3g}")
        assert not got.size or not np.abs(got).max(), tag
        return 0.0
    err = float(np.abs(got - ref).max()) / s
    drift = float(np.abs(f32 - ref).max()) / s
    bound = max(4.0 * drift, FLOOR)
    print(f"ROWOPS {tag}: err/S {err:.3g} bound {bound:.3g} ratio {err / bound:.3f} (drift {drift:.3g}, S {s:.3g})")
    assert np.isfinite(got).all() and err <= bound and err <= NORTH_STAR, tag
    return err / bound


def check_rows(got, ref, f32, tag):
    """The rule row by row: row r against S_r = max |ref_r|, with its own drift.  An all-zero reference row must be all
    zero.  Prints the worst row before asserting."""
    got, ref, f32 = (_f64(a).reshape(len(a), -1) for a in (got, ref, f32))
    s = np.abs(ref).max(1)
    zero = s == 0.0
    assert not np.abs(got[zero]).max(initial=0.0), tag
    s = np.where(zero, 1.0, s)
    err = np.abs(got - ref).max(1) / s
    bound = np.maximum(4.0 * np.abs(f32 - ref).max(1) / s, FLOOR)
    ratio = err / bound
    r = int(np.argmax(ratio)) if ratio.size else 0
    if ratio.size:
        print(f"ROWOPS {tag}: worst row {r}: err/S {err[r]:.3g} bound {bound[r]:.3g} ratio {ratio[r]:.3f} (S {s[r]:.3g}); "
              f"largest err/S {err.max():.3g}")
    assert np.isfinite(got).all() and (err <= bound).all() and (err <= NORTH_STAR).all(), tag
    return float(ratio.max(initial=0.0))


def drift_of(f32, ref, apart=None):
    """The drift `check` will use, relative to S (for the CPU test)."""
    f32, ref = _f64(f32), _f64(ref)
    if apart is not None:
        f32, ref = f32[~apart], ref[~apart]
    return float(np.abs(f32 - ref).max()) / float(np.abs(ref).max())


def row_drift_of(f32, ref):
    f32, ref = (_f64(a).reshape(len(a), -1) for a in (f32, ref))
    s = np.abs(ref).max(1)
    return np.abs(f32 - ref).max(1) / np.where(s == 0.0, 1.0, s)


# ------------------------------------------------------------------------------------------------------------------
# the restatements: float32 arrays in, a float64 array out, computed in `dtype`
# ------------------------------------------------------------------------------------------------------------------
def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _out(t):
    return t.detach().double().numpy()


def inv_norm(x, eps, dtype):
    """1 / clamp(norm, eps); eps is the float32 the entry is handed."""
    return _out(1.0 / torch.linalg.vector_norm(_t(x, dtype), dim=1).clamp_min(float(np.float32(eps))))


def _scaled(a, s, dtype):
    a = _t(a, dtype)
    return a if s is None else a * _t(s, dtype)[:, None]


def pos_logit(a, sa, b, sb, pos, scale, dtype):
    """scale * (a sa)[i] . (b sb)[p], p = pos[i] (i when pos is None); NaN where p is outside [0, n)."""
    at, bt = _scaled(a, sa, dtype), _scaled(b, sb, dtype)
    p = torch.arange(len(a)) if pos is None else torch.from_numpy(pos)
    ok = (p >= 0) & (p < len(b))
    out = torch.full((len(a),), float("nan"), dtype=dtype)
    out[ok] = float(np.float32(scale)) * (at[ok] * bt[p[ok]]).sum(1)
    return _out(out)


def pos_bwd(x, sx, y, sy, pos, coef, inv_tau, gx_in, gy_in, dtype):
    """(gx_in + c_i (y sy)[p_i], gy_in + index_add over p of c_i (x sx)[i]), c = coef * inv_tau; ids outside [0, ny) are
    skipped on both sides."""
    xt, yt = _scaled(x, sx, dtype), _scaled(y, sy, dtype)
    p = torch.arange(len(x)) if pos is None else torch.from_numpy(pos)
    ok = (p >= 0) & (p < len(y))
    c = (_t(coef, dtype) * float(np.float32(inv_tau)))[:, None]
    gx, gy = _t(gx_in, dtype).clone(), _t(gy_in, dtype).clone()
    gx[ok] += c[ok] * yt[p[ok]]
    gy.index_add_(0, p[ok], c[ok] * xt[ok])
    return _out(gx), _out(gy)


def normalize_bwd(x, inv, g, dtype):
    """gcr_normalize_bwd_f32 from the raw rows: inv (g - xhat <xhat, g>), xhat = x inv."""
    xt, it, gt = _t(x, dtype), _t(inv, dtype)[:, None], _t(g, dtype)
    xh = xt * it
    return _out(it * (gt - xh * (xh * gt).sum(1, keepdim=True)))


def normalize_bwd_n(nrm, inv, g, g_raw, dtype, from_raw=False):
    """gcr_normalize_bwd_n_f32 / _raw_f32: (g - n <n, g>) inv (+ g_raw); from_raw: `nrm` holds the raw rows, n = raw inv."""
    nt, it, gt = _t(nrm, dtype), _t(inv, dtype)[:, None], _t(g, dtype)
    if from_raw:
        nt = nt * it
    out = (gt - nt * (nt * gt).sum(1, keepdim=True)) * it
    return _out(out if g_raw is None else out + _t(g_raw, dtype))


def normalize_autograd(x, g, g_raw=None):
    """The same by float64 autograd of F.normalize on the raw rows (the CPU test's yardstick for the three above)."""
    xt = _t(x, torch.float64).requires_grad_(True)
    torch.nn.functional.normalize(xt, dim=1, eps=EPS).backward(_t(g, torch.float64))
    return _out(xt.grad if g_raw is None else xt.grad + _t(g_raw, torch.float64))


def rows_dot_vec(x, v, dtype):
    return _out(_t(x, dtype) @ _t(v, dtype))


def weighted_colsum(x, w, dtype):
    """w @ x, written as a column sum of the scaled rows: torch sums a column pairwise, where its float32 vector-matrix
    product adds 262147 rows one after the other and drifts by 3.8e-6 of S (over the 1e-5 / 4 a case may have)."""
    return _out((_t(w, dtype)[:, None] * _t(x, dtype)).sum(0))


def gram(x, g, dtype):
    return _out(_t(x, dtype).t() @ _t(g, dtype))


def gather(table, idx):
    """`table[idx]` as functional.gather_rows documents it: an id outside [0, N) gives a zero row.  Exact."""
    ok = (idx >= 0) & (idx < len(table))
    out = np.zeros((len(idx), table.shape[1]), dtype=table.dtype)
    out[ok] = table[idx[ok]]
    return out


def scatter(src, idx, n_rows, dtype):
    """index_put(accumulate=True) of the rows whose id is inside [0, N)."""
    ok = torch.from_numpy((idx >= 0) & (idx < n_rows))
    out = torch.zeros(n_rows, src.shape[1], dtype=dtype)
    out.index_put_((torch.from_numpy(idx)[ok],), _t(src, dtype)[ok], accumulate=True)
    return _out(out)


def bitmap(idx, n_bits, words_in):
    """The bitmap as a Python set on top of the words already there (uint32 words, bit b of word b >> 5)."""
    have = {b for b in set(idx.tolist()) if 0 <= b < n_bits}
    out = words_in.copy()
    for b in have:
        out[b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    return out


def csr_of(dense):
    """(rowptr int64, col int32 ascending in a row, val float32) of a dense matrix' non-zeros."""
    r, c = np.nonzero(dense)
    rowptr = np.zeros(dense.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=dense.shape[0]), out=rowptr[1:])
    return rowptr, c.astype(np.int32), dense[r, c].astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# the optimisers
# ------------------------------------------------------------------------------------------------------------------
ADAM_HYPERS = {                                               # (betas, eps, lr, weight_decay)
    "default": ((0.9, 0.999), 1e-8, 1e-2, 0.0),
    "b.5_.9_eps1e-3": ((0.5, 0.9), 1e-3, 1e-2, 1e-4),
    "b1_0": ((0.0, 0.999), 1e-8, 1e-2, 0.0),
    "b2_0": ((0.9, 0.0), 1e-8, 1e-2, 1e-4),
    "lr_0": ((0.9, 0.999), 1e-8, 0.0, 1e-4),
}
# one element; one tail alone; whole float4s + a 3-tail in the second workgroup's reach; 4 x 256 x 3 + 3: three workgroups
# of float4s and the 3-element tail (gcr_ops.hip: `ops_grid(n / 4 + 1, 256)`, tail = n & 3)
ADAM_SIZES = (1, 5, 1027, 4 * 256 * 3 + 3)
# (n_users, d): the item block of a stacked [U + I, d] table starts U d 4 bytes in: 8 mod 16 and 12 mod 16
MISALIGNED = ((7, 50), (1, 3))
N_ITEMS = 9


def adam_steps(p0, grads, hyper, dtype, grad_scale=1.0, state=None):
    """torch.optim.Adam (single-tensor, foreach=False) on the CPU in `dtype`.  grads: one entry per step, each a list of
    float32 pieces that are summed in `dtype`, then scaled by grad_scale (the decay is not scaled: it is the optimiser's).
    state: (step_before, exp_avg, exp_avg_sq) to start from.  Returns float64 dict(p, exp_avg, exp_avg_sq)."""
    betas, eps, lr, wd = hyper
    p = torch.nn.Parameter(_t(p0, dtype).clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    if state is not None:
        opt.state[p] = dict(step=torch.tensor(float(state[0]), dtype=torch.float64), exp_avg=_t(state[1], dtype).clone(),
                            exp_avg_sq=_t(state[2], dtype).clone())
    for pieces in grads:
        g = _t(pieces[0], dtype).clone()
        for extra in pieces[1:]:
            g += _t(extra, dtype)
        p.grad = g * grad_scale if grad_scale != 1.0 else g
        opt.step()
    st = opt.state[p]
    return dict(p=_out(p), exp_avg=_out(st["exp_avg"]), exp_avg_sq=_out(st["exp_avg_sq"]))


def sgd_steps(p0, grads, lr, momentum, wd, dtype):
    """torch.optim.SGD (dampening 0, no nesterov, foreach=False) on the CPU in `dtype`: float64 dict(p[, momentum_buffer])."""
    p = torch.nn.Parameter(_t(p0, dtype).clone())
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=wd, foreach=False)
    for g in grads:
        p.grad = _t(g, dtype).clone()
        opt.step()
    out = dict(p=_out(p))
    if momentum:
        out["momentum_buffer"] = _out(opt.state[p]["momentum_buffer"])
    return out


@functools.lru_cache(maxsize=None)
def adam_case(n, pieces=1, steps=5, seed=0):
    """p0 [n] and `steps` gradients of `pieces` pieces each (float32)."""
    rng = np.random.default_rng([n, pieces, steps, seed])
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = tuple(tuple(rng.standard_normal(n).astype(np.float32) for _ in range(pieces)) for _ in range(steps))
    return p0, grads


@functools.lru_cache(maxsize=None)
def adam_state_case(n, step, seed=0):
    """A state as it stands before step number `step`: p, exp_avg ~ N(0, 0.1), exp_avg_sq in [1e-3, 1) and one gradient."""
    rng = np.random.default_rng([n, step, seed, 11])
    p0, m = rng.standard_normal(n).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    if step == 1:
        m[:], v[:] = 0.0, 0.0
    return p0, m, v, rng.standard_normal(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def stacked_case(n_u, d, steps=5):
    """table [n_u + N_ITEMS, d] and `steps` gradients of the same shape; the optimiser's parameters are the two row blocks."""
    rng = np.random.default_rng([n_u, d, steps])
    table = rng.standard_normal((n_u + N_ITEMS, d)).astype(np.float32)
    return table, tuple(rng.standard_normal(table.shape).astype(np.float32) for _ in range(steps))


# ------------------------------------------------------------------------------------------------------------------
# the case builders: dicts of float32 inputs, `ref` (float64 restatement) and `f32` (the same in float32), shared and
# never written to
# ------------------------------------------------------------------------------------------------------------------
# (n, d): the scalar path (d % 4), a second column trip that only lanes 0 (d = 68) or 0..8 (d = 100) take, four full
# trips (256), and the second grid-stride trip on either path
INV_NORM_SHAPES = ((33, 1), (33, 3), (33, 50), (33, 68), (33, 100), (33, 256), (SECOND_TRIP_INFONCE, 4),
                   (SECOND_TRIP_INFONCE, 5))


@functools.lru_cache(maxsize=None)
def inv_norm_case(n, d):
    """Row 3 is exactly zero and row 7 is 1e-14 everywhere (norm 1e-14 sqrt(d) < eps, and not zero): both clamp to 1 / eps."""
    rng = np.random.default_rng([1, n, d])
    x = (rng.standard_normal((n, d)) * rng.uniform(0.01, 100.0, (n, 1))).astype(np.float32)
    x[3], x[7] = 0.0, 1e-14
    return dict(x=x, ref=inv_norm(x, EPS, torch.float64), f32=inv_norm(x, EPS, torch.float32))


# (m, n, d, pos given, a_scale given, b_scale given)
POS_LOGIT_SHAPES = ((100, 100, 64, False, True, True), (100, 37, 64, True, False, True), (100, 37, 64, True, True, False),
                    (100, 37, 50, True, False, False), (100, 100, 3, False, True, True), (100, 37, 68, True, True, True),
                    (100, 37, 100, True, True, True), (SECOND_TRIP_INFONCE, SECOND_TRIP_INFONCE, 4, False, True, True),
                    (SECOND_TRIP_INFONCE, 1000, 5, True, True, True))


@functools.lru_cache(maxsize=None)
def pos_logit_case(m, n, d, with_pos, with_sa, with_sb):
    """With pos: rows 2 and 5 name -1 and n (NaN there and nowhere else)."""
    rng = np.random.default_rng([2, m, n, d, with_pos, with_sa, with_sb])
    a, b = rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    sa = rng.uniform(0.5, 2.0, m).astype(np.float32) if with_sa else None
    sb = rng.uniform(0.5, 2.0, n).astype(np.float32) if with_sb else None
    pos = None
    if with_pos:
        pos = rng.integers(0, n, m).astype(np.int64)
        pos[2], pos[5] = -1, n
    args = (a, sa, b, sb, pos, 5.0)
    return dict(a=a, sa=sa, b=b, sb=sb, pos=pos, scale=5.0, ref=pos_logit(*args, torch.float64), f32=pos_logit(*args, torch.float32))


HOT_ANCHORS = 300      # anchors that name one table row: several hundred terms keep a sequential float32 sum and an atomic
                       # one both near one ulp of S
# (mx, ny, d, pos given, scales given): d < 64, d no multiple of 64 (one lane trip and a part), and the second trip
POS_BWD_SHAPES = ((700, 90, 1, True, True), (700, 90, 17, True, False), (700, 90, 64, True, True), (700, 90, 100, True, True),
                  (700, 90, 192, True, True), (90, 90, 50, False, True), (SECOND_TRIP_POS_BWD, 4096, 4, True, True))


@functools.lru_cache(maxsize=None)
def pos_bwd_case(mx, ny, d, with_pos, with_scales):
    """pos: uniform over [0, ny) (ordinary repeats), HOT_ANCHORS anchors on row 11, ids -1 and ny on anchors 0..3.  gx and
    gy start from random contents."""
    rng = np.random.default_rng([3, mx, ny, d, with_pos, with_scales])
    x, y = rng.standard_normal((mx, d)).astype(np.float32), rng.standard_normal((ny, d)).astype(np.float32)
    sx = rng.uniform(0.5, 2.0, mx).astype(np.float32) if with_scales else None
    sy = rng.uniform(0.5, 2.0, ny).astype(np.float32) if with_scales else None
    coef = rng.standard_normal(mx).astype(np.float32)
    pos = None
    if with_pos:
        pos = rng.integers(0, ny, mx).astype(np.int64)
        pos[rng.choice(np.arange(4, mx), HOT_ANCHORS, replace=False)] = 11
        pos[0], pos[1], pos[2], pos[3] = -1, ny, -1, ny
    gx_in, gy_in = rng.standard_normal((mx, d)).astype(np.float32), rng.standard_normal((ny, d)).astype(np.float32)
    args = (x, sx, y, sy, pos, coef, 5.0, gx_in, gy_in)
    return dict(x=x, sx=sx, y=y, sy=sy, pos=pos, coef=coef, inv_tau=5.0, gx_in=gx_in, gy_in=gy_in,
                ref=pos_bwd(*args, torch.float64), f32=pos_bwd(*args, torch.float32))


def _normalised(n, d, seed):
    """Raw rows z (row 5 exactly zero: clamped), their float32 inverse norms and normalised rows, g and g_raw."""
    rng = np.random.default_rng([4, n, d, seed])
    z = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    z[5] = 0.0
    norm = np.maximum(np.linalg.norm(z.astype(np.float64), axis=1), EPS)
    inv = (1.0 / norm).astype(np.float32)
    nrm = (z / norm[:, None]).astype(np.float32)
    g, g_raw = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    apart = np.zeros(n, dtype=bool)
    apart[5] = True
    return z, inv, nrm, g, g_raw, apart


# (n, d): the stride-16 scalar loop with one lane, one trip and a lane, three trips and two lanes; the second grid-stride
# trip with two column trips
NORMALIZE_BWD_SHAPES = ((37, 1), (37, 17), (37, 50), (37, 64), (SECOND_TRIP_INFONCE, 20))
# d = 1: xhat = +-1 and every output is g - g = 0 in exact arithmetic; what the float64 restatement gives is the rounding
# residue of the float32 `inv` it is handed (below 1e-6 of the terms that cancel).  There is no output scale to be relative
# to, so the case is compared against the scale of those terms, max |inv g|
NORMALIZE_BWD_ILL = {(37, 1): "d = 1: the output is g - xhat <xhat, g> with xhat = +-1, zero but for the rounding of inv"}


@functools.lru_cache(maxsize=None)
def normalize_bwd_case(n, d):
    z, inv, _, g, _, apart = _normalised(n, d, 0)
    out = dict(x=z, inv=inv, g=g, apart=apart, ref=normalize_bwd(z, inv, g, torch.float64), f32=normalize_bwd(z, inv, g, torch.float32),
               scale=None)
    if (n, d) in NORMALIZE_BWD_ILL:
        out["scale"] = float(np.abs(inv[~apart, None].astype(np.float64) * g[~apart]).max())
    return out


# (rows, d, g_raw given): one q trip (4), a second that one lane takes (68), exactly three (192), four (256), the old 100,
# and the second grid-stride trip
NORMALIZE_BWD_N_SHAPES = ((37, 4, True), (37, 68, True), (37, 68, False), (37, 100, True), (37, 192, True), (37, 256, True),
                          (37, 256, False), (SECOND_TRIP_ROW_GRID, 4, True))


@functools.lru_cache(maxsize=None)
def normalize_bwd_n_case(rows, d, with_raw, from_raw):
    z, inv, nrm, g, g_raw, apart = _normalised(rows, d, 1)
    g_raw = g_raw if with_raw else None
    src = z if from_raw else nrm
    return dict(src=src, z=z, inv=inv, g=g, g_raw=g_raw, apart=apart,
                ref=normalize_bwd_n(src, inv, g, g_raw, torch.float64, from_raw),
                f32=normalize_bwd_n(src, inv, g, g_raw, torch.float32, from_raw))


# (n, d): scalar paths of four and nine trips, four float4 trips, the second grid-stride trip, the wrapper's d > 256
ROWS_DOT_VEC_SHAPES = ((77, 50), (77, 130), (77, 256), (SECOND_TRIP_ROW_GRID, 4), (77, 260))
# (n, d): dp = 1; dp = 256 with the loop's four remainders; dp = 64 with mixed remainders; several workgroups; over the cap
COLSUM_SHIFTED = ((OVER_CAP_GRAM, 1),)
COLSUM_SHAPES = ((1000, 1), (8, 200), (9, 200), (10, 130), (11, 256), (23, 50), (700, 129), (OVER_CAP_GRAM, 4), (OVER_CAP_GRAM, 1))


@functools.lru_cache(maxsize=None)
def dot_case(n, d):
    """x [n, d], v [d], w [n]: out = x @ v and colsum = w @ x.  S of the column sums is their largest, about sqrt(n) of
    n cancelling zero-mean terms.  With one column only its |sum| is whatever the draw leaves: at (262147, 1) 141 of
    sum |terms| = 1.7e5, a condition number of 1200 (`colsum_condition`).  On the MI355X the kernel was 2.2e-6 of that S
    away from float64 (EXPERIMENTS.md), 1.8e-9 of the terms it added, while torch's pairwise float32 sum drifts 8e-8: the
    drift is no measure of an honest float32 sum there.  So the cases of COLSUM_SHIFTED get a mean of 0.5 on x and w (the sum
    is n / 4); every other case, (1000, 1) included, keeps zero-mean data of both signs."""
    rng = np.random.default_rng([5, n, d])
    x, v, w = (rng.standard_normal(s).astype(np.float32) for s in ((n, d), (d,), (n,)))
    if (n, d) in COLSUM_SHIFTED:
        x, w = x + np.float32(0.5), w + np.float32(0.5)
    return dict(x=x, v=v, w=w, ref=rows_dot_vec(x, v, torch.float64), f32=rows_dot_vec(x, v, torch.float32),
                ref_colsum=weighted_colsum(x, w, torch.float64), f32_colsum=weighted_colsum(x, w, torch.float32))


def colsum_condition(case):
    """sum_r |w_r x_rc| / |sum_r w_r x_rc| of the column that sets S: how many times larger than S the added terms are."""
    terms = case["w"].astype(np.float64)[:, None] * case["x"]
    c = int(np.abs(case["ref_colsum"]).argmax())
    return float(np.abs(terms[:, c]).sum() / abs(case["ref_colsum"][c]))


@functools.lru_cache(maxsize=None)
def gram_case(n, dx, dg):
    rng = np.random.default_rng([6, n, dx, dg])
    x, g = rng.standard_normal((n, dx)).astype(np.float32), rng.standard_normal((n, dg)).astype(np.float32)
    return dict(x=x, g=g, ref=gram(x, g, torch.float64), f32=gram(x, g, torch.float32))


# (N, d, b, kind): kind "mixed" = uniform ids with -1, -7, N and N + 3 among them; "one_row" = every id is row 5
GATHER_SHAPES = ((50, 1, 300, "mixed"), (50, 100, 300, "mixed"), (50, 130, 300, "mixed"), (50, 100, 300, "one_row"),
                 (1000, 1, SECOND_TRIP_GATHER, "mixed"))


@functools.lru_cache(maxsize=None)
def gather_case(n_rows, d, b, kind):
    rng = np.random.default_rng([7, n_rows, d, b])
    table, up = rng.standard_normal((n_rows, d)).astype(np.float32), rng.standard_normal((b, d)).astype(np.float32)
    if kind == "one_row":
        idx = np.full(b, 5, dtype=np.int64)
    else:
        idx = rng.integers(0, n_rows, b).astype(np.int64)
        idx[1], idx[2], idx[b - 1], idx[b - 2] = -1, n_rows, -7, n_rows + 3
    return dict(table=table, idx=idx, up=up, fwd=gather(table, idx), ref=scatter(up, idx, n_rows, torch.float64),
                f32=scatter(up, idx, n_rows, torch.float32))
