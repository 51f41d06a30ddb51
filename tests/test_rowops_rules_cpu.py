"""tests/rowops_rules.py on a machine without a GPU: every restatement against plain float64 autograd, every shape
constant against the arithmetic it claims, and the float32 drift the rule will use for every case (finite and below
1e-5 / 4 wherever a case is not declared ill-conditioned, so that the 1e-5 clause can be met at all)."""
import numpy as np
import pytest
import torch

import rowops_rules as R

F = torch.nn.functional
MAX_DRIFT = R.NORTH_STAR / 4.0


def test_launch_constants_give_the_trips_they_claim():
    for n in (R.SECOND_TRIP_INFONCE,):
        assert R.trips(n, R.INFONCE_ROWS, R.INFONCE_WGS) == 2 and R.trips(n - 5, R.INFONCE_ROWS, R.INFONCE_WGS) == 1
    assert R.trips(R.SECOND_TRIP_POS_BWD, R.POS_BWD_ROWS, R.INFONCE_WGS) == 2
    assert R.trips(R.SECOND_TRIP_POS_BWD - 5, R.POS_BWD_ROWS, R.INFONCE_WGS) == 1
    assert R.trips(R.SECOND_TRIP_ROW_GRID, R.ROW_GRID_ROWS, R.ROW_GRID_WGS) == 2
    assert R.trips(R.SECOND_TRIP_ROW_GRID - 5, R.ROW_GRID_ROWS, R.ROW_GRID_WGS) == 1
    assert R.trips(R.SECOND_TRIP_GATHER, R.GATHER_ROWS, R.OPS_WGS) == 2
    assert R.trips(R.SECOND_TRIP_GATHER - 5, R.GATHER_ROWS, R.OPS_WGS) == 1
    # every family has its second-trip shape among its cases, and no other case is that large
    assert [s for s in R.INV_NORM_SHAPES if R.trips(s[0], 16, 8192) > 1] == [(R.SECOND_TRIP_INFONCE, 4), (R.SECOND_TRIP_INFONCE, 5)]
    assert sum(R.trips(s[0], 16, 8192) > 1 for s in R.POS_LOGIT_SHAPES) == 2
    assert sum(R.trips(s[0], 4, 8192) > 1 for s in R.POS_BWD_SHAPES) == 1
    assert sum(R.trips(s[0], 16, 8192) > 1 for s in R.NORMALIZE_BWD_SHAPES) == 1
    assert sum(R.trips(s[0], 16, 16384) > 1 for s in R.NORMALIZE_BWD_N_SHAPES) == 1
    assert sum(R.trips(s[0], 16, 16384) > 1 for s in R.ROWS_DOT_VEC_SHAPES) == 1
    assert sum(R.trips(s[2], 4, 65536) > 1 for s in R.GATHER_SHAPES) == 1
    # column trips of the 16-lane loops: float4 path `c = l16 * 4; c += 64`, scalar path `c = l16; c += 16`
    assert {d for _, d in R.INV_NORM_SHAPES if d % 4} == {1, 3, 50, 5} and {68, 100, 256} <= {d for _, d in R.INV_NORM_SHAPES}
    assert [l for l in range(16) if 4 * l + 64 < 68] == [0] and [l for l in range(16) if 4 * l + 64 < 100] == list(range(9))
    assert {s[1] for s in R.NORMALIZE_BWD_N_SHAPES} >= {4, 68, 192, 256}
    assert {s[1] for s in R.NORMALIZE_BWD_SHAPES} >= {1, 17, 50}
    assert {-(-d // 16) for _, d in R.ROWS_DOT_VEC_SHAPES if d % 4} == {4, 9}
    assert max(d for _, d in R.ROWS_DOT_VEC_SHAPES) > 256


def test_gram_launch_and_masked_tiles():
    assert R.gram_launch(R.OVER_CAP_GRAM) == (1024, 258) and R.gram_launch(R.GRAM_WGS * R.GRAM_MIN_ROWS) == (1024, 256)
    assert [R.gram_launch(n) for n in R.GRAM_SMALL_N] == [(1, 2), (1, 2), (1, 16), (1, 16), (1, 18), (2, 130), (3, 172)]
    # n = 1, 15, 17, 257 (129 rows per workgroup of 130 ...) leave the second row of a pair masked: `row < r1`
    assert all(R.gram_launch(n)[1] % 2 == 0 for n in range(1, 3000))
    masked = {p: R.gram_masked_tiles(*p) for p in R.GRAM_PAIRS}
    # tile counts that are no multiple of four leave a wave with a masked slot ...
    assert {p for p, (_, w) in masked.items() if w} == {(32, 32), (32, 64), (64, 32), (32, 96), (96, 32), (64, 96), (96, 64), (96, 96)}
    # ... and with more than one tile per wave that slot is a second or third one, after a live tile on the same wave
    assert {p: m for p, m in masked.items() if m[0] > 1 and m[1]} == {(64, 96): (2, (2, 3)), (96, 64): (2, (2, 3)),
                                                                       (96, 96): (3, (1, 2, 3))}
    # (32, 96) and (96, 32) hold three tiles, one per wave: wave 3 is masked from its first slot on
    assert masked[(32, 96)] == masked[(96, 32)] == (1, (3,))


def test_weighted_colsum_cases_land_where_they_claim():
    want = {(1000, 1): (4, 250, 1, 256), (8, 200): (1, 8, 256, 1), (9, 200): (1, 9, 256, 1), (10, 130): (1, 10, 256, 1),
            (11, 256): (1, 11, 256, 1), (23, 50): (1, 23, 64, 4), (700, 129): (3, 234, 256, 1),
            (R.OVER_CAP_GRAM, 4): (1024, 257, 4, 64), (R.OVER_CAP_GRAM, 1): (1024, 257, 1, 256)}
    assert set(want) == set(R.COLSUM_SHAPES)
    for shape, launch in want.items():
        assert R.colsum_launch(*shape) == launch, shape
    assert [R.colsum_remainders(n, d) for n, d in ((8, 200), (9, 200), (10, 130), (11, 256))] == [{0}, {1}, {2}, {3}]
    assert R.colsum_remainders(23, 50) == {2, 1}                  # lane rows 0..2 sum six rows, lane row 3 five
    assert set(R.COLSUM_SHIFTED) <= set(R.COLSUM_SHAPES) and (1000, 1) not in R.COLSUM_SHIFTED
    assert R.colsum_remainders(1000, 1) == {1, 0}                 # 250 rows over 256 lane rows: one or none each
    assert R.colsum_launch(R.OVER_CAP_GRAM, 4)[1] > R.GRAM_MIN_ROWS
    assert R.colsum_remainders(R.OVER_CAP_GRAM, 4) >= {1, 0}      # 257 rows over 64 lane rows: five for lane row 0, four else


def test_restatements_against_float64_autograd():
    rng = np.random.default_rng(0)
    n, m, d = 23, 31, 10
    a, b = rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    a[4] = 0.0
    # 1 / clamp(norm, eps) is F.normalize's denominator: x * inv == F.normalize(x)
    inv = R.inv_norm(a, R.EPS, torch.float64)
    at = torch.from_numpy(a).double()
    np.testing.assert_allclose(at.numpy() * inv[:, None], F.normalize(at, dim=1, eps=R.EPS).numpy(), rtol=1e-12, atol=0)
    assert inv[4] == 1.0 / float(np.float32(R.EPS))
    # positive logit and its backward: cross_entropy's positive term  -sum_i coef_i * inv_tau * <x_i sx_i, y_p sy_p>
    sx, sy = rng.uniform(0.5, 2, m).astype(np.float32), rng.uniform(0.5, 2, n).astype(np.float32)
    pos, coef = rng.integers(0, n, m).astype(np.int64), rng.standard_normal(m).astype(np.float32)
    pos[:6] = 3
    xt, yt = torch.from_numpy(a).double().requires_grad_(True), torch.from_numpy(b).double().requires_grad_(True)
    logit = 5.0 * ((xt * torch.from_numpy(sx).double()[:, None]) * (yt * torch.from_numpy(sy).double()[:, None])[pos]).sum(1)
    np.testing.assert_allclose(R.pos_logit(a, sx, b, sy, pos, 5.0, torch.float64), logit.detach().numpy(), rtol=1e-12)
    (logit * torch.from_numpy(coef).double()).sum().backward()
    gx_in, gy_in = rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    gx, gy = R.pos_bwd(a, sx, b, sy, pos, coef, 5.0, gx_in, gy_in, torch.float64)
    # the kernel's gradients are those of the SCALED rows (the scale's own chain rule is the caller's): d / d(x sx)
    np.testing.assert_allclose(gx - gx_in, xt.grad.numpy() / sx[:, None], rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(gy - gy_in, yt.grad.numpy() / sy[:, None], rtol=1e-11, atol=1e-12)
    # out-of-range ids: NaN in that row only; skipped by the backward
    bad = pos.copy()
    bad[1], bad[8] = -1, n
    out = R.pos_logit(a, None, b, None, bad, 1.0, torch.float64)
    assert np.isnan(out[[1, 8]]).all() and np.isfinite(np.delete(out, [1, 8])).all()
    gx2, gy2 = R.pos_bwd(a, None, b, None, bad, coef, 1.0, gx_in, gy_in, torch.float64)
    assert np.array_equal(gx2[[1, 8]], gx_in[[1, 8]].astype(np.float64))
    keep = np.ones(m, bool)
    keep[[1, 8]] = False
    _, gy3 = R.pos_bwd(a[keep], None, b, None, bad[keep], coef[keep], 1.0, gx_in[keep], gy_in, torch.float64)
    np.testing.assert_allclose(gy2, gy3, rtol=1e-13)
    # pos None is the diagonal
    np.testing.assert_allclose(R.pos_logit(b, None, b, None, None, 1.0, torch.float64), (b.astype(np.float64) ** 2).sum(1), rtol=1e-14)


@pytest.mark.parametrize("d", [4, 17, 68])
def test_normalise_restatements_are_autograd_of_normalize(d):
    """All three from the float32 inputs the kernels get (inv and the normalised rows are rounded to float32: half an ulp
    each, which the 1e-6 below allows for) against autograd on the raw rows; the clamped row is g / eps (+ g_raw)."""
    z, inv, nrm, g, g_raw, apart = R._normalised(37, d, 3)
    want, want_raw = R.normalize_autograd(z, g), R.normalize_autograd(z, g, g_raw)
    live = ~apart
    s = np.abs(want[live]).max()
    for got, ref in ((R.normalize_bwd(z, inv, g, torch.float64), want),
                     (R.normalize_bwd_n(nrm, inv, g, None, torch.float64), want),
                     (R.normalize_bwd_n(nrm, inv, g, g_raw, torch.float64), want_raw),
                     (R.normalize_bwd_n(z, inv, g, g_raw, torch.float64, from_raw=True), want_raw)):
        assert np.abs(got[live] - ref[live]).max() <= 1e-6 * s
        np.testing.assert_allclose(got[apart], ref[apart], rtol=1e-7)
    assert np.abs(want[apart]).max() > 1e11


def test_exact_restatements():
    rng = np.random.default_rng(1)
    table = rng.standard_normal((9, 3)).astype(np.float32)
    idx = np.array([0, 8, -1, 9, 4, 4, 4, -7, 12], dtype=np.int64)
    ok = (idx >= 0) & (idx < 9)
    out = R.gather(table, idx)
    assert np.array_equal(out[ok], table[idx[ok]]) and not out[~ok].any()
    tt = torch.from_numpy(table).double().requires_grad_(True)
    up = rng.standard_normal((9, 3)).astype(np.float32)
    (tt[torch.from_numpy(idx[ok])] * torch.from_numpy(up[ok]).double()).sum().backward()
    np.testing.assert_allclose(R.scatter(up, idx, 9, torch.float64), tt.grad.numpy(), rtol=1e-14)
    words = np.array([0x80000001, 0, 5], dtype=np.uint32)
    got = R.bitmap(np.array([0, 31, 32, 32, 69, 70, -1, 1 << 40], dtype=np.int64), 70, words)
    assert got.tolist() == [0x80000001, 1, 5 | (1 << 5)]
    dense = np.array([[0, 2, 0], [0, 0, 0], [1, 0, 3]], dtype=np.float32)
    rowptr, col, val = R.csr_of(dense)
    assert rowptr.tolist() == [0, 1, 1, 3] and col.tolist() == [1, 0, 2] and val.tolist() == [2, 1, 3]


def test_optimiser_restatements():
    """adam_steps / sgd_steps are torch's own optimisers; what is restated is the feeding: the pieces summed, the scale on
    the gradient and not on the decay, and a state to start from."""
    p0, grads = R.adam_case(5, pieces=3, steps=2)
    hyper = ((0.9, 0.999), 1e-8, 1e-2, 1e-2)
    betas, eps, lr, wd = hyper
    got = R.adam_steps(p0, grads, hyper, torch.float64, grad_scale=0.5)
    p, m, v = p0.astype(np.float64), np.zeros(5), np.zeros(5)
    for t, pieces in enumerate(grads, 1):
        g = 0.5 * sum(x.astype(np.float64) for x in pieces) + wd * p
        m, v = betas[0] * m + (1 - betas[0]) * g, betas[1] * v + (1 - betas[1]) * g * g
        p = p - lr / (1 - betas[0] ** t) * m / (np.sqrt(v / (1 - betas[1] ** t)) + eps)
    np.testing.assert_allclose(got["p"], p, rtol=1e-13)
    np.testing.assert_allclose(got["exp_avg_sq"], v, rtol=1e-13)
    # a state to start from: two steps == one step, then one from its state at step count 1
    one = R.adam_steps(p0, grads[:1], hyper, torch.float64, grad_scale=0.5)
    two = R.adam_steps(one["p"].astype(np.float32), grads[1:], hyper, torch.float64, grad_scale=0.5,
                       state=(1, one["exp_avg"].astype(np.float32), one["exp_avg_sq"].astype(np.float32)))
    np.testing.assert_allclose(two["p"], p, rtol=1e-6)
    s = R.sgd_steps(p0, [g[0] for g in grads], 0.1, 0.9, 1e-2, torch.float64)
    p, buf = p0.astype(np.float64), None
    for pieces in grads:
        g = pieces[0] + 1e-2 * p
        buf = g if buf is None else 0.9 * buf + g
        p = p - 0.1 * buf
    np.testing.assert_allclose(s["p"], p, rtol=1e-13)
    np.testing.assert_allclose(s["momentum_buffer"], buf, rtol=1e-13)
    assert len(R.MISALIGNED) == 2 and [(u * d * 4) % 16 for u, d in R.MISALIGNED] == [8, 12]
    assert [n % 4 for n in R.ADAM_SIZES] == [1, 1, 3, 3] and R.ADAM_SIZES[-1] // 4 > 2 * 256


def _ok(drift, tag):
    print(f"DRIFT {tag}: {drift:.3g}")
    assert np.isfinite(drift) and drift < MAX_DRIFT, tag


def test_drift_of_the_row_cases():
    for s in R.INV_NORM_SHAPES:
        c = R.inv_norm_case(*s)
        _ok(float(R.row_drift_of(c["f32"], c["ref"]).max()), f"inv_norm{s}")
        assert c["ref"][3] == c["ref"][7] == 1.0 / float(np.float32(R.EPS)) and np.abs(c["x"][7]).min() > 0
    for s in R.POS_LOGIT_SHAPES:
        c = R.pos_logit_case(*s)
        live = ~np.isnan(c["ref"])
        assert (~live).sum() == (2 if s[3] else 0) and np.array_equal(np.isnan(c["f32"]), ~live)
        _ok(R.drift_of(c["f32"][live], c["ref"][live]), f"pos_logit{s}")
    for s in R.POS_BWD_SHAPES:
        c = R.pos_bwd_case(*s)
        for k in (0, 1):
            _ok(R.drift_of(c["f32"][k], c["ref"][k]), f"pos_bwd{s}[{'gx gy'.split()[k]}]")
        if s[3]:
            assert (c["pos"] == 11).sum() >= R.HOT_ANCHORS and (c["pos"][:4] == [-1, s[1], -1, s[1]]).all()
    for s in R.NORMALIZE_BWD_SHAPES:
        c = R.normalize_bwd_case(*s)
        live = ~c["apart"]
        if s in R.NORMALIZE_BWD_ILL:                  # declared ill-conditioned: it really is — no output scale at all
            assert np.abs(c["ref"][live]).max() <= 1e-6 * c["scale"] and c["scale"] > 0
            _ok(float(np.abs(c["f32"][live]).max()) / c["scale"], f"normalize_bwd{s} (against max |inv g|)")
        else:
            _ok(R.drift_of(c["f32"], c["ref"], c["apart"]), f"normalize_bwd{s}")
        _ok(float(R.row_drift_of(c["f32"][c["apart"]], c["ref"][c["apart"]]).max()), f"normalize_bwd{s} clamped")
        assert c["inv"][5] == np.float32(1e12) and np.abs(c["ref"][5]).max() > 1e11
    for s in R.NORMALIZE_BWD_N_SHAPES:
        for from_raw in (False, True):
            c = R.normalize_bwd_n_case(*s, from_raw)
            _ok(R.drift_of(c["f32"], c["ref"], c["apart"]), f"normalize_bwd_n{s} raw={from_raw}")
            _ok(float(R.row_drift_of(c["f32"][c["apart"]], c["ref"][c["apart"]]).max()), f"normalize_bwd_n{s} clamped")


def test_drift_of_the_dense_cases():
    for s in R.ROWS_DOT_VEC_SHAPES:
        c = R.dot_case(*s)
        _ok(R.drift_of(c["f32"], c["ref"]), f"rows_dot_vec{s}")
        _ok(R.drift_of(c["f32_colsum"], c["ref_colsum"]), f"rows_dot_vec{s} grad v")
        assert R.colsum_condition(c) <= np.sqrt(s[0]), s
    for s in R.COLSUM_SHAPES:
        c = R.dot_case(*s)
        _ok(R.drift_of(c["f32_colsum"], c["ref_colsum"]), f"weighted_colsum{s}")
        # S is not a matter of luck: the terms added are at most sqrt(n) times S, what n zero-mean terms leave on average
        print(f"CONDITION weighted_colsum{s}: {R.colsum_condition(c):.3g}")
        assert R.colsum_condition(c) <= np.sqrt(s[0]), s
    for dx, dg in R.GRAM_PAIRS:
        for n in R.GRAM_SMALL_N:
            c = R.gram_case(n, dx, dg)
            _ok(R.drift_of(c["f32"], c["ref"]), f"gram{(n, dx, dg)}")
    for s in ((R.OVER_CAP_GRAM, 32, 32), (257, 48, 64)):
        c = R.gram_case(*s)
        _ok(R.drift_of(c["f32"], c["ref"]), f"gram{s}")
    for s in R.GATHER_SHAPES:
        c = R.gather_case(*s)
        _ok(R.drift_of(c["f32"], c["ref"]), f"scatter{s}")
        ok = (c["idx"] >= 0) & (c["idx"] < s[0])
        assert (~ok).sum() == (0 if s[3] == "one_row" else 4)
        assert not c["fwd"][~ok].any() and np.array_equal(c["fwd"][ok], c["table"][c["idx"][ok]])


def test_drift_of_the_optimiser_cases():
    for name, hyper in R.ADAM_HYPERS.items():
        for n in R.ADAM_SIZES:
            p0, grads = R.adam_case(n)
            ref, f32 = R.adam_steps(p0, grads, hyper, torch.float64), R.adam_steps(p0, grads, hyper, torch.float32)
            for k in ref:
                if np.abs(ref[k]).max() > 0:
                    _ok(R.drift_of(f32[k], ref[k]), f"adam {name} n={n} {k}")
    for step in (1, 2, 1000, 10 ** 6):
        p0, m, v, g = R.adam_state_case(1027, step)
        args = (p0, ((g,),), R.ADAM_HYPERS["default"])
        ref = R.adam_steps(*args, torch.float64, state=(step - 1, m, v))
        f32 = R.adam_steps(*args, torch.float32, state=(step - 1, m, v))
        for k in ref:
            _ok(R.drift_of(f32[k], ref[k]), f"adam at step {step} {k}")
    for n_u, d in R.MISALIGNED:
        table, grads = R.stacked_case(n_u, d)
        for mu in (0.0, 0.9):
            ref, f32 = (R.sgd_steps(table, grads, 0.05, mu, 1e-3, t) for t in (torch.float64, torch.float32))
            for k in ref:
                _ok(R.drift_of(f32[k], ref[k]), f"sgd {(n_u, d)} mu={mu} {k}")
