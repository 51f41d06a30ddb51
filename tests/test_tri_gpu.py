"""functional.tri_training_loss (gcr_tri_fwd_f32 / gcr_tri_bwd_f32) against univariate/sept_social.py:394-420 restated on
float64 CPU tensors (`restate`): label_prediction x3, generate_pesudo_labels x3, neighbor_discrimination x3.

Labels: per row the selected SET equals the float64 set; rows whose float64 gap (v_k - v_{k+1}) / v_k of the combined
probability is below 1e-5 are left out, and their share (from the float64 values alone) is at most 2 % per case.
Loss and the four gradients: against the restatement evaluated AT THE KERNEL'S OWN label sets (a boundary swap can neither
hide nor fake an error), by the bound rule of tests/test_mim_gpu.py with the fp32 torch composition on the GPU as the drift:

    err / S  <=  max(4 x err of the composition, 2^-20)  and  <= 1e-5

S = sum_i |lse_all| + |lse_pos| for a loss (oracle/gen_golden.py:1112-1121: the loss is a difference of the two), max |f64|
for a gradient.  A zero row's gradient is 1e12 x its upstream (F.normalize's eps), which makes max |f64| of its table a
normaliser the other rows cannot miss: the same bound is also asserted on the other rows alone.

Measured on an MI355X, worst of the 63 cases (printed by `test_kernel_matches_float64_restatement`, copied into DESIGN.md's
parity table): loss 3.3e-7 (bound 9.5e-7), gradient 1.0e-6 (`d_friend`, d = 128, k = 20, m = 33, bound 1.4e-6), worst
err / bound 0.74 (`d_sharing` without its zero row, d = 32, k = 5).  Worst of the 21 further cases (k = 32 at `rows_for(32)`,
and `SPLIT_CASES`: every split count, up to 342 tiles per split, the per-row kernels' second grid-stride trip): loss 4.0e-8,
gradient 5.9e-6 (`d_rec`, m = 10940, where the fp32 composition itself is 6.3e-6 off: bound 2.5e-5, and 0.59 of the 1e-5
cap), worst err / bound 0.41 (`d_rec`, d = 128, k = 32, m = 33); undecided rows at most 1.08 % (m = 31) and 0.82 % among the
new cases (m = 2000, k = 20).  k = 32, m = 33 is where the sharing table's zero row first missed its bound, by 1.66-1.76x at
every width (1.6e-6 to 2.2e-6 against 9.5e-7 to 1.3e-6): the backward subtracted two float reciprocals that agree to 1 / 33
there.  The kernel now forms that difference from double sums (csrc/gcr_tri.hip, `tri_finish_kernel`): 1.8e-7 to 1.9e-7.
At the lowest temperature, t = 1 / 40 (`test_lowest_temperature_with_positives_at_the_lowest_scores`): loss 8.2e-8,
gradient 9.4e-7 (`d_aug`, bound 4.4e-6), worst err / bound 0.22.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, NORTH_STAR, MIN_GAP, MAX_AMBIGUOUS = 2.0 ** -20, 1e-5, 1e-5, 0.02
T = 0.1
WIDTHS, KS = (32, 64, 128), (1, 5, 20)
COMBOS = ((1, 2), (0, 2), (0, 1))               # pos_f <- P_s + P_r, pos_s <- P_f + P_r, pos_r <- P_f + P_s
MAX_K = 32                                      # kMaxK
T_LOWEST, FLT_MIN = 0.025, 2.0 ** -126          # 1 / kMaxInvT; the smallest normal float
# (m, d, k, column splits = min(8, tiles, ceil(256 / tiles)) of the ceil(m / 32) column tiles).  rows_for() stops at 9 tiles:
# splits 1, 2, 4, 8 and at most two tiles per split.  Here every other split count, and sweeps that carry a lane's candidate
# list and its threshold over many tiles:
SPLIT_CASES = (
    (1000, 64, 32, 8),      # 32 tiles, 4 per split; the finish kernel's candidate LDS full
    (1100, 32, 32, 8),      # 35 tiles, uneven: 3 splits sweep 5 tiles, 5 sweep 4
    (1200, 128, 5, 7),      # 38 tiles
    (1500, 32, 20, 6),      # 47 tiles
    (2000, 64, 20, 5),      # 63 tiles
    (2100, 128, 1, 4),      # 66 tiles: 16-17 per split
    (2900, 32, 5, 3),       # 91 tiles
    (4100, 64, 1, 2),       # 129 tiles: 64-65 per split
    (10940, 32, 5, 1),      # 342 tiles in one split; 4 m and 3 m waves > 8192 workgroups x 4: the second grid-stride trip of
)                           # tri_prepare_kernel, tri_bwd_rows_kernel and tri_finish_kernel


def rows_for(k):
    return sorted({k, k + 1, 31, 32, 33, 97, 257} - set(range(k)))


def make_inputs(m, d, seed, k=1):
    """Four tables [U, d] with U = 2 m + 3, uniq = 1, 3, 5, ... (strict, non-contiguous), one all-zero row in the sharing
    table and one in the augmented table, upstream g not all ones.  m = k has no zero rows: every column is a positive
    there, every gradient cancels to rounding noise, and a zero row would scale that noise by F.normalize's 1e12."""
    g = torch.Generator().manual_seed(seed)
    n = 2 * m + 3
    tabs = [torch.randn(n, d, generator=g) for _ in range(4)]
    uniq = 2 * torch.arange(m) + 1
    if m > k:
        tabs[1][uniq[m // 2]] = 0.0
        tabs[3][uniq[m - 1]] = 0.0
    return tabs, uniq, torch.tensor([0.7, -1.3, 2.1])


def scores(tabs, uniq):
    a = F.normalize(tabs[3][uniq])
    return [torch.matmul(F.normalize(x[uniq]), a.T) for x in tabs[:3]]


def combined(tabs, uniq):
    p = [F.softmax(s, dim=1) for s in scores(tabs, uniq)]                  # :394-399
    return [(p[a] + p[b]) / 2 for a, b in COMBOS]                          # :404-405


def restate(tabs, uniq, positives, t=T):
    """:408-420 for the three views at given label sets -> (loss [3], S = sum_i |lse_all| + |lse_pos| [3])."""
    loss, mag = [], []
    for v, s in enumerate(scores(tabs, uniq)):
        pos = torch.gather(s, 1, positives[v])
        pos_score = torch.sum(torch.exp(pos / t), dim=1)
        ttl_score = torch.sum(torch.exp(s / t), dim=1)
        loss.append(-torch.sum(torch.log(pos_score / ttl_score)))
        mag.append((torch.log(pos_score).abs() + torch.log(ttl_score).abs()).sum())
    return torch.stack(loss), torch.stack(mag)


def with_grads(tabs, uniq, positives, g, t=T):
    tabs = [x.detach().clone().requires_grad_(True) for x in tabs]
    loss, mag = restate(tabs, uniq, positives, t)
    (loss * g.to(loss)).sum().backward()
    return loss.detach(), mag.detach(), [x.grad for x in tabs]


def float64_labels(tabs, uniq, k):
    """(label sets as sorted int64 [3, m, k], decided [3, m] bool: the float64 gap is at least MIN_GAP)."""
    sets, decided = [], []
    for v in combined([x.double() for x in tabs], uniq):
        top = torch.topk(v, min(k + 1, v.shape[1]), dim=1)
        sets.append(torch.sort(top.indices[:, :k], dim=1).values)
        if v.shape[1] > k:
            decided.append((top.values[:, k - 1] - top.values[:, k]) / top.values[:, k - 1] >= MIN_GAP)
        else:
            decided.append(torch.ones(v.shape[0], dtype=torch.bool))
    return torch.stack(sets), torch.stack(decided)


def check(what, got, ref, comp, scale=None, mag=None):
    """The bound rule; prints err / bound before asserting.  mag: the size of the un-cancelled terms, the normaliser where
    the float64 value cancels to nothing (m = k: every column is a positive and w = 0)."""
    ref = ref.double().cpu().numpy()
    scale = float(np.abs(ref).max()) if scale is None else float(scale)
    if mag is not None and scale <= 1e-9 * mag:
        scale = mag
    assert scale > 0, what
    err = float(np.abs(got.double().cpu().numpy() - ref).max()) / scale
    drift = float(np.abs(comp.double().cpu().numpy() - ref).max()) / scale
    bound = max(4.0 * drift, FLOOR) if math.isfinite(drift) else FLOOR
    print(f"TRI {what}: err={err:.3e} composition={drift:.3e} bound={bound:.3e} ratio={err / bound:.3f}")
    assert math.isfinite(err) and err <= bound and err <= NORTH_STAR, (what, err, bound, drift)
    return err, bound


def run_fused(tabs, uniq, k, g, positives=None, t=T):
    from recommendation_amd import functional as Fn
    dev = [x.to(DEV).requires_grad_(True) for x in tabs]
    loss, pos = Fn.tri_training_loss(*dev, uniq.to(DEV), k, t, positives)
    (loss * g.to(DEV)).sum().backward()
    return loss.detach(), pos, [x.grad for x in dev]


def check_case(d, k, m, worst):
    """One (d, k, m) against the float64 restatement: the label rules, then the loss and the four gradients at the kernel's own
    label sets; the seed is 1000 d + 10 k + m.  Updates `worst` (name -> (err, bound)) for the caller's summary line."""
    from recommendation_amd import functional as Fn
    assert Fn.tri_training_supported(d, k)
    tabs, uniq, g = make_inputs(m, d, 1000 * d + 10 * k + m, k)
    loss, pos, grads = run_fused(tabs, uniq, k, g)
    assert pos.shape == (3, m, k) and pos.dtype == torch.int64
    pos_cpu = pos.cpu()
    assert int(pos_cpu.min()) >= 0 and int(pos_cpu.max()) < m
    got_sets = torch.sort(pos_cpu, dim=2).values
    assert bool((got_sets[:, :, 1:] > got_sets[:, :, :-1]).all()), "a row selected one column twice"

    # labels: sets equal to float64's where float64 decides; the undecided share from float64 alone
    want_sets, decided = float64_labels(tabs, uniq, k)
    share = 1.0 - float(decided.double().mean())
    same = (got_sets == want_sets).all(dim=2)
    print(f"TRI d={d} k={k} m={m}: undecided rows {share:.4f}, rows differing {int((~same).sum())}")
    assert share <= MAX_AMBIGUOUS, (m, share)
    assert bool(same[decided].all()), (m, torch.nonzero(~same & decided).tolist())
    # descending order of the combined probability inside every row
    comb = torch.stack(combined([x.double() for x in tabs], uniq))
    vals = torch.gather(comb, 2, pos_cpu)
    assert bool((vals[:, :, 1:] <= vals[:, :, :-1] * (1 + MIN_GAP)).all()), "rows are not in descending order"

    check_values(f"d={d} k={k} m={m}", tabs, uniq, g, k, loss, pos, grads, worst)


def check_values(tag, tabs, uniq, g, k, loss, pos, grads, worst, t=T):
    """The loss and the four gradients of `run_fused` against the restatement at the label sets `pos` (the kernel's own, or
    the replayed ones), by the bound rule, the zero rows' tables also without their zero row."""
    m, d = uniq.numel(), tabs[0].shape[1]
    l64, mag, g64 = with_grads([x.double() for x in tabs], uniq, pos.cpu(), g, t)
    l32, _, g32 = with_grads([x.to(DEV) for x in tabs], uniq.to(DEV), pos, g.to(DEV), t)
    for v, name in enumerate(("loss_f", "loss_s", "loss_r")):
        e = check(f"{tag} {name}", loss[v], l64[v], l32[v], scale=mag[v])
        worst[name] = max(worst.get(name, (0, 0)), e)
    zero_rows = {1: int(uniq[m // 2]), 3: int(uniq[m - 1])} if m > k else {}
    w_mag = float(g.abs().max()) / t / math.sqrt(d)          # |g_v| / t x 1 / |x|: one of the two cancelling parts
    for s, name in enumerate(("d_friend", "d_sharing", "d_rec", "d_aug")):
        assert bool((grads[s].cpu()[::2] == 0).all()), "a row outside uniq received a gradient"
        e = check(f"{tag} {name}", grads[s], g64[s], g32[s], mag=w_mag)
        worst[name] = max(worst.get(name, (0, 0)), e)
        if s in zero_rows:
            keep = torch.ones(grads[s].shape[0], dtype=torch.bool)
            keep[zero_rows[s]] = False
            e = check(f"{tag} {name} (non-zero rows)", grads[s].cpu()[keep], g64[s][keep], g32[s].cpu()[keep])
            worst[name + "*"] = max(worst.get(name + "*", (0, 0)), e)


def print_worst(d, k, worst):
    print(f"TRI worst d={d} k={k}: " + ", ".join(f"{n} err {e:.2e} bound {b:.2e}" for n, (e, b) in worst.items()))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", WIDTHS)
def test_kernel_matches_float64_restatement(d, k):
    worst = {}
    for m in rows_for(k):
        check_case(d, k, m, worst)
    print_worst(d, k, worst)


@pytest.mark.parametrize("d", WIDTHS)
def test_kernel_matches_float64_restatement_at_the_largest_k(d):
    """k = kMaxK = 32: the largest dynamic LDS of the selecting sweep, and at m = 257 (8 splits) tri_finish_kernel's
    cv / cc[4][2 * 8 * 32] filled to the last word.  At m = 32 every column is a positive."""
    worst = {}
    for m in rows_for(MAX_K):
        check_case(d, MAX_K, m, worst)
    print_worst(d, MAX_K, worst)


@pytest.mark.parametrize("m,d,k,n_splits", SPLIT_CASES)
def test_kernel_matches_float64_restatement_at_every_split_count(m, d, k, n_splits):
    """SPLIT_CASES: every split count, sweeps of many tiles per split, and the second grid-stride trip of the per-row
    kernels.  tests/test_launch_geometry_cpu.py asserts that each m reaches the n_splits named here."""
    worst = {}
    check_case(d, k, m, worst)
    print_worst(d, k, worst)


def test_lowest_temperature_with_positives_at_the_lowest_scores():
    """t = 1 / 40, the lowest temperature the kernels take (below it `tri_training_loss` composes): a term
    e = exp((S - 1) / t) is as small as exp(-80) = 1.8e-35, a normal float, but the product of two sums of such terms is not.
    Three rows per view are the negative of a row of the augmented table (S = -1) and every row's replayed label is its
    lowest-scoring column (k = 1), so in those rows sum_pos e x sum_j e is far below the smallest normal float — asserted
    from the float64 scores — while both sums, their reciprocals and 1 / sum_j e - 1 / sum_pos e all are representable.
    Then the selecting path at that temperature on the same tables."""
    m, d, k = 97, 64, 1
    tabs, uniq, g = make_inputs(m, d, 1000 * d + 10 * k + m + 1, k)
    planted = []
    for v in range(3):
        for i in (3, 40, 70):                                    # not m // 2, the sharing table's zero row
            j = i + 7 + v                                        # not m - 1, the augmented table's zero row
            tabs[v][uniq[i]] = -tabs[3][uniq[j]] * (1.5 + v)
            planted.append((v, i, j))
    s64 = torch.stack(scores([x.double() for x in tabs], uniq))
    lowest = s64.argmin(dim=2, keepdim=True)                     # [3, m, 1]
    e64 = torch.exp((s64 - 1.0) / T_LOWEST)
    for v, i, j in planted:
        assert int(lowest[v, i, 0]) == j and float(s64[v, i, j]) < -1 + 1e-12
        assert float(e64[v, i, j]) > 1e-35 and float(e64[v, i].sum()) > 1e-35             # either sum: a normal float
        assert float(e64[v, i, j] * e64[v, i].sum()) < 1e-3 * FLT_MIN                     # their product: not even a denormal one
    worst = {}
    loss, pos, grads = run_fused(tabs, uniq, k, g, positives=lowest.to(DEV), t=T_LOWEST)
    assert torch.equal(pos.cpu(), lowest)
    assert all(bool(torch.isfinite(x).all()) for x in [loss] + grads)
    check_values(f"t={T_LOWEST} replayed lowest", tabs, uniq, g, k, loss, pos, grads, worst, T_LOWEST)
    loss, pos, grads = run_fused(tabs, uniq, k, g, t=T_LOWEST)
    want_sets, decided = float64_labels(tabs, uniq, k)
    assert bool((pos.cpu() == want_sets)[decided].all()) and float(decided.double().mean()) >= 1 - MAX_AMBIGUOUS
    assert all(bool(torch.isfinite(x).all()) for x in [loss] + grads)
    check_values(f"t={T_LOWEST} selected", tabs, uniq, g, k, loss, pos, grads, worst, T_LOWEST)
    print(f"TRI worst t={T_LOWEST}: " + ", ".join(f"{n} err {e:.2e} bound {b:.2e}" for n, (e, b) in worst.items()))


def test_ties_go_to_the_smaller_column():
    """Two identical rows of the augmented table at columns j < j': equal scores in every row and view, so every row that
    selects either ranks j before j', and never takes j' without j."""
    m, d, k = 97, 64, 5
    tabs, uniq, g = make_inputs(m, d, 7, 5)
    j, jp = 11, 70                                  # different 32-column tiles: the candidate lists meet only in the merge
    attractive = F.normalize(tabs[0][uniq[:40]]).sum(0) + F.normalize(tabs[2][uniq[:40]]).sum(0)
    tabs[3][uniq[j]] = attractive
    tabs[3][uniq[jp]] = attractive
    j2, jp2 = 40, 41                                # the same tile, one lane's list
    tabs[3][uniq[j2]] = -attractive
    tabs[3][uniq[jp2]] = -attractive
    _, pos, _ = run_fused(tabs, uniq, k, g)
    pos = pos.cpu()
    seen = 0
    for a, b in ((j, jp), (j2, jp2)):
        for v in range(3):
            for i in range(m):
                row = pos[v, i].tolist()
                if b in row:
                    assert a in row and row.index(a) + 1 == row.index(b), (v, i, row)
                if a in row:
                    seen += 1
                    if row.index(a) == k - 1:
                        assert b not in row
    assert seen >= 20, "the planted columns were hardly ever selected: the test checks nothing"


def test_two_runs_are_bitwise_equal():
    for (m, d, seed, k_in), k in (((257, 64, 3, 5), 10), ((2000, 64, 3, 20), 20)):         # 8 splits x 2 tiles; 5 splits x 13
        tabs, uniq, g = make_inputs(m, d, seed, k_in)
        a = run_fused(tabs, uniq, k, g)
        b = run_fused(tabs, uniq, k, g)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for x, y in zip(a[2], b[2]):
            assert torch.equal(x, y)


def test_replay_reproduces_the_loss_and_the_gradients():
    # the replay sweep (MODE 1) is an instantiation of its own: 4 splits at m = 97, 7 splits of 5-6 tiles at m = 1200
    for m, d in ((1200, 128), (97, 32)):
        tabs, uniq, g = make_inputs(m, d, 5, 5)
        loss, pos, grads = run_fused(tabs, uniq, 5, g)
        given = pos.clone()
        loss2, pos2, grads2 = run_fused(tabs, uniq, 5, g, positives=given)
        assert torch.equal(pos2, pos) and torch.equal(given, pos)
        assert float((loss2 - loss).abs().max()) <= 1e-6 * float(loss.abs().max())
        for x, y in zip(grads, grads2):
            rows = x.abs().amax(1) < 1e6             # leave the 1e12-scaled zero rows to the relative check below
            assert float((x - y)[rows].abs().max()) <= 1e-6 * float(x[rows].abs().max())
            assert float((x - y).abs().max()) <= 1e-6 * float(x.abs().max())
        # label sets in another order: the same loss up to the order of a k-term sum
        loss3, _, _ = run_fused(tabs, uniq, 5, g, positives=pos.flip(2))
        assert float((loss3 - loss).abs().max()) <= 1e-5 * float(loss.abs().max())
    with pytest.raises(ValueError):
        run_fused(tabs, uniq, 5, g, positives=pos[:, :, :4])


def test_fewer_rows_than_labels_raises_and_no_rows_is_zero():
    from recommendation_amd import _lib
    from recommendation_amd import functional as Fn
    tabs, uniq, g = make_inputs(4, 32, 1)
    with pytest.raises(ValueError):
        run_fused(tabs, uniq, 5, g)
    L = _lib.lib()                                   # the C entry point itself: GCR_EINVAL, nothing launched
    dev = [x.to(DEV) for x in tabs]
    out = torch.zeros(64, device=DEV)
    rc = L.gcr_tri_fwd_f32(*(_lib.dptr(x) for x in dev), dev[0].shape[0], 32, _lib.dptr(uniq.to(DEV)), 4, 5, 10.0, 0,
                           _lib.dptr(out), None, None, None, None, None, _lib.cur_stream(dev[0].device))
    assert rc != 0 and rc > -1000
    loss, pos = Fn.tri_training_loss(*dev, torch.zeros(0, dtype=torch.int64, device=DEV), 5)
    assert loss.tolist() == [0.0, 0.0, 0.0] and pos.shape == (3, 0, 5)


def test_unsupported_shapes_take_the_composed_path():
    """d = 48 and k = 33 are outside the kernel family: the same function answers from torch.topk +
    losses.neighbor_discrimination.  At the supported neighbour (d = 64, k = 5) the two paths agree."""
    from recommendation_amd import functional as Fn
    for d, k in ((48, 5), (16, 5), (64, 33)):
        assert not Fn.tri_training_supported(d, k)
        tabs, uniq, g = make_inputs(97, d, 11, k)
        loss, pos, grads = run_fused(tabs, uniq, k, g)
        l64, mag, g64 = with_grads([x.double() for x in tabs], uniq, pos.cpu(), g)
        assert float(((loss.cpu().double() - l64).abs() / mag).max()) <= 1e-5
        for s in (0, 2):                             # the tables without a 1e12-scaled zero row
            assert float((grads[s].cpu().double() - g64[s]).abs().max()) <= 1e-4 * float(g64[s].abs().max())
    tabs, uniq, g = make_inputs(97, 64, 12, 5)
    loss, pos, grads = run_fused(tabs, uniq, 5, g)
    dev = [x.to(DEV).requires_grad_(True) for x in tabs]
    loss_c, pos_c = Fn.tri_training_loss_composed(*dev, uniq.to(DEV), 5, T)
    (loss_c * g.to(DEV)).sum().backward()
    _, decided = float64_labels(tabs, uniq, 5)
    same = (torch.sort(pos, dim=2).values == torch.sort(pos_c, dim=2).values).all(dim=2).cpu()
    assert bool(same[decided].all())
    if bool(same.all()):
        assert float((loss - loss_c).abs().max()) <= 1e-5 * float(loss.abs().max())
        for s in (0, 2):
            assert float((grads[s] - dev[s].grad).abs().max()) <= 1e-4 * float(grads[s].abs().max())
