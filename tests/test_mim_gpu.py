"""functional.mim_loss (gcr_mim_fwd_f32 / gcr_mim_bwd_f32): MHCN's hierarchical mutual-information loss, mhcn.py:496-505.

Second opinion: the reference's lines restated on float64 CPU tensors with `edge` as an independent input (`restate`).
Bound rule (tests/f64_pins.py) with the torch fp32 composition on the GPU as the drift:

    err = max|got - f64| / S  <=  max(4 * err of the composition, 2^-20)  and  err <= 1e-5,   S = max|f64|

(the loss is a sum of positive terms, so S = the loss itself).  Where the composition is not finite (its
log(sigmoid(x)) is -inf at x = -100) it sets no drift and the floor 2^-20 holds alone.  Where a float64 gradient cancels
to nothing (n = 2 with identity permutations: neg1 = neg2 = pos, d_em = -edge / 2 + edge / 2), max|f64| is no normaliser
and S is the magnitude of the un-cancelled terms instead: sum_k |dL / d score_k| |d score_k / d x| over the five scores.

Measured on an MI355X, worst err / bound (every bound is the floor 2^-20 there) of the 28 cases of ROWS x WIDTHS: loss 0.48
(n = 1, d = 256: 4.6e-7), d_em 0.16, d_edge 0.17; of the 6 cases of FOLD_CASES (18 to 1024 workgroups: the folds' second
batch of loads, every chain count, both grid caps): loss 0.045 (n = 33025, d = 32: 4.3e-8), d_em 0.16 (n = 4353, d = 256:
1.5e-7), d_edge 0.19 (n = 131080, d = 256: 1.8e-7)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, NORTH_STAR = 2.0 ** -20, 1e-5
WIDTHS = (32, 64, 128, 256)
ROWS = (1, 2, 63, 64, 65, 257, 775)           # 64 rows: one pass of a workgroup at d = 32; 257, 775: 2 and 4 workgroups


def restate(em, edge, perms, up=1.0, dtype=torch.float64, device="cpu"):
    """mhcn.py:496-505 as written -> (loss, d_em, d_edge) of up * loss, edge an independent leaf."""
    em = em.detach().to(device=device, dtype=dtype).requires_grad_(True)
    edge = edge.detach().to(device=device, dtype=dtype).requires_grad_(True)
    p = [torch.as_tensor(q).to(device) for q in perms]

    def score(x1, x2):
        return torch.sum(torch.multiply(x1, x2), 1)

    pos = score(em, edge)
    neg1 = score(em[p[0]], edge)
    neg2 = score(edge[p[1]], em)
    local_loss = torch.sum(-torch.log(torch.sigmoid(pos - neg1)) - torch.log(torch.sigmoid(neg1 - neg2)))
    graph = torch.mean(edge, 0, keepdim=True)
    gpos = score(edge, graph.expand_as(edge))
    gneg = score(edge[p[2]], graph.expand_as(edge))
    loss = torch.sum(-torch.log(torch.sigmoid(gpos - gneg))) + local_loss
    w = [abs(up) * t.abs() for t in torch.autograd.grad(loss, [pos, neg1, neg2, gpos, gneg], retain_graph=True)]
    (up * loss).backward()
    diffs = torch.stack([pos - neg1, neg1 - neg2, gpos - gneg]).detach()
    # the un-cancelled magnitude of each gradient: the five scores' own gradients, all signs made positive
    a_em, a_edge = em.detach().abs().requires_grad_(True), edge.detach().abs().requires_grad_(True)
    a_graph = torch.mean(a_edge, 0, keepdim=True).expand_as(a_edge)
    scores = (score(a_em, a_edge), score(a_em[p[0]], a_edge), score(a_edge[p[1]], a_em), score(a_edge, a_graph),
              score(a_edge[p[2]], a_graph))
    sum((wk * sk).sum() for wk, sk in zip(w, scores)).backward()
    mags = (float(loss.detach()), float(a_em.grad.max()), float(a_edge.grad.max()))
    return loss.detach(), em.grad, edge.grad, diffs, mags


def kernel(em, edge, perms, up=1.0):
    from recommendation_amd import functional as Fn
    em = em.detach().to(DEV).requires_grad_(True)
    edge = edge.detach().to(DEV).requires_grad_(True)
    loss = Fn.mim_loss(em, edge, perms)
    (up * loss).backward()
    return loss.detach(), em.grad, edge.grad


def check(what, got, ref, comp, mag=None):
    """The bound rule; prints err / bound before asserting.  got: the kernel's, ref: float64, comp: the fp32 composition,
    mag: the magnitude of the un-cancelled terms, the normaliser where ref cancels to nothing."""
    ref = ref.double().cpu().numpy()
    scale = float(np.abs(ref).max())
    if mag is not None and scale <= 1e-12 * mag:
        scale = mag
    assert scale > 0, what
    err = float(np.abs(got.double().cpu().numpy() - ref).max()) / scale
    drift = float(np.abs(comp.double().cpu().numpy() - ref).max()) / scale
    bound = max(4.0 * drift, FLOOR) if math.isfinite(drift) else FLOOR
    print(f"MIM {what}: err={err:.3e} composition={drift:.3e} bound={bound:.3e} ratio={err / bound:.3f}")
    assert math.isfinite(err) and err <= bound and err <= NORTH_STAR, (what, err, bound, drift)


def rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    em = torch.randn(n, d, generator=g) * d ** -0.25           # every dot is O(1)
    edge = torch.randn(n, d, generator=g) * d ** -0.25
    perms = [torch.randperm(n, generator=g) for _ in range(3)]
    return em, edge, perms


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("d", WIDTHS)
def test_mim_loss_and_gradients_match_the_float64_restatement(n, d):
    em, edge, perms = rows(n, d, 1000 * d + n)
    for up in (1.0, -2.5):
        ref = restate(em, edge, perms, up)
        comp = restate(em, edge, perms, up, torch.float32, DEV)
        got = kernel(em, edge, perms, up)
        for name, g, r, c, mag in zip(("loss", "d_em", "d_edge"), got, ref, comp, ref[4]):
            check(f"n={n} d={d} up={up} {name}", g, r, c, mag)


# (n, d, workgroups nb = min(1024, ceil(n / 256)), rows per workgroup = ceil(n / nb)).  ROWS stops at nb = 4; the last workgroup
# folds the nb partials per column in 256 / d interleaved chains, 16 loads in flight at a time, and the loss over 64 lanes:
FOLD_CASES = (
    (4353, 256, 18, 242),       # one chain of 18: its second batch of 16 loads
    (4353, 128, 18, 242),       # two chains of 9
    (16641, 64, 66, 253),       # four chains of 16-17: the second batch; the loss fold loads twice in lanes 0-1
    (33025, 32, 130, 255),      # eight chains of 16-17: the second batch; the loss fold three deep
    (263000, 32, 1024, 257),    # the cap of 1024 workgroups: more than 256 rows each
    (131080, 256, 513, 256),    # 16385 > 16384 workgroups wanted by mim_bwd_kernel: its second grid-stride trip
)


@pytest.mark.parametrize("up", (1.0, -2.5))
@pytest.mark.parametrize("n,d,nb,per", FOLD_CASES)
def test_mim_matches_the_float64_restatement_beyond_one_fold_batch(n, d, nb, per, up):
    """FOLD_CASES, loss and both gradients by the bound rule; tests/test_launch_geometry_cpu.py asserts that each shape reaches
    the nb and the rows per workgroup named there.  Left out on purpose: the 16384-workgroup cap of mim_inverse_kernel needs
    n > 1.39 M rows; that kernel is a plain grid-stride scatter, and a float64 restatement at that n takes far longer than a
    test may."""
    em, edge, perms = rows(n, d, 1000 * d + n)
    ref = restate(em, edge, perms, up)
    comp = restate(em, edge, perms, up, torch.float32, DEV)
    got = kernel(em, edge, perms, up)
    for name, g, r, c, mag in zip(("loss", "d_em", "d_edge"), got, ref, comp, ref[4]):
        check(f"n={n} d={d} up={up} {name}", g, r, c, mag)


@pytest.mark.parametrize("d", WIDTHS)
def test_single_row_is_three_log_two(d):
    """n = 1: the only permutation is the identity, every difference is 0."""
    em, edge, perms = rows(1, d, d)
    assert all(p.tolist() == [0] for p in perms)
    loss, d_em, d_edge = kernel(em, edge, perms)
    assert float(loss) == pytest.approx(3 * math.log(2), rel=1e-6)
    ref = restate(em, edge, perms)
    assert torch.isfinite(d_em).all() and torch.isfinite(d_edge).all()
    assert float((d_em.cpu().double() - ref[1]).abs().max()) <= 1e-6 * max(float(ref[1].abs().max()), 1.0)
    assert float((d_edge.cpu().double() - ref[2]).abs().max()) <= 1e-6 * max(float(ref[2].abs().max()), 1.0)


@pytest.mark.parametrize("d", [32, 128])
def test_saturated_differences_stay_finite(d):
    """Rows scaled so that pos - neg1 reaches +-100 and +-60: the reference's fp32 expression is inf at -100, its float64
    run (what is pinned) gives 100, and so does the softplus."""
    n = 65
    em, edge, perms = rows(n, d, 7 + d)
    g = torch.Generator().manual_seed(d)
    for r, (mag, sign) in enumerate(((100.0, 1.0), (100.0, -1.0), (60.0, 1.0), (60.0, -1.0))):
        v = torch.nn.functional.normalize(torch.randn(d, generator=g), dim=0)
        em[r], edge[r] = math.sqrt(mag) * v, sign * math.sqrt(mag) * v
    ref = restate(em, edge, perms)
    diffs = ref[3]
    print("MIM saturation: differences in", float(diffs.min()), float(diffs.max()))
    assert float(diffs.max()) > 80 and float(diffs.min()) < -80 and torch.isfinite(ref[0])
    comp = restate(em, edge, perms, 1.0, torch.float32, DEV)
    got = kernel(em, edge, perms)
    assert torch.isfinite(got[0])
    rel = abs(float(got[0]) - float(ref[0])) / float(ref[0])
    print(f"MIM saturation d={d}: loss {float(got[0])!r} f64 {float(ref[0])!r} rel {rel:.3e}; composition {float(comp[0])!r}")
    assert rel <= 1e-6
    for name, gk, r, c in zip(("d_em", "d_edge"), got[1:], ref[1:3], comp[1:]):
        check(f"saturation d={d} {name}", gk, r, c)


@pytest.mark.parametrize("n,d", [(775, 64), (20011, 32)])
def test_two_runs_are_bit_identical(n, d):
    """Fixed-order partial sums and one writer per output row: 4 and 79 workgroups."""
    em, edge, perms = rows(n, d, n)
    a, b = kernel(em, edge, perms, 0.3), kernel(em, edge, perms, 0.3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _random_graph(n, m, seed):
    import recommendation_amd as ra
    rng = np.random.default_rng(seed)
    nnz = 6 * n
    row, col = rng.integers(0, n, nnz), rng.integers(0, m, nnz)
    return ra.CsrGraph.row_normalised(torch.from_numpy(row).to(DEV), torch.from_numpy(col).to(DEV), None, n, m, DEV)


def _dense(g):
    out = np.zeros((g.n_rows, g.n_cols))
    r = np.repeat(np.arange(g.n_rows), np.diff(g.rowptr_host))
    np.add.at(out, (r, g.col.cpu().numpy()), g.val.cpu().numpy())
    return torch.from_numpy(out)


def test_unsupported_width_is_refused_and_the_encoder_falls_back(monkeypatch):
    from recommendation_amd import _lib, functional as Fn
    from recommendation_amd.mhcn import MHCNEncoder
    L = _lib.lib()
    assert [d for d in range(1, 300) if L.gcr_mim_supported(d)] == list(WIDTHS)
    n, d = 70, 48
    em, edge, perms = rows(n, d, 48)
    em_d, edge_d = em.to(DEV), edge.to(DEV)
    p_d = [p.to(DEV) for p in perms]
    loss, coef, gvec = torch.zeros((), device=DEV), torch.zeros(3, n, device=DEV), torch.zeros(2, d, device=DEV)
    ws = torch.zeros(1024, dtype=torch.float64, device=DEV)
    assert L.gcr_mim_workspace_bytes(n, d) == 0
    rc = L.gcr_mim_fwd_f32(_lib.dptr(em_d), _lib.dptr(edge_d), _lib.dptr(p_d[0]), _lib.dptr(p_d[1]), _lib.dptr(p_d[2]), n, d,
                           _lib.dptr(loss), _lib.dptr(coef), _lib.dptr(gvec), _lib.dptr(ws), _lib.cur_stream())
    assert rc == -2                                             # GCR_EUNSUPPORTED
    with pytest.raises(_lib.GcrError):
        Fn.mim_loss(em_d, edge_d, p_d)
    # n = 0 returns 0 and launches nothing
    assert L.gcr_mim_fwd_f32(None, None, None, None, None, 0, 64, None, None, None, None, _lib.cur_stream()) == 0

    calls = []
    real = Fn.mim_loss
    monkeypatch.setattr(Fn, "mim_loss", lambda *a, **k: calls.append(a[0].shape[1]) or real(*a, **k))
    h, r = _random_graph(n, n, 1), _random_graph(n, 50, 2)
    hd = _dense(h)
    for width, fused in ((48, False), (64, True)):
        enc = MHCNEncoder(h, h, h, r, emb_size=width, n_layers=1)
        x = rows(n, width, width)[0]
        xg = x.to(DEV).requires_grad_(True)
        got = enc.hierarchical_self_supervision(xg, h, p_d)
        got.backward()
        assert (calls == [width]) == fused and (not fused) == (calls == [])
        calls.clear()
        x64 = x.double().requires_grad_(True)
        e64 = hd @ x64
        ref = restate(x64, e64, perms)
        grad = ref[1] + hd.t() @ ref[2]                         # through edge = H em a second time
        assert float(got) == pytest.approx(float(ref[0]), rel=1e-5)
        assert float((xg.grad.cpu().double() - grad).abs().max()) <= 1e-5 * float(grad.abs().max())


def test_a_non_permutation_is_refused_on_the_host():
    from recommendation_amd import functional as Fn
    n, d = 65, 64
    em, edge, perms = rows(n, d, 3)
    em, edge = em.to(DEV), edge.to(DEV)
    repeated = perms[1].clone()
    repeated[5] = repeated[6]
    too_large = perms[2].clone()
    too_large[int((too_large == 0).nonzero())] = n
    for bad in ([perms[0], repeated, perms[2]], [perms[0], perms[1], too_large], [perms[0][:-1], perms[1], perms[2]],
                perms[:2]):
        with pytest.raises(ValueError):
            Fn.mim_loss(em, edge, bad)
    assert torch.isfinite(Fn.mim_loss(em, edge))                # permutations drawn inside


@pytest.mark.parametrize("family", ["mhcn", "mhcn_wide"])
def test_reference_fixture_replay(golden, family):
    """The reference's recorded permutations on its own gated rows: Fn.spmm + mim_loss against the composition (the
    parent's code) and the float64 restatement, per channel, loss and the whole gradient of the gated rows."""
    import recommendation_amd as ra
    from recommendation_amd import functional as Fn
    from recommendation_amd.mhcn import MHCNEncoder
    z = golden(f"{family}.npz")
    fu = torch.from_numpy(z["final_user"]).double()
    for c, name in enumerate(("H_s", "H_j", "H_p")):
        shape = z[f"{name}_shape"]
        adj = ra.CsrGraph(z[f"{name}_indptr"], z[f"{name}_indices"], z[f"{name}_data"], int(shape[0]), int(shape[1]), DEV)
        w, b = torch.from_numpy(z[f"sgw{c + 1}"]).double(), torch.from_numpy(z[f"sgb{c + 1}"]).double()
        gated = (fu * torch.sigmoid(fu @ w + b)).float()        # mhcn.py:408-410
        perms = [torch.from_numpy(p.astype(np.int64)) for p in z["perms"][3 * c:3 * c + 3]]
        p_d = [p.to(DEV) for p in perms]
        hd = _dense(adj)
        x64 = gated.double().requires_grad_(True)
        ref = restate(x64, hd @ x64, perms)
        ref_grad = ref[1] + hd.t() @ ref[2]
        xk = gated.to(DEV).requires_grad_(True)
        loss_k = Fn.mim_loss(xk, Fn.spmm(adj, xk), p_d)
        loss_k.backward()
        xc = gated.to(DEV).requires_grad_(True)
        loss_c = MHCNEncoder.hierarchical_self_supervision_composed(xc, adj, p_d)
        loss_c.backward()
        check(f"{family} {name} loss", loss_k.detach(), ref[0], loss_c.detach())
        check(f"{family} {name} grad", xk.grad, ref_grad, xc.grad)
