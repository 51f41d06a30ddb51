"""tests/diffuse_rules.py on the CPU: the sparse restatement is the dense one and the stored float64 component cases, the
large-n builder zeroes at most 1e-3 of g, and the float64 reference it returns passes the comparison rule itself."""
import numpy as np
import pytest
import torch

import diffnet_fixture as dfx
import diffuse_rules as dr


def _random_case(n, d, seed, ones=False):
    rng = np.random.default_rng([n, d, seed])
    deg = rng.choice(dr.UNROLL_DEGREES, n)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    col = rng.integers(0, n, row.size).astype(np.int64)
    val = None if ones else rng.uniform(0.1, 1.0, row.size).astype(np.float32)
    return (row, col, val, n) + dfx.component_inputs(d, seed, n=n)


@pytest.mark.parametrize("ones", [False, True])
def test_the_sparse_restatement_is_the_dense_one(ones):
    case = _random_case(257, 64, 5, ones)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-5)):        # the two sum in different orders
        dense, dense_pre = dr.dense_restatement(*case, dtype)
        sparse, sparse_pre = dr.sparse_restatement(*case, dtype)
        for have, want in [(sparse[k], dense[k]) for k in dr.KEYS] + [(sparse_pre, dense_pre)]:
            assert have.shape == want.shape and np.abs(have - want).max() <= tol * np.abs(want).max()


@pytest.mark.parametrize("d", dfx.COMP_WIDTHS)
def test_the_sparse_restatement_gives_the_stored_component_cases(d):
    c = dfx.component(dfx.load(), d)
    got, _ = dr.sparse_restatement(c["row"], c["col"], c["val"], dfx.COMP_N, c["x"], c["w"], c["g"], torch.float64)
    for k in dr.KEYS:
        assert np.abs(got[k] - c[k]).max() <= 1e-12 * c[f"scale/{k}"], k


@pytest.mark.parametrize("n,d", dr.MULTI_TRIP_SHAPES)
def test_the_large_case_zeroes_little_of_g_and_its_reference_passes_the_rule(n, d):
    c = dr.large_case(n, d)
    print(f"DIFFUSE zeroed share n={n} d={d}: {c['share']:.3g}; drift " + " ".join(f"{k} {c['drift'][k]:.3g}" for k in dr.KEYS))
    assert 0 < c["share"] <= dr.MAX_ZEROED_SHARE
    deg = np.bincount(c["row"], minlength=n)
    assert (deg[0], deg[1], deg[-1]) == (1000, 0, 9) and c["col"].max() == n - 1 and c["col"].min() == 0
    assert set(dr.UNROLL_DEGREES) <= set(deg[2:-1].tolist()) and np.median(deg) <= 4
    # every element the mask could differ on carries no gradient; the float32 run of the source is inside the rule
    _, pre64 = dr.sparse_restatement(c["row"], c["col"], c["val"], n, c["x"], c["w"], c["g"], torch.float64)
    _, pre32 = dr.sparse_restatement(c["row"], c["col"], c["val"], n, c["x"], c["w"], c["g"], torch.float32)
    assert not c["g"][(pre64 > 0) != (pre32 > 0)].any()
    for k in dr.KEYS:
        assert c["drift"][k] <= dr.NORTH_STAR / 4, k


def test_the_exact_case_is_exact_in_float32_and_has_pre_activations_at_zero():
    for d in dfx.COMP_WIDTHS:
        for ones in (False, True):
            row, col, val, x, w, g = dr.exact_case(d, ones)
            f64, pre = dr.sparse_restatement(row, col, val, len(x), x, w, g, torch.float64)
            f32, _ = dr.sparse_restatement(row, col, val, len(x), x, w, g, torch.float32)
            for k in dr.KEYS:
                assert np.array_equal(f32[k], f64[k]) and np.abs(f64[k]).max() < 2 ** 24, (d, ones, k)
            at_zero = (pre == 0) & (g != 0)
            assert at_zero[1].all() and at_zero[:, 3].all() and at_zero.sum() > at_zero[1].sum() + at_zero[:, 3].sum() - 1
            assert not f64["dw"][:, 3].any()                   # what `h >= 0` in the backward's mask would fill
