"""Shared by the GPU parity tests and the CPU oracle tests: float64 pins of the component fixtures.

tests/golden/<family>_f64.npz (oracle/gen_golden.py --f64) holds, for every output key k of the fp32 fixture
<family>.npz, the reference's own float64 run on the fixture's inputs (k), a normaliser S (k__scale: max|f64| for
arrays, the magnitude of the un-cancelled terms for scalar losses) and the reference's fp32 drift
(k__drift = max|fp32 golden - f64| / S).  One bound rule for a result `got`:

    err = max|got - f64| / S  <=  max(4 * drift, 2^-20),  and  err <= 1e-5  unless k is in `ill_conditioned`

4 * drift: a different but equally correct fp32 evaluation order rounds by about as much as the reference's own order;
2^-20 (16 fp32 ulps of S) covers outputs whose drift is near zero by chance.  `ill_conditioned` (4 * drift > 1e-5) is
fixed by tests/test_oracle_golden.py::test_f64_fixture_consistency; `dropped` lists fp32 keys left out for size."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 2.0 ** -20
NORTH_STAR = 1e-5
FAMILIES = ("propagation", "contrast", "bpr", "mhcn", "mhcn_wide", "sept_social", "buir", "grace", "rownorm")
_cache = {}


def _numpy(got):
    if hasattr(got, "detach"):
        got = got.detach().cpu().double().numpy()
    return np.asarray(got, dtype=np.float64)


class Pins:
    def __init__(self, family):
        self.family = family
        self.z = np.load(os.path.join(GOLDEN, f"{family}_f64.npz"), allow_pickle=False)
        self.ill = set(self.z["ill_conditioned"].tolist())
        self.dropped = set(self.z["dropped"].tolist())
        self.keys = sorted(k for k in self.z.files if "__" not in k and k not in ("ill_conditioned", "dropped"))

    def ref(self, key):
        return self.z[key]

    def scale(self, key):
        return float(self.z[f"{key}__scale"])

    def bound(self, key):
        return max(4.0 * float(self.z[f"{key}__drift"]), FLOOR)

    def err(self, key, got):
        got, ref = _numpy(got), self.z[key]
        assert got.shape == ref.shape, (self.family, key, got.shape, ref.shape)
        return float(np.abs(got - ref).max()) / self.scale(key) if ref.size else 0.0

    def check(self, key, got):
        """Asserts the bound rule for `got` against key (printing err / bound); returns err."""
        if key in self.dropped:
            raise KeyError(f"{self.family}_f64.npz: {key} was dropped for size; the caller must not pin it")
        err = self.err(key, got)
        b = self.bound(key)
        where = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        print(f"F64PIN {self.family}:{key} err={err:.3e} bound={b:.3e} ratio={err / b:.3f} {where}")
        msg = f"{self.family}_f64.npz {key}: err {err:.3e} > bound {b:.3e} (drift {float(self.z[f'{key}__drift']):.3e})"
        assert err <= b, msg
        if key not in self.ill:
            assert err <= NORTH_STAR, msg + f"; above the north star {NORTH_STAR:g}"
        return err


def pins(family):
    if family not in _cache:
        _cache[family] = Pins(family)
    return _cache[family]
