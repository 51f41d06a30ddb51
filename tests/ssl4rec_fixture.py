"""Reader of tests/golden/ssl4rec_steps.npz (written by scripts/gen_golden_ssl4rec_steps.py, which imports this module
too, so that both sides share one definition of what is regenerated instead of stored).

What the fixture does not store, to stay under the size limit for a committed file:
  * the initial values of every weight matrix with a 1024-wide side ("wide" matrices: user_net / item_net weights of
    n.layers >= 2).  They are `wide_init`: integers drawn by numpy's PCG64 from a stored seed, times 2^-12, uniform
    inside nn.Linear's own bound 1 / sqrt(fan_in).  The generator loads them into the reference model in place of the
    constructor's draw; the fixture keeps a CRC-32 of each so that a changed numpy stream fails loudly.
  * the final values of those matrices outside a seeded sample of SAMPLE entries (`sample_index`, CRC-checked too).
Every other tensor is stored whole.
"""
import os
import zlib

import numpy as np

import step_pins as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssl4rec_steps.npz")
GRID = 2.0 ** -12
SAMPLE = 4096
WIDE = 1024
TERMS = ("rec_loss", "cl_loss", "batch_loss")
SENSITIVITY = ("alpha", "reg_weight")


def is_wide(shape):
    return len(shape) == 2 and WIDE in shape


def wide_init(shape, seed):
    """float32 [out, in]: uniform on the 2^-12 grid inside +-1 / sqrt(in), nn.Linear's default bound."""
    levels = int(np.floor(1.0 / np.sqrt(shape[1]) / GRID))
    rng = np.random.default_rng(int(seed))
    return (rng.integers(-levels, levels + 1, size=tuple(shape)) * GRID).astype(np.float32)


def sample_index(size, seed):
    """SAMPLE distinct flat positions of a tensor of `size` entries, ascending."""
    return np.sort(np.random.default_rng(int(seed)).choice(int(size), SAMPLE, replace=False)).astype(np.int64)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def unpack_bits(words, n):
    """bool [n]: bit e of the little-endian 32-bit words (gcr_edge_mask_bits order)."""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def pack_bits(keep):
    """int32 words of a bool vector, bit e <-> entry e."""
    pad = (-keep.size) % 32
    return np.packbits(np.concatenate([keep, np.zeros(pad, bool)]), bitorder="little").view(np.int32)


class Config:
    """One configuration of the fixture: hyper-parameters, initial state, masks, and what the reference computed."""

    def __init__(self, g, c):
        self.g, self.pre = g, f"c{c}/"
        p = self.pre
        self.n_layers, self.emb = int(g[p + "n_layers"]), int(g[p + "emb"])
        self.drop, self.tau, self.alpha = float(g[p + "drop"]), float(g[p + "tau"]), float(g[p + "alpha"])
        self.reg_weight = float(g[p + "reg_weight"])
        self.names = [str(s) for s in g[p + "names"]]
        self.shapes = {k: tuple(int(x) for x in g[f"{p}shape/{k}"]) for k in self.names}
        self.keep_bits = g[p + "keep_bits"]                      # int32 [steps, 2, ceil(B * emb / 32)]

    def conf(self):
        g = self.g
        return {"embedding.size": self.emb, "batch.size": int(g["batch_size"]), "learning.rate": float(g["learning_rate"]),
                "reg.lambda": 1e-4, "max.epoch": 1, "item.ranking.topN": [10], "n.layers": self.n_layers,
                "reg.weight": self.reg_weight, "SSL4Rec": {"alpha": self.alpha, "tau": self.tau, "drop": self.drop}}

    def sampled(self, name):
        return is_wide(self.shapes[name])

    def index(self, name):
        """Flat positions at which `final(name)` is stored (None: the whole tensor)."""
        if not self.sampled(name):
            return None
        idx = sample_index(int(np.prod(self.shapes[name])), int(self.g[f"{self.pre}sample_seed/{name}"]))
        assert crc(idx) == int(self.g[f"{self.pre}sample_crc/{name}"]), f"numpy stream changed: sample of {name}"
        return idx

    def init(self, name):
        if not self.sampled(name):
            return self.g[f"{self.pre}init/{name}"]
        w = wide_init(self.shapes[name], int(self.g[f"{self.pre}init_seed/{name}"]))
        assert crc(w) == int(self.g[f"{self.pre}init_crc/{name}"]), f"numpy stream changed: initial {name}"
        return w

    def at(self, name, full):
        """The entries of a whole tensor `full` that `final(name)` holds."""
        idx = self.index(name)
        full = np.asarray(full)
        return full if idx is None else full.reshape(-1)[idx]

    def record(self):
        """The trajectory of this configuration as tests/step_pins.py takes it: finals at the stored entries (`at`), the
        MOVED rule against the initial values there, the dropped-term deltas for the CPU test's DROPPED_CPU claim."""
        g, p, names = self.g, self.pre, self.names
        slack = {k: float(g[f"{p}slack/{k}"]) for k in names}
        return sp.Record("ssl4rec", f"config {p[1:-1]}", TERMS, *sp.stack_terms(g, p, TERMS), {k: g[f"{p}f64/final/{k}"] for k in names},
                         slack, dropped={k: {t: float(g[f"{p}delta_{t}/{k}"]) for t in SENSITIVITY} for k in names}, factor=None,
                         moved={k: (self.at(k, self.init(k)), slack[k]) for k in names})


def load():
    g = np.load(GOLDEN, allow_pickle=False)
    return g, [Config(g, c) for c in range(int(g["configs"]))]
