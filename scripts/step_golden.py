"""TEST INFRASTRUCTURE ONLY — what the writers of tests/golden/*_steps.npz (scripts/gen_golden_*_steps.py and
scripts/gen_golden_directau.py) share: the social data set of the MHCN, SEPT and BUIR fixtures, "the first N full batches
of a seeded sampler", the id and triple arrays, the step that records one table under the rule of tests/step_pins.py (whose
constants and tolerance functions it imports, so that writer and readers share one definition), and the save tail.

Regenerating a fixture, for every one of them:  python scripts/gen_golden_<name>.py [--out DIR]  — where the reference
sources are; without --out it rewrites tests/golden/.  Nothing of the reference is in this file: each writer lifts what it
runs through oracle/gen_golden.py."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]              # for the writers too: `oracle`, the fixture readers
import step_pins as sp  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SIZE_CAP = 1_000_000
N_USERS, N_ITEMS, N_TRAIN, GROUPS = 200, 120, 1400, 5       # of `synthetic_lists`


def synthetic_lists(rng):
    """(train triples, social triples) over raw integer ids: a planted group structure, one repeated interaction, one
    repeated social pair, two social pairs naming a user that never interacts."""
    raw_u = np.sort(rng.choice(np.arange(10_000, 99_999), N_USERS + 2, replace=False))
    ghosts, raw_u = raw_u[[7, 150]], np.delete(raw_u, [7, 150])           # two ids that never interact
    raw_i = np.sort(rng.choice(np.arange(100_000, 999_999), N_ITEMS, replace=False))
    pairs = {(u, int(rng.integers(0, N_ITEMS))) for u in range(N_USERS)}
    pairs |= {(int(rng.integers(0, N_USERS)), i) for i in range(N_ITEMS)}
    while len(pairs) < N_TRAIN:
        u = int(rng.integers(0, N_USERS))
        i = int(rng.integers(0, N_ITEMS // GROUPS)) * GROUPS + u % GROUPS if rng.random() < 0.8 \
            else int(rng.integers(0, N_ITEMS))
        pairs.add((u, i))
    pairs = sorted(pairs)
    rng.shuffle(pairs)
    train = [[int(raw_u[u]), int(raw_i[i]), 1.0] for u, i in pairs]
    train.append(list(train[0]))                                           # a repeated interaction: 2 in Y
    soc = set()
    while len(soc) < 1200:
        a = int(rng.integers(0, N_USERS))
        b = (a + GROUPS * int(rng.integers(1, 12))) % N_USERS if rng.random() < 0.7 else int(rng.integers(0, N_USERS))
        if a != b:
            soc.add((a, b))
    soc = sorted(soc)
    rng.shuffle(soc)
    have = set(soc)
    soc = soc + [(b, a) for a, b in soc[:400] if (b, a) not in have]       # reciprocated pairs
    social = [[int(raw_u[a]), int(raw_u[b]), 1.0] for a, b in soc]
    social.insert(100, list(social[3]))                                    # a repeated social pair: 2 in S
    social.insert(50, [int(ghosts[0]), int(raw_u[1]), 1.0])                # unknown follower
    social.append([int(raw_u[2]), int(ghosts[1]), 1.0])                    # unknown followee
    return train, social


def synthetic_pairs(rng, n_users, n_items, n_train, groups):
    """Unique (user, item) pairs with a planted group structure; every user and every item occurs."""
    pairs = {(u, int(rng.integers(0, n_items))) for u in range(n_users)}
    pairs |= {(int(rng.integers(0, n_users)), i) for i in range(n_items)}
    while len(pairs) < n_train:
        u = int(rng.integers(0, n_users))
        i = int(rng.integers(0, n_items // groups)) * groups + u % groups if rng.random() < 0.8 \
            else int(rng.integers(0, n_items))
        pairs.add((u, i))
    pairs = sorted(pairs)
    rng.shuffle(pairs)
    return np.array(pairs, dtype=np.int64)


def csr_dict(prefix, m):
    m = m.tocsr().astype(np.float32)
    m.sum_duplicates()
    m.sort_indices()
    m.eliminate_zeros()
    return {f"{prefix}_indptr": m.indptr.astype(np.int32), f"{prefix}_indices": m.indices.astype(np.int16),
            f"{prefix}_data": m.data.astype(np.float32), f"{prefix}_shape": np.array(m.shape, dtype=np.int32)}


def first_batches(sampler, steps, batch_size, convert=tuple):
    """The first `steps` batches of the reference's own sampler, which the caller has seeded; all of them full."""
    out = []
    for b in sampler:
        if len(out) == steps:
            break
        assert len(b[0]) == batch_size
        out.append(convert(b))
    return out


def id_arrays(train, data, social=None):
    """The raw training triples (and social pairs) and the reference's dense-id maps, as the readers' preamble wants them."""
    out = dict(train_user=np.array([t[0] for t in train]), train_item=np.array([t[1] for t in train]),
               user_ids=np.array([data.id2user[k] for k in range(data.user_num)]),
               item_ids=np.array([data.id2item[k] for k in range(data.item_num)]))
    if social is not None:
        out.update(social_follower=np.array([t[0] for t in social]), social_followee=np.array([t[1] for t in social]))
    return out


def store_batches(out, batches, names, dtype, prefix=""):
    for n, b in enumerate(batches):
        for s, t in zip(names, b):
            out[f"{prefix}batch{n}_{s}"] = np.asarray(t).astype(dtype)


def record_table(out, pre, family, k, p64, p32, reruns, init=None, store_init=True, exact=2e-9, unreached=None,
                 factor=sp.DROPPED, extra=""):
    """One table of one configuration: its float64 final (whole under f64/final, or with `init` as float32(final - init)
    under f64/delta, asserted exact), its float32 slack and, per dropped term of `reruns` = {term: finals of the float64
    rerun without it}, what the term moves; prints the row and asserts the family's sensitivity rule.  Returns the slack."""
    if init is None:
        out[f"{pre}f64/final/{k}"] = p64
    else:
        assert init.dtype == np.float32
        delta = (p64 - init.astype(np.float64)).astype(np.float32)
        assert np.abs(init.astype(np.float64) + delta.astype(np.float64) - p64).max() < exact
        out[f"{pre}f64/delta/{k}"] = delta
        if store_init:
            out[f"{pre}init/{k}"] = init
    slack = out[f"{pre}slack/{k}"] = float(np.abs(p32 - p64).max())
    atol = sp.TABLE_FORM[family](slack)
    row = [f"{k:16s} slack {slack:.3g}{extra}"]
    for term, final in reruns.items():
        d = out[f"{pre}delta_{term}/{k}"] = float(np.abs(final[k] - p64).max())
        row.append(f"d_{term} {d:.3g} ({d / atol:.0f}x atol)")
        assert sp.sees_dropped(d, atol, k in (unreached or {}).get(term, ()), factor), (k, term, d, atol)
    print("  " + "  ".join(row))
    return slack


def save(out_dir, name, out, write=None):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, name + ".npz")
    write(path, out) if write else np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", os.path.abspath(path), size, "bytes")
    assert size < SIZE_CAP


def out_dir():
    return sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
