"""The cases of tests/test_gpu_map_nearest.py: the smallest shapes at which voe_map_nearest* can go wrong, each with what it is
there for, and their references (tests/map_nearest_restatement.py), computed once.

A case: dict(map_app (M, 10), frames [ (rows, 10) ], n_rows (list or None), n_max, radius, ratio, unique, dup_rows, dyadic).
DYADIC cases are the deliberate ties and boundaries: every coordinate is a small multiple of 2^-13, so every difference, square
and sum is exact in float32 AND in float64 and the two evaluations agree although the decisions are at equality.  Every other
case takes no decision that float32 and float64 evaluate differently (tests/test_map_nearest_cpu.py asserts both)."""
import functools

import numpy as np

import map_nearest_restatement as N

ROW_COUNTS_14 = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 700, 1000, 1499, 1500]


def _case(map_app, frames, n_max=None, n_rows=None, radius=0.1, ratio=0.0, unique=0, dup_rows=0, dyadic=False):
    frames = [np.asarray(a, np.float32).reshape(-1, 10) for a in frames]
    if n_max is None:
        n_max = max([len(a) for a in frames] + [0])
    return dict(map_app=np.asarray(map_app, np.float32).reshape(-1, 10), frames=frames, n_rows=n_rows, n_max=n_max, radius=radius,
                ratio=ratio, unique=unique, dup_rows=dup_rows, dyadic=dyadic)


def _noisy(rng, E, n, sigma=0.005, stray=0.1):
    """n rows: pushed copies of random entries, a tenth of them rows of their own"""
    idx = rng.integers(0, len(E), n)
    q = E[idx] + rng.normal(0, sigma, (n, 10))
    k = rng.random(n) < stray
    q[k] = rng.uniform(-1, 1, (int(k.sum()), 10))
    return q.astype(np.float32)


def _random(M, rows, seed, close_pairs=0, **kw):
    """M entries U(-1, 1)^10 (close_pairs of them 0.03 beside another: second candidates for the ratio), frames of pushed copies;
    rows are drawn with replacement, so several rows of a frame meet one entry (unique)"""
    rng = np.random.default_rng(seed)
    E = rng.uniform(-1, 1, (M, 10))
    for j in range(min(close_pairs, M // 2)):
        d = rng.normal(0, 1, 10)
        E[M - 1 - j] = E[j] + 0.03 * d / np.linalg.norm(d)
    E = E.astype(np.float32)
    return _case(E, [_noisy(rng, E, n) for n in rows], **kw)


def _dyadic(ratio, unique):
    """radius 0.25; groups 4 apart along component 1, the geometry along component 0 (and 5 where a tie needs a second axis)"""
    E, Q0, Q1 = [], [], []
    at = lambda g, x, y=0.0: [x, 4.0 * g, 0, 0, 0, y, 0, 0, 0, 0]
    # g0: the entry exactly at r (d2 == r2 must miss); g1: at r (1 - 2^-10), just inside
    E += [at(0, 0.25), at(1, 0.25 * (1 - 2.0 ** -10))]
    Q0 += [at(0, 0.0), at(1, 0.0)]
    # g2: two entries at exactly equal d2, the HIGHER index entered first in every order a sort by coordinate would give
    #     (entry 2 at +0.0625, entry 3 at -0.0625: the lowest index wins; with a ratio the row is ambiguous)
    E += [at(2, 0.0625), at(2, -0.0625)]
    Q0 += [at(2, 0.0)]
    # g3: the ratio exactly at equality: best d2 = 2^-8, second d2 = 2^-6, ratio 0.5: 2^-8 < 0.25 * 2^-6 is false
    E += [at(3, 0.0625), at(3, -0.125)]
    Q0 += [at(3, 0.0)]
    # g4: best at 0.125, the second just inside r: it counts, 2^-6 < 0.25 * 2^-4 (1 - 2^-10)^2 is false: ambiguous at ratio 0.5
    # g5: best at 0.125 (1 + 2^-9), the second just outside r: it does not count (counted, it would make the row ambiguous)
    E += [at(4, 0.125), at(4, -0.25 * (1 - 2.0 ** -10)), at(5, 0.125 * (1 + 2.0 ** -9)), at(5, -0.25 * (1 + 2.0 ** -10))]
    Q0 += [at(4, 0.0), at(5, 0.0)]
    # g6: three rows on one entry, two of them tied, the third closer; g7: two tied rows alone (the lower row keeps the entry)
    E += [at(6, 0.0), at(7, 0.0)]
    Q0 += [at(6, 0.0625), at(6, -0.0625), at(6, 0.0, 0.03125), at(7, 0.0, 0.0625), at(7, -0.0625)]
    # frame 1: the same entries again (uniqueness is per frame), and a lattice at spacing exactly r whose midpoints miss
    Q1 += [at(6, 0.0625), at(7, 0.0625)]
    E += [at(8, 0.5 * k) for k in range(5)]
    Q1 += [at(8, 0.5 * k + 0.25) for k in range(4)] + [at(8, 0.5 * k + 0.125) for k in range(4)]
    return _case(E, [Q0, Q1], radius=0.25, ratio=ratio, unique=unique, dyadic=True)


def _special():
    rng = np.random.default_rng(5)
    E = rng.uniform(-1, 1, (12, 10)).astype(np.float32)
    E[2, 3], E[4, 0], E[5, 9] = np.nan, np.inf, -np.inf
    E[6] = 0.0
    E[6, [1, 4]] = -0.0                                       # an entry of zeros, two of them negative
    Q = np.stack([E[0] + 0.001, E[2], E[2], E[4], E[5], np.zeros(10), -np.zeros(10), E[7] + 0.002, E[8]]).astype(np.float32)
    Q[2, 3] = 0.3                                             # beside the NaN entry: its other nine components agree
    Q[3, 1] += 0.01                                           # an infinity in the row and in the entry
    Q[4, 9] = E[5, 8]                                         # finite where the entry is -inf
    Q[8, 5] = np.inf                                          # an infinity in the row alone
    return _case(E, [Q, Q[::-1].copy()], ratio=0.8, unique=1)


def _one_cell(seed=11):
    """3000 entries inside one cell (spread 0.09 < R in every component): every query walks all of them"""
    rng = np.random.default_rng(seed)
    E = rng.uniform(0, 0.09, (3000, 10)).astype(np.float32)
    return _case(E, [(E[rng.integers(0, 3000, n)] + rng.normal(0, 0.002, (n, 10))).astype(np.float32) for n in (40, 7)], ratio=0.5, unique=1)


def _flat(seed=12):
    """entries that differ in components 0 and 1 only: the grid has two components of zero spread"""
    rng = np.random.default_rng(seed)
    E = np.zeros((400, 10), np.float32)
    E[:, :2] = rng.uniform(-1, 1, (400, 2))
    Q = E[rng.integers(0, 400, 90)] + np.concatenate([rng.normal(0, 0.004, (90, 2)), np.zeros((90, 8))], axis=1)
    Q[::7, 6] += 0.3                                          # off the map's plane: beyond the radius in a flat component
    return _case(E, [Q.astype(np.float32)], ratio=0.8, unique=0)


def _outside(seed=13):
    """5000 entries, more than the 2048 sampled with stride 2: the odd entries lie 5 beyond the even ones' range (edge cells), and
    so do the rows pushed from them"""
    rng = np.random.default_rng(seed)
    E = rng.uniform(-1, 1, (5000, 10))
    E[1::2] += 5.0 * np.sign(rng.normal(0, 1, (2500, 10)))
    E = E.astype(np.float32)
    return _case(E, [_noisy(rng, E, 300, stray=0.0), _noisy(rng, E, 200)], ratio=0.8, unique=1)


CASES = {
    "empty_map": lambda: _case(np.zeros((0, 10)), [np.random.default_rng(1).uniform(-1, 1, (5, 10)), np.zeros((2, 10))], ratio=0.8, unique=1),
    "one_entry": lambda: _case(np.full((1, 10), 0.5), [np.array([[0.5] * 10, [0.51] * 10, [0.6] * 10, [0.5] * 9 + [0.45]])], ratio=0.8, unique=1),
    "zero_rows": lambda: _random(50, [3, 3], 2, n_rows=[0, 2], ratio=0.8),
    "n_max_1": lambda: _random(70, [1, 1, 1], 3, unique=1),
    "frames14": lambda: _random(3000, ROW_COUNTS_14, 4, close_pairs=200, ratio=0.8, unique=1),
    "frames14_few": lambda: _random(1, ROW_COUNTS_14[:6], 6, ratio=0.8, unique=1),
    "frames3_plain": lambda: _random(300, [300, 17, 128], 7, close_pairs=30),
    "bound_above_size": lambda: _random(300, [100, 64], 8, close_pairs=20, ratio=0.8, unique=1, dup_rows=50),
    "one_cell": _one_cell,
    "flat_grid": _flat,
    "outside_bounds": _outside,
    "dyadic": lambda: _dyadic(0.5, 0),
    "dyadic_plain": lambda: _dyadic(0.0, 0),
    "dyadic_unique": lambda: _dyadic(0.5, 1),
    "special": _special,
}
DYADIC = ("dyadic", "dyadic_plain", "dyadic_unique")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, fault=None):
    c = case(name)
    return N.run(c["map_app"], c["frames"], c["n_rows"], c["n_max"], c["radius"], c["ratio"], c["unique"], fault=fault)
