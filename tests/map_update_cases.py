"""Rows that meet the device map's table (csrc/map.hip) where random data does not: a numpy restatement of map_hash and
map_home_slot (vo_math.h; tests/test_map_update_cpu.py holds it to the host build bit for bit), builders of rows with equal
32-bit tags, of rows of different tags with one home slot in every table size, of such rows at the table's end, and the
reference of an update that overflows.  CPU only.

The rows are MADE, not found: the hash takes component 9 in by an addition after everything else, and its finaliser is a
bijection of 32-bit words, so component 9 can be solved for any hash wanted once components 0..8 are drawn.  A draw whose
solution is a NaN pattern or -0 (which hashes as +0) is thrown away."""
import numpy as np

M32 = 0xFFFFFFFF
GOLD = 0x9E3779B1                       # map_home_slot's multiplier
C1, C2 = 0x2C1B3C6D, 0x297A2D39         # the finaliser's
ZERO_AT, NEG_ZERO_AT, NAN_AT = 2, 5, 4  # every made row holds +0 and -0 here; nan_copy() puts its NaN there
LOG_T_MIN, LOG_T_MAX = 12, 20           # table sizes the chains hold for: 2^12 .. 2^20 slots


# ---- the restatement (vectorised) ---------------------------------------------------------------------------------------
def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def map_words(app):
    """the ten 32-bit words the hash reads per row: the float's bits, 0 for a zero of either sign"""
    A = np.ascontiguousarray(app, np.float32).reshape(-1, 10)
    w = A.view(np.uint32).copy()
    w[A == 0] = 0
    return w


def map_prestate(app, upto=10):
    """the hash's state after components 0 .. upto-1, before the finaliser"""
    w = map_words(app)
    x = np.full(len(w), 0x9E3779B9, np.uint32)
    with np.errstate(over="ignore"):
        for k in range(upto):
            x = (_rotl(x, 7) + w[:, k]) if (k & 1) else (_rotl(x, 11) ^ w[:, k])
    return x


def _finalise(x):
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(15)); x = x * np.uint32(C1)
        x = x ^ (x >> np.uint32(12)); x = x * np.uint32(C2)
        x = x ^ (x >> np.uint32(15))
    return x


def map_hash(app):
    return _finalise(map_prestate(app))


def map_home_slot(h, tmask):
    with np.errstate(over="ignore"):
        return (np.asarray(h, np.uint32) * np.uint32(GOLD)) & np.uint32(tmask)


def has_nan(app):
    return np.isnan(np.asarray(app, np.float32).reshape(-1, 10)).any(axis=1)


# ---- the finaliser backwards (python integers) ---------------------------------------------------------------------------
def _unfinalise(h):
    x = h
    x ^= x >> 15; x ^= x >> 30
    x = (x * pow(C2, -1, 1 << 32)) & M32
    x ^= x >> 12; x ^= x >> 24
    x = (x * pow(C1, -1, 1 << 32)) & M32
    x ^= x >> 15; x ^= x >> 30
    return x & M32


def _usable_word(w):
    """a float's bits that are neither a NaN nor -0 (+-inf, subnormals and +0 are rows like any other)"""
    return w != 0x80000000 and not ((w & 0x7F800000) == 0x7F800000 and (w & 0x007FFFFF))


def _draw_head(rng):
    """components 0..8 of a made row: random, with +0 and -0 at their fixed places"""
    r = np.zeros(10, np.float32)
    r[:9] = rng.uniform(-1, 1, 9).astype(np.float32)
    r[ZERO_AT] = np.float32(0.0); r[NEG_ZERO_AT] = np.float32(-0.0)
    return r


def _row_with_hash(rng, h):
    """a row whose hash is h: draw components 0..8, solve component 9 (w9 = state wanted - rotl(state after 8, 7))"""
    want = _unfinalise(int(h))
    while True:
        r = _draw_head(rng)
        x8 = int(map_prestate(r[None], 9)[0])
        w9 = (want - (((x8 << 7) | (x8 >> 25)) & M32)) & M32
        if _usable_word(w9):
            r.view(np.uint32)[9] = w9
            return r


# ---- the builders ---------------------------------------------------------------------------------------------------------
def tag_family(rng, K=6):
    """K rows, pairwise different under ==, of ONE 32-bit hash: a random row, and rows that differ from it in component 8
    (and the others, but for the zeros) with component 9 solved"""
    assert K >= 4
    first = _draw_head(rng)
    first[9] = np.float32(rng.uniform(-1, 1))
    h = int(map_hash(first[None])[0])
    rows = [first]
    while len(rows) < K:
        r = _row_with_hash(rng, h)
        if all(not np.all(r == o) for o in rows):
            rows.append(r)
    return np.stack(rows)


def _chain(rng, n, low20s):
    """n rows of n different tags whose h * GOLD has the low 20 bits low20s[i]: the high 12 bits are free, 4096 tags each"""
    inv = pow(GOLD, -1, 1 << 32)
    his = rng.choice(1 << 12, n, replace=False)
    return np.stack([_row_with_hash(rng, (((int(hi) << 20) | int(lo)) * inv) & M32) for hi, lo in zip(his, low20s)])


def slot_chain(rng, n=32):
    """n >= 32 rows, each of a different tag, with ONE home slot in every table of 2^12 .. 2^20 slots"""
    assert n >= 32
    lo = int(rng.integers(0, (1 << LOG_T_MAX) - 64))          # (not at the end: that is wrap_chain's)
    return _chain(rng, n, [lo] * n)


def wrap_chain(rng, n=32):
    """the same with every home slot among the LAST 8 of every such table (bits 3..19 of h * GOLD set): n rows claim n slots
    in a row from there, over the table's end"""
    assert n >= 32
    return _chain(rng, n, [0xFFFF8 | int(r) for r in rng.integers(0, 8, n)])


def flip_zeros(rows):
    """the same classes with the sign of every zero flipped: equal under ==, other bits"""
    r = np.array(rows, np.float32).reshape(-1, 10).copy()
    z = r == 0
    w = r.view(np.uint32)
    w[z] ^= np.uint32(0x80000000)
    return r


def nan_copy(rows):
    """copies with one NaN each: rows that equal nothing, themselves included"""
    r = np.array(rows, np.float32).reshape(-1, 10).copy()
    r[:, NAN_AT] = np.nan
    return r


# ---- the properties, as assertions (the CPU tests on the builders; the GPU tests on the rows they were handed) ------------
def _pairwise_different(rows):
    rows = np.asarray(rows, np.float32)
    eq = (rows[:, None, :] == rows[None, :, :]).all(axis=2)
    return bool((eq == np.eye(len(rows), dtype=bool)).all())


def check_family(rows):
    assert len(rows) >= 4 and not has_nan(rows).any()
    assert _pairwise_different(rows)
    assert len(set(map_hash(rows).tolist())) == 1


def check_chain(rows, wrap=False):
    assert len(rows) >= 32 and not has_nan(rows).any()
    h = map_hash(rows)
    assert len(set(h.tolist())) == len(rows)                   # every member a tag of its own
    for lg in range(LOG_T_MIN, LOG_T_MAX + 1):
        tmask = (1 << lg) - 1
        s = map_home_slot(h, tmask)
        if wrap:
            assert (s >= tmask - 7).all()                      # so len(rows) >= 32 slots in a row run over the end
        else:
            assert len(set(s.tolist())) == 1


def check_zero_flip(rows, flipped):
    rows = np.asarray(rows, np.float32); flipped = np.asarray(flipped, np.float32)
    assert (rows == flipped).all() and rows.tobytes() != flipped.tobytes()
    assert ((rows == 0).sum(axis=1) >= 2).all()
    assert np.array_equal(map_hash(rows), map_hash(flipped))


# ---- the reference of an update that does not fit --------------------------------------------------------------------------
def cut_update(m, pts, app, cap):
    """oracle.vo_pipeline.Map.update, then the lists cut to cap entries and the keys of the cut entries forgotten (a class
    that was cut is new again the next time).  Returns the number of entries cut."""
    m.update(list(pts), list(app))
    cut = max(0, len(m.pts) - cap)
    if cut:
        del m.pts[cap:]
        del m.app[cap:]
        m.idx = {k: j for k, j in m.idx.items() if j < cap}
    return cut
