"""The cases shared by tests/test_map_covis_cpu.py (which asserts that every case is what it says) and
tests/test_gpu_map_covis.py (which runs them on the device and compares every byte with tests/map_covis_restatement.py).

A covisibility case is a dict: map_pts (M, 3), map_app (M, 10), frames [(uv, app)], n_rows (or None), n_words (or None: the
words the map needs), dup_rows (rows of the map entered TWICE by the update that builds it, so that the host's bound of the size
lies above the size the device holds), windows [dict(query, k_free, k_fixed, min_shared)].  A window case is a dict: bits (F, W)
uint32, n_rows (or None), n_max, windows -- voe_map_window* reads the bits alone, so its ties are made by hand.

The scenes come from tests/map_refine_cases.hand(...) where its shape fits (the map sizes, the content) and from frames_over()
below where it does not: hand() bounds a landmark's count by the number of frames, which leaves a single frame no 40 rows."""
import numpy as np

import map_covis_restatement as V
import map_refine_cases as Rc
import map_refine_restatement as R

TILE, CHUNK = 32, 64                                         # map_covis.hip: frames along a tile's edge, words per staged chunk
MAP_SIZES = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2016, 2047, 2048, 2049, 4097)      # 2048 entries are one chunk of 64 words: 63, 64, 65, 129 words
FRAME_COUNTS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)                    # the edges of every power-of-two tile up to 64 (the kernel's: 32)
EXAMPLE_WINDOWS = [dict(query=q, k_free=8, k_fixed=8, min_shared=15) for q in (0, 60, 120)]


def _windows(F, *more):
    k = min(3, F)
    return [dict(query=0, k_free=k, k_fixed=k, min_shared=2)] + list(more)


def example():
    P = R.example_problem()
    pts = np.asarray(P["world_pts"], np.float32)
    return dict(K=P["K"], map_pts=pts, map_app=P["world_app"], frames=P["frames"], poses=P["poses"], n_rows=None, n_words=None, dup_rows=0,
                windows=EXAMPLE_WINDOWS)


def map_size(size, n_words=None, dup_rows=0):
    """a map of `size` entries seen by 5 frames: the first and the last entry, the entries around every word edge below the size"""
    counts = np.zeros(size, int)
    rng = np.random.default_rng(100 + size)
    who = {0, size - 1, size - 2, size // 2} | {e for e in (31, 32, 33, 63, 64, 1023, 1024, 2047, 2048) if e < size}
    who |= set(int(e) for e in rng.integers(0, size, 12))
    for e in sorted(x for x in who if 0 <= x < size):
        counts[e] = 1 + (e % 5)
    c = Rc.hand(list(counts), 5, 200 + size)
    F = len(c["frames"])
    return dict(map_pts=c["map_pts"], map_app=c["map_app"], frames=c["frames"], n_rows=c["n_rows"], n_words=n_words, dup_rows=dup_rows,
                windows=_windows(F))


def frames_over(app, F, rows, seed, spread=60):
    """F frames of `rows` rows each: frame f sees a random draw from the entries within `spread` of f * M / F (wrapping), so that
    near frames share many entries and far ones none"""
    rng = np.random.default_rng(seed)
    M = len(app)
    frames = []
    for f in range(F):
        centre = (f * M) // max(F, 1)
        pool = (centre + np.arange(-spread, spread + 1)) % M
        ids = rng.choice(np.unique(pool), min(rows, len(np.unique(pool))), replace=False)
        frames.append((rng.uniform(0, 600, (len(ids), 2)).astype(np.float32), app[ids].copy()))
    return frames


def frame_count(F, M=300):
    rng = np.random.default_rng(300 + F)
    app = rng.uniform(-1, 1, (M, 10)).astype(np.float32)
    pts = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    return dict(map_pts=pts, map_app=app, frames=frames_over(app, F, 40, 400 + F), n_rows=None, n_words=None, dup_rows=0,
                windows=_windows(F, dict(query=F - 1, k_free=min(8, F), k_fixed=min(8, F), min_shared=5)))


def large_map(M=65537):
    """many word chunks, few pairs: 3 frames over 65 537 entries, the first and the last entry among them"""
    rng = np.random.default_rng(65537)
    app = rng.uniform(-1, 1, (M, 10)).astype(np.float32)
    pts = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    frames = []
    for f in range(3):
        ids = np.unique(np.concatenate([[0, M - 1, 1024 * 32 + f], rng.integers(0, M, 50), np.arange(40000, 40020)]))
        ids = rng.permutation(ids)
        frames.append((np.zeros((len(ids), 2), np.float32), app[ids].copy()))
    return dict(map_pts=pts, map_app=app, frames=frames, n_rows=None, n_words=None, dup_rows=0, windows=_windows(3))


def content():
    """hand()'s extras -- a frame with 0 live rows, garbage behind the live rows, two rows of one frame on one entry, a NaN
    appearance row, -0 against +0, rows of no map -- plus two identical frames and two disjoint ones"""
    c = Rc.hand([9, 7, 5, 3, 9, 8, 2, 6, 4, 9, 0, 5], 9, 77, map_size=40, extras=True)
    frames, n_rows = list(c["frames"]), list(c["n_rows"])
    frames.append((frames[0][0].copy(), frames[0][1].copy())); n_rows.append(n_rows[0])      # identical to frame 0
    app = c["map_app"]
    for ids in (np.arange(20, 30), np.arange(30, 40)):                                        # disjoint from each other (and unseen by the rest)
        frames.append((np.zeros((len(ids), 2), np.float32), app[ids].copy())); n_rows.append(len(ids))
    F = len(frames)
    return dict(map_pts=c["map_pts"], map_app=app, frames=frames, n_rows=np.array(n_rows, np.int32), n_words=None, dup_rows=0,
                windows=_windows(F, dict(query=3, k_free=2, k_fixed=2, min_shared=1)), identical=(0, F - 3), disjoint=(F - 2, F - 1), empty=3)


# ---- the window's ties, by hand ----
QUERY_ROW = 24                                               # frame 0 sees entries 0 .. 23
SHARED = {1: 12, 2: 12, 3: 12, 4: 9, 5: 9, 6: 6, 7: 20, 8: 2, 14: 12}      # frame g sees the first SHARED[g] entries of frame 0's
PRIVATE = {7: range(30, 40), 8: range(30, 32), 9: range(30, 36), 10: range(30, 36), 11: range(30, 34), 12: range(40, 51)}


def window_ties():
    """15 frames over 96 bits.  With min_shared 3 the candidates of query 0 rank 7 (20), 1, 2, 3, 14 (12 each), 4, 5 (9), 6 (6).
    Frame 13 is empty; frame 14 is the last.  With frames 0, 7, 1 free, U is entries 0 .. 23 and 30 .. 39 and the frames not free
    rank 2, 3, 14 (12), 4, 5 (9), 6, 9, 10 (6), 8, 11 (4); frame 12 shares nothing."""
    F, W = 15, 3
    S = np.zeros((F, 32 * W), bool)
    S[0, :QUERY_ROW] = True
    for g, c in SHARED.items():
        S[g, :c] = True
    for g, r in PRIVATE.items():
        S[g, list(r)] = True
    w = lambda **kw: dict(dict(query=0, k_free=3, k_fixed=2, min_shared=3), **kw)
    windows = dict(tie_across_k_free=w(), ties_inside=w(k_free=6, k_fixed=4), tie_across_k_fixed=w(), k_free_1=w(k_free=1), k_fixed_0=w(k_fixed=0),
                   above_candidates=w(k_free=F, k_fixed=F), no_candidate=w(min_shared=25), query_unseen=w(query=13), query_last=w(query=14))
    return dict(bits=V.pack_bits(S, W), n_rows=np.arange(10, 10 + F, dtype=np.int32), n_max=40, windows=list(windows.values()),
                window_names=list(windows))


def window_no_row_counts():
    c = window_ties()
    return dict(c, n_rows=None, n_max=17, windows=c["windows"][:2], window_names=c["window_names"][:2])


CASES = {"example": example, "content": content, "large_map": large_map, "padded_words": lambda: map_size(65, n_words=7),
         "bound_above_size": lambda: map_size(60, n_words=3, dup_rows=10)}
CASES.update({f"map_{n}": (lambda n=n: map_size(n)) for n in MAP_SIZES})
CASES.update({f"frames_{n}": (lambda n=n: frame_count(n)) for n in FRAME_COUNTS})
WINDOW_CASES = {"window_ties": window_ties, "window_no_row_counts": window_no_row_counts}

_cache, _ref, _win = {}, {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = (CASES.get(name) or WINDOW_CASES[name])()
    return _cache[name]


def n_max_of(c):
    return max([len(a) for _, a in c["frames"]] + [1])


def n_words_of(c):
    return c["n_words"] if c["n_words"] is not None else V.words_for(len(c["map_app"]) + c["dup_rows"])


def reference(name):
    """the restatement's covisibility of a case, computed once and shared"""
    if name not in _ref:
        c = case(name)
        _ref[name] = V.covis(c["map_app"], c["frames"], n_rows=c["n_rows"], n_words=n_words_of(c))
    return _ref[name]


def live_rows(c):
    """what the window hands on as a frame's live rows"""
    if "bits" in c:
        return c["n_rows"], c["n_max"]
    return c["n_rows"], n_max_of(c)


def window_reference(name, k):
    """the restatement's window k of a case (on the restatement's own bits), computed once and shared"""
    if (name, k) not in _win:
        c = case(name)
        bits = c["bits"] if "bits" in c else reference(name)["bits"]
        n_rows, n_max = live_rows(c)
        _win[(name, k)] = V.window(bits, n_rows=n_rows, n_max=n_max, **c["windows"][k])
    return _win[(name, k)]
