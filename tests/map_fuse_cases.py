"""The cases of tests/test_gpu_map_fuse.py, their references (tests/map_fuse_restatement.py), the experiment on the example data, and
what tests/test_map_fuse_cpu.py checks about them: no gate or tie decision of any case differs between the float32 rules and a
float64 evaluation (the boundaries and ties of the DYADIC case are built from dyadic values, exact in both), and the cases cover what
they are there for -- `cells` restates the device's grid only to COUNT the partners that lie across a face, an edge and a corner
of it; no reference depends on it."""
import functools

import numpy as np

import map_fuse_restatement as Fr
import map_refine_restatement as R


def _case(map_pts, map_app, frames=None, n_rows=None, n_max=None, radius_xyz=0.04, radius=0.1, position=1, veto=0, dry_run=0, capacity=0, dup_rows=0,
          dyadic=False):
    map_pts, map_app = np.asarray(map_pts, np.float32).reshape(-1, 3), np.asarray(map_app, np.float32).reshape(-1, 10)
    if frames is not None:
        frames = [np.asarray(a, np.float32).reshape(-1, 10) for a in frames]
        n_max = max([len(a) for a in frames] + [0]) if n_max is None else n_max
    return dict(map_pts=map_pts, map_app=map_app, frames=frames, n_rows=n_rows, n_max=n_max if frames is not None else 0, radius_xyz=radius_xyz,
                radius=radius, position=position, veto=veto, dry_run=dry_run, capacity=capacity, dup_rows=dup_rows, dyadic=dyadic)


def _scene(M, n_dup, seed, box=(4.0, 4.0, 4.0), push=0.015, noise=0.005, classes=0, where="end"):
    """M landmarks in a box with distinct (or, with classes, folded) appearances, and n_dup of them entered a second time: the point
    pushed by U(-push, push), the appearance by N(0, noise).  `where`: the copies at the end, or shuffled among the entries."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0, 1, (M, 3)) * np.asarray(box)
    A = rng.uniform(-1, 1, (M, 10)) if not classes else rng.uniform(-1, 1, (classes, 10))[np.arange(M) % classes] + rng.normal(0, 0.002, (M, 10))
    ch = np.sort(rng.permutation(M)[:n_dup])
    P = np.concatenate([P, P[ch] + rng.uniform(-push, push, (n_dup, 3))]).astype(np.float32)
    A = np.concatenate([A, A[ch] + rng.normal(0, noise, (n_dup, 10))]).astype(np.float32)
    twin = np.concatenate([np.full(M, -1), ch])               # the landmark an entry is a copy of
    if where == "shuffled":
        order = rng.permutation(M + n_dup)
        P, A, twin = P[order], A[order], twin[order]
    return P, A, twin


def _rows(A, rng, picks, noise=0.0):
    a = A[picks].copy()
    return (a + rng.normal(0, noise, a.shape)).astype(np.float32) if noise else a


# ---- boundaries and ties from dyadic values: exact in float32 and in float64 ----
def _dyadic(position=1):
    """clusters 4 apart along y (all z are 0: zero extent on an axis; x spans less than a cell), cluster c's appearances at c in
    component 9; radius_xyz = 2^-2, radius = 2^-3.  Entry numbers in the comments."""
    ulp_x, ulp_a = np.float32(2.0 ** -26), np.float32(2.0 ** -27)      # below 2^-2 and below 2^-3
    P, A = [], []

    def add(c, x, a0, a1=0.0):
        P.append((x, 4.0 * c, 0.0))
        A.append((a0, a1, 0, 0, 0, 0, 0, 0, 0, float(c)))

    add(0, 0.0, 0.0); add(0, 0.25, 2.0 ** -4)                 # 0, 1: g2 exactly on the radius: excluded, both ALONE
    add(1, 0.0, 0.0); add(1, np.float32(0.25) - ulp_x, 2.0 ** -4)      # 2, 3: one ulp inside: a pair
    add(2, 0.0, 0.0); add(2, 0.125, 0.125)                    # 4, 5: d2 exactly on the radius: excluded
    add(3, 0.0, 0.0); add(3, 0.125, np.float32(0.125) - ulp_a)      # 6, 7: one ulp inside: a pair
    add(4, 0.0, 0.0); add(4, 0.0625, 2.0 ** -4); add(4, 0.125, -2.0 ** -4)      # 8, 9, 10: 9 and 10 tie for 8: the lower wins; 10 NOT_MUTUAL
    add(5, 0.125, -2.0 ** -4); add(5, 0.0625, 2.0 ** -4); add(5, 0.0, 0.0)      # 11, 12, 13: the same with the middle entry last: 13 takes 11
    add(6, 0.0, 0.0); add(6, 0.0625, 3 * 2.0 ** -5); add(6, 0.125, 2.0 ** -3)      # 14 -> 15 <-> 16: the chain is not followed
    add(7, 0.0, 0.0, 0.0); add(7, 0.0, 2.0 ** -5, 0.0)        # 17, 18: the same point (g2 = 0): a pair
    add(8, 0.0, 0.0)                                          # 19: nobody near
    return _case(P, A, radius_xyz=0.25, radius=0.125, position=position, dyadic=True)


def _sized(n, seed):
    """n entries with copies FIRST (entry 1 is a copy of entry 0), in a RUN in the middle and LAST: the compaction's block edges"""
    if n < 2:
        P, A, _ = _scene(n, 0, seed)
        return _case(P, A)
    D = max(1, min(n // 3, 100))
    L = n - D
    P, A, _ = _scene(L, 0, seed)
    rng = np.random.default_rng(seed + 1)
    dp = (P[:D] + rng.uniform(-0.015, 0.015, (D, 3))).astype(np.float32)
    da = (A[:D] + rng.normal(0, 0.005, (D, 10))).astype(np.float32)
    mid = max(D, L // 2)
    order = [("L", 0), ("D", 0)] + [("L", i) for i in range(1, mid)] + [("D", i) for i in range(1, D - 1)] + [("L", i) for i in range(mid, L)]
    if D > 1:
        order.append(("D", D - 1))
    pts = np.array([P[i] if k == "L" else dp[i] for k, i in order], np.float32)
    app = np.array([A[i] if k == "L" else da[i] for k, i in order], np.float32)
    assert len(pts) == n
    return _case(pts, app, position=n % 2)


def _special(seed=21):
    """NaN and infinities in points and appearances, each next to a would-be copy that has to stay ALONE; two clean pairs"""
    P, A, _ = _scene(24, 0, seed)
    P, A = np.concatenate([P, P[:10] + np.float32(0.004)]).astype(np.float32), np.concatenate([A, A[:10] + np.float32(0.002)]).astype(np.float32)
    P[0, 1] = np.nan; P[1, 2] = np.inf; P[2, 0] = -np.inf
    A[3, 4] = np.nan; A[4, 9] = np.inf; A[5, 0] = -np.inf
    P[30] = np.nan; A[31, 2] = np.nan                         # the copy is the one that is not finite
    return _case(P, A)


def _frames_case(seed, veto, n_rows_given, position=1, dry_run=0):
    """3 frames whose rows hit survivors, absorbed entries and nothing; in frame 2 some pairs are seen TOGETHER (both copies have a
    row there): with the veto they are CONFLICTs.  With n_rows_given rows lie behind the live count, among them rows that would hit."""
    P, A, twin = _scene(300, 60, seed, where="shuffled")
    rng = np.random.default_rng(seed + 7)
    M = len(A)
    copies = np.nonzero(twin >= 0)[0]
    lm = np.nonzero(twin < 0)[0]
    f0 = np.concatenate([_rows(A, rng, rng.permutation(M)[:90]), rng.uniform(-1, 1, (20, 10)).astype(np.float32)])      # either copy, and strangers
    f1 = _rows(A, rng, copies[:40])                           # copies only
    together = np.concatenate([copies[40:50], lm[:30]])
    f2 = _rows(A, rng, together)
    frames = [f0, f1, f2]
    n_rows = [100, 25, len(f2)] if n_rows_given else None
    if not n_rows_given:                                      # d_n_rows NULL: every frame has n_max live rows
        L = max(len(a) for a in frames)
        frames = [np.concatenate([a, rng.uniform(-1, 1, (L - len(a), 10)).astype(np.float32)]) for a in frames]
    return _case(P, A, frames=frames, n_rows=n_rows, veto=veto, position=position, dry_run=dry_run)


def _together(seed=33, veto=1):
    """every copy's frame row sits in the same frame as its original's: with the veto every pair is a CONFLICT, without it fuses"""
    P, A, twin = _scene(40, 12, seed)
    rng = np.random.default_rng(seed)
    f0 = _rows(A, rng, np.arange(len(A)))
    f1 = _rows(A, rng, np.arange(40, 52))
    return _case(P, A, frames=[f0, f1], veto=veto)


CASES = {
    "dyadic": lambda: _dyadic(1),
    "dyadic_keep": lambda: _dyadic(0),
    "grid": lambda: _case(*_scene(2000, 400, 41, box=(1.0, 1.0, 1.0), push=0.04, where="shuffled")[:2], radius_xyz=0.075),      # ~13 cells of 0.077 per axis
    "classes": lambda: _case(*_scene(1000, 300, 42, classes=50, where="shuffled")[:2], position=0),
    "one_point": lambda: _case(np.full((300, 3), 1.5, np.float32), _scene(240, 60, 43)[1]),      # all points identical: one cell holds everything
    "flat": lambda: _case(_scene(400, 80, 44)[0] * np.float32([1, 1, 0]) + np.float32([0, 0, 2.5]), _scene(400, 80, 44)[1]),      # zero extent on z
    "clamped": lambda: _case(*_scene(500, 100, 45, box=(1000.0, 1000.0, 10.0), push=0.006)[:2], radius_xyz=0.01),      # extent / R ~ 10^5 >> the cell clamp
    "size_0": lambda: _sized(0, 50), "size_1": lambda: _sized(1, 51), "size_255": lambda: _sized(255, 52), "size_256": lambda: _sized(256, 53),
    "size_257": lambda: _sized(257, 54), "size_513": lambda: _sized(513, 55),
    "special": _special,
    "frames": lambda: _frames_case(61, veto=1, n_rows_given=True),
    "frames_no_veto": lambda: _frames_case(61, veto=0, n_rows_given=True, position=0),
    "frames_no_count": lambda: _frames_case(62, veto=1, n_rows_given=False),
    "frames_dry_run": lambda: _frames_case(61, veto=1, n_rows_given=True, dry_run=1),
    "together": lambda: _together(veto=1),
    "together_no_veto": lambda: _together(veto=0),
    "nothing": lambda: _case(*_scene(120, 0, 63)[:2], frames=[_scene(120, 0, 63)[1][:50]]),      # NOTHING_FUSED, with rows that hit
    "dry_run": lambda: _case(*_scene(300, 50, 64, where="shuffled")[:2], dry_run=1),
    "bound_above_size": lambda: dict(_case(*_scene(300, 50, 65, where="shuffled")[:2]), dup_rows=37),
    "zero_rows": lambda: _case(*_scene(60, 10, 66)[:2], frames=[np.zeros((0, 10), np.float32)] * 2),      # frames given, n_max == 0
}
DYADIC = ("dyadic", "dyadic_keep")


@functools.lru_cache(maxsize=None)
def _cached(name):
    return CASES[name]()


def case(name):
    return dict(_cached(name))


def run(c, fault=None, **kw):
    c = dict(c, **kw)
    return Fr.run(c["map_pts"], c["map_app"], c["frames"], c["n_rows"], c["n_max"], c["radius_xyz"], c["radius"], c["position"], c["veto"],
                  c["dry_run"], fault=fault)


@functools.lru_cache(maxsize=None)
def reference(name, fault=None):
    return run(case(name), fault=fault)


def margins(c):
    return Fr.margins(c["map_pts"], c["map_app"], c["radius_xyz"], c["radius"])


def cells(c, nc_max=128):
    """the device's grid restated in float32 (map_fuse.hip, fuse_grid_kernel): the cell of every finite entry per axis, (M, 3), -1
    where the entry is not finite.  For COUNTING what the cases cover; no reference uses it."""
    P, fin = c["map_pts"], Fr.finite(c["map_pts"], c["map_app"])
    out = np.full((len(P), 3), -1, np.int64)
    if not fin.any():
        return out
    R_ = np.float32(c["radius_xyz"]) * np.float32(1.001)
    lim = 2
    while lim < nc_max and lim ** 3 < len(P):
        lim += 1
    for k in range(3):
        lo, hi = P[fin, k].min(), P[fin, k].max()
        span = np.float32(hi - lo)
        if span > 0 and np.isfinite(span) and np.isfinite(R_):
            q = np.float32(span / R_)
            nc = max(1, lim if q >= lim else int(q))
            out[fin, k] = np.clip((P[fin, k] - lo) * np.float32(np.float32(nc) / span), 0, nc - 1).astype(np.int64)
        else:
            out[fin, k] = 0
    return out


# ---- the experiment: the example world with repeated appearance and planted duplicates ----
@functools.lru_cache(maxsize=None)
def experiment():
    """world.dat's 1000 landmarks, their appearances folded into 50 classes of 20 near-copies (tests/test_map_guided_cpu.py's
    construction, default_rng(2)), and 300 of them entered a second time (default_rng(5)): positions pushed by U(-0.015, 0.015),
    then appearances by N(0, 0.005).  Returns (pts, app, ch): entry 1000 + j is the copy of entry ch[j]."""
    E = R.example_problem()
    rng = np.random.default_rng(2)
    W = (rng.uniform(-1, 1, (50, 10))[np.arange(1000) % 50] + rng.normal(0, 0.002, (1000, 10))).astype(np.float32)
    assert len(E["world_pts"]) == 1000
    rng = np.random.default_rng(5)
    ch = np.sort(rng.permutation(1000)[:300])
    dp = (E["world_pts"][ch] + rng.uniform(-0.015, 0.015, (300, 3))).astype(np.float32)
    da = (W[ch] + rng.normal(0, 0.005, (300, 10))).astype(np.float32)
    return np.concatenate([np.asarray(E["world_pts"], np.float32), dp]), np.concatenate([W, da]), ch


def pairs_of(r):
    """the fused pairs (survivor, absorbed) of a result"""
    s = np.nonzero(np.asarray(r["verdict"]) == Fr.SURVIVOR)[0]
    return {(int(a), int(r["partner"][a])) for a in s}
