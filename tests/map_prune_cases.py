"""The cases shared by tests/test_map_prune_cpu.py (which asserts that the restatement takes no marginal decision on them and
that every planted fault shows) and tests/test_gpu_map_prune.py (which runs them on the device): the smallest shapes at which
the kernels of map_prune.hip can go wrong.

A case is a dict: K (3, 3), map_pts (M, 3) float32, map_app (M, 10), frames [(uv, app)], poses [4x4], n_rows (or None), n_max,
params (the keywords of the restatement's prune()), and what was planted where a test asks for it.

The hand-made scenes come from scene(): a list of (landmark, frame, dx, dy) -- one row per item, in the order the rows take
their places in their frames --, cameras on a path along x that look along +z, pixels = the float64 projection plus a uniform
noise of +-0.1 px (so that no two |e|^2 of a landmark come close, let alone to 0) plus (dx, dy).  With max_err_px = 1 a row
moved by 3 px is HIGH_ERROR and one moved by 0.8 px is RELATIVE against a median near 0.01 px^2 and a floor of 0.5 px."""
import numpy as np

import map_cull_cases as Cc
import map_prune_restatement as Q
import map_refine_restatement as R

K_HAND = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]], np.float32)
N_MAX = 12
LISTS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 48]             # observations per landmark around the 16 lanes and the 16 x 16 tiles
BAD, REL = 3.0, 0.8                                          # pixels: HIGH_ERROR at max_err_px 1, RELATIVE under it
EXAMPLE_SEEDS = dict(wrong=1, pushed=2, n_wrong=100, n_pushed=20, frames=(30, 60, 90), min_obs=5)


def _params(**kw):
    return dict(Q.DEFAULT, **kw)


def pose(f):
    a = 0.002 * f
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = [-0.03 * f, 0.0, 0.0]
    return T.astype(np.float32)


def project(K, T, p):
    pc = T[:3, :3].astype(np.float64) @ np.asarray(p, np.float64) + T[:3, 3].astype(np.float64)
    q = np.asarray(K, np.float64) @ pc
    return q[:2] / q[2]


def scene(obs, n_frames, n_landmarks, seed, params, n_max=N_MAX, noise_px=0.1):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-1, 1, n_landmarks), rng.uniform(-1, 1, n_landmarks), rng.uniform(4, 7, n_landmarks)], 1).astype(np.float32)
    app = rng.uniform(-1, 1, (n_landmarks, 10)).astype(np.float32)
    assert len(set(r.tobytes() for r in app)) == n_landmarks
    poses = [pose(f) for f in range(n_frames)]
    rows = [([], []) for _ in range(n_frames)]
    where = []
    for l, f, dx, dy in obs:
        uv = project(K_HAND, poses[f], pts[l]) + rng.uniform(-noise_px, noise_px, 2) + (dx, dy)
        where.append((f, len(rows[f][0])))
        rows[f][0].append(uv.astype(np.float32)); rows[f][1].append(app[l].copy())
    frames = [(np.array(u, np.float32).reshape(-1, 2), np.array(a, np.float32).reshape(-1, 10)) for u, a in rows]
    assert max(len(a) for _, a in frames) <= n_max
    return dict(K=K_HAND.copy(), map_pts=pts, map_app=app, frames=frames, poses=poses, n_rows=None, n_max=n_max, params=_params(**params),
                where=where)


# ---- list lengths ----
def _list_obs():
    """landmark k seen LISTS[k] times, one row per frame from frame 5 k on (mod 64); from 3 observations on the third is moved by
    3 px and the second by 0.8 px"""
    obs = []
    for k, n in enumerate(LISTS):
        for j in range(n):
            d = (BAD, 0.0) if (n >= 3 and j == 2) else (0.0, REL) if (n >= 3 and j == 1) else (0.0, 0.0)
            obs.append((k, (5 * k + j) % 64, d[0], d[1]))
    return obs


def lists_case(**kw):
    return scene(_list_obs(), 64, len(LISTS), 11, dict(dict(max_err_px=1.0, rel_factor=3.0, rel_floor_px=0.5, rel_min_obs=3), **kw))


# ---- duplicate runs ----
def duplicates_case(**kw):
    """landmark 0: 20 observations, the rows of list positions 14, 15 and 16 in ONE frame (a run of three across the 16th lane);
    landmark 1: 4 observations, two of them in one frame with bit-equal pixels (an exact tie: the lower key stays); landmark 2: 5
    observations, a pair in one frame (the short list: the row goes round); landmark 3: three rows in one frame, the one with the
    smallest error has a NaN pixel (NOT_FINITE, so the second best stays), plus 17 single rows; landmark 4: two rows in a frame
    that looks away -- camera z is the frame's, so a run is BEHIND as a whole and nobody in it is DUPLICATE."""
    obs = [(0, f, 0, 0) for f in range(14)] + [(0, 14, 0.8, 0), (0, 14, 0.3, 0), (0, 14, 0.55, 0)] + [(0, f, 0, 0) for f in (15, 16, 17)]
    obs += [(1, 20, 0, 0), (1, 21, 0.4, 0), (1, 21, 0.4, 0), (1, 22, 0, 0)]
    obs += [(2, 30, 0, 0), (2, 31, 0.7, 0), (2, 31, 0.3, 0), (2, 32, 0, 0), (2, 33, 0, 0)]
    obs += [(3, 40, 0.0, 0), (3, 40, 0.8, 0), (3, 40, 0.3, 0)] + [(3, f, 0, 0) for f in range(41, 58)]
    obs += [(4, 60, 0, 0), (4, 61, 0, 0), (4, 62, 0, 0), (4, 63, 0.2, 0), (4, 63, 0.7, 0)]
    c = scene(obs, 64, 5, 12, dict(dict(max_err_px=1.0, unique=1), **kw))
    c["frames"] = [(uv.copy(), a.copy()) for uv, a in c["frames"]]
    c["frames"][21][0][1] = c["frames"][21][0][0]            # bit-equal pixels
    c["frames"][40][0][0, 1] = np.nan
    c["poses"][63] = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ c["poses"][63].astype(np.float64)).astype(np.float32)
    return c


# ---- the guards at equality ----
def guards_case(**kw):
    """max_err_px 1, both guards at 500 per mille.  Landmarks: 0 has 1 soft of 2 and 1 has 2 of 4 (at the share: NOT at fault,
    the rows go), 2 has 3 of 4 and 3 and 16 have 2 of 2 (at fault, the rows stay).  4 .. 9 are clean filler of frames 0 .. 4 and
    9; 10 .. 15, 17 and 18 are clean in frames 0 .. 3 (and 9) and carry the soft rows of the frames under test: frame 6 has 1
    soft of 2 and frame 7 has 2 of 4 (not at fault), frame 8 has 3 of 4 (at fault).  Frame 5 holds the soft rows of landmarks 3
    and 16, one soft row of landmark 17 and a clean one: after rule 7 it has 1 soft of 4 and is not named; a frame guard run
    FIRST would see 3 of 4."""
    S = (BAD, 0.0)
    obs = [(0, 0) + S, (0, 1, 0, 0)]
    obs += [(1, 0, 0, 0), (1, 1, 0, 0), (1, 2) + S, (1, 3) + S]
    obs += [(2, 0, 0, 0), (2, 1) + S, (2, 2) + S, (2, 3) + S]
    obs += [(3, 4) + S, (3, 5) + S, (16, 4) + S, (16, 5) + S]
    obs += [(l, f, 0, 0) for l in range(4, 10) for f in (0, 1, 2, 3, 4, 9)]
    obs += [(l, f, 0, 0) for l in list(range(10, 16)) + [17, 18] for f in (0, 1, 2, 3)] + [(l, 9, 0, 0) for l in range(10, 16)]
    obs += [(10, 6) + S, (11, 6, 0, 0)]
    obs += [(11, 7) + S, (12, 7) + S, (13, 7, 0, 0), (14, 7, 0, 0)]
    obs += [(13, 8) + S, (14, 8) + S, (15, 8) + S, (10, 8, 0, 0)]
    obs += [(17, 5) + S, (18, 5, 0, 0)]
    return scene(obs, 10, 19, 13, dict(dict(max_err_px=1.0, max_share_landmark=500, max_share_frame=500), **kw), n_max=20)


# ---- corner rows ----
def corners_case():
    """landmark 0: a NaN pixel among 6 rows (NOT_FINITE); landmark 1: an infinite point (every row NOT_FINITE); landmark 2: frame 7
    has the identity rotation and t_z = -p_z, so camera z is 0 exactly in any order of evaluation and |e|^2 is not finite
    (NOT_FINITE goes before BEHIND); landmark 3: a row in a frame that looks away (BEHIND); landmark 4: clean, and one of its rows
    carries a NaN appearance (MISS); a row of no map (MISS)."""
    obs = [(l, f, 0, 0) for l in range(5) for f in range(6)] + [(2, 7, 0, 0), (3, 8, 0, 0)]
    c = scene(obs, 9, 5, 14, dict(max_err_px=1.0, rel_factor=3.0, rel_floor_px=0.5))
    c["frames"] = [(uv.copy(), a.copy()) for uv, a in c["frames"]]
    c["frames"][2][0][0, 0] = np.nan
    c["map_pts"][1, 2] = np.inf
    T = np.eye(4, dtype=np.float32); T[2, 3] = -c["map_pts"][2, 2]
    c["poses"][7] = T
    c["frames"][7][0][0] = (320.0, 240.0)
    c["poses"][8] = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ c["poses"][8].astype(np.float64)).astype(np.float32)
    c["frames"][3][1][4, 5] = np.nan
    uv, a = c["frames"][4]
    c["frames"][4] = (np.concatenate([uv, [[100.0, 100.0]]]).astype(np.float32), np.concatenate([a, np.full((1, 10), 0.5, np.float32)]))
    return c


# ---- the frames' layout ----
def layout_case(counts=True):
    """lists_case() with row counts: frame 6 has n_rows = 0, frame 11 loses its last row, frame 12 counts more rows than n_max;
    counts=False: the same observations with d_n_rows NULL (the frames cut to their live rows)"""
    c = lists_case(rel_min_obs=17)
    n = np.array([len(a) for _, a in c["frames"]], np.int32)
    n[6] = 0; n[11] -= 1; n[12] = N_MAX + 5
    if counts:
        return dict(c, n_rows=n)
    live = np.minimum(n, [len(a) for _, a in c["frames"]])
    return dict(c, frames=[(uv[:k], a[:k]) for (uv, a), k in zip(c["frames"], live)])


# ---- the launch's stride ----
def stride_case(size=20000):
    """one frame of `size` rows against `size` entries: more than 4 n_cu 16 landmarks, so the striding loop of the landmark
    kernel turns; every 97th row is moved by 3 px.  One camera at the origin."""
    rng = np.random.default_rng(15)
    pts = np.stack([rng.uniform(-1, 1, size), rng.uniform(-1, 1, size), rng.uniform(4, 7, size)], 1).astype(np.float32)
    app = rng.uniform(-1, 1, (size, 10)).astype(np.float32)
    ids = rng.permutation(size)
    q = pts[ids].astype(np.float64) @ K_HAND.astype(np.float64).T
    uv = q[:, :2] / q[:, 2:3] + rng.uniform(-0.1, 0.1, (size, 2))
    planted = np.arange(0, size, 97)
    uv[planted, 0] += BAD
    return dict(K=K_HAND.copy(), map_pts=pts, map_app=app, frames=[(uv.astype(np.float32), app[ids].copy())], poses=[np.eye(4, dtype=np.float32)],
                n_rows=None, n_max=size, params=_params(max_err_px=1.0), planted=planted)


# ---- the example data with the three kinds of fault ----
def example_case(**kw):
    """The example data on its ground truth, then three kinds of fault.  n_pushed landmarks with >= min_obs observations, each at
    least 1 in front of every camera that sees it (a push of up to 0.4 per coordinate must not put an innocent row BEHIND), moved
    by +-0.2 .. 0.4 per coordinate (seed `pushed`, the draw of tests/map_cull_cases.py).  The poses of `frames` moved by 0.05 in
    t.  n_wrong rows of landmarks with >= min_obs observations, outside the pushed frames, given the appearance of a random OTHER
    such landmark that is not pushed (seed `wrong`): the hard tests need no context, so a wrong row that lands BEHIND is pruned
    also on a named landmark or in a named frame, and the draw keeps the two apart.  planted: (frame, row) of the wrong rows."""
    S = EXAMPLE_SEEDS
    P = R.example_problem()
    pts = np.asarray(P["world_pts"], np.float32)
    app = np.asarray(P["world_app"], np.float32)
    lists, n_max, _ = R.observation_lists(app, P["frames"])
    well = np.array(sorted(e for e, v in lists.items() if len(v) >= S["min_obs"]))
    poses = [np.asarray(X, np.float64).copy() for X in P["poses"]]
    z_min = {e: min(float(poses[k // n_max][2, :3] @ pts[e].astype(np.float64) + poses[k // n_max][2, 3]) for k in lists[e]) for e in well}
    pushed, moved = Cc.pushed_landmarks(pts, np.array([e for e in well if z_min[e] > 1.0]), seed=S["pushed"], n=S["n_pushed"])
    for f in S["frames"]:
        poses[f][:3, 3] += 0.05
    rng = np.random.default_rng(S["wrong"])
    keys = np.array(sorted(k for e in well for k in lists[e] if k // n_max not in S["frames"]))
    chosen = np.sort(rng.choice(keys, S["n_wrong"], replace=False))
    owner = {k: e for e in well for k in lists[e]}
    targets = np.array([e for e in well if e not in set(int(x) for x in pushed)])
    frames = [(np.asarray(uv, np.float32).copy(), np.asarray(a, np.float32).copy()) for uv, a in P["frames"]]
    planted = []
    for k in chosen:
        f, i = int(k) // n_max, int(k) % n_max
        other = int(rng.choice(targets[targets != owner[int(k)]]))
        frames[f][1][i] = app[other]
        planted.append((f, i))
    params = _params(**dict(dict(max_err_px=1.0, rel_factor=5.0, rel_floor_px=0.5, rel_min_obs=5, max_share_landmark=500, max_share_frame=300), **kw))
    return dict(K=P["K"], map_pts=moved, map_app=app, frames=frames, poses=[X.astype(np.float32) for X in poses], n_rows=None, n_max=n_max,
                params=params, planted=planted, pushed=pushed, pushed_frames=list(S["frames"]), truth=pts)


CASES = {
    "lists": lists_case,
    "lists_rel_min_17": lambda: lists_case(rel_min_obs=17),          # n_el 17 is evaluated (at n_el), 16 is not (n_el + 1)
    "lists_guarded": lambda: lists_case(max_share_landmark=300, max_share_frame=500),
    "lists_all_off": lambda: lists_case(max_err_px=0.0, rel_factor=0.0, unique=0),
    "duplicates": duplicates_case,
    "duplicates_not_unique": lambda: duplicates_case(unique=0),
    "duplicates_relative": lambda: duplicates_case(rel_factor=3.0, rel_floor_px=0.25),
    "guards": guards_case,
    "guards_share_0": lambda: guards_case(max_share_landmark=0, max_share_frame=0),
    "guards_frame_0": lambda: guards_case(max_share_landmark=1000, max_share_frame=0),
    "guards_off": lambda: guards_case(max_share_landmark=1000, max_share_frame=1000),
    "corners": corners_case,
    "layout": layout_case,
    "layout_no_row_counts": lambda: layout_case(False),
    "stride": stride_case,
    "example": example_case,
}
SMALL = [n for n in CASES if n not in ("stride", "example")]

_cache, _ref = {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def run(c, **kw):
    return Q.prune(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], n_rows=c["n_rows"], n_max=c["n_max"], **dict(c["params"], **kw))


def reference(name, **kw):
    """the restatement on a case, computed once and shared"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _ref:
        _ref[key] = run(case(name), **kw)
    return _ref[key]


def pruned_rows(res):
    return set(zip(*np.nonzero(Q.pruned(res["status"]))))
