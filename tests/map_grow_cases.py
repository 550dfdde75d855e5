"""The cases shared by tests/test_map_grow_cpu.py (which asserts that the restatement takes no marginal decision on them and
re-measures profiles/map_grow_budget.json) and tests/test_gpu_map_grow.py (which runs them on the device).

A case is a dict: K (3, 3), map_pts (M, 3) float32, map_app (M, 10) (the map BEFORE the call: what is left of the scene's
landmarks), frames [(uv, app)], poses [4x4], n_rows (or None), params (the keywords of Map.grow), truth / truth_app (the
scene's landmarks, to measure the added points against).  The scenes come from tests/map_refine_cases.py (hand, sequence_case)
and the example data."""
import numpy as np

import map_cull_cases as Cc
import map_grow_restatement as G
import map_refine_cases as Rc
import map_refine_restatement as R

REMOVE_SEED, N_REMOVED = 4, 60
OBS = [2, 15, 16, 17, 31, 32, 33, 64, 65]                    # observations per track around the 16 lanes and the 16 x 16 tiles
LISTS = [1, 2, 15, 16, 17, 31, 32, 33, 64, 64, 65, 66]        # what the scene 'lists' has, the row seen once included
TRACKS = (1, 15, 16, 17, 255, 256, 257)                      # tracks around the 16 per workgroup and the 256 per block of the ranks


def _params(**kw):
    return dict(G.DEFAULT, **kw)


def _keep(c, keep, params):
    """the scene with only the landmarks `keep` (indices) left in the map, ON their truth"""
    keep = np.asarray(keep, int)
    truth = np.asarray(c["truth"], np.float32)
    return dict(c, map_pts=truth[keep].copy(), map_app=np.asarray(c["map_app"], np.float32)[keep].copy(), truth=truth,
                truth_app=np.asarray(c["map_app"], np.float32), params=_params(**params))


# ---- the example data ----
def example(keep=None, **params):
    P = R.example_problem()
    pts = np.asarray(P["world_pts"], np.float32)
    c = dict(K=P["K"], map_app=P["world_app"], frames=P["frames"], poses=P["poses"], n_rows=None, truth=pts)
    return _keep(c, np.arange(len(pts)) if keep is None else keep, params)


def example_removed(**params):
    """N_REMOVED seeded well-seen entries taken out of world.dat"""
    P = R.example_problem()
    who = np.sort(np.random.default_rng(REMOVE_SEED).choice(Cc.well_seen(P), N_REMOVED, replace=False))
    c = example(np.setdiff1d(np.arange(len(P["world_pts"])), who), **params)
    c["removed"] = who
    return c


def example_after_cull(**params):
    """world.dat after the cull of its 40 pushed landmarks (map_cull_cases: example_pushed): the map the cull leaves"""
    r, cc = Cc.reference("example_pushed"), Cc.case("example_pushed")
    c = example(np.nonzero(r["keep"])[0], **params)
    assert c["map_pts"].tobytes() == r["points"].tobytes() and c["map_app"].tobytes() == r["app"].tobytes()
    c["removed"] = cc["pushed"]
    return c


# ---- a noisy synthetic sequence ----
def sequence_noisy():
    c = Rc.sequence_case(0.5, {}, seed=3001)
    n = len(c["truth"])
    return _keep(c, np.arange(0, n, 3), dict(n_rounds=5, min_obs=3, min_frames=3, max_rms_px=3.0, min_parallax_deg=1.0))


# ---- hand-made scenes ----
def lists_case():
    """tracks of 2 ... 66 observations; the last two landmarks stay in the map (rows that hit); hand()'s extras: two rows of one
    frame in a track, garbage behind the live rows, an empty frame, -0 against +0, a NaN appearance row, a row seen once"""
    counts = OBS[:-1] + [65, 66, 67]                          # (the extras add a row here and empty a frame there: the lists come out as LISTS)
    c = Rc.hand(counts + [9, 12], 67, 54, extras=True, noise_px=0.3)
    return _keep(c, [len(counts), len(counts) + 1], dict(min_obs=2, min_frames=2, max_rms_px=2.0, min_parallax_deg=0.5))


def n_tracks_case(n, seed=60, **kw):
    c = Rc.hand([4] * n, 6, seed + n, noise_px=0.3)
    return _keep(c, [], dict(dict(min_obs=3, min_frames=3, max_rms_px=2.0, min_parallax_deg=1.0), **kw))


def n_frames_case(F, seed=70):
    """F frames, every landmark in min(F, 5) of them; with one frame every track is FEW_FRAMES"""
    k = min(F, 5)
    c = Rc.hand([k] * 6 + [min(F, 40)], F, seed + F, noise_px=0.3)
    return _keep(c, [5], dict(min_obs=2, min_frames=2, max_rms_px=2.0, min_parallax_deg=0.2 if F > 2 else 0.0))


def room_case(delta):
    """11 tracks qualify; max_added = 11 + delta (delta 'far' = 1000): NO_ROOM on exactly the last tracks"""
    c = n_tracks_case(11, seed=80)
    c["params"] = dict(c["params"], max_added=1011 if delta == "far" else 11 + delta)
    return c


def grows_past_capacity():
    """1100 tracks into a map of 3 entries: more than a fresh map's 1024 entries"""
    c = Rc.hand([3] * 1103, 6, 90, noise_px=0.3)
    return _keep(c, [0, 1, 2], dict(min_obs=3, min_frames=3, max_rms_px=2.0, min_parallax_deg=1.0))


def verdicts_case():
    """0 behind a camera, 1 one mismatched row (HIGH_ERROR), 2 rays parallel to 0.02 degrees (LOW_PARALLAX), 3 seen twice in ONE
    frame (FEW_FRAMES), 4 seen once (FEW_OBS), 5 a NaN pixel (DEGENERATE: a sum is not finite), 6 ... 8 fine"""
    c = Rc.hand([6, 6, 6, 1, 1, 6, 6, 5, 4], 6, 95)
    c["frames"] = [(uv.copy(), a.copy()) for uv, a in c["frames"]]
    c["poses"] = list(c["poses"])
    app, truth = c["map_app"], np.asarray(c["truth"], np.float32)
    # 0: one more camera that looks the other way
    flip = np.diag([-1.0, 1.0, -1.0, 1.0]) @ c["poses"][0].astype(np.float64)
    pc = flip[:3, :3] @ truth[0].astype(np.float64) + flip[:3, 3]
    assert pc[2] < -1
    q = Rc.K_HAND.astype(np.float64) @ pc
    c["poses"].append(flip.astype(np.float32))
    c["frames"].append(((q[:2] / q[2]).astype(np.float32).reshape(1, 2), app[0:1].copy()))
    # 1: one row 40 px off
    f, i = Cc._rows_of(c, 1)[2]
    c["frames"][f][0][i] += np.float32(40.0)
    # 2: seen from frame 0 and from a twin of it 2 mm to the side: two frames, rays parallel to 0.02 degrees -- a tiny POSITIVE
    # pivot and a point that the parallax test refuses
    rows = Cc._rows_of(c, 2)
    for f, i in rows[1:]:
        c["frames"][f] = (np.delete(c["frames"][f][0], i, 0), np.delete(c["frames"][f][1], i, 0))
    twin = c["poses"][rows[0][0]].astype(np.float64).copy()
    twin[0, 3] += 0.002
    pc = twin[:3, :3] @ truth[2].astype(np.float64) + twin[:3, 3]
    q = Rc.K_HAND.astype(np.float64) @ pc
    c["poses"].append(twin.astype(np.float32))
    c["frames"].append(((q[:2] / q[2]).astype(np.float32).reshape(1, 2), app[2:3].copy()))
    # 3: a second row in its one frame
    (f, i), = Cc._rows_of(c, 3)
    uv, a = c["frames"][f]
    c["frames"][f] = (np.concatenate([uv, uv[i: i + 1] + np.float32(0.125)]), np.concatenate([a, a[i: i + 1]]))
    # 5: a NaN pixel
    f, i = Cc._rows_of(c, 5)[0]
    c["frames"][f][0][i, 0] = np.nan
    return _keep(c, [], dict(min_obs=2, min_frames=2, max_rms_px=2.0, min_parallax_deg=1.0))


def nothing_added():
    """open rows there are, but every track is seen once"""
    c = Rc.hand([1, 1, 1, 4], 4, 97)
    return _keep(c, [3], dict(min_obs=2, min_frames=2))


def no_open_rows():
    c = Rc.hand([4, 3, 5], 5, 98)
    return _keep(c, [0, 1, 2], {})


CASES = {
    "example_from_empty": lambda: example([], n_rounds=0),
    "example_from_empty_two_views": lambda: example([], n_rounds=0, min_obs=2, min_frames=2, min_parallax_deg=0.0),
    "example_removed": lambda: example_removed(n_rounds=0),
    "example_after_cull": lambda: example_after_cull(n_rounds=0),
    "example_refined": lambda: example_removed(n_rounds=2, huber_px=1.0, damping=1e-3),
    "sequence_noisy": sequence_noisy,
    "lists": lists_case,
    "verdicts": verdicts_case,
    "room_equal": lambda: room_case(0),
    "room_one_below": lambda: room_case(-1),
    "room_far_above": lambda: room_case("far"),
    "dry_run": lambda: dict(room_case(-1), params=dict(room_case(-1)["params"], dry_run=True)),
    "grows_past_capacity": grows_past_capacity,
    "nothing_added": nothing_added,
    "no_open_rows": no_open_rows,
    "damped_round": lambda: n_tracks_case(17, seed=61, n_rounds=1, damping=1e5),      # ONE heavily damped round: half of the start's error stays
    "frames_1": lambda: n_frames_case(1),
    "frames_2": lambda: n_frames_case(2),
    "frames_512": lambda: n_frames_case(512),
    "frames_513": lambda: n_frames_case(513),
}
CASES.update({f"tracks_{n}": (lambda n=n: n_tracks_case(n)) for n in TRACKS})

_cache, _ref = {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def run(c, **kw):
    return G.grow(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], n_rows=c["n_rows"], **dict(c["params"], **kw))


def reference(name, reverse=False):
    """the restatement on a case, computed once and shared"""
    key = (name, reverse)
    if key not in _ref:
        _ref[key] = run(case(name), reverse=reverse)
    return _ref[key]


def scored(r):
    """the tracks whose point and statistics mean something"""
    return np.isin(r["verdict"], (G.ADDED, G.BEHIND, G.HIGH_ERROR, G.LOW_PARALLAX, G.NO_ROOM))


def spreads(name):
    """what the budget file records for a case: the distance between the forward and the reversed order of summation of the
    DOUBLE point (relative to its largest coordinate) and of mean_sq_px (relative)"""
    a, r = reference(name), reference(name, reverse=True)
    ok = scored(a) & scored(r)
    rel = lambda p, q: float(np.max(np.abs(p[ok] - q[ok]) / np.maximum(np.abs(p[ok]), 1e-300), initial=0.0))
    pt = float(np.max(np.abs(a["p64"][ok] - r["p64"][ok]).max(1) / np.maximum(np.abs(a["p64"][ok]).max(1), 1e-300), initial=0.0))
    return dict(point_order_rel=pt, mean_order_rel=rel(a["mean_sq_px"], r["mean_sq_px"]))


def ceilings(name, budget):
    """per track (point, mean, max, z, cos): 4 x the case's recorded spread (on the quantity's own size) + twice the restatement's
    a-priori rounding bound.  The point's ceiling is that of the DOUBLE point; it lies far below half a float32 ulp wherever the
    case is not marginal, so two implementations within it store the same float32."""
    a = reference(name)
    return (4 * budget["point_order_rel"] * np.abs(a["p64"]).max(1) + 2 * a["b_point"], 4 * budget["mean_order_rel"] * np.abs(a["mean_sq_px"]) + 2 * a["b_mean"],
            2 * a["b_max"], 2 * a["b_z"], 2 * a["b_cos"])


# ---- many tracks whose answer is known by construction ----
def many_tracks(n=65537, seed=7):
    """n landmarks in front of three cameras on a line; every landmark is seen by all three, every second one by the first alone
    (FEW_OBS).  Returns (case, expected verdict per track, the landmark of every track).  Track t is landmark t: frame 0 lists
    them in order."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(4, 7, n)], 1)
    app = rng.uniform(-1, 1, (n, 10)).astype(np.float32)
    app[:, 0] = np.arange(n, dtype=np.float32)                # distinct by construction
    K = Rc.K_HAND.astype(np.float64)
    poses, frames = [], []
    full = np.arange(n) % 2 == 0
    for f, x in enumerate((-1.0, 0.0, 1.0)):
        T = np.eye(4, dtype=np.float32); T[0, 3] = -x
        ids = np.arange(n) if f == 0 else rng.permutation(np.nonzero(full)[0])
        q = (pts[ids] + T[:3, 3].astype(np.float64)) @ K.T
        poses.append(T); frames.append(((q[:, :2] / q[:, 2:3]).astype(np.float32), app[ids].copy()))
    c = dict(K=Rc.K_HAND.copy(), map_pts=np.zeros((0, 3), np.float32), map_app=np.zeros((0, 10), np.float32), frames=frames, poses=poses, n_rows=None,
             truth=pts.astype(np.float32), truth_app=app, params=_params(n_rounds=0, min_obs=3, min_frames=3, max_rms_px=1.0, min_parallax_deg=1.0))
    return c, np.where(full, G.ADDED, G.FEW_OBS).astype(np.int32), np.arange(n)
