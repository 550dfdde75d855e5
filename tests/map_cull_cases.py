"""The cases shared by tests/test_map_cull_cpu.py (which asserts that the restatement takes no marginal decision on them and
re-measures profiles/map_cull_budget.json) and tests/test_gpu_map_cull.py (which runs them on the device).

A case is a dict: K (3, 3), map_pts (M, 3) float32, map_app (M, 10), frames [(uv, app)], poses [4x4], n_rows (or None),
params (the keywords of Map.cull).  The scenes come from tests/map_refine_cases.py: hand(...) with the map put back ON its
truth, so that a clean landmark's error is the float32 rounding of its pixels and a pushed one stands out."""
import numpy as np

import map_cull_restatement as Q
import map_refine_cases as Rc
import map_refine_restatement as R

PUSH_SEED, N_PUSHED = 2, 40                                  # (seed 1 puts one pushed landmark behind a camera: BEHIND, dropped all the same)
LISTS = [0, 1, 2, 3, 15, 16, 17, 33, 257]                    # observations per landmark around the 16 lanes and the 16 x 16 tiles


def _params(**kw):
    return dict(Q.DEFAULT, **kw)


def _rows_of(case, landmark):
    """[(frame, row)] of the rows that carry the landmark's appearance"""
    key = case["map_app"][landmark].tobytes()
    return [(f, i) for f, (_, a) in enumerate(case["frames"]) for i in range(len(a)) if a[i].tobytes() == key]


def _remove_rows(case, landmark, frames):
    for f in frames:
        uv, a = case["frames"][f]
        keep = np.array([a[i].tobytes() != case["map_app"][landmark].tobytes() for i in range(len(a))], bool)
        case["frames"][f] = (uv[keep], a[keep])


def on_truth(c, params):
    return dict(c, map_pts=np.asarray(c["truth"], np.float32).copy(), params=_params(**params))


# ---- the example data ----
def well_seen(P):
    lists, _, _ = R.observation_lists(P["world_app"], P["frames"])
    return np.array(sorted(e for e, v in lists.items() if len(v) >= 3))


def pushed_landmarks(world_pts, candidates, seed=PUSH_SEED, n=N_PUSHED):
    """(the n landmarks pushed, the map with them moved by +-0.2 ... 0.4 per coordinate)"""
    rng = np.random.default_rng(seed)
    who = np.sort(rng.choice(candidates, n, replace=False))
    step = rng.uniform(0.2, 0.4, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    pts = np.asarray(world_pts, np.float32).copy()
    pts[who] = (pts[who].astype(np.float64) + step).astype(np.float32)
    return who, pts


def example(pushed=False, **params):
    P = R.example_problem()
    pts = np.asarray(P["world_pts"], np.float32)
    c = dict(K=P["K"], map_pts=pts, map_app=P["world_app"], frames=P["frames"], poses=P["poses"], n_rows=None, truth=pts,
             params=_params(**params))
    if pushed:
        c["pushed"], c["map_pts"] = pushed_landmarks(pts, well_seen(P))
    return c


# ---- hand-made scenes ----
def lists_case():
    """landmarks seen 0, 1, 2, 3, 15, 16, 17, 33 and 257 times; hand()'s extras: a landmark seen twice in one frame, an empty frame,
    garbage behind the live rows, -0 against +0, a NaN row and rows of no map.  Landmarks 3 and 6 are pushed."""
    c = on_truth(Rc.hand(LISTS, 257, 31, extras=True), dict(min_obs=2, min_frames=2, max_rms_px=1.0, max_err_px=3.0, min_parallax_deg=3.0))
    c["map_pts"][3] += np.float32(0.3)
    c["map_pts"][6, 0] -= np.float32(0.25)
    return c


def lists_no_row_counts():
    c = lists_case()
    c["frames"] = [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], c["n_rows"])]
    c["n_rows"] = None
    return c


def precedence():
    """every verdict decided by exactly one landmark (two for NOT_FINITE and UNSEEN, which have two causes):
    0 never seen (UNSEEN), 1 an appearance with a NaN (UNSEEN), 2 seen once (FEW_OBS), 3 seen twice in ONE frame (FEW_FRAMES),
    4 a NaN point, 5 a NaN pixel (NOT_FINITE), 6 one camera turned away (BEHIND), 7 pushed (HIGH_ERROR), 8 seen from two
    neighbouring frames alone (LOW_PARALLAX), 9 ... 11 fine (KEPT).  Landmarks 4 ... 6 are pushed as well, and 4, 5 and 7 are
    narrow too: the earlier verdict wins."""
    c = on_truth(Rc.hand([0, 6, 1, 1, 6, 6, 6, 6, 6, 6, 5, 4], 6, 37), dict(min_obs=2, min_frames=2, max_rms_px=1.0, min_parallax_deg=12.0))
    c["frames"] = [(uv.copy(), a.copy()) for uv, a in c["frames"]]
    app, pts = c["map_app"], c["map_pts"]
    app[1, 3] = np.nan                                       # its rows in the frames stay clean: they find nothing
    (f, i), = _rows_of(c, 3)
    uv, a = c["frames"][f]
    c["frames"][f] = (np.concatenate([uv, uv[i: i + 1] + np.float32(0.125)]), np.concatenate([a, a[i: i + 1]]))
    for j in (4, 5, 7):
        _remove_rows(c, j, [2, 3, 4, 5])
    _remove_rows(c, 8, [2, 3, 4, 5])
    pts[4:8] += np.float32(0.3)
    pts[4, 1] = np.nan
    f, i = _rows_of(c, 5)[0]
    c["frames"][f][0][i, 0] = np.nan
    flip = np.diag([-1.0, 1.0, -1.0, 1.0]) @ c["poses"][0].astype(np.float64)
    pc = flip[:3, :3] @ pts[6].astype(np.float64) + flip[:3, 3]
    assert pc[2] < -1
    q = Rc.K_HAND.astype(np.float64) @ pc
    c["poses"] = list(c["poses"]) + [flip.astype(np.float32)]
    c["frames"].append(((q[:2] / q[2]).astype(np.float32).reshape(1, 2), app[6:7].copy()))
    return c


def thresholds_off():
    """precedence() with every threshold 0 and min_obs = min_frames = 1: only NOT_FINITE and BEHIND drop"""
    return dict(precedence(), params=_params(min_obs=1, min_frames=1, max_rms_px=0.0))


def max_err_alone():
    """the single-error test alone: landmark 2 has ONE bad pixel among 12 (its mean stays small), landmark 0 is pushed"""
    c = on_truth(Rc.hand([12, 12, 12, 7], 12, 41), dict(min_obs=3, min_frames=2, max_rms_px=0.0, max_err_px=2.0))
    c["frames"] = [(uv.copy(), a.copy()) for uv, a in c["frames"]]
    f, i = _rows_of(c, 2)[5]
    c["frames"][f][0][i] += np.float32(4.0)
    c["map_pts"][0] += np.float32(0.3)
    return c


def drop_unseen_case():
    c = lists_case()
    return dict(c, params=dict(c["params"], drop_unseen=True))


def dry_run_case():
    c = lists_case()
    return dict(c, params=dict(c["params"], dry_run=True))


def nothing_dropped():
    """a clean scene: every landmark seen and fine, plus unseen ones that stay"""
    return on_truth(Rc.hand([5, 4, 3, 6, 0, 3], 6, 43, map_size=9), dict(min_obs=3, min_frames=2, max_rms_px=1.0, min_parallax_deg=2.0))


CASES = {
    "example_clean": lambda: example(min_obs=1, min_frames=1, max_rms_px=1.0),
    "example_pushed": lambda: example(pushed=True, min_obs=1, min_frames=1, max_rms_px=1.0),
    "example_parallax": lambda: example(min_obs=3, min_frames=2, max_rms_px=1.0, min_parallax_deg=5.0),
    "lists": lists_case,
    "lists_no_row_counts": lists_no_row_counts,
    "precedence": precedence,
    "thresholds_off": thresholds_off,
    "max_err_alone": max_err_alone,
    "drop_unseen": drop_unseen_case,
    "dry_run": dry_run_case,
    "nothing_dropped": nothing_dropped,
}

_cache, _ref = {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def run(c, **kw):
    return Q.cull(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], n_rows=c["n_rows"], **dict(c["params"], **kw))


def reference(name, reverse=False, alt=False):
    """the restatement on a case, computed once and shared"""
    key = (name, reverse, alt)
    if key not in _ref:
        _ref[key] = run(case(name), reverse=reverse, alt=alt)
    return _ref[key]


def spreads(name):
    """what the budget file records for a case: the relative distance of mean_sq_px between the forward and the reversed order of
    summation, and what another expression order moves: mean_sq_px and max_sq_px (relative), min_z and cos_parallax (absolute)"""
    a, r, x = reference(name), reference(name, reverse=True), reference(name, alt=True)
    ok = (a["n_obs"] > 0) & (a["verdict"] != Q.NOT_FINITE)
    rel = lambda p, q: float(np.max(np.abs(p[ok] - q[ok]) / np.maximum(np.abs(p[ok]), 1e-300), initial=0.0))
    dist = lambda p, q: float(np.max(np.abs(p[ok] - q[ok]), initial=0.0))
    return dict(mean_order_rel=rel(a["mean_sq_px"], r["mean_sq_px"]), mean_expr_rel=rel(a["mean_sq_px"], x["mean_sq_px"]),
                max_expr_rel=rel(a["max_sq_px"], x["max_sq_px"]), z_expr_abs=dist(a["min_z"], x["min_z"]),
                cos_expr_abs=dist(a["cos_parallax"], x["cos_parallax"]))


def ceilings(name, budget):
    """per entry (mean, max, z, cos): 4 x the case's recorded spread (on the statistic's own size where it is relative) + twice the
    restatement's a-priori rounding bound.  The expression spread of the mean is NOT added to the order spread: the bound covers it."""
    a = reference(name)
    return (4 * budget["mean_order_rel"] * np.abs(a["mean_sq_px"]) + 2 * a["b_mean"], 4 * budget["max_expr_rel"] * np.abs(a["max_sq_px"]) + 2 * a["b_max"],
            4 * budget["z_expr_abs"] + 2 * a["b_z"], 4 * budget["cos_expr_abs"] + 2 * a["b_cos"])


# ---- compaction: maps of any size whose survivors are known by construction ----
PATTERNS = ("first", "last", "every_second", "all", "none")


def compaction(size, pattern, seed=5):
    """a map of `size` landmarks in front of ONE camera at the origin; the frame holds the rows of the landmarks that stay, in a
    shuffled order, and the call drops the unseen: (case, keep mask).  Every threshold is off."""
    rng = np.random.default_rng(seed + size)
    pts = np.stack([rng.uniform(-1, 1, size), rng.uniform(-1, 1, size), rng.uniform(4, 7, size)], 1).astype(np.float32)
    app = rng.uniform(-1, 1, (size, 10)).astype(np.float32)
    assert len(set(r.tobytes() for r in app)) == size
    keep = np.ones(size, bool)
    if pattern == "first":
        keep[0] = False
    elif pattern == "last":
        keep[-1] = False
    elif pattern == "every_second":
        keep[1::2] = False
    elif pattern == "all":
        keep[:] = False
    ids = rng.permutation(np.nonzero(keep)[0])
    uv = rng.uniform(0, 600, (len(ids), 2)).astype(np.float32)
    c = dict(K=Rc.K_HAND.copy(), map_pts=pts, map_app=app, frames=[(uv, app[ids].copy())], poses=[np.eye(4, dtype=np.float32)], n_rows=None,
             params=_params(min_obs=1, min_frames=1, max_rms_px=0.0, drop_unseen=True))
    return c, keep
