"""The cases shared by tests/test_map_bundle_cpu.py (which asserts that the restatement takes no marginal decision on them and
re-measures the budget) and tests/test_gpu_map_bundle.py (which runs them on the device), built with `hand` of
tests/map_pose_refine_cases.py and `perturbed` of tests/map_refine_restatement.py: the example data and hand-made windows around
the kernels' edges (16 lanes per landmark, 256 threads per frame, 256 partial sums over the frames).

A case is a dict: K, map_pts (M, 3) float32 (the START, already pushed), map_app, frames [(uv, app)], poses [4x4 float32] (the
start), fixed (F,) bool or None, n_rows or None, params (the fields of vox_map_bundle_params)."""
import numpy as np

import map_bundle_restatement as B
import map_pose_refine_cases as Cs
import map_pose_refine_restatement as P
import map_refine_restatement as R

DEFAULT = dict(B.DEFAULT)
FRAME_HITS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025]
LANDMARK_SEEN_BY = [1, 2, 3, 15, 16, 17, 33]


def _case(c, params=None, points_push=None, fixed="keep"):
    out = dict(K=c["K"], map_pts=np.asarray(c["map_pts"], np.float32).copy(), map_app=c["map_app"], frames=c["frames"], poses=list(c["poses"]),
               fixed=c["fixed"] if fixed == "keep" else (None if fixed is None else np.asarray(fixed, bool)), n_rows=c["n_rows"],
               params=dict(DEFAULT, **(params or {})))
    if points_push:
        out["map_pts"] = R.perturbed(out["map_pts"], *points_push)
    return out


def sculpt(c, visible):
    """keeps of every frame the rows whose landmark e has visible[f, e] (and the rows that hit nothing)"""
    obs = P.frame_observations(c["map_app"], c["frames"])
    frames = []
    for f, ((uv, app), (i, e)) in enumerate(zip(c["frames"], obs)):
        keep = np.ones(len(app), bool)
        keep[i] = visible[f, e]
        frames.append((uv[keep], app[keep]))
    c["frames"] = frames
    return c


def frame_edges(extras):
    """every hit count at an edge of the frame's workgroup in one window, the largest frame held; with extras an empty frame, two
    rows of one landmark, garbage behind the live rows under n_rows"""
    hits = FRAME_HITS[:5] + [0] + FRAME_HITS[5:] if extras else FRAME_HITS
    F = len(hits)
    c = Cs.hand(hits, 51 if extras else 52, extras=extras, misses=0 if extras else 2, t_amount=0.01, a_amount=0.005, fixed=np.arange(F) == F - 1)
    if extras:
        c["frames"][5] = (np.zeros((0, 2), np.float32), np.zeros((0, 10), np.float32)); c["n_rows"][5] = 0
    c["poses"][F - 1] = P.to_f32_pose(c["truth"][F - 1])
    return _case(c, dict(n_rounds=2, n_cg=8, cg_tol=1e-12), points_push=(53, 0.01))


def landmark_edges():
    """33 frames of a map of 42 landmarks, six of them seen by each of 1, 2, 3, 15, 16, 17 and 33 frames: the edges of the group
    of 16 lanes; frame 0 held"""
    c = Cs.hand([42] * 33, 54, map_size=42, noise_px=0.2, misses=1, t_amount=0.01, a_amount=0.005, fixed=np.arange(33) == 0)
    rng = np.random.default_rng(55)
    vis = np.zeros((33, 42), bool)
    for e in range(42):
        vis[rng.choice(33, LANDMARK_SEEN_BY[e % 7], replace=False), e] = True
    c["poses"][0] = P.to_f32_pose(c["truth"][0])
    return _case(sculpt(c, vis), dict(n_rounds=2, n_cg=24, cg_tol=1e-12, min_obs_point=2), points_push=(56, 0.01))


def two_groups():
    """frames 0 .. 2 see landmarks 0 .. 31 only, frames 3 .. 5 landmarks 32 .. 63 only; the first frame of each group held"""
    c = Cs.hand([64] * 6, 57, map_size=64, noise_px=0.2, misses=1, t_amount=0.01, a_amount=0.005, fixed=[1, 0, 0, 1, 0, 0])
    vis = np.zeros((6, 64), bool)
    vis[:3, :32] = True; vis[3:, 32:] = True
    return _case(sculpt(c, vis), dict(n_rounds=2, n_cg=12, cg_tol=1e-6), points_push=(58, 0.01))


def frames_257():
    c = Cs.hand(list(np.random.default_rng(5).integers(3, 40, 257)), 59, noise_px=0.2, t_amount=0.01, a_amount=0.005, fixed=(np.arange(257) % 50 == 0))
    return _case(c, dict(n_rounds=2, n_cg=16, cg_tol=1e-6, min_obs_point=2), points_push=(60, 0.01))


def failures(kind):
    c = _case(Cs.hand_adjust(), dict(n_rounds=2, n_cg=12))
    obs = P.frame_observations(c["map_app"], c["frames"])
    if kind == "nan_pixel":
        c["frames"] = [(uv.copy(), a) for uv, a in c["frames"]]
        c["frames"][1][0][obs[1][0][0], 1] = np.nan
    elif kind == "nan_point":
        c["map_pts"][obs[2][1][3], 0] = np.nan
    else:                                                     # a camera turned away
        c["poses"][2] = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ c["poses"][2].astype(np.float64)).astype(np.float32)
    return c


def rejected_then_accepted():
    """lambda0 = 0.1 from 6 too far along the optical axis (cost_rose of tests/map_pose_refine_cases.py): the first round
    overshoots (its candidate costs 25 x the start) and is rejected, the second one, at ten times the damping, is accepted -- the
    CPU test asserts that pattern.  (From lambda0 = 0 the rejections only reach 1e-5 in three rounds: no round is accepted.)"""
    c = Cs.cost_rose()
    return _case(c, dict(n_rounds=3, n_cg=12, lambda0=0.1, min_obs_point=1000))


# On the example data PCG needs about 80 iterations for |r| / |r0| = 1e-10.  Cut off at 64 it is not converged, and conjugate
# gradients that are not converged amplify the order of the sums: the restatement's own forward and reversed runs then differ
# by 5e-7 relative in the candidate's cost.  So these two cases run 96 iterations with cg_tol = 0 -- PCG converges to its
# rounding floor, no stop is marginal, and the costs are a function of the problem to 1e-13.
CASES = {
    "example": lambda: _case(Cs.example_adjust(), dict(n_rounds=2, n_cg=96, cg_tol=0.0)),
    "example_large_push": lambda: _case(Cs.example_adjust(0.05, 0.02, 0.1), dict(n_rounds=3, n_cg=96, cg_tol=0.0)),
    "hand": lambda: _case(Cs.hand_adjust(), dict(n_rounds=3, n_cg=20)),
    "frame_edges": lambda: frame_edges(True),
    "frame_edges_no_row_counts": lambda: frame_edges(False),
    "landmark_edges": landmark_edges,
    "one_frame": lambda: _case(Cs.hand([65], 33, noise_px=0.2, t_amount=0.01, a_amount=0.005), dict(n_rounds=2, n_cg=6, min_obs_point=2)),
    "two_frames_one_held": lambda: _case(Cs.hand([40, 40], 61, map_size=40, noise_px=0.2, fixed=[1, 0], t_amount=0.01, a_amount=0.005),
                                         dict(n_rounds=2, n_cg=6, min_obs_point=2), points_push=(62, 0.01)),
    "frames_257": frames_257,
    "every_frame_held": lambda: _case(Cs.hand_adjust(), dict(n_rounds=2, n_cg=4), fixed=[1, 1, 1]),
    "poses_alone": lambda: _case(Cs.hand_adjust(), dict(n_rounds=2, n_cg=8, min_obs_point=1000)),
    "nothing_free": lambda: _case(Cs.hand_adjust(), dict(n_rounds=2, n_cg=4, min_obs_point=1000), fixed=[1, 1, 1]),
    "two_groups": two_groups,
    "nan_pixel": lambda: failures("nan_pixel"),
    "nan_point": lambda: failures("nan_point"),
    "camera_turned_away": lambda: failures("behind"),
    "rejected_then_accepted": rejected_then_accepted,
    # the first round of rejected_then_accepted alone: 1 PCG iteration, the candidate at 1.43e6 against 5.59e4, status NO_STEP.
    # The driver's other branches stay without a case: `nostep` (p.q not > 0 at the first iteration), `bad` (a pivot of D_f not > 0)
    # and status COST_ROSE are reached only by inputs on which the restatement's own decision is marginal (a rank-deficient D_f has
    # a pivot that is zero only up to rounding).
    "no_step": lambda: _case(Cs.cost_rose(), dict(n_rounds=1, n_cg=12, lambda0=0.1, min_obs_point=1000)),
    "one_cg_iteration": lambda: _case(Cs.hand_adjust(), dict(n_rounds=3, n_cg=1)),
    "zero_rounds": lambda: _case(Cs.hand_adjust(), dict(n_rounds=0)),
    "huber_noisy": lambda: _case(Cs.hand([65, 65, 65, 65], 63, map_size=65, noise_px=0.5, fixed=[1, 0, 0, 0], misses=1, t_amount=0.01, a_amount=0.005),
                                 dict(n_rounds=3, n_cg=18, huber_px=1.0), points_push=(64, 0.01)),
}
WRITES = ("example", "example_large_push", "hand", "frame_edges", "frame_edges_no_row_counts", "landmark_edges", "one_frame",
          "two_frames_one_held", "frames_257", "every_frame_held", "poses_alone", "two_groups", "rejected_then_accepted",
          "one_cg_iteration", "huber_noisy")                 # the cases whose status is OK after at least one round

_cache, _ref = {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def run(c, **kw):
    return B.bundle(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], c["fixed"], n_rows=c["n_rows"], **dict(c["params"], **kw))


def reference(name, reverse=False):
    """the restatement on a case, computed once and shared"""
    key = (name, reverse)
    if key not in _ref:
        _ref[key] = run(case(name), reverse=reverse)
    return _ref[key]


def reach(name):
    """(poses, points): the distance between the restatement's forward-order and reversed-order runs, in pixels"""
    return B.distance(reference(name), reference(name, True))
