"""One window of frames per state of tests/map_states.py, shared by tests/test_map_states_cpu.py (which runs the float64
restatements alone and asserts the conditions that keep a GPU test from passing vacuously) and tests/test_gpu_map_states.py
(which runs every `_dev` call on the state's map and on its twin).

A case is a dict: K, map_pts (M, 3) float32 and map_app (M, 10) -- the rows the state is BUILT from, unique and free of NaN --,
kept (the entries the state's map holds: M, or the capacity where the state drops rows), edge (the smaller bound a faulty path
would use: 300 for the slack states and the capture in front of an update, 600 for `replayed`, 800 for `overflowed` -- what the
host had counted), frames [(uv, app)] of ROWS rows each (n_rows None), poses (the start, pushed off the truth; frame 0 held at
its truth), fixed, truth, and the parameters of every call.  Every frame holds rows of random classes of ALL M rows (those at or
above `kept` are dropped classes: they must behave as misses), rows of N_NEW classes no map holds (the tracks voe_map_grow
triangulates; under `overflowed` the dropped classes are open rows as well) and two rows of no class at all.  PUSHED landmarks on
both sides of the edge stand 0.3 off their truth, so that the cull has something to drop for its error too.

The slack states hold 300 entries: no entry lies at or above their edge -- what lies in [300, bound) is what no call may touch --
so "both sides of the edge" is asked of the three cases whose map is larger than its edge.

THE SEEDS (SEEDS below) are fixed so that the conditions of tests/test_map_states_cpu.py hold with the margins it asserts; they
were chosen by running that test, which needs no device."""
import numpy as np

import map_cull_restatement as Q
import map_grow_restatement as Gr
import map_localise_restatement as M
import map_bundle_restatement as B
import map_pose_refine_restatement as P
import map_refine_restatement as R
import map_covis_restatement as Cv

K_HAND = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]], np.float32)
F, ROWS, HITS, N_NEW, N_PUSHED = 7, 312, 250, 60, 40
STATES = ("slack_1", "slack_300", "replayed", "overflowed")
SHAPE = dict(slack_1=(300, 300, 300), slack_300=(300, 300, 300), replayed=(900, 900, 600), overflowed=(1200, 1024, 800))      # rows, kept, edge
SEEDS = dict(slack_1=101, slack_300=102, replayed=103, overflowed=104)
CAPTURE_EDGES = (300, 600)                                     # the pre-update capture replays on the `replayed` case's rows: 300, 600, 900 entries

REFINE = dict(n_rounds=3, min_obs=2, huber_px=0.0, damping=0.0)
POSES = dict(n_rounds=3, min_obs=3, huber_px=0.0, damping=0.0)
ADJUST = dict(n_sweeps=2, pose_rounds=2, point_rounds=2, min_obs_pose=3, min_obs_point=2, huber_px=0.0, damping=0.0)
BUNDLE = dict(B.DEFAULT, n_rounds=2, n_cg=24, cg_tol=0.0, lambda0=1e-4, min_obs_pose=3, min_obs_point=2)
CULL = dict(Q.DEFAULT, min_obs=2, min_frames=2, max_rms_px=2.0, min_parallax_deg=0.5)
GROW = dict(Gr.DEFAULT, n_rounds=3, min_obs=3, min_frames=3, max_rms_px=2.0, min_parallax_deg=0.5, max_added=100)      # (room for 100: only the full map has to grow)
WINDOW = dict(query=3, k_free=3, k_fixed=2, min_shared=5)
N_WORDS = 32                                                  # 1024 bits: every state's bound and every twin's fit

_cache, _ref = {}, {}


def make(n_map, kept, edge, seed):
    rng = np.random.default_rng(seed)
    n_all = n_map + N_NEW
    truth_pts = np.stack([rng.uniform(-2.5, 2.5, n_all), rng.uniform(-1.8, 1.8, n_all), rng.uniform(4, 9, n_all)], 1).astype(np.float32)
    app = rng.uniform(-1, 1, (n_all, 10)).astype(np.float32)
    assert len({r.tobytes() for r in app}) == n_all and not np.isnan(app).any()
    Kd = K_HAND.astype(np.float64)
    truth, frames = [], []
    for f in range(F):
        T = P.v2t(np.concatenate([[-0.9 + 1.8 * f / (F - 1)], rng.uniform(-0.2, 0.2, 2), rng.uniform(-0.04, 0.04, 3)]))
        truth.append(T)
        ids = np.concatenate([rng.choice(n_map, HITS, replace=False), n_map + np.nonzero(rng.random(N_NEW) < 0.6)[0]])
        pc = truth_pts[ids].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        q = pc @ Kd.T
        uv = (q[:, :2] / q[:, 2:3] + rng.normal(0, 0.2, (len(ids), 2))).astype(np.float32)
        a = app[ids].copy()
        n_miss = ROWS - len(ids)
        assert n_miss >= 2
        uv = np.concatenate([uv, rng.uniform(0, 600, (n_miss, 2)).astype(np.float32)])
        a = np.concatenate([a, rng.uniform(-1, 1, (n_miss, 10)).astype(np.float32)])
        order = rng.permutation(ROWS)
        frames.append((uv[order], a[order]))
    start = P.push(truth, seed + 7, 0.002, 0.001)
    start[0] = P.to_f32_pose(truth[0])
    map_pts = R.perturbed(truth_pts[:n_map], seed + 8, 0.005)
    lo = min(edge, kept)
    pushed = np.sort(np.concatenate([rng.choice(lo, N_PUSHED // 2, replace=False), lo + rng.choice(max(kept - lo, 1), N_PUSHED // 2, replace=False)
                                     if kept > lo else rng.choice(lo, 0)]))
    map_pts[pushed] += np.float32(0.3)
    return dict(K=K_HAND.copy(), map_pts=map_pts, map_app=app[:n_map].copy(), kept=kept, edge=edge, frames=frames, poses=start,
                fixed=np.arange(F) == 0, n_rows=None, truth=truth, pushed=pushed, new_app=app[n_map:].copy())


def case(state):
    if state not in _cache:
        _cache[state] = make(*SHAPE[state], SEEDS[state])
    return _cache[state]


def cut(c, n=None):
    """(points, appearances) of the first n rows the case is built from (default: what the state's map holds)"""
    n = c["kept"] if n is None else n
    return c["map_pts"][:n], c["map_app"][:n]


def run(call, c, n=None, pts=None, poses=None, **kw):
    """the float64 restatement of one call on the case's frames against the first n rows of its map"""
    p, a = cut(c, n)
    p = p if pts is None else pts
    T = c["poses"] if poses is None else poses
    if call == "lookup":
        tab = M.table(a)
        return [M.lookup(a, q, p, tab=tab) for _, q in c["frames"]]
    if call == "refine":
        return R.refine(c["K"], p, a, c["frames"], T, **dict(REFINE, **kw))
    if call == "poses":
        return P.refine_poses(c["K"], p, a, c["frames"], T, c["fixed"], **dict(POSES, **kw))
    if call == "adjust":
        return P.adjust(c["K"], p, a, c["frames"], T, c["fixed"], **dict(ADJUST, **kw))
    if call == "bundle":
        return B.bundle(c["K"], p, a, c["frames"], T, c["fixed"], **dict(BUNDLE, **kw))
    if call == "cull":
        return Q.cull(c["K"], p, a, c["frames"], T, **dict(CULL, **kw))
    if call == "grow":
        return Gr.grow(c["K"], p, a, c["frames"], T, **dict(GROW, **kw))
    if call == "covis":
        return Cv.covis(a, c["frames"], n_words=N_WORDS)
    raise KeyError(call)


def reference(state, call, n=None):
    """the restatement on a state's case, computed once and shared"""
    key = (state, call, n)
    if key not in _ref:
        _ref[key] = run(call, case(state), n)
    return _ref[key]


# ---- a second map for the alignment and the merge -----------------------------------------------------------------------------
ALIGN = dict(seed=5, n_hypotheses=32, with_scale=1, n_refits=1, min_inliers=3, threshold=0.05)
N_SHARED, N_OWN = 80, 40                                      # (120 rows: merged into the `replayed` map they fit its capacity)


def other_map(state):
    """(points, appearances) of a map that shares N_SHARED of the state's entries, half of them on either side of the edge where
    the map reaches beyond it, seen from another frame (p_state = c R p_other + t), and holds N_OWN entries of its own"""
    import map_align_cases as Ac
    c = case(state)
    rng = np.random.default_rng(SEEDS[state] + 50)
    kept, edge = c["kept"], min(c["edge"], c["kept"])
    ids = rng.choice(edge, N_SHARED, replace=False) if kept == edge else np.concatenate(
        [rng.choice(edge, N_SHARED // 2, replace=False), edge + rng.choice(kept - edge, N_SHARED // 2, replace=False)])
    Rm = Ac.rotation(rng.normal(size=3), 0.4)
    pts = np.concatenate([Ac.inverse_moved(c["map_pts"][ids], 1.3, Rm, np.array([0.4, -0.7, 1.1])),
                          rng.uniform(-3, 3, (N_OWN, 3)).astype(np.float32)])
    app = np.concatenate([c["map_app"][ids], rng.uniform(-1, 1, (N_OWN, 10)).astype(np.float32)])
    order = rng.permutation(len(pts))
    return pts[order], app[order]


def align_case(state, state_is):
    """the case of tests/map_align_restatement.py with the state's map as `state_is` ("dst" or "src") and other_map as the other"""
    key = (state, "align_case", state_is)
    if key not in _ref:
        sp, sa = cut(case(state))
        op, oa = other_map(state)
        _ref[key] = (dict(dst_pts=sp, dst_app=sa, src_pts=op, src_app=oa, params=dict(ALIGN)) if state_is == "dst" else
                     dict(dst_pts=op, dst_app=oa, src_pts=sp, src_app=sa, params=dict(ALIGN)))
    return _ref[key]


def align_reference(state, state_is):
    import map_align_restatement as A
    key = (state, "align", state_is)
    if key not in _ref:
        _ref[key] = A.run(align_case(state, state_is))
    return _ref[key]
