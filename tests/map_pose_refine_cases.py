"""The cases shared by tests/test_map_pose_refine_cpu.py (which asserts that the restatement takes no marginal decision on
them and re-measures the ceiling) and tests/test_gpu_map_pose_refine.py (which runs them on the device): the example data
and hand-made windows around the kernel's edges (16 lanes per DPP row, 64 lanes per wave, 256 threads per workgroup, several
trips of the row loop, 1024 threads of the statistics workgroup).

A case is a dict: K (3, 3), map_pts (M, 3) float32, map_app (M, 10), frames [(uv, app)], poses [4x4 float32] (the START,
already pushed), fixed (F,) bool or None, n_rows or None, params dict(n_rounds, min_obs, huber_px, damping), truth [4x4]."""
import numpy as np

import map_pose_refine_restatement as P
import map_refine_restatement as R

PB = 256                                                      # threads per workgroup (map_pose_refine.hip: PB)
K_HAND = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]], np.float32)
DEFAULT = dict(n_rounds=10, min_obs=3, huber_px=0.0, damping=0.0)
EDGE_HITS = [1, 2, 3, 6, 63, 64, 65, 255, 256, 257, 1025]


def example():
    E = R.example_problem()
    return dict(K=E["K"], map_pts=E["world_pts"], map_app=E["world_app"], frames=E["frames"], poses=P.push(E["poses"], 0, 0.2, 0.1),
                fixed=None, n_rows=None, params=dict(DEFAULT), truth=[np.asarray(T, np.float64) for T in E["poses"]])


def hand(hits, seed, map_size=1100, noise_px=0.0, params=None, fixed=None, extras=False, t_amount=0.05, a_amount=0.02, misses=2):
    """frame f sees hits[f] landmarks of a map of map_size entries in front of cameras that look along +z with small rotations,
    plus `misses` rows that are in no map, in a shuffled order; the start is the truth pushed off.  extras: frame 3 holds two
    rows of one landmark, every third frame carries garbage behind its live rows (n_rows says so), -0 stands against +0."""
    rng = np.random.default_rng(seed)
    Mn = int(map_size)
    pts = np.stack([rng.uniform(-2.5, 2.5, Mn), rng.uniform(-1.8, 1.8, Mn), rng.uniform(4, 9, Mn)], 1).astype(np.float32)
    app = rng.uniform(-1, 1, (Mn, 10)).astype(np.float32)
    if extras:
        app[:, 4] = np.where(rng.uniform(size=Mn) < 0.1, np.float32(0.0), app[:, 4])
    K = K_HAND.astype(np.float64)
    truth, frames, n_rows = [], [], []
    for f, h in enumerate(hits):
        T = P.v2t(np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.05, 0.05, 3)]))
        truth.append(T)
        ids = rng.choice(Mn, int(h), replace=False)
        pc = pts[ids].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        q = pc @ K.T
        uv = (q[:, :2] / q[:, 2:3] + (rng.normal(0, noise_px, (len(ids), 2)) if noise_px else 0)).astype(np.float32).reshape(-1, 2)
        a = app[ids].copy().reshape(-1, 10)
        if extras and f == 3 and h:                           # two rows of one landmark: a second, slightly different pixel
            uv = np.concatenate([uv, uv[:1] + np.float32(0.25)]); a = np.concatenate([a, a[:1]])
        uv = np.concatenate([uv, rng.uniform(0, 600, (misses, 2)).astype(np.float32)])
        a = np.concatenate([a, rng.uniform(-1, 1, (misses, 10)).astype(np.float32)])
        order = rng.permutation(len(a))
        uv, a = uv[order], a[order]
        if extras:
            a = np.where((a == 0) & (f % 2 == 0), np.float32(-0.0), a).astype(np.float32)
        live = len(a)
        if extras and f % 3 == 0:                             # garbage behind the live rows: real rows with wild pixels
            uv = np.concatenate([uv, rng.uniform(0, 600, (3, 2)).astype(np.float32)])
            a = np.concatenate([a, app[rng.integers(0, Mn, 3)]])
        frames.append((uv, a)); n_rows.append(live)
    start = P.push(truth, seed + 7, t_amount, a_amount)
    return dict(K=K_HAND.copy(), map_pts=pts, map_app=app, frames=frames, poses=start, fixed=None if fixed is None else np.asarray(fixed, bool),
                n_rows=np.array(n_rows, np.int32) if extras else None, params=dict(DEFAULT, **(params or {})), truth=truth)


def edges():
    """every hit count at a wave or workgroup edge in one call, an empty frame in between, two rows of one landmark, garbage
    behind the live rows under n_rows"""
    c = hand(EDGE_HITS[:5] + [0] + EDGE_HITS[5:], 31, extras=True, misses=0)
    c["frames"][5] = (np.zeros((0, 2), np.float32), np.zeros((0, 10), np.float32)); c["n_rows"][5] = 0
    return c


def failures():
    """frame 0 has a NaN pixel, frame 1 sees a landmark whose point is NaN (both NOT_FINITE), frame 2 has a NaN appearance row (it
    finds nothing: one observation fewer, OK), frame 3's camera is turned away (BEHIND), frame 4 is fine, frame 5 has 2 hits"""
    c = hand([8, 8, 8, 8, 8, 2], 37, map_size=64)
    obs = P.frame_observations(c["map_app"], c["frames"])
    c["frames"][0][0][obs[0][0][0], 1] = np.nan
    c["map_pts"][obs[1][1][0], 0] = np.nan
    for f in (0, 2, 3, 4, 5):                                  # (no other frame may see the NaN point)
        assert obs[1][1][0] not in obs[f][1]
    c["frames"][2][1][obs[2][0][0], 7] = np.nan
    c["poses"][3] = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ c["poses"][3].astype(np.float64)).astype(np.float32)
    return c


def cost_rose():
    """one round from 6 too far along the optical axis overshoots: the cost of the frame rises and every point stays in front of
    the camera (COST_ROSE, the 64 bytes kept; twenty rounds from the same start converge); the second frame starts close and is
    replaced"""
    c = hand([12, 12], 41, map_size=64, params=dict(n_rounds=1), t_amount=0.01, a_amount=0.005)
    c["poses"][0] = P.to_f32_pose(P.v2t(np.array([0, 0, 6.0, 0, 0, 0])) @ c["truth"][0])
    return c


CASES = {
    "example": example,
    "edges": edges,
    "edges_no_row_counts": lambda: hand(EDGE_HITS, 32),                                 # padding behind the rows, d_n_rows NULL
    "one_frame": lambda: hand([65], 33),
    "two_frames_one_held": lambda: hand([40, 30], 34, fixed=[1, 0]),
    "frames_257": lambda: hand(list(np.random.default_rng(5).integers(3, 40, 257)), 35, fixed=(np.arange(257) % 50 == 0)),
    "huber_noisy_damped": lambda: hand([20, 65, 300, 6], 36, noise_px=0.5, params=dict(huber_px=1.0, damping=1e-3)),
    "failures": failures,
    "cost_rose": cost_rose,
    "zero_rounds": lambda: hand([5, 70, 2], 38, params=dict(n_rounds=0)),
}

_cache, _ref = {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def reference(name, dtype=np.float64):
    """the restatement on a case, computed once and shared"""
    key = (name, np.dtype(dtype).name)
    if key not in _ref:
        c = case(name)
        _ref[key] = P.refine_poses(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], c["fixed"], n_rows=c["n_rows"], dtype=dtype,
                                   **c["params"])
    return _ref[key]


def float32_reach(name):
    """the largest H-norm distance between the restatement's float32 mode and its float64 mode over the case's OK frames"""
    r64, r32 = reference(name), reference(name, np.float32)
    worst = 0.0
    for f in np.nonzero((r64["status"] == P.OK) & np.isfinite(r64["H"]).all((1, 2)))[0]:
        worst = max(worst, P.h_norm(P.pose_delta(r64["T64"][f], r32["T64"][f]), r64["H"][f]))
    return worst


def one_round_small_push():
    """the planted-fault case of tests/test_map_pose_refine_cpu.py: 0.5 px noise, a push of 0.01 / 0.005 rad and ONE round, so
    that a faulty step still lowers the cost -- its frames stay OK and the measure, not a status, has to show the fault"""
    return hand([20, 65, 300, 6], 36, noise_px=0.5, params=dict(n_rounds=1), t_amount=0.01, a_amount=0.005)


# the alternation's cases (tests/test_gpu_map_adjust.py, the descent test of tests/test_map_pose_refine_cpu.py)
def example_adjust(t_amount=0.01, a_amount=0.005, p_amount=0.02):
    """the example data with points and poses pushed, frames 0 and 120 held at their ground truth"""
    E = R.example_problem()
    start = P.push(E["poses"], 6, t_amount, a_amount)
    fixed = np.zeros(len(start), bool)
    for f in (0, len(start) - 1):
        fixed[f] = True
        start[f] = P.to_f32_pose(E["poses"][f])
    return dict(K=E["K"], map_pts=R.perturbed(E["world_pts"], 5, p_amount), map_app=E["world_app"], frames=E["frames"], poses=start,
                fixed=fixed, n_rows=None, truth=[np.asarray(T, np.float64) for T in E["poses"]], truth_pts=E["world_pts"])


def hand_adjust():
    """3 frames x 65 rows of one map of 65 landmarks, the first frame held, 0.3 px noise"""
    c = hand([65, 65, 65], 43, map_size=65, noise_px=0.3, fixed=[1, 0, 0], misses=0, t_amount=0.02, a_amount=0.01)
    c["map_pts"] = R.perturbed(c["map_pts"], 44, 0.03)
    return c
