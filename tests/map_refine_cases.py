"""The cases shared by tests/test_map_refine_cpu.py (which asserts that the restatement has no marginal landmark on them and
re-measures the ceiling) and tests/test_gpu_map_refine.py (which runs them on the device): the example data, two small
synthetic sequences and hand-made scenes around the kernel's edges (16 lanes per landmark, 64 lanes per wave, 256 entries per
workgroup of the list kernels, 512 frames staged in LDS).

A case is a dict: K (3, 3), map_pts (M, 3) float32 (the START, already perturbed), map_app (M, 10), frames [(uv, app)],
poses [4x4], n_rows (or None), params dict(n_rounds, min_obs, huber_px, damping), truth (M, 3) or None."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import map_refine_restatement as R

G = 16                                                        # lanes per landmark (map_refine.hip: RG)
LDS_FRAMES = 512                                              # poses staged in LDS up to here (map_refine.hip: REFINE_LDS_FRAMES)
K_HAND = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]], np.float32)
DEFAULT = dict(n_rounds=10, min_obs=3, huber_px=0.0, damping=0.0)


def _synth():
    import __graft_entry__ as g
    return g.load_package().synth


def example():
    P = R.example_problem()
    return dict(K=P["K"], map_pts=R.perturbed(P["world_pts"]), map_app=P["world_app"], frames=P["frames"], poses=P["poses"], n_rows=None,
                params=dict(DEFAULT), truth=P["world_pts"])


def sequence_case(noise_px, params, seed=3000, n_frames=12, n_visible=40, amount=0.05):
    synth = _synth()
    s = synth.sequence(seed=seed, n_frames=n_frames, n_visible=n_visible, noise_px=noise_px)
    poses = [np.linalg.inv(synth.planar_pose(*g) @ synth.CAM_IN_ROBOT) for g in s["gt"]]
    return dict(K=s["K"], map_pts=R.perturbed(s["world_xyz"], seed + 1, amount), map_app=s["world_app"],
                frames=[(f["pts"], f["app"]) for f in s["frames"]], poses=poses, n_rows=None, params=dict(DEFAULT, **params),
                truth=s["world_xyz"], ids=[f["ids"] for f in s["frames"]])


def hand(counts, n_frames, seed, map_size=None, noise_px=0.0, params=None, extras=False, amount=0.05):
    """landmark k is seen by counts[k] frames spread over a camera path along x (the cameras look along +z with small
    rotations); map_size pads the map with unseen entries.  extras: a frame with two rows of one landmark, garbage behind the
    live rows, an empty frame, -0 against +0, a NaN appearance row and rows that are in no map."""
    rng = np.random.default_rng(seed)
    L = len(counts)
    Mn = max(map_size or L, L)
    F = int(n_frames)
    truth = np.stack([rng.uniform(-1.5, 1.5, Mn), rng.uniform(-1, 1, Mn), rng.uniform(4, 7, Mn)], 1).astype(np.float32)
    app = rng.uniform(-1, 1, (Mn, 10)).astype(np.float32)
    if extras:
        app[0, 4] = 0.0                                       # +0 in the map, -0 in the frames
    poses = []
    for f in range(F):
        a = rng.uniform(-0.03, 0.03, 3)
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        T = np.eye(4)
        T[:3, :3] = Rx @ Ry @ Rz
        c = np.array([-1.5 + 3.0 * f / max(F - 1, 1), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
        T[:3, 3] = -T[:3, :3] @ c
        poses.append(T.astype(np.float32))
    seen = [[] for _ in range(F)]
    for k, c in enumerate(counts):
        for f in (np.round(np.linspace(0, F - 1, c)).astype(int) if c <= F and c > 0 else []):
            seen[int(f)].append(k)
        assert c <= F and (c == 0 or len(set(np.round(np.linspace(0, F - 1, c)).astype(int))) == c)
    K = K_HAND.astype(np.float64)
    frames, n_rows = [], []
    for f in range(F):
        ids = rng.permutation(seen[f]).astype(int)
        T = poses[f].astype(np.float64)
        pc = truth[ids].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        q = pc @ K.T
        uv = q[:, :2] / q[:, 2:3] + (rng.normal(0, noise_px, (len(ids), 2)) if noise_px else 0)
        uv, a = uv.astype(np.float32).reshape(-1, 2), app[ids].copy().reshape(-1, 10)
        live = len(ids)
        if extras:
            if f == 1 and live:                               # two rows of one landmark: a second, slightly different pixel
                uv = np.concatenate([uv, uv[:1] + np.float32(0.25)]); a = np.concatenate([a, a[:1]])
            if f == 2:                                        # a NaN row (finds nothing) and a row of no map
                bad = app[:1].copy(); bad[0, 7] = np.nan
                uv = np.concatenate([uv, uv[:1], uv[:1]]) if live else np.zeros((2, 2), np.float32)
                a = np.concatenate([a, bad, rng.uniform(-1, 1, (1, 10)).astype(np.float32)])
            if f == 3:                                        # an empty frame
                uv, a = uv[:0], a[:0]
            a = np.where((a == 0) & (f % 2 == 0), np.float32(-0.0), a).astype(np.float32)
            live = len(a)
            if f % 3 == 0:                                    # garbage behind the live rows: real rows with wild pixels
                uv = np.concatenate([uv, rng.uniform(0, 600, (3, 2)).astype(np.float32)])
                a = np.concatenate([a, app[rng.integers(0, Mn, 3)]])
        frames.append((uv, a)); n_rows.append(live)
    return dict(K=K_HAND.copy(), map_pts=R.perturbed(truth, seed + 7, amount), map_app=app, frames=frames, poses=poses,
                n_rows=np.array(n_rows, np.int32) if extras else None, params=dict(DEFAULT, **(params or {})), truth=truth)


def failures():
    """every status but COST_ROSE (that one: cost_rose() below): landmark 0 has one observation from a camera that looks the other way (BEHIND, and a clean
    fit all the same), landmark 1 starts at a NaN, landmark 2 has a NaN pixel (NOT_FINITE), 3 and 4 are fine, 5 is seen twice
    (FEW_OBS), 6 never (UNSEEN)"""
    c = hand([5, 5, 5, 5, 6, 2, 0], 6, 19)
    flip = np.diag([-1.0, 1.0, -1.0, 1.0]) @ c["poses"][0].astype(np.float64)
    pc = flip[:3, :3] @ c["truth"][0].astype(np.float64) + flip[:3, 3]
    q = K_HAND.astype(np.float64) @ pc
    assert pc[2] < -1
    c["poses"].append(flip.astype(np.float32))
    c["frames"].append(((q[:2] / q[2]).astype(np.float32).reshape(1, 2), c["map_app"][:1].copy()))
    c["map_pts"][1, 0] = np.nan
    tab = {r.tobytes(): k for k, r in enumerate(c["map_app"])}
    for f, (uv, a) in enumerate(c["frames"]):
        hit = [i for i in range(len(a)) if tab.get(a[i].tobytes()) == 2]
        if hit:
            uv[hit[0], 1] = np.nan
            break
    return c


def cost_rose():
    """one round from z = 9 towards a landmark at z = 5 overshoots: its cost rises, it stays in front of the four cameras
    (COST_ROSE, the 12 bytes kept); the second landmark starts close and is replaced"""
    truth = np.array([[0.3, -0.2, 5.0], [-0.5, 0.4, 6.0]], np.float32)
    app = np.random.default_rng(21).uniform(-1, 1, (2, 10)).astype(np.float32)
    poses, frames = [], []
    for x in (-1.0, 0.0, 1.0, 2.0):
        T = np.eye(4, dtype=np.float32); T[0, 3] = -x
        q = (truth.astype(np.float64) + T[:3, 3].astype(np.float64)) @ K_HAND.astype(np.float64).T
        poses.append(T); frames.append(((q[:, :2] / q[:, 2:3]).astype(np.float32), app.copy()))
    return dict(K=K_HAND.copy(), map_pts=np.array([[0.3, -0.2, 9.0], [-0.5, 0.4, 6.1]], np.float32), map_app=app, frames=frames, poses=poses,
                n_rows=None, params=dict(DEFAULT, n_rounds=1), truth=truth)


def _counts_around_edges():
    return [2, 3, G - 1, G, G + 1, 63, 64, 65, 257, 0, 1]


CASES = {
    "example": example,
    "sequence_exact": lambda: sequence_case(0.0, {}),
    "sequence_noisy_huber_damped": lambda: sequence_case(0.5, dict(huber_px=1.0, damping=1e-3), seed=3001),
    "edges_257_frames": lambda: hand(_counts_around_edges(), 257, 11, extras=True),
    "edges_min_obs_2": lambda: hand([2, 3, 5, 2, 1, 0, 4], 6, 12, params=dict(min_obs=2), noise_px=0.5),
    "map_of_1": lambda: hand([5], 5, 13),
    "map_of_255": lambda: hand(list(np.random.default_rng(1).integers(0, 7, 255)), 6, 14, extras=True),
    "map_of_256": lambda: hand(list(np.random.default_rng(2).integers(0, 7, 256)), 6, 15),
    "map_of_257": lambda: hand(list(np.random.default_rng(3).integers(0, 7, 257)), 6, 16, map_size=257, extras=True),
    "failures": failures,
    "cost_rose": cost_rose,
    "one_frame": lambda: hand([1, 1, 1, 0], 1, 17),
    "frames_beyond_lds": lambda: hand(list(np.random.default_rng(4).integers(3, 40, 20)), LDS_FRAMES + 1, 18, noise_px=0.5),
}

_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


_ref = {}


def reference(name, dtype=np.float64):
    """the restatement on a case, computed once and shared"""
    key = (name, np.dtype(dtype).name)
    if key not in _ref:
        c = case(name)
        _ref[key] = R.refine(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], n_rows=c["n_rows"], dtype=dtype, **c["params"])
    return _ref[key]


def half_ulp_px(point, H):
    """half an ulp of every stored float32 coordinate, carried through H (an upper bound: |H| and the ulps as they come)"""
    u = 0.5 * np.spacing(np.abs(np.asarray(point, np.float32))).astype(np.float64)
    return float(np.sqrt(u @ np.abs(np.asarray(H, np.float64)) @ u))


def float32_reach(name):
    """the largest H-norm distance between the restatement's float32 mode and its float64 mode over the case's OK landmarks"""
    r64, r32 = reference(name), reference(name, np.float32)
    worst = 0.0
    for e in np.nonzero(r64["status"] == R.OK)[0]:
        worst = max(worst, R.h_norm(r32["p64"][e] - r64["p64"][e], r64["H"][e]))
    return worst
