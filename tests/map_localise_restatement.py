"""NumPy restatement of vo_map_lookup* and vo_map_localise* (include/vo_hip.h), written from the header text.

Lookup: a dictionary keyed by the entry's row with -0 turned into +0; rows with a NaN are never keyed (a NaN entry is never
found) and never looked up (a NaN query finds nothing); the FIRST entry of equal rows wins.  Hits are compacted in query order.

Localisation: the composition the header names, in float64 from tests/pose_ransac_restatement.py -- lookup, the P3P RANSAC
winner on the pairs (query index, k) over the gathered points, the Gauss-Newton PICP from the winner on its inliers -- and the
status rule of the finishing launch."""
import os

import numpy as np

import pose_ransac_restatement as P

OK, FEW_MATCHES, NO_CONSENSUS, FEW_INLIERS, NOT_FINITE = range(5)


def _key(row):
    return (np.asarray(row, np.float32) + np.float32(0.0)).tobytes()          # -0 + 0 = +0: rows equal under == share a key


def table(map_app):
    d = {}
    for j, row in enumerate(np.asarray(map_app, np.float32).reshape(-1, 10)):
        if not np.isnan(row).any():
            d.setdefault(_key(row), j)
    return d


def lookup(map_app, queries, map_pts=None, n_live=None, tab=None):
    """(entries (n,) int32 with -1 for no hit and for the positions behind n_live, pairs (k, 2) = (query index, entry),
    gathered points (k, 3) or None)"""
    q = np.asarray(queries, np.float32).reshape(-1, 10)
    tab = table(map_app) if tab is None else tab
    n = len(q) if n_live is None else max(0, min(int(n_live), len(q)))
    ent = np.full(len(q), -1, np.int32)
    for i in range(n):
        if not np.isnan(q[i]).any():
            ent[i] = tab.get(_key(q[i]), -1)
    hit = np.nonzero(ent >= 0)[0]
    pairs = np.stack([hit, ent[hit]], 1).astype(np.int32).reshape(-1, 2)
    xyz = None if map_pts is None else np.asarray(map_pts, np.float32).reshape(-1, 3)[ent[hit]]
    return ent, pairs, xyz


def localise(K, cam, map_pts, map_app, uv, app, thr_px=2.0, n_hyp=64, seed=0, thr=10000.0, n_iters=50, min_inliers=6, T0=None,
             tab=None):
    """(T (4, 4) float64, status, info dict).  cam = (rows, cols, z_near, z_far).  n_hyp == 0: no RANSAC, T0 is the start."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    ent, pairs, world = lookup(map_app, app, map_pts, tab=tab)
    local = np.stack([pairs[:, 0], np.arange(len(pairs))], 1).astype(np.int64).reshape(-1, 2)
    back = np.eye(4) if T0 is None else np.asarray(T0, np.float64)
    info = dict(n_hits=len(pairs), ransac_status=0, ransac_inliers=len(pairs))
    if len(pairs) < 6:
        return back, FEW_MATCHES, info
    if n_hyp > 0:
        counts, win, mask, T_start = P.ransac(K, world, uv, local, thr_px, n_hyp, seed, *cam)
        if win < 0 or int(mask.sum()) < 6:
            info["ransac_status"] = 2 if win < 0 else 3
            return back, NO_CONSENSUS, info
        handed = local[mask]
        info["ransac_inliers"] = len(handed)
    else:
        T_start, handed = back, local
    T = P.picp(K, T_start, world, uv, handed, thr, n_iters, *cam)
    if not np.isfinite(T).all():
        return back, NOT_FINITE, info
    n_in = int(P.inliers(K, T, world, uv, handed, np.sqrt(thr), *cam).sum())      # chi^2 = squared pixel error < threshold
    info["num_inliers"] = n_in
    if n_in < min_inliers:
        return back, FEW_INLIERS, info
    return T, OK, info


# ---- the example data (tests/golden/example_data): the map is world.dat, every measurement file names its landmarks ----
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example_data", "data")


def example_data():
    """dict(K, C (cam_transform), cam, world_pts, world_app, frames [(uv, app, ids)], gt [4x4 robot poses])"""
    import re
    from oracle import vo_pipeline as vp
    files = sorted(f for f in os.listdir(DATA) if re.search(r"^meas-\d.*\.dat$", f))
    K, C, ints = vp.read_camera(os.path.join(DATA, "camera.dat"))
    pts, app = vp.read_world(os.path.join(DATA, "world.dat"))
    frames = [vp.read_meas(os.path.join(DATA, f)) for f in files]
    return dict(K=K, C=C.astype(np.float64), cam=(ints["height"], ints["width"], ints["z_near"], ints["z_far"]), world_pts=pts,
                world_app=app, frames=frames, gt=vp.read_gt(os.path.join(DATA, "trajectory.dat")))


def robot_pose(T, C):
    """the data's convention: T takes map points into the camera, C is the camera in the robot: robot in map = T^-1 C^-1"""
    return np.linalg.inv(np.asarray(T, np.float64)) @ np.linalg.inv(C)
