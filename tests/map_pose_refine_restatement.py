"""NumPy restatement of vo_map_refine_poses* and vo_map_adjust* (include/vo_map_adjust.h), written from the header's rules.

Observations: the lookup of tests/map_localise_restatement.py on every frame's live rows; a frame consumes the rows that hit an
entry in ascending position, the point is the entry's float32 point widened.  The point half of the adjustment is
tests/map_refine_restatement.py.  Everything is float64; `dtype=np.float32` evaluates the per-observation terms (projection,
residual, Jacobian, the products that go into the sums) in float32 and still sums, solves and carries the pose in float64 --
that switch exists for the tolerance rule of tests/test_gpu_map_pose_refine.py alone.  `fault` plants a mistake, to show that
the measures of the tests see it."""
import numpy as np

import map_localise_restatement as M
import map_refine_restatement as R

OK, FIXED, FEW_OBS, BEHIND, NOT_FINITE, COST_ROSE = range(6)
FAULTS = ("sign_in_J", "right_multiply", "angles_swapped", "dropped_observation", "jacobian_from_map_point")


def v2t(dx):
    """the solver's v2t: translation dx[0:3], R = Rx(dx3) Ry(dx4) Rz(dx5)"""
    a, b, c = dx[3], dx[4], dx[5]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry @ Rz
    T[:3, 3] = dx[:3]
    return T


def ldlt_solve(H, b):
    """x = H^-1 b by LDL^T in natural order; None when a pivot is not > 0 or the step is not finite"""
    n = len(b)
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        d = H[j, j] - sum(L[j, m] * L[j, m] * D[m] for m in range(j))
        if not d > 0:
            return None
        D[j] = d
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - sum(L[i, m] * L[j, m] * D[m] for m in range(j))) / d
    y = np.zeros(n)
    for i in range(n):
        y[i] = b[i] - sum(L[i, m] * y[m] for m in range(i))
    x = np.zeros(n)
    for i in reversed(range(n)):
        x[i] = y[i] / D[i] - sum(L[m, i] * x[m] for m in range(i + 1, n))
    return x if np.isfinite(x).all() else None


def evaluate(K, T, uv, pts, huber, dt=np.float64, fault=None):
    """the sums of one evaluation at the pose T (4x4) over the observations (uv (n, 2), pts (n, 3)): (H (6, 6), b (6,), cost,
    camera z (n,)) in float64"""
    K, T, uv, p = (np.asarray(x, np.float64).astype(dt) for x in (K, T, uv, pts))
    with np.errstate(all="ignore"):
        pc = p @ T[:3, :3].T + T[:3, 3]
        q = pc @ K.T
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        e = np.stack([u - uv[:, 0], v - uv[:, 1]], 1)
        j0 = (K[0][None] - u[:, None] * K[2][None]) / q[:, 2:3]
        j1 = (K[1][None] - v[:, None] * K[2][None]) / q[:, 2:3]
        x = p if fault == "jacobian_from_map_point" else pc
        J = np.zeros((len(p), 2, 6), dt)
        for k, j in enumerate((j0, j1)):                      # j [I, -[x]x] = (j, x cross j)
            J[:, k, :3] = j
            J[:, k, 3:] = np.cross(x, j)
        if fault == "sign_in_J":
            J[:, 0, 4] = -J[:, 0, 4]
        r2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        w, rho = np.ones_like(r2), r2
        if huber > 0:
            r = np.sqrt(r2)
            out = r > dt(huber)
            w = np.where(out, dt(huber) / r, dt(1))
            rho = np.where(out, dt(huber) * (dt(2) * r - dt(huber)), r2)
        wJ = w[:, None, None] * J
        H = np.einsum("nka,nkb->nab", wJ, J).astype(np.float64).sum(0)
        b = np.einsum("nka,nk->na", wJ, e).astype(np.float64).sum(0)
        cost = float(rho.astype(np.float64).sum())
        z = pc[:, 2].astype(np.float64)
    return H, b, cost, z


def to_f32_pose(T):
    """the stored pose: 12 entries rounded to float32, the bottom row 0, 0, 0, 1"""
    with np.errstate(all="ignore"):
        out = np.asarray(T, np.float64).astype(np.float32)
    out[3] = (0, 0, 0, 1)
    return out


def refine_pose(K, T0, uv, pts, n_rounds, huber, damping, dt=np.float64, fault=None):
    """one frame with its observations in row order; T0 float32 4x4.  dict(status, pose float32 4x4, T64 (the pose before it
    was rounded), H (damped, of the last solved round), cost0, cost1, marginal)"""
    T0 = np.asarray(T0, np.float32).reshape(4, 4)
    T = T0.astype(np.float64)
    T[3] = (0, 0, 0, 1)                                       # (only the 12 entries are read)
    out = dict(status=OK, pose=T0.copy(), T64=T.copy(), H=np.full((6, 6), np.nan), cost0=0.0, cost1=0.0, marginal=False)
    if fault == "dropped_observation":
        uv, pts = uv[:-1], pts[:-1]
    behind = False
    Tf = T0.copy()
    for r in range(n_rounds + 1):
        H, b, cost, z = evaluate(K, T, uv, pts, huber, dt, fault)
        if not (np.isfinite(H).all() and np.isfinite(b).all() and np.isfinite(cost)):
            out["status"] = NOT_FINITE
            return out
        behind = behind or not bool((z > 0).all())
        out["marginal"] = out["marginal"] or bool((np.abs(z) < 1e-5).any())
        if r == 0:
            out["cost0"] = cost
        if r == n_rounds:
            out["cost1"] = cost
            break
        H = H + damping * np.eye(6)
        x = ldlt_solve(H, b)
        if x is None:
            out["status"] = NOT_FINITE
            return out
        out["H"] = H
        dx = -x
        if fault == "angles_swapped":
            dx = dx[[0, 1, 2, 4, 3, 5]]
        T = T @ v2t(dx) if fault == "right_multiply" else v2t(dx) @ T
        if r == n_rounds - 1:
            out["T64"] = T.copy()
            Tf = to_f32_pose(T)
            T = Tf.astype(np.float64)
        if not np.isfinite(T).all():
            out["status"] = NOT_FINITE
            return out
    if behind:
        out["status"] = BEHIND
    elif out["cost1"] > out["cost0"]:
        out["status"] = COST_ROSE
    if n_rounds > 0 and out["status"] in (OK, COST_ROSE) and abs(out["cost1"] - out["cost0"]) < 1e-6 * abs(out["cost0"]):
        out["marginal"] = True
    if out["status"] == OK and n_rounds > 0:
        out["pose"] = Tf
    return out


def frame_observations(map_app, frames, n_rows=None, n_max=None, tab=None):
    """per frame (positions (k,), entries (k,)) of the live rows that hit an entry, in ascending position"""
    n_max = max([len(np.asarray(a).reshape(-1, 10)) for _, a in frames] + [0]) if n_max is None else int(n_max)
    tab = M.table(map_app) if tab is None else tab
    out = []
    for f, (_, app) in enumerate(frames):
        app = np.asarray(app, np.float32).reshape(-1, 10)
        live = len(app) if n_rows is None else max(0, min(int(n_rows[f]), len(app), n_max))
        ent = M.lookup(map_app, app, n_live=live, tab=tab)[0]
        i = np.nonzero(ent >= 0)[0]
        out.append((i, ent[i]))
    return out


def fixed_order_sum(values, ok):
    """the device's fixed order: item k goes to partial sum k mod 1024 in order, the partial sums are added in order"""
    part = np.zeros(1024)
    for k in np.nonzero(ok)[0]:
        part[k % 1024] += values[k]
    s = 0.0
    for t in range(1024):
        s += part[t]
    return float(s)


def refine_poses(K, map_pts, map_app, frames, poses, fixed=None, n_rounds=10, min_obs=3, huber_px=0.0, damping=0.0, dtype=np.float64,
                 n_rows=None, n_max=None, fault=None, obs=None):
    """The whole call.  poses: one 4x4 per frame (p_cam = T p_map), taken as the float32 the device call is given.  Returns
    dict(poses (F, 4, 4) float32, status (F,), n_obs (F,), T64 (F, 4, 4), H (F, 6, 6), cost0, cost1 (F,), marginal (F,), stats)."""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    pts = np.asarray(map_pts, np.float32).reshape(-1, 3)
    F = len(frames)
    T0 = np.stack([np.asarray(X, np.float32).reshape(4, 4) for X in poses])
    obs = frame_observations(map_app, frames, n_rows, n_max) if obs is None else obs
    res = dict(poses=T0.copy(), status=np.full(F, -1, np.int32), n_obs=np.array([len(i) for i, _ in obs], np.int32),
               T64=T0.astype(np.float64), H=np.full((F, 6, 6), np.nan), cost0=np.zeros(F), cost1=np.zeros(F), marginal=np.zeros(F, bool))
    for f in range(F):
        i, e = obs[f]
        if fixed is not None and fixed[f]:
            res["status"][f] = FIXED
            continue
        if len(i) < min_obs:
            res["status"][f] = FEW_OBS
            continue
        uv = np.asarray(frames[f][0], np.float32).reshape(-1, 2)[i]
        o = refine_pose(K, T0[f], uv, pts[e], n_rounds, float(np.float32(huber_px)), float(np.float32(damping)), dtype, fault)
        res["status"][f] = o["status"]; res["poses"][f] = o["pose"]; res["T64"][f] = o["T64"]; res["H"][f] = o["H"]
        res["cost0"][f] = o["cost0"]; res["cost1"][f] = o["cost1"]; res["marginal"][f] = o["marginal"]
    ok = res["status"] == OK
    res["stats"] = dict(n_frames=F, n_obs=int(res["n_obs"].sum()), by_status=[int((res["status"] == s).sum()) for s in range(6)],
                        cost_before=fixed_order_sum(res["cost0"], ok), cost_after=fixed_order_sum(res["cost1"], ok))
    return res


def total_cost(K, map_pts, map_app, frames, poses, huber_px=0.0, n_rows=None, obs=None):
    """the cost both halves minimise, over ALL rows that hit an entry, whatever any status says -- evaluated on its own"""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    pts = np.asarray(map_pts, np.float32).astype(np.float64).reshape(-1, 3)
    obs = frame_observations(map_app, frames, n_rows) if obs is None else obs
    h = float(np.float32(huber_px))
    total = 0.0
    for f, (i, e) in enumerate(obs):
        if not len(i):
            continue
        T = np.asarray(poses[f], np.float32).astype(np.float64).reshape(4, 4)
        pc = pts[e] @ T[:3, :3].T + T[:3, 3]
        q = pc @ K.T
        r = np.linalg.norm(q[:, :2] / q[:, 2:3] - np.asarray(frames[f][0], np.float32).reshape(-1, 2)[i].astype(np.float64), axis=1)
        total += float(np.where((h > 0) & (r > h), h * (2 * r - h), r * r).sum())
    return total


def adjust(K, map_pts, map_app, frames, poses, fixed=None, n_sweeps=6, pose_rounds=2, point_rounds=2, min_obs_pose=3, min_obs_point=3,
           huber_px=0.0, damping=0.0, n_rows=None, dtype=np.float64):
    """The alternation: per sweep the pose half in place on the poses, then the point half (tests/map_refine_restatement.py)
    in place on the points.  Returns dict(poses (F, 4, 4) float32, points (M, 3) float32, pose_status, point_status, sweeps
    [dict(poses=stats, points=stats)], costs: the total cost at the start and after every half-sweep (2 n_sweeps + 1 values))."""
    pts = np.asarray(map_pts, np.float32).reshape(-1, 3).copy()
    T = np.stack([np.asarray(X, np.float32).reshape(4, 4) for X in poses])
    obs = frame_observations(map_app, frames, n_rows)
    costs = [total_cost(K, pts, map_app, frames, T, huber_px, obs=obs)]
    sweeps, ps, qs = [], None, None
    for _ in range(n_sweeps):
        a = refine_poses(K, pts, map_app, frames, T, fixed, pose_rounds, min_obs_pose, huber_px, damping, dtype, n_rows, obs=obs)
        T, ps = a["poses"], a["status"]
        costs.append(total_cost(K, pts, map_app, frames, T, huber_px, obs=obs))
        b = R.refine(K, pts, map_app, frames, T, point_rounds, min_obs_point, huber_px, damping, dtype, n_rows)
        pts, qs = b["points"], b["status"]
        costs.append(total_cost(K, pts, map_app, frames, T, huber_px, obs=obs))
        sweeps.append(dict(poses=a["stats"], points=b["stats"]))
    return dict(poses=T, points=pts, pose_status=ps, point_status=qs, sweeps=sweeps, costs=costs)


def pose_delta(T_from, T_to):
    """the 6-vector d with T_to = v2t(d) T_from to first order: the small angles of R_to R_from^T and the translation left"""
    A, B = np.asarray(T_from, np.float64), np.asarray(T_to, np.float64)
    dR = B[:3, :3] @ A[:3, :3].T
    alpha = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return np.concatenate([B[:3, 3] - dR @ A[:3, 3], alpha])


def h_norm(d, H):
    """sqrt(d^T H d): a pose difference in the frame's own final H, in pixels"""
    d = np.asarray(d, np.float64)
    return float(np.sqrt(max(d @ np.asarray(H, np.float64) @ d, 0.0)))


def half_ulp_px(T_f32, H):
    """half an ulp of each of the 12 stored float32 entries, carried through |H|.  A change dR, dt of the stored entries moves
    the pose by d = (dt - dR R^T t, the antisymmetric part of dR R^T): every entry's half ulp enters with the absolute value of
    its factor, so this is an upper bound."""
    T = np.asarray(T_f32, np.float32).reshape(4, 4)
    u = 0.5 * np.spacing(np.abs(T[:3])).astype(np.float64)
    Rm, t = np.abs(T[:3, :3].astype(np.float64)), T[:3, 3].astype(np.float64)
    A = u[:, :3] @ Rm.T                                       # |dR R^T| entry by entry
    d = np.concatenate([u[:, 3] + u[:, :3] @ np.abs(T[:3, :3].astype(np.float64).T @ t),
                        0.5 * np.array([A[2, 1] + A[1, 2], A[0, 2] + A[2, 0], A[1, 0] + A[0, 1]])])
    return float(np.sqrt(d @ np.abs(np.asarray(H, np.float64)) @ d))


def push(poses, seed, t_amount, a_amount):
    """every pose pushed off by v2t(uniform(+-t_amount) translation, uniform(+-a_amount) angles), as float32"""
    rng = np.random.default_rng(seed)
    return [to_f32_pose(v2t(np.concatenate([rng.uniform(-t_amount, t_amount, 3), rng.uniform(-a_amount, a_amount, 3)])) @
                        np.asarray(T, np.float64)) for T in poses]
