"""NumPy restatement of vo_map_refine* (include/vo_hip.h), written from the header's rules.

Observations: the lookup of tests/map_localise_restatement.py on every frame's live rows; the observation of entry e made by
row i of frame f has the key f * n_max + i, and a landmark consumes its observations in ascending key order.  Everything is
float64; `dtype=np.float32` evaluates the per-observation terms (projection, residual, Jacobian, the products that go into
the sums) in float32 and still sums, solves and carries the point in float64 -- that switch exists for the tolerance rule of
tests/test_gpu_map_refine.py alone.  `fault` plants a mistake, to show that the measures of the tests see it."""
import numpy as np

import map_localise_restatement as M

OK, UNSEEN, FEW_OBS, BEHIND, NOT_FINITE, COST_ROSE = range(6)
FAULTS = ("dropped_observation", "sign_in_J", "translation_dropped", "neighbour_mixed_in")


def observation_lists(map_app, frames, n_rows=None, n_max=None, tab=None):
    """(lists: entry -> ascending keys, n_max, entries per frame).  frames: [(uv, app)]; n_rows[f] live rows (default: all)."""
    n_max = max([len(np.asarray(a).reshape(-1, 10)) for _, a in frames] + [0]) if n_max is None else int(n_max)
    tab = M.table(map_app) if tab is None else tab
    lists, ents = {}, []
    for f, (_, app) in enumerate(frames):
        app = np.asarray(app, np.float32).reshape(-1, 10)
        live = len(app) if n_rows is None else max(0, min(int(n_rows[f]), len(app), n_max))
        ent = M.lookup(map_app, app, n_live=live, tab=tab)[0]
        ents.append(ent)
        for i in np.nonzero(ent >= 0)[0]:
            lists.setdefault(int(ent[i]), []).append(f * n_max + int(i))
    for e in lists:
        lists[e].sort()
    return lists, n_max, ents


def ldlt3_solve(H, b):
    """x = H^-1 b by LDL^T in natural order; None when a pivot is not > 0 or the step is not finite"""
    d0 = H[0, 0]
    if not d0 > 0:
        return None
    l10, l20 = H[0, 1] / d0, H[0, 2] / d0
    d1 = H[1, 1] - l10 * l10 * d0
    if not d1 > 0:
        return None
    l21 = (H[1, 2] - l20 * l10 * d0) / d1
    d2 = H[2, 2] - l20 * l20 * d0 - l21 * l21 * d1
    if not d2 > 0:
        return None
    y0 = b[0]; y1 = b[1] - l10 * y0; y2 = b[2] - l20 * y0 - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = y0 / d0 - l10 * x1 - l20 * x2
    x = np.array([x0, x1, x2])
    return x if np.isfinite(x).all() else None


def evaluate(K, R, t, uv, p, huber, dt=np.float64, fault=None):
    """the sums of one evaluation at p: (H (3, 3), b (3,), cost, smallest camera z, all z > 0) in float64"""
    K, R, t, uv, p = (np.asarray(x, np.float64).astype(dt) for x in (K, R, t, uv, p))
    with np.errstate(all="ignore"):
        pc = np.einsum("nrc,c->nr", R, p) + (0 if fault == "translation_dropped" else t)
        q = pc @ K.T
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        e = np.stack([u - uv[:, 0], v - uv[:, 1]], 1)
        j0 = (K[0][None] - u[:, None] * K[2][None]) / q[:, 2:3]
        j1 = (K[1][None] - v[:, None] * K[2][None]) / q[:, 2:3]
        J = np.stack([np.einsum("nr,nrc->nc", j0, R), np.einsum("nr,nrc->nc", j1, R)], 1)      # (n, 2, 3)
        if fault == "sign_in_J":
            J[:, 0, 0] = -J[:, 0, 0]
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


def refine_point(K, R, t, uv, p0, n_rounds, huber, damping, dt=np.float64, fault=None):
    """one landmark with its observations in key order; p0 float32.  dict(status, point float32, p64, H, cost0, cost1, marginal)"""
    p0 = np.asarray(p0, np.float32)
    p = p0.astype(np.float64)
    out = dict(status=OK, point=p0.copy(), p64=p.copy(), H=np.full((3, 3), np.nan), cost0=0.0, cost1=0.0, marginal=False)
    behind = False
    pf = p0.copy()
    for r in range(n_rounds + 1):
        H, b, cost, z = evaluate(K, R, t, uv, p, huber, dt, fault)
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
        H = H + damping * np.eye(3)
        x = ldlt3_solve(H, b)
        if x is None:
            out["status"] = NOT_FINITE
            return out
        out["H"] = H
        p = p - x
        if r == n_rounds - 1:
            out["p64"] = p.copy()
            with np.errstate(all="ignore"):
                pf = p.astype(np.float32)
            p = pf.astype(np.float64)
        if not np.isfinite(p).all():
            out["status"] = NOT_FINITE
            return out
    if behind:
        out["status"] = BEHIND
    elif out["cost1"] > out["cost0"]:
        out["status"] = COST_ROSE
    if n_rounds > 0 and out["status"] in (OK, COST_ROSE) and abs(out["cost1"] - out["cost0"]) < 1e-6 * abs(out["cost0"]):
        out["marginal"] = True
    if out["status"] == OK and n_rounds > 0:
        out["point"] = pf
    return out


def refine(K, map_pts, map_app, frames, poses, n_rounds=10, min_obs=3, huber_px=0.0, damping=0.0, dtype=np.float64, n_rows=None,
           n_max=None, fault=None, only=None):
    """The whole call.  poses: one 4x4 per frame (p_cam = T p_map), taken as the float32 the device call is given.  Returns
    dict(points (M, 3) float32, status (M,), n_obs (M,), p64 (M, 3), H (M, 3, 3), cost0, cost1 (M,), marginal (M,) bool, stats).
    only: the entries to refine (default all) -- the others keep status -1."""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    pts = np.asarray(map_pts, np.float32).reshape(-1, 3)
    Mn = len(pts)
    T = np.stack([np.asarray(X, np.float32).astype(np.float64).reshape(4, 4) for X in poses])
    lists, n_max, _ = observation_lists(map_app, frames, n_rows, n_max)
    uvs = [np.asarray(uv, np.float32).reshape(-1, 2) for uv, _ in frames]
    res = dict(points=pts.copy(), status=np.full(Mn, -1, np.int32), n_obs=np.zeros(Mn, np.int32), p64=pts.astype(np.float64),
               H=np.full((Mn, 3, 3), np.nan), cost0=np.zeros(Mn), cost1=np.zeros(Mn), marginal=np.zeros(Mn, bool))
    for e in (range(Mn) if only is None else only):
        keys = list(lists.get(e, []))
        res["n_obs"][e] = len(keys)
        if fault == "neighbour_mixed_in" and e + 1 in lists:
            keys = sorted(keys + lists[e + 1][:1])
        if fault == "dropped_observation" and len(keys) > min_obs:
            keys = keys[:-1]
        if len(keys) == 0:
            res["status"][e] = UNSEEN
            continue
        if len(keys) < min_obs:
            res["status"][e] = FEW_OBS
            continue
        f = np.array([k // n_max for k in keys]); i = np.array([k % n_max for k in keys])
        uv = np.stack([uvs[a][b] for a, b in zip(f, i)])
        o = refine_point(K, T[f, :3, :3], T[f, :3, 3], uv, pts[e], n_rounds, float(np.float32(huber_px)), float(np.float32(damping)),
                         dtype, fault)
        res["status"][e] = o["status"]; res["points"][e] = o["point"]; res["p64"][e] = o["p64"]; res["H"][e] = o["H"]
        res["cost0"][e] = o["cost0"]; res["cost1"][e] = o["cost1"]; res["marginal"][e] = o["marginal"]
    ok = res["status"] == OK
    # the device's fixed order: entry e goes to partial sum e mod 1024 in entry order, the partial sums are added in order
    part = np.zeros((1024, 2))
    for e in np.nonzero(ok)[0]:
        part[e % 1024, 0] += res["cost0"][e]; part[e % 1024, 1] += res["cost1"][e]
    c0 = c1 = 0.0
    for t in range(1024):
        c0 += part[t, 0]; c1 += part[t, 1]
    c0, c1 = float(c0), float(c1)
    res["stats"] = dict(n_entries=Mn, n_obs=int(sum(len(v) for v in lists.values())),
                        by_status=[int((res["status"] == s).sum()) for s in range(6)], cost_before=c0, cost_after=c1)
    return res


def h_norm(d, H):
    """sqrt(d^T H d): a point difference in the landmark's own final H, in pixels"""
    d = np.asarray(d, np.float64)
    return float(np.sqrt(max(d @ np.asarray(H, np.float64) @ d, 0.0)))


def example_problem():
    """the example data with its ground-truth poses: dict(K, cam, world_pts, world_app, frames [(uv, app)], poses, ids)"""
    d = M.example_data()
    poses = [np.linalg.inv(g @ d["C"]) for g in d["gt"][: len(d["frames"])]]
    return dict(K=d["K"], cam=d["cam"], world_pts=d["world_pts"], world_app=d["world_app"], frames=[(uv, app) for uv, app, _ in d["frames"]],
                poses=poses, ids=[ids for _, _, ids in d["frames"]])


def perturbed(world_pts, seed=0, amount=0.3):
    return (np.asarray(world_pts, np.float64) + np.random.default_rng(seed).uniform(-amount, amount, (len(world_pts), 3))).astype(np.float32)
