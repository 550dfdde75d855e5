"""NumPy restatement of voe_map_grow* (include/vo_map_grow.h), written from the header's rules, in float64: the open rows, the
tracks and their order, the linear point with its nine sums in the lane / tree order (Q.lane_tree_sum), the rounds
(map_refine_restatement's evaluate and LDL^T, started at the double point), the score (map_cull_restatement's terms, sums and
pair minimum), verdicts, ranks, rows, statistics and the map afterwards (an update of the added rows).

`reverse=True` deals every ordered list out backwards: the forward-against-reversed distance is the spread that
profiles/map_grow_budget.json records.  `fault` plants a mistake, to show that the measures of the tests see it.

THE A-PRIORI BOUND OF THE POINT (b_point), first order in eps = 2^-53, from magnitudes and the conditioning of the data alone
(no value of any implementation under test goes into it):
    m = K^-1 (u, v, 1)      three roundings per entry on |K^-1| |(u, v, 1)|
    d = R^T m, c = -R^T t   three roundings each on |R|^T |m| and |R|^T |t|, plus the carried error of m
    u = d / |d|             |d| and the division: every entry of u is good to 8 eps (|u| <= 1), relative to the unit length,
                            once the error of d (at most 8 eps |d| with |R| <= 1 entrywise and rows of unit length) is in
    I - u u^T               entries at most 1 in size: 2 * 8 eps + 2 eps <= 20 eps each
    (I - u u^T) c           |c| (20 eps + 4 eps), the 4 eps being c's own
    a sum of n terms        in ANY order adds at most n eps times the sum of the terms' sizes
so that dA <= (20 + n) eps n entrywise and db <= (24 + n) eps sum |c_k| entrywise.  The solve p = A^-1 b moves by
    |dp| <= |A^-1| (sqrt(3) db + 3 dA |p|) + 10 eps cond(A) |p|,        |A^-1| = 1 / lambda_min(A), cond = lambda_max / lambda_min
(the last term: the LDL^T's own backward error).  A refined point has the error of its LAST step instead -- Gauss-Newton
forgets the start to second order: |dp| <= |H^-1| sum_k |J_k| (du_k + dv_k) * 4 + 10 eps cond(H) |p| with du, dv the cull's bounds
of a projected pixel (map_cull_restatement's docstring) and H the last round's.  Two correct implementations lie within TWICE the
bound of one another.  The stored point is the float32 nearest to that double.  Where some coordinate lies within MARGIN times
the bound of the midpoint of two neighbouring float32 (`rounding`), two correct implementations may store either neighbour;
elsewhere both store the same bits, and the score (taken from the stored point) has the cull's bounds.  `marginal` is about the
decisions: a threshold comparison, a camera z, a pivot or the acceptance of a refined point that rounding could flip."""
import numpy as np

import map_cull_restatement as Q
import map_localise_restatement as M
import map_refine_restatement as R

ADDED, FEW_OBS, FEW_FRAMES, DEGENERATE, NOT_FINITE, BEHIND, HIGH_ERROR, LOW_PARALLAX, NO_ROOM = range(9)
VERDICTS = ("ADDED", "FEW_OBS", "FEW_FRAMES", "DEGENERATE", "NOT_FINITE", "BEHIND", "HIGH_ERROR", "LOW_PARALLAX", "NO_ROOM")
OK, NO_OPEN_ROWS, NOTHING_ADDED = 0, 1, 2
STATUS = ("OK", "NO_OPEN_ROWS", "NOTHING_ADDED")
assert (NOT_FINITE, BEHIND, HIGH_ERROR, LOW_PARALLAX) == (Q.NOT_FINITE, Q.BEHIND, Q.HIGH_ERROR, Q.LOW_PARALLAX)
FAULTS = ("centre_of_the_next_lane", "tracks_by_last_key", "rounded_before_the_rounds")
EPS = 2.0 ** -53
MARGIN = 8.0                                                  # how many bounds a stored coordinate keeps away from rounding the other way
DEFAULT = dict(n_rounds=5, min_obs=3, min_frames=3, huber_px=0.0, damping=0.0, max_rms_px=2.0, max_err_px=0.0, min_parallax_deg=2.0,
               max_added=0, dry_run=False)


def open_rows(map_app, frames, n_rows=None, n_max=None):
    """(codes (F, n_max) int: 0 open, -1 not live, -2 NaN appearance, -3 a hit; hits (F, n_max) the map's entry or -1; n_max)"""
    _, n_max, ents = R.observation_lists(map_app, frames, n_rows, n_max)
    F = len(frames)
    code, hit = np.full((F, max(n_max, 0)), -1, np.int64), np.full((F, max(n_max, 0)), -1, np.int32)
    for f, (_, app) in enumerate(frames):
        app = np.asarray(app, np.float32).reshape(-1, 10)
        live = len(app) if n_rows is None else max(0, min(int(n_rows[f]), len(app), n_max))
        for i in range(min(live, n_max)):
            if np.isnan(app[i]).any():
                code[f, i] = -2
            elif ents[f][i] >= 0:
                code[f, i], hit[f, i] = -3, ents[f][i]
            else:
                code[f, i] = 0
    return code, hit, n_max


def tracks_of(code, frames, n_max, fault=None):
    """[ascending keys] per track, numbered by ascending smallest key (by LAST key under the fault)"""
    cls = {}
    for f, i in zip(*np.nonzero(code == 0)):
        cls.setdefault(M._key(np.asarray(frames[f][1], np.float32).reshape(-1, 10)[i]), []).append(int(f) * n_max + int(i))
    lists = list(cls.values())                                # (np.nonzero walks in key order: the lists are ascending)
    lists.sort(key=(lambda v: v[-1]) if fault == "tracks_by_last_key" else (lambda v: v[0]))
    return lists


def linear_point(Kinv, R_, t, uv, reverse=False, fault=None):
    """(p or None, A (3, 3), the a-priori bound, degenerate) from the nine sums in the lane / tree order"""
    n = len(uv)
    with np.errstate(all="ignore"):
        m = np.concatenate([uv, np.ones((n, 1))], 1) @ Kinv.T
        d = np.einsum("ncr,nc->nr", R_, m)
        c = -np.einsum("ncr,nc->nr", R_, t)
        if fault == "centre_of_the_next_lane":
            c = np.roll(c, -1, axis=0)
        nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        u = d / nrm[:, None]
        uc = u[:, 0] * c[:, 0] + u[:, 1] * c[:, 1] + u[:, 2] * c[:, 2]
        terms = [1.0 - u[:, 0] * u[:, 0], -(u[:, 0] * u[:, 1]), -(u[:, 0] * u[:, 2]), 1.0 - u[:, 1] * u[:, 1], -(u[:, 1] * u[:, 2]),
                 1.0 - u[:, 2] * u[:, 2], c[:, 0] - u[:, 0] * uc, c[:, 1] - u[:, 1] * uc, c[:, 2] - u[:, 2] * uc]
        s = [Q.lane_tree_sum(x, reverse) for x in terms]
    A = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    b = np.array(s[6:9])
    if not (np.isfinite(A).all() and np.isfinite(b).all()) or not (nrm > 0).all():
        return None, A, 0.0, True
    p = R.ldlt3_solve(A, b)
    if p is None:
        return None, A, 0.0, True
    lam = np.linalg.eigvalsh(A)
    dA, db = (20 + n) * EPS * n, (24 + n) * EPS * float(np.abs(c).sum())
    pn = float(np.abs(p).max())
    bound = (np.sqrt(3) * db + 3 * dA * pn) / lam[0] + 10 * EPS * (lam[2] / lam[0]) * pn
    return p, A, float(bound), False


def rounds(K, R_, t, uv, p_lin, n_rounds, huber, damping, fault=None):
    """vo_map_refine's rounds from the DOUBLE point: dict(refined, point float32 (when refined), p64, H, cost0, cost1, z_min)"""
    p = np.array(p_lin, np.float64)
    if fault == "rounded_before_the_rounds":
        p = p.astype(np.float32).astype(np.float64)
    out = dict(refined=False, point=None, p64=p.copy(), H=None, cost0=0.0, cost1=0.0, z_min=np.inf)
    if n_rounds <= 0:
        return out
    behind, pf = False, None
    for r in range(n_rounds + 1):
        H, b, cost, z = R.evaluate(K, R_, t, uv, p, huber)
        if not (np.isfinite(H).all() and np.isfinite(b).all() and np.isfinite(cost)):
            return out
        behind = behind or not bool((z > 0).all())
        out["z_min"] = min(out["z_min"], float(np.abs(z).min()))
        if r == 0:
            out["cost0"] = cost
        if r == n_rounds:
            out["cost1"] = cost
            break
        H = H + damping * np.eye(3)
        x = R.ldlt3_solve(H, b)
        if x is None:
            return out
        out["H"] = H
        p = p - x
        if r == n_rounds - 1:
            out["p64"] = p.copy()
            with np.errstate(all="ignore"):
                pf = p.astype(np.float32)
            p = pf.astype(np.float64)
        if not np.isfinite(p).all():
            return out
    out["refined"] = bool(not behind and not out["cost1"] > out["cost0"])
    out["point"] = pf
    return out


def refined_bound(K, R_, t, uv, p, H):
    """the a-priori bound of a refined point: the error of its last step (see the module's docstring)"""
    sq, z, ray, dsq, dz, dur = Q.observation_terms(K, R_, t, uv, p)
    pc = np.einsum("nrc,c->nr", R_, p) + t
    q = pc @ K.T
    aR = np.abs(R_)
    dpc = 4 * EPS * (np.einsum("nrc,c->nr", aR, np.abs(p)) + np.abs(t))
    dq = 4 * EPS * (np.abs(pc) @ np.abs(K).T) + dpc @ np.abs(K).T
    du = (dq[:, 0] + np.abs(q[:, 0] / q[:, 2]) * dq[:, 2]) / np.abs(q[:, 2]) + 3 * EPS * np.abs(q[:, 0] / q[:, 2])
    dv = (dq[:, 1] + np.abs(q[:, 1] / q[:, 2]) * dq[:, 2]) / np.abs(q[:, 2]) + 3 * EPS * np.abs(q[:, 1] / q[:, 2])
    Jn = np.linalg.norm(K[:2, :2]) / np.abs(q[:, 2])         # |de / dp| up to the rotation
    lam = np.linalg.eigvalsh(H)
    return float(4 * (Jn * (du + dv)).sum() / lam[0] + 10 * EPS * (lam[2] / lam[0]) * np.abs(p).max())


def near_float32_midpoint(p64, bound):
    """whether some coordinate of the double point lies within MARGIN * bound of the midpoint of two neighbouring float32"""
    p64 = np.asarray(p64, np.float64)
    with np.errstate(all="ignore"):
        f = p64.astype(np.float32)
        other = np.where(f.astype(np.float64) > p64, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf)))
        mid = 0.5 * (f.astype(np.float64) + other.astype(np.float64))
    return bool((np.abs(p64 - mid) <= MARGIN * bound).any())


def grow(K, map_pts, map_app, frames, poses, n_rounds=5, min_obs=3, min_frames=3, huber_px=0.0, damping=0.0, max_rms_px=2.0,
         max_err_px=0.0, min_parallax_deg=2.0, max_added=0, dry_run=False, n_rows=None, n_max=None, reverse=False, fault=None):
    """The whole call.  poses: one 4x4 per frame (p_cam = T p_map), taken as the float32 the device call is given.  Returns
    dict(rows (F, n_max) int32, per track: verdict, n_obs, n_frames, entry, first_key, refined, xyz float32 (T, 3), mean_sq_px,
    max_sq_px, min_z, cos_parallax, the bounds b_point, b_mean, b_max, b_z, b_cos, p64 (T, 3), marginal, rounding; keys [list]; points, app
    (the map afterwards); added_rows [(point, appearance row)] in track order; stats)."""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    Kinv = np.linalg.inv(K)
    pts = np.asarray(map_pts, np.float32).reshape(-1, 3)
    app = np.asarray(map_app, np.float32).reshape(-1, 10)
    T = np.stack([np.asarray(X, np.float32).astype(np.float64).reshape(4, 4) for X in poses])
    code, hit, n_max = open_rows(app, frames, n_rows, n_max)
    F = len(frames)
    uvs = [np.asarray(uv, np.float32).reshape(-1, 2) for uv, _ in frames]
    apps = [np.asarray(a, np.float32).reshape(-1, 10) for _, a in frames]
    lists = tracks_of(code, frames, n_max, fault)
    nT = len(lists)
    huber, damp = float(np.float32(huber_px)), float(np.float32(damping))
    thr_mean, thr_max = float(np.float32(max_rms_px)) ** 2, float(np.float32(max_err_px)) ** 2
    parallax = float(np.float32(min_parallax_deg)) > 0
    cos_thr = float(np.cos(float(np.float32(min_parallax_deg)) * np.pi / 180.0)) if parallax else 1.0
    z8 = np.zeros(nT)
    res = dict(verdict=np.zeros(nT, np.int32), n_obs=np.zeros(nT, np.int32), n_frames=np.zeros(nT, np.int32), entry=np.full(nT, -1, np.int32),
               first_key=np.zeros(nT, np.int32), refined=np.zeros(nT, np.int32), xyz=np.zeros((nT, 3), np.float32), mean_sq_px=z8.copy(),
               max_sq_px=z8.copy(), min_z=z8.copy(), cos_parallax=np.ones(nT), b_point=z8.copy(), b_mean=z8.copy(), b_max=z8.copy(),
               b_z=z8.copy(), b_cos=z8.copy(), p64=np.zeros((nT, 3)), marginal=np.zeros(nT, bool), rounding=np.zeros(nT, bool), keys=lists,
               sum_n_obs_sq=int(sum(len(v) ** 2 for v in lists)))
    for t_, keys in enumerate(lists):
        n = len(keys)
        f = np.array([k // n_max for k in keys]); i = np.array([k % n_max for k in keys])
        n_fr = 1 + int((f[1:] != f[:-1]).sum())
        res["n_obs"][t_], res["n_frames"][t_], res["first_key"][t_] = n, n_fr, keys[0]
        if n < min_obs:
            res["verdict"][t_] = FEW_OBS
            continue
        if n_fr < min_frames:
            res["verdict"][t_] = FEW_FRAMES
            continue
        uv = np.stack([uvs[a][b] for a, b in zip(f, i)]).astype(np.float64)
        Rm, tv = T[f, :3, :3], T[f, :3, 3]
        p_lin, A, bound, deg = linear_point(Kinv, Rm, tv, uv, reverse, fault)
        if deg:
            res["verdict"][t_] = DEGENERATE
            continue
        lam = np.linalg.eigvalsh(A)
        marginal = bool(lam[0] < 1e-9 * lam[2])              # a pivot near 0: DEGENERATE could flip
        o = rounds(K, Rm, tv, uv, p_lin, n_rounds, huber, damp, fault)
        chosen = p_lin
        if o["refined"]:
            chosen, bound = o["p64"], refined_bound(K, Rm, tv, uv, o["p64"], o["H"])
            res["refined"][t_] = 1
        if n_rounds > 0 and o["H"] is not None:
            marginal = marginal or abs(o["cost1"] - o["cost0"]) <= 1e-6 * abs(o["cost0"]) or o["z_min"] < 1e-5
        with np.errstate(all="ignore"):
            pf = chosen.astype(np.float32)
        res["xyz"][t_], res["p64"][t_], res["b_point"][t_] = pf, chosen, bound
        res["rounding"][t_] = near_float32_midpoint(chosen, bound)
        sq, z, ray, dsq, dz, dur = Q.observation_terms(K, Rm, tv, uv, pf.astype(np.float64))
        with np.errstate(all="ignore"):
            mean = Q.lane_tree_sum(sq, reverse) / n
            mx, mz = float(np.max(sq)), float(np.min(z))
            cosp = Q.pair_minimum(ray) if parallax and n >= 2 else 1.0
        res["mean_sq_px"][t_], res["max_sq_px"][t_], res["min_z"][t_], res["cos_parallax"][t_] = mean, mx, mz, cosp
        finite = bool(np.isfinite(sq).all() and np.isfinite(z).all() and np.isfinite(ray).all())
        if finite:
            res["b_mean"][t_] = float(dsq.sum()) / n + n * EPS * mean
            res["b_max"][t_], res["b_z"][t_], res["b_cos"][t_] = float(dsq.max()), float(dz.max()), 2 * float(dur.max()) + 4 * EPS
        v = ADDED
        if not finite:
            v = NOT_FINITE
        elif not mz > 0:
            v = BEHIND
        elif (thr_mean > 0 and mean > thr_mean) or (thr_max > 0 and mx > thr_max):
            v = HIGH_ERROR
        elif parallax and cosp > cos_thr:
            v = LOW_PARALLAX
        res["verdict"][t_] = v
        if finite:
            marginal = marginal or bool((np.abs(z) < 1e-5).any())
            if v != BEHIND:
                marginal = marginal or (thr_mean > 0 and Q.near(mean, thr_mean)) or (thr_max > 0 and Q.near(mx, thr_max))
            if v in (ADDED, LOW_PARALLAX):
                marginal = marginal or (parallax and Q.near(cosp, cos_thr))
        res["marginal"][t_] = marginal
    # ranks: NO_ROOM on the tracks behind the first max_added that qualify
    room = int(max_added) if max_added > 0 else max(F * n_max, 1)
    qualify = np.nonzero(res["verdict"] == ADDED)[0]
    n_before = len(pts)
    for g, t_ in enumerate(qualify):
        if g < room:
            res["entry"][t_] = n_before + g
        else:
            res["verdict"][t_] = NO_ROOM
    added = qualify[:room]
    res["added_rows"] = [(res["xyz"][t_].copy(), apps[lists[t_][0] // n_max][lists[t_][0] % n_max].copy()) for t_ in added]
    rows = np.full((F, max(n_max, 0)), -1, np.int32)
    rows[code == -3] = hit[code == -3]
    for t_, keys in enumerate(lists):
        for k in keys:
            rows[k // n_max, k % n_max] = res["entry"][t_] if res["verdict"][t_] == ADDED else -2 - t_
    res["rows"] = rows
    if len(added) and not dry_run:
        res["points"] = np.concatenate([pts, np.stack([r[0] for r in res["added_rows"]])]).astype(np.float32)
        res["app"] = np.concatenate([app, np.stack([r[1] for r in res["added_rows"]])]).astype(np.float32)
    else:
        res["points"], res["app"] = pts.copy(), app.copy()
    n_open = int((code == 0).sum())
    res["stats"] = dict(status=NO_OPEN_ROWS if n_open == 0 else (NOTHING_ADDED if len(added) == 0 else OK), n_live=int((code != -1).sum()),
                        n_hits=int((code == -3).sum()), n_nan=int((code == -2).sum()), n_open=n_open, n_tracks=nT, n_added=int(len(added)),
                        n_before=n_before, n_after=n_before + int(len(added)), by_verdict=[int((res["verdict"] == k).sum()) for k in range(12)])
    return res
