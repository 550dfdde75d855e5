"""NumPy restatement of voe_map_cull* (include/vo_map_cull.h), written from the header's rules, in float64 on the observation
lists of tests/map_refine_restatement.py (R.observation_lists).

The sum of |e|^2 is taken as the header says: observation k of the ordered list in lane k mod 16, a lane's terms in ascending
k, the 16 lanes by the balanced tree ((0+1)+(2+3)) + ((4+5)+(6+7)) ... -- `reverse=True` deals the list out backwards
instead, which is the forward-against-reversed distance of profiles/map_cull_budget.json.  `alt=True` evaluates every
per-observation expression in another order (the matrix products summed z, y, x instead of x, y, z; the ray normalised by a
multiplication with the reciprocal): the spread between the two is what expression order and fused multiply-adds can move.
`fault` plants a mistake, to show that the measures of the tests see it.

BOUNDS.  Next to every statistic the restatement hands out an a-priori bound of its rounding error, first order in
eps = 2^-53, from the magnitudes alone (no value of any implementation under test goes into it):
    p_cam   four roundings on |R| |p| + |t|:                 dpc = 4 eps (|R| |p| + |t|)
    q       four roundings on |K| |p_cam|, plus |K| dpc:     dq  = 4 eps |K| |p_cam| + |K| dpc
    u = q0 / q2 (v alike):                                   du  = (dq0 + |u| dq2) / |q2| + 2 eps |u|
    e = u - uv:                                              de  = du + eps |e|
    |e|^2:                                                   dsq = 2 (|e0| de0 + |e1| de1) + de0^2 + de1^2 + 3 eps |e|^2
    z:                                                       dz  = dpc_z
    d = R^T p_cam:                                           dd  = 4 eps |R|^T |p_cam| + |R|^T dpc
    u_ray = d / |d|:                                         dur = 2 sum(dd) / |d| + 4 eps
    u_k . u_l:                                               dcos = dur_k + dur_l + 4 eps
Two correct implementations lie within TWICE the bound of one another; the mean of n terms adds n eps times the mean."""
import numpy as np

import map_refine_restatement as R

KEPT, UNSEEN, FEW_OBS, FEW_FRAMES, NOT_FINITE, BEHIND, HIGH_ERROR, LOW_PARALLAX = range(8)
VERDICTS = ("KEPT", "UNSEEN", "FEW_OBS", "FEW_FRAMES", "NOT_FINITE", "BEHIND", "HIGH_ERROR", "LOW_PARALLAX")
OK, NOTHING_DROPPED = 0, 1
FAULTS = ("dropped_last_observation", "pairs_k_le_l", "R_for_Rt", "mean_over_16")
EPS = 2.0 ** -53
DEFAULT = dict(min_obs=3, min_frames=2, max_rms_px=2.0, max_err_px=0.0, min_parallax_deg=0.0, drop_unseen=False, dry_run=False)


def lane_tree_sum(terms, reverse=False):
    """the fixed order: 16 lane sums (term k in lane k mod 16, ascending k), then the balanced tree over the lanes"""
    t = np.asarray(terms, np.float64)
    if reverse:
        t = t[::-1]
    lanes = np.zeros(16)
    for k in range(len(t)):
        lanes[k % 16] = lanes[k % 16] + t[k]
    while len(lanes) > 1:
        lanes = lanes[0::2] + lanes[1::2]
    return float(lanes[0])


def observation_terms(K, R_, t, uv, p, alt=False, fault=None):
    """per observation: |e|^2, camera z, the unit ray (n, 3), and the bounds dsq, dz, dur (see the module's docstring)"""
    K, R_, t, uv, p = (np.asarray(x, np.float64) for x in (K, R_, t, uv, p))
    with np.errstate(all="ignore"):
        if alt:
            pc = ((R_[:, :, 2] * p[2] + R_[:, :, 1] * p[1]) + R_[:, :, 0] * p[0]) + t
            q = (pc[:, 2:3] * K[None, :, 2] + pc[:, 1:2] * K[None, :, 1]) + pc[:, 0:1] * K[None, :, 0]
        else:
            pc = np.einsum("nrc,c->nr", R_, p) + t
            q = pc @ K.T
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        e0, e1 = u - uv[:, 0], v - uv[:, 1]
        sq = e1 * e1 + e0 * e0 if alt else e0 * e0 + e1 * e1
        Rd = R_ if fault == "R_for_Rt" else R_.transpose(0, 2, 1)
        if alt:
            d = (Rd[:, :, 2] * pc[:, 2:3] + Rd[:, :, 1] * pc[:, 1:2]) + Rd[:, :, 0] * pc[:, 0:1]
            ray = d * (1.0 / np.sqrt(d[:, 2] * d[:, 2] + d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0]))[:, None]
        else:
            d = np.einsum("nrc,nc->nr", Rd, pc)
            ray = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
        aR = np.abs(R_)
        dpc = 4 * EPS * (np.einsum("nrc,c->nr", aR, np.abs(p)) + np.abs(t))
        dq = 4 * EPS * (np.abs(pc) @ np.abs(K).T) + dpc @ np.abs(K).T
        du = (dq[:, 0] + np.abs(u) * dq[:, 2]) / np.abs(q[:, 2]) + 2 * EPS * np.abs(u) + EPS * np.abs(e0)
        dv = (dq[:, 1] + np.abs(v) * dq[:, 2]) / np.abs(q[:, 2]) + 2 * EPS * np.abs(v) + EPS * np.abs(e1)
        dsq = 2 * (np.abs(e0) * du + np.abs(e1) * dv) + du * du + dv * dv + 3 * EPS * sq
        dd = 4 * EPS * np.einsum("ncr,nc->nr", aR, np.abs(pc)) + np.einsum("ncr,nc->nr", aR, dpc)
        dur = 2 * dd.sum(1) / np.sqrt((d * d).sum(1)) + 4 * EPS
    return sq, pc[:, 2].copy(), ray, dsq, dpc[:, 2], dur


def pair_minimum(ray, alt=False, fault=None):
    """the smallest u_k . u_l over k < l (k <= l under the fault), the dot product summed x, y, z"""
    n = len(ray)
    best = np.inf
    for k in range(n):
        lo = k if fault == "pairs_k_le_l" else k + 1
        if lo >= n:
            continue
        o = ray[lo:]
        dots = (ray[k, 2] * o[:, 2] + ray[k, 1] * o[:, 1]) + ray[k, 0] * o[:, 0] if alt else ray[k, 0] * o[:, 0] + ray[k, 1] * o[:, 1] + ray[k, 2] * o[:, 2]
        best = min(best, float(dots.min()))
    return best


def near(x, thr):
    return abs(x - thr) < 1e-6 * abs(thr)


def cull(K, map_pts, map_app, frames, poses, min_obs=3, min_frames=2, max_rms_px=2.0, max_err_px=0.0, min_parallax_deg=0.0,
         drop_unseen=False, dry_run=False, n_rows=None, n_max=None, reverse=False, alt=False, fault=None):
    """The whole call.  poses: one 4x4 per frame (p_cam = T p_map), taken as the float32 the device call is given.  Returns
    dict(verdict, remap, keep, n_obs, n_frames, mean_sq_px, max_sq_px, min_z, cos_parallax, b_mean, b_max, b_z, b_cos (the
    bounds), marginal (M,) bool, points, app (the map afterwards), stats)."""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    pts = np.asarray(map_pts, np.float32).reshape(-1, 3)
    app = np.asarray(map_app, np.float32).reshape(-1, 10)
    Mn = len(pts)
    T = np.stack([np.asarray(X, np.float32).astype(np.float64).reshape(4, 4) for X in poses])
    lists, n_max, _ = R.observation_lists(app, frames, n_rows, n_max)
    uvs = [np.asarray(uv, np.float32).reshape(-1, 2) for uv, _ in frames]
    thr_mean, thr_max = float(np.float32(max_rms_px)) ** 2, float(np.float32(max_err_px)) ** 2
    parallax = float(np.float32(min_parallax_deg)) > 0
    cos_thr = float(np.cos(float(np.float32(min_parallax_deg)) * np.pi / 180.0)) if parallax else 1.0
    z8, o8 = np.zeros(Mn), np.ones(Mn)
    res = dict(verdict=np.full(Mn, -1, np.int32), n_obs=np.zeros(Mn, np.int32), n_frames=np.zeros(Mn, np.int32), mean_sq_px=z8.copy(),
               max_sq_px=z8.copy(), min_z=z8.copy(), cos_parallax=o8.copy(), b_mean=z8.copy(), b_max=z8.copy(), b_z=z8.copy(), b_cos=z8.copy(),
               marginal=np.zeros(Mn, bool), sum_n_obs_sq=int(sum(len(v) ** 2 for v in lists.values())))
    for e in range(Mn):
        keys = list(lists.get(e, []))
        if fault == "dropped_last_observation" and len(keys) > 1:
            keys = keys[:-1]
        n = len(keys)
        res["n_obs"][e] = n
        if n == 0:
            res["verdict"][e] = UNSEEN
            continue
        f = np.array([k // n_max for k in keys]); i = np.array([k % n_max for k in keys])
        n_fr = 1 + int((f[1:] != f[:-1]).sum())
        res["n_frames"][e] = n_fr
        uv = np.stack([uvs[a][b] for a, b in zip(f, i)])
        sq, z, ray, dsq, dz, dur = observation_terms(K, T[f, :3, :3], T[f, :3, 3], uv, pts[e].astype(np.float64), alt, fault)
        with np.errstate(all="ignore"):
            mean = lane_tree_sum(sq, reverse) / (16 if fault == "mean_over_16" else n)
            mx, mz = float(np.max(sq)), float(np.min(z))
            cosp = pair_minimum(ray, alt, fault) if parallax and n >= 2 else 1.0
        res["mean_sq_px"][e], res["max_sq_px"][e], res["min_z"][e], res["cos_parallax"][e] = mean, mx, mz, cosp
        finite = bool(np.isfinite(sq).all() and np.isfinite(z).all() and np.isfinite(ray).all())
        if finite:
            res["b_mean"][e] = float(dsq.sum()) / n + n * EPS * mean
            res["b_max"][e], res["b_z"][e], res["b_cos"][e] = float(dsq.max()), float(dz.max()), 2 * float(dur.max()) + 4 * EPS
        v = KEPT
        if n < min_obs:
            v = FEW_OBS
        elif n_fr < min_frames:
            v = FEW_FRAMES
        elif not finite:
            v = NOT_FINITE
        elif not mz > 0:
            v = BEHIND
        elif (thr_mean > 0 and mean > thr_mean) or (thr_max > 0 and mx > thr_max):
            v = HIGH_ERROR
        elif parallax and cosp > cos_thr:
            v = LOW_PARALLAX
        res["verdict"][e] = v
        if finite and v in (KEPT, BEHIND, HIGH_ERROR, LOW_PARALLAX):
            m = bool((np.abs(z) < 1e-5).any())
            if v != BEHIND:
                m = m or (thr_mean > 0 and near(mean, thr_mean)) or (thr_max > 0 and near(mx, thr_max))
            if v in (KEPT, LOW_PARALLAX):
                m = m or (parallax and near(cosp, cos_thr))
            res["marginal"][e] = m
    keep = (res["verdict"] == KEPT) | ((res["verdict"] == UNSEEN) & (not drop_unseen))
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    n_kept = int(keep.sum())
    res["keep"], res["remap"] = keep, remap
    changes = n_kept != Mn and not dry_run
    res["points"], res["app"] = (pts[keep].copy(), app[keep].copy()) if changes else (pts.copy(), app.copy())
    res["stats"] = dict(status=OK if n_kept != Mn else NOTHING_DROPPED, n_before=Mn, n_kept=n_kept,
                        n_obs=int(sum(len(v) for v in lists.values())), by_verdict=[int((res["verdict"] == k).sum()) for k in range(8)])
    return res


def parallax_deg(res):
    """the largest angle between two rays of every landmark, in degrees (from cos_parallax)"""
    return np.degrees(np.arccos(np.clip(res["cos_parallax"], -1.0, 1.0)))
