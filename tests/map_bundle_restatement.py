"""NumPy restatement of vox_map_bundle* (include/vo_map_bundle.h), written from the header's rules, in float64.

Observations: the lookup of tests/map_localise_restatement.py through map_pose_refine_restatement.frame_observations -- all
observations in ascending key f * n_max + i, which is a frame's rows in ascending i and, filtered by entry, a landmark's list in
ascending key.  The cost, the residual and both Jacobians are those of tests/map_pose_refine_restatement.py (evaluate: Jc) and
tests/map_refine_restatement.py (evaluate: Jp): `terms` states them per observation, because the coupling W = w Jc^T Jp needs
them side by side, and tests/test_map_bundle_cpu.py holds its sums to the two evaluate functions.  v2t, the 6x6 and 3x3 LDL^T,
the float32 rounding of a pose and the total cost are imported, not restated.

Two solvers for the reduced system: the header's PCG (two passes, never forming S) and `dense`, numpy.linalg.solve on the
explicitly formed S.  `reverse` takes every sum in the reversed order (the budget of the GPU test).  `fault` plants a mistake."""
import numpy as np

import map_pose_refine_restatement as P
import map_refine_restatement as R

OK, NOT_FINITE, BEHIND, NOTHING_FREE, NO_STEP, COST_ROSE = range(6)
POSE_OK, POSE_FIXED, POSE_FEW_OBS = 0, 1, 2
POINT_OK, POINT_UNSEEN, POINT_FEW_OBS = 0, 1, 2
FAULTS = ("sign_in_Jp", "W_transposed_in_pass_B", "dropped_observation", "backsubstitution_without_Wx")
CONTROLS = ("preconditioner_from_U",)                        # not a fault: PCG must still converge to the same step
DEFAULT = dict(n_rounds=3, n_cg=64, cg_tol=1e-8, lambda0=1e-4, min_obs_pose=3, min_obs_point=3, huber_px=0.0)


def terms(K, T, pts, of, oe, uv, huber, fault=None):
    """per observation k (frame of[k], entry oe[k], pixel uv[k]) at the poses T (F, 4, 4) and points pts (M, 3):
    e (n, 2), w (n,), rho (n,), Jc (n, 2, 6) = j [I, -[p_cam]x], Jp (n, 2, 3) = j R, camera z (n,)"""
    with np.errstate(all="ignore"):
        Rm, t = T[of, :3, :3], T[of, :3, 3]
        pc = np.einsum("nrc,nc->nr", Rm, pts[oe]) + t
        q = pc @ K.T
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        e = np.stack([u - uv[:, 0], v - uv[:, 1]], 1)
        j0 = (K[0][None] - u[:, None] * K[2][None]) / q[:, 2:3]
        j1 = (K[1][None] - v[:, None] * K[2][None]) / q[:, 2:3]
        Jc = np.zeros((len(of), 2, 6))
        for k, j in enumerate((j0, j1)):
            Jc[:, k, :3] = j
            Jc[:, k, 3:] = np.cross(pc, j)
        Jp = np.stack([np.einsum("nr,nrc->nc", j0, Rm), np.einsum("nr,nrc->nc", j1, Rm)], 1)
        if fault == "sign_in_Jp":
            Jp[:, :, 0] = -Jp[:, :, 0]
        r2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        w, rho = np.ones_like(r2), r2
        if huber > 0:
            r = np.sqrt(r2)
            out = r > huber
            w = np.where(out, huber / r, 1.0)
            rho = np.where(out, huber * (2 * r - huber), r2)
    return e, w, rho, Jc, Jp, pc[:, 2]


def group_sum(values, group, n_groups, reverse=False):
    """out[g] = the sum of values[k] over group[k] == g, one term after the other in the order of k (or the reversed order)"""
    out = np.zeros((n_groups,) + values.shape[1:])
    if len(values):
        if reverse:
            np.add.at(out, group[::-1], values[::-1])
        else:
            np.add.at(out, group, values)
    return out


def ordered_sum(values, reverse=False):
    s = 0.0
    for v in (values[::-1] if reverse else values):
        s += v
    return float(s)


def inverse_by_ldlt(H, solve):
    """H^-1 column by column by the header's LDL^T; None when a pivot is not > 0"""
    n = len(H)
    cols = []
    for k in range(n):
        x = solve(H, np.eye(n)[k])
        if x is None:
            return None
        cols.append(x)
    return np.stack(cols, 1)


class Problem:
    """the observations of a call and what is free"""

    def __init__(self, K, map_pts, map_app, frames, poses, fixed, min_obs_pose, min_obs_point, n_rows=None, n_max=None):
        self.K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
        self.pts0 = np.asarray(map_pts, np.float32).reshape(-1, 3)
        self.T0 = np.stack([np.asarray(X, np.float32).reshape(4, 4) for X in poses])
        self.F, self.M = len(frames), len(self.pts0)
        obs = P.frame_observations(map_app, frames, n_rows, n_max)
        self.of = np.concatenate([np.full(len(i), f, np.int64) for f, (i, _) in enumerate(obs)] + [np.zeros(0, np.int64)])
        self.oe = np.concatenate([np.asarray(e, np.int64) for _, e in obs] + [np.zeros(0, np.int64)])
        uvs = [np.asarray(uv, np.float32).reshape(-1, 2) for uv, _ in frames]
        self.uv = np.concatenate([uvs[f][i] for f, (i, _) in enumerate(obs)] + [np.zeros((0, 2), np.float32)]).astype(np.float64)
        self.n_obs_f = np.array([len(i) for i, _ in obs], np.int32)
        self.n_obs_p = np.bincount(self.oe, minlength=self.M).astype(np.int32)
        held = np.zeros(self.F, bool) if fixed is None else np.asarray(fixed).astype(bool)
        self.pose_status = np.where(held, POSE_FIXED, np.where(self.n_obs_f < min_obs_pose, POSE_FEW_OBS, POSE_OK)).astype(np.int32)
        self.point_status = np.where(self.n_obs_p == 0, POINT_UNSEEN, np.where(self.n_obs_p < min_obs_point, POINT_FEW_OBS, POINT_OK)).astype(np.int32)
        self.free_f, self.free_p = self.pose_status == POSE_OK, self.point_status == POINT_OK
        self.min_obs_point = min_obs_point

    def cost(self, T, pts, huber, reverse=False):
        """(total cost: per frame in row order, the frames in order; the smallest camera z)"""
        _, _, rho, _, _, z = terms(self.K, T, pts, self.of, self.oe, self.uv, huber)
        per_frame = group_sum(rho, self.of, self.F, reverse)
        return ordered_sum(per_frame, reverse), z


def linearise(pr, T, pts, huber, lam, reverse=False, fault=None):
    """the blocks of one round: dict(U (F, 6, 6) damped, gf, Vinv (M, 3, 3) of the free landmarks, gj, W (n, 6, 3), D, r, bad)"""
    e, w, _, Jc, Jp, _ = terms(pr.K, T, pts, pr.of, pr.oe, pr.uv, huber, fault)
    wJc, wJp = w[:, None, None] * Jc, w[:, None, None] * Jp
    keep = np.ones(len(pr.of), bool)
    if fault == "dropped_observation":                        # the last observation of every landmark that can spare one
        last = {}
        for k, j in enumerate(pr.oe):
            last[int(j)] = k
        for j, k in last.items():
            if pr.n_obs_p[j] > pr.min_obs_point:
                keep[k] = False
    V = group_sum(np.einsum("nka,nkb->nab", wJp, Jp)[keep], pr.oe[keep], pr.M, reverse)
    gj = group_sum(np.einsum("nka,nk->na", wJp, e)[keep], pr.oe[keep], pr.M, reverse)
    U = group_sum(np.einsum("nka,nkb->nab", wJc, Jc), pr.of, pr.F, reverse)
    gf = group_sum(np.einsum("nka,nk->na", wJc, e), pr.of, pr.F, reverse)
    i3, i6 = np.arange(3), np.arange(6)
    V[:, i3, i3] += lam * V[:, i3, i3]
    U[:, i6, i6] += lam * U[:, i6, i6]
    bad = False
    Vinv = np.zeros_like(V)
    for j in np.nonzero(pr.free_p)[0]:
        inv = inverse_by_ldlt(V[j], R.ldlt3_solve) if np.isfinite(V[j]).all() and np.isfinite(gj[j]).all() else None
        if inv is None:
            bad = True
        else:
            Vinv[j] = 0.5 * (inv + inv.T)                      # (the device stores the upper triangle)
    W = np.einsum("nka,nkb->nab", wJc, Jp)                     # (n, 6, 3)
    sel = pr.free_p[pr.oe]
    Y = np.einsum("nab,nbc->nac", W, Vinv[pr.oe])
    D = U - group_sum(np.einsum("nac,nbc->nab", Y, W)[sel], pr.of[sel], pr.F, reverse)
    r = -gf + group_sum(np.einsum("nac,nc->na", Y, gj[pr.oe])[sel], pr.of[sel], pr.F, reverse)
    if fault == "preconditioner_from_U":
        D = U.copy()
    return dict(U=U, gf=gf, V=V, Vinv=Vinv, gj=gj, W=W, D=D, r=r, bad=bad)


def apply_S(pr, L, p, reverse=False, fault=None):
    """S p by the two passes: t_j = V_j^-1 sum over the observations in free frames of W^T p_f; (S p)_f = U_f p_f - sum over the
    rows of free landmarks of W t_j"""
    W = L["W"]
    in_f, in_p = pr.free_f[pr.of], pr.free_p[pr.oe]
    s = group_sum(np.einsum("nac,na->nc", W, p[pr.of])[in_f], pr.oe[in_f], pr.M, reverse)
    t = np.einsum("jab,jb->ja", L["Vinv"], s)
    if fault == "W_transposed_in_pass_B":                     # each 3x3 half of W transposed
        Wb = np.concatenate([W[:, :3].transpose(0, 2, 1), W[:, 3:].transpose(0, 2, 1)], 1)
    else:
        Wb = W
    back = group_sum(np.einsum("nac,nc->na", Wb, t[pr.oe])[in_p], pr.of[in_p], pr.F, reverse)
    q = np.einsum("fab,fb->fa", L["U"], p) - back
    q[~pr.free_f] = 0.0
    return q


def dense_S(pr, L):
    """the reduced camera system formed explicitly over the free frames: (S (6 n, 6 n), the free frames)"""
    ff = np.nonzero(pr.free_f)[0]
    pos = -np.ones(pr.F, np.int64); pos[ff] = np.arange(len(ff))
    S = np.zeros((len(ff), 6, len(ff), 6))
    for a, f in enumerate(ff):
        S[a, :, a, :] = L["U"][f]
    use = pr.free_f[pr.of] & pr.free_p[pr.oe]
    order = np.argsort(pr.oe[use], kind="stable")
    ks = np.nonzero(use)[0][order]
    es = pr.oe[ks]
    for j in np.unique(es):
        k = ks[es == j]
        Wj = L["W"][k]
        blocks = np.einsum("kac,cd,lbd->kalb", Wj, L["Vinv"][j], Wj)
        a = pos[pr.of[k]]
        for x in range(len(k)):
            for y in range(len(k)):
                S[a[x], :, a[y], :] -= blocks[x, :, y, :]
    return S.reshape(6 * len(ff), 6 * len(ff)), ff


def solve_reduced(pr, L, n_cg, cg_tol, solver, reverse=False, fault=None):
    """dict(x (F, 6), iterations, residual, nostep, bad, marginal)"""
    out = dict(x=np.zeros((pr.F, 6)), iterations=0, residual=0.0, nostep=False, bad=False, marginal=False)
    ff = np.nonzero(pr.free_f)[0]
    if len(ff) == 0:
        return out
    Dinv = np.zeros((pr.F, 6, 6))
    for f in ff:
        inv = inverse_by_ldlt(L["D"][f], P.ldlt_solve) if np.isfinite(L["D"][f]).all() and np.isfinite(L["r"][f]).all() else None
        if inv is None:
            out["bad"] = True
            return out
        Dinv[f] = inv
    r = L["r"].copy(); r[~pr.free_f] = 0.0
    if solver == "dense":
        S, ff = dense_S(pr, L)
        x = np.linalg.solve(S, r[ff].ravel()).reshape(-1, 6)
        out["x"][ff] = x
        out["iterations"] = -1
        return out
    dot = lambda a, b: ordered_sum(np.einsum("fa,fa->f", a, b), reverse)
    z = np.einsum("fab,fb->fa", Dinv, r)
    p = z.copy()
    rz, rr0 = dot(r, z), dot(r, r)
    rr = rr0
    x = np.zeros((pr.F, 6))
    for it in range(n_cg):
        q = apply_S(pr, L, p, reverse, fault)
        pSp = dot(p, q)
        if not (pSp > 0 and np.isfinite(pSp)):
            out["nostep"] = it == 0
            break
        alpha = rz / pSp
        x += alpha * p
        r -= alpha * q
        z = np.einsum("fab,fb->fa", Dinv, r)
        rz_new, rr = dot(r, z), dot(r, r)
        out["iterations"] = it + 1
        rel = np.sqrt(rr) / np.sqrt(rr0) if rr0 > 0 else 0.0
        if not np.sqrt(rr) > cg_tol * np.sqrt(rr0):
            out["marginal"] |= bool(rel > 0.5 * cg_tol)
            break
        out["marginal"] |= bool(rel < 2.0 * cg_tol)
        p = z + (rz_new / rz) * p
        rz = rz_new
    out["x"] = x
    out["residual"] = float(np.sqrt(rr / rr0)) if rr0 > 0 else 0.0
    return out


def bundle(K, map_pts, map_app, frames, poses, fixed=None, n_rounds=3, n_cg=64, cg_tol=1e-8, lambda0=1e-4, min_obs_pose=3, min_obs_point=3,
           huber_px=0.0, n_rows=None, n_max=None, solver="pcg", reverse=False, fault=None):
    """The whole call.  Returns dict(status, poses (F, 4, 4) float32, points (M, 3) float32, T64, P64 (the state before it was
    rounded), pose_status, point_status, rounds [dict(cost, cost_candidate, lambda_, residual, cg_iterations, accepted)], stats,
    marginal, U (F, 6, 6) and V (M, 3, 3): the undamped blocks at the final state, the metric of the GPU test's measure)."""
    pr = Problem(K, map_pts, map_app, frames, poses, fixed, min_obs_pose, min_obs_point, n_rows, n_max)
    huber, tol, lam = float(np.float32(huber_px)), float(np.float32(cg_tol)), float(np.float32(lambda0))
    T = pr.T0.astype(np.float64)
    T[:, 3] = (0, 0, 0, 1)
    pts = pr.pts0.astype(np.float64)
    cost0, z0 = pr.cost(T, pts, huber, reverse)
    res = dict(status=OK, poses=pr.T0.copy(), points=pr.pts0.copy(), T64=T.copy(), P64=pts.copy(), pose_status=pr.pose_status,
               point_status=pr.point_status, rounds=[], marginal=bool((np.abs(z0) < 1e-5).any()), problem=pr)
    stats = dict(status=OK, n_frames=pr.F, n_entries=pr.M, n_obs=len(pr.of), n_free_frames=int(pr.free_f.sum()),
                 n_free_points=int(pr.free_p.sum()), n_accepted=0, cost_before=cost0, cost_after=cost0)
    res["stats"] = stats
    if not np.isfinite(cost0):
        stats["status"] = NOT_FINITE
    elif not (z0 > 0).all():
        stats["status"] = BEHIND
    elif not (pr.free_f.any() or pr.free_p.any()):
        stats["status"] = NOTHING_FREE
    if stats["status"] != OK:
        res["status"] = stats["status"]
        res["rounds"] = [dict(cost=0.0, cost_candidate=0.0, lambda_=0.0, residual=0.0, cg_iterations=0, accepted=0)] * n_rounds
        return res
    cur = cost0
    for _ in range(n_rounds):
        L = linearise(pr, T, pts, huber, lam, reverse, fault)
        rec = dict(cost=cur, cost_candidate=0.0, lambda_=lam, residual=0.0, cg_iterations=0, accepted=0)
        formed = not L["bad"]
        if formed:
            s = solve_reduced(pr, L, n_cg, tol, solver, reverse, fault)
            res["marginal"] |= s["marginal"]
            rec["cg_iterations"], rec["residual"] = s["iterations"], s["residual"]
            formed = not (s["bad"] or s["nostep"])
            if s["bad"]:
                rec["residual"] = 0.0
        if formed:
            x = s["x"]
            in_f = pr.free_f[pr.of]
            wx = group_sum(np.einsum("nac,na->nc", L["W"], x[pr.of])[in_f], pr.oe[in_f], pr.M, reverse)
            if fault == "backsubstitution_without_Wx":
                wx[:] = 0.0
            dp = -np.einsum("jab,jb->ja", L["Vinv"], L["gj"] + wx)
            dp[~pr.free_p] = 0.0
            Tc = T.copy()
            for f in np.nonzero(pr.free_f)[0]:
                Tc[f] = P.v2t(x[f]) @ T[f]
            pc = pts + dp
            cand, z = pr.cost(Tc, pc, huber, reverse)
            rec["cost_candidate"] = cand
            accept = bool(np.isfinite(cand) and (z > 0).all() and cand <= cur)
            res["marginal"] |= bool((np.abs(z) < 1e-5).any()) or (np.isfinite(cand) and abs(cand - cur) < 1e-6 * abs(cur))
        else:
            accept = False
        if accept:
            T, pts, cur = Tc, pc, cand
            rec["accepted"] = 1
            stats["n_accepted"] += 1
            if lam > 0:
                lam = max(lam / 10.0, 1e-12)
        else:
            lam = max(10.0 * lam, 1e-6)
        res["rounds"].append(rec)
    res["T64"], res["P64"] = T.copy(), pts.copy()
    Tf = np.stack([P.to_f32_pose(X) for X in T])
    with np.errstate(all="ignore"):
        pf = pts.astype(np.float32)
    final, _ = pr.cost(Tf.astype(np.float64), pf.astype(np.float64), huber, reverse)
    stats["cost_after"] = final
    if n_rounds > 0 and stats["n_accepted"] == 0:
        stats["status"] = NO_STEP
    elif not final <= cost0:
        stats["status"] = COST_ROSE
    if n_rounds > 0 and stats["status"] in (OK, COST_ROSE) and abs(final - cost0) < 1e-6 * abs(cost0):
        res["marginal"] = True
    res["status"] = stats["status"]
    if stats["status"] == OK and stats["n_accepted"] > 0:
        res["poses"] = np.where(pr.free_f[:, None, None], Tf, pr.T0)
        res["points"] = np.where(pr.free_p[:, None], pf, pr.pts0)
    Lf = linearise(pr, T, pts, huber, 0.0)
    res["U"], res["V"] = Lf["U"], Lf["V"]
    return res


def point_norm(d, V):
    """sqrt(d^T V d): a point difference in the landmark's own final V, in pixels"""
    d = np.asarray(d, np.float64)
    return float(np.sqrt(max(d @ np.asarray(V, np.float64) @ d, 0.0)))


def half_ulp_point_px(p_f32, V):
    """half an ulp of each stored float32 coordinate, carried through |V|"""
    u = 0.5 * np.spacing(np.abs(np.asarray(p_f32, np.float32))).astype(np.float64)
    return float(np.sqrt(u @ np.abs(np.asarray(V, np.float64)) @ u))


def distance(a, b):
    """the largest distance of b's state from a's over the free frames (H-norm of the pose difference in a's final U_f) and over
    the free landmarks (in a's final V_j), in pixels: (poses, points).  b: a result of `bundle`, or (poses (F, 4, 4), points)."""
    Tb, pb = (b["T64"], b["P64"]) if isinstance(b, dict) else b
    pr = a["problem"]
    if "U" not in a:                                          # (no round ran: nothing moved)
        return 0.0, 0.0
    dp = max([P.h_norm(P.pose_delta(a["T64"][f], np.asarray(Tb[f], np.float64)), a["U"][f]) for f in np.nonzero(pr.free_f)[0]] + [0.0])
    dq = max([point_norm(np.asarray(pb[j], np.float64) - a["P64"][j], a["V"][j]) for j in np.nonzero(pr.free_p)[0]] + [0.0])
    return dp, dq
