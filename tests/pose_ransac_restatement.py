"""Float64 NumPy restatement of vo_estimate_pose_ransac (include/vo_hip.h): the 4-of-64 sample rule, Grunert's P3P with the
4th sample choosing among the solutions, reprojection scoring behind Camera::projectPoint's gates and the selection -- written
from the header, independently of pose_ransac.hip (the quartic's roots come from np.roots, the companion matrix, and R, t
from a least-squares (Kabsch) alignment instead of the kernel's closed form and triads) -- plus the Gauss-Newton PICP of
tests/np_restatement.py that the CPU tests run after it."""
import numpy as np

import np_restatement as NR
import ransac_restatement as RR


def samples4(seed, n_hyp, n):
    """(idx (n_hyp, 4), valid (n_hyp,)): the first 4 distinct of draw(h, 0..63)"""
    d = RR.draws(seed, n_hyp, n)
    idx = np.zeros((n_hyp, 4), np.int64)
    valid = np.zeros(n_hyp, bool)
    for h in range(n_hyp):
        _, first = np.unique(d[h], return_index=True)
        first = np.sort(first)
        if len(first) >= 4:
            idx[h] = d[h, first[:4]]
            valid[h] = True
    return idx, valid


def bearings(K, uv):
    iK = np.linalg.inv(np.asarray(K, np.float32).astype(np.float64))
    b = np.concatenate([np.asarray(uv, np.float64).reshape(-1, 2), np.ones((len(uv), 1))], 1) @ iK.T
    return b / np.linalg.norm(b, axis=1)[:, None]


def grunert_coefficients(P, j):
    """A4..A0 of Grunert's quartic in v (Haralick et al. 1994) and the quantities u(v), s1(v) need"""
    a2 = np.sum((P[1] - P[2]) ** 2); b2 = np.sum((P[0] - P[2]) ** 2); c2 = np.sum((P[0] - P[1]) ** 2)
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    amc, apc = (a2 - c2) / b2, (a2 + c2) / b2
    A = np.array([
        (amc - 1) ** 2 - 4 * c2 / b2 * ca ** 2,
        4 * (amc * (1 - amc) * cb - (1 - apc) * ca * cg + 2 * c2 / b2 * ca ** 2 * cb),
        2 * (amc ** 2 - 1 + 2 * amc ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2 - 4 * apc * ca * cb * cg + 2 * (b2 - a2) / b2 * cg ** 2),
        4 * (-amc * (1 + amc) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - apc) * ca * cg),
        (1 + amc) ** 2 - 4 * a2 / b2 * cg ** 2])
    return A, dict(b2=b2, amc=amc, ca=ca, cb=cb, cg=cg)


def kabsch(P, Q):
    """R, t minimising |R P + t - Q| (rows are points)"""
    cp, cq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - cq).T @ (P - cp))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, cq - R @ cp


def p3p(K, P, uv):
    """every solution of the three world points P (3, 3) seen at uv (3, 2): list of (v, R, t)"""
    P = np.asarray(P, np.float64)
    j = bearings(K, uv)
    A, g = grunert_coefficients(P, j)
    if not np.all(np.isfinite(A)) or A[0] == 0:
        return []
    out = []
    for r in np.roots(A):
        if abs(r.imag) > 1e-7 * max(1.0, abs(r.real)):
            continue
        v = r.real
        u = ((g["amc"] - 1) * v * v - 2 * g["amc"] * g["cb"] * v + 1 + g["amc"]) / (2 * (g["cg"] - v * g["ca"]))
        s1sq = g["b2"] / (1 + v * v - 2 * v * g["cb"])
        if not (v > 0 and u > 0 and s1sq > 0 and np.isfinite(u) and np.isfinite(s1sq)):
            continue
        s1 = np.sqrt(s1sq)
        Q = np.stack([s1 * j[0], u * s1 * j[1], v * s1 * j[2]])
        R, t = kabsch(P, Q)
        out.append((v, R, t))
    return out


def degenerate(P):
    e12, e13 = P[1] - P[0], P[2] - P[0]
    return not np.linalg.norm(np.cross(e12, e13)) > 1e-9 * np.linalg.norm(e12) * np.linalg.norm(e13)


def hypothesis(K, world4, uv4, n_solutions=False):
    """the hypothesis of one 4-point sample: (R, t) in float64, or None when invalid (n_solutions: also the number of
    admissible solutions the 4th point chose among)"""
    world4 = np.asarray(world4, np.float64)
    if degenerate(world4[:3]):
        return (None, 0) if n_solutions else None
    K64 = np.asarray(K, np.float32).astype(np.float64)
    best, sols = None, p3p(K, world4[:3], uv4[:3])
    for v, R, t in sols:
        q = R @ world4[3] + t
        h = K64 @ q
        err = np.sum((h[:2] / h[2] - uv4[3]) ** 2) if q[2] > 0 else np.inf
        if not np.isfinite(err) and err != np.inf:
            err = np.inf
        if best is None or err < best[0] or (err == best[0] and v < best[1]):
            best = (err, v, R, t)
    r = None if best is None else (best[2], best[3])
    return (r, len(sols)) if n_solutions else r


def hypotheses(K, world, meas, pairs, n_hyp, seed):
    """(poses (n_hyp, 4, 4) rounded to float32 then widened, valid (n_hyp,), sample indices (n_hyp, 4))"""
    pairs = np.asarray(pairs, np.int64)
    idx, valid = samples4(seed, n_hyp, len(pairs))
    T = np.tile(np.eye(4), (n_hyp, 1, 1))
    for h in np.nonzero(valid)[0]:
        p = pairs[idx[h]]
        r = hypothesis(K, np.asarray(world, np.float64)[p[:, 1]], np.asarray(meas, np.float64)[p[:, 0]])
        if r is None:
            valid[h] = False
            continue
        T[h, :3, :3], T[h, :3, 3] = r
    return T.astype(np.float32).astype(np.float64), valid, idx


def hypotheses_at(K, world, meas, pairs, hs, n_hyp, seed):
    """hypotheses() restated for the hypotheses hs of n_hyp only: (poses (len(hs), 4, 4), valid, sample indices, number of
    admissible solutions) -- equal to hypotheses()[.][hs]"""
    pairs = np.asarray(pairs, np.int64)
    hs = np.asarray(hs, np.int64)
    assert hs.min() >= 0 and hs.max() < n_hyp
    d = RR.draws(seed, n_hyp, len(pairs))[hs]
    idx = np.zeros((len(hs), 4), np.int64)
    valid = np.zeros(len(hs), bool)
    nsol = np.zeros(len(hs), np.int64)
    T = np.tile(np.eye(4), (len(hs), 1, 1))
    for k in range(len(hs)):
        _, first = np.unique(d[k], return_index=True)
        first = np.sort(first)
        if len(first) < 4:
            continue
        idx[k] = d[k, first[:4]]
        p = pairs[idx[k]]
        r, nsol[k] = hypothesis(K, np.asarray(world, np.float64)[p[:, 1]], np.asarray(meas, np.float64)[p[:, 0]], True)
        if r is not None:
            valid[k] = True
            T[k, :3, :3], T[k, :3, 3] = r
    return T.astype(np.float32).astype(np.float64), valid, idx, nsol


def sq_errors(K, T, world, meas, pairs, rows, cols, z_near, z_far):
    """the squared reprojection error of every pair under one pose, +inf where Camera::projectPoint's gates fail and NaN
    where the error is NaN: (n,)"""
    pairs = np.asarray(pairs, np.int64)
    _, uv_ok, pc, uv = _project(K, T, np.asarray(world, np.float64)[pairs[:, 1]], rows, cols, z_near, z_far)
    e = uv - np.asarray(meas, np.float64)[pairs[:, 0]]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(uv_ok, (e * e).sum(1), np.inf)


def error_bands(K, T, world, meas, pairs, thr_px, delta, rows, cols, z_near, z_far):
    """for one pose: (exact count, lower bound, upper bound) -- the pairs inside the gates with e^2 < thr^2, < thr^2 (1 - delta)
    and < thr^2 (1 + delta)"""
    e2 = sq_errors(K, T, world, meas, pairs, rows, cols, z_near, z_far)
    thr2 = float(thr_px) ** 2
    with np.errstate(invalid="ignore"):
        return tuple(int((e2 < thr2 * f).sum()) for f in (1.0, 1.0 - delta, 1.0 + delta))


def inliers(K, T, world, meas, pairs, thr_px, rows, cols, z_near, z_far):
    """the scoring predicate for one pose: (n,) bool"""
    pairs = np.asarray(pairs, np.int64)
    _, uv_ok, pc, uv = _project(K, T, np.asarray(world, np.float64)[pairs[:, 1]], rows, cols, z_near, z_far)
    e = uv - np.asarray(meas, np.float64)[pairs[:, 0]]
    with np.errstate(invalid="ignore"):
        return uv_ok & ((e * e).sum(1) < float(thr_px) ** 2)


def _project(K, T, pw, rows, cols, z_near, z_far):
    K = np.asarray(K, np.float32).astype(np.float64)
    pc = pw @ T[:3, :3].T + T[:3, 3]
    ph = pc @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = ph[:, :2] / ph[:, 2:3]
    ok = ~((pc[:, 2] > z_far) | (pc[:, 2] < z_near))
    ok &= ~((uv[:, 0] < 0) | (uv[:, 0] > cols - 1) | (uv[:, 1] < 0) | (uv[:, 1] > rows - 1))
    return None, ok, pc, uv


def ransac(K, world, meas, pairs, thr_px=2.0, n_hyp=2048, seed=0, rows=480, cols=640, z_near=0, z_far=10):
    """(counts (-1 invalid), winner, mask, T_winner) -- the winner is the first maximum (ties to the lowest h)"""
    T, valid, _ = hypotheses(K, world, meas, pairs, n_hyp, seed)
    counts = np.full(n_hyp, -1, np.int64)
    for h in np.nonzero(valid)[0]:
        counts[h] = int(inliers(K, T[h], world, meas, pairs, thr_px, rows, cols, z_near, z_far).sum())
    win = int(np.argmax(counts))
    if counts[win] < 0:
        return counts, -1, np.zeros(len(pairs), bool), np.eye(4)
    return counts, win, inliers(K, T[win], world, meas, pairs, thr_px, rows, cols, z_near, z_far), T[win]


def picp(K, T0, world, meas, pairs, thr=10000.0, n_iters=50, rows=480, cols=640, z_near=0, z_far=10):
    """Gauss-Newton PICP (PICPSolver::oneRound restated, keep_outliers = false) from T0: the final pose"""
    T, _ = NR.solve(K, T0, world, meas, np.asarray(pairs, np.int64), n_iters, thr, False, rows, cols, z_near, z_far)
    return T


def pose_errors(T, T_ref):
    """(rotation angle between the two, rad; |t - t_ref|)"""
    T, T_ref = np.asarray(T, np.float64), np.asarray(T_ref, np.float64)
    c = (np.trace(T[:3, :3].T @ T_ref[:3, :3]) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1))), float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3]))


def tracking_problem(vo, n, seed=2001, noise_px=0.5, frac=0.0, max_angle=0.05, max_t=0.1, corrupt_seed=1):
    """synth.frame_pair as a 2D-3D problem: world = the model points (reference frame), meas = the current image, pairs
    (cur_idx, model_idx), a fraction `frac` of the model indices replaced at random.  Returns (fp, world, meas, pairs, bad)."""
    fp = vo.synth.frame_pair(n, seed=seed, noise_px=noise_px, max_angle=max_angle, max_t=max_t)
    model_of_ref = np.full(len(fp["ref_pts"]), -1, np.int64)
    model_of_ref[fp["model_pairs"][:, 0]] = fp["model_pairs"][:, 1]
    gm = fp["gt_matches"]
    keep = model_of_ref[gm[:, 0]] >= 0
    clean = np.stack([gm[keep, 1], model_of_ref[gm[keep, 0]]], 1).astype(np.int32)
    rng = np.random.default_rng(corrupt_seed)
    pairs = clean.copy()
    hit = rng.uniform(size=len(pairs)) < frac
    pairs[hit, 1] = rng.integers(0, len(fp["model"]), int(hit.sum()))
    bad = pairs[:, 1] != clean[:, 1]
    return fp, fp["model"], fp["cur_pts"], pairs, bad, clean


# ---- constructed minimal problems (geometries random samples never reach) ---------------------------------------------------
K_WIDE = np.array([[100.0, 0.0, 320.0], [0.0, 100.0, 240.0], [0.0, 0.0, 1.0]], np.float32)     # +-73 degrees across 640 px


def _pixels(K, Q):
    h = np.asarray(Q, np.float64) @ np.asarray(K, np.float64).T
    return (h[:, :2] / h[:, 2:3]).astype(np.float32)


def quartic_terms(K, world4, uv4):
    """Grunert's quartic of the sample's first three points, its depressed form's p, q, r (Ferrari: x = v + B/4) and the
    roots' (real parts, imaginary parts) -- what the constructed cases claim properties of"""
    A, _ = grunert_coefficients(np.asarray(world4, np.float64)[:3], bearings(K, np.asarray(uv4)[:3]))
    B, C, D, E = A[1] / A[0], A[2] / A[0], A[3] / A[0], A[4] / A[0]
    p = C - 3 * B * B / 8
    q = D - B * C / 2 + B ** 3 / 8
    r = E - B * D / 4 + B * B * C / 16 - 3 * B ** 4 / 256
    roots = np.roots(A)
    return dict(A=A, p=p, q=q, r=r, scale=max(abs(p), abs(r), 1.0), re=roots.real, im=roots.imag)


def constructed(name):
    """one 4-point sample: (K, world4 (4, 3) float32, uv4 (4, 2) float32).  World = camera frame (T = identity) unless said.
      collinear_above / collinear_below  |(P2-P1) x (P3-P1)| = (1 +- 1e-3) 1e-9 |P2-P1| |P3-P1|, exactly in double
      danger_cylinder                    the camera centre on the cylinder through the triangle's circumcircle: a double root
      near_cylinder                      the centre 1e-4 of the radius outside it: two roots close together
      biquadratic                        K_WIDE and bearings with j3 . j1 = j3 . j2 = 0 to rounding: A3 = A1 = 0, q = 0
      tie_behind                         a 4th point behind the camera under every solution: +inf each, the smaller v wins
      behind_one                         a 4th point behind the camera under one solution and in front under another"""
    K = np.array([[180.0, 0.0, 320.0], [0.0, 180.0, 240.0], [0.0, 0.0, 1.0]], np.float32)      # synth.K_REF
    if name in ("collinear_above", "collinear_below"):
        f = 1 + 1e-3 if name == "collinear_above" else 1 - 1e-3
        dy = np.float32(2e-9 * f)            # e12 = (1, 0, 0), e13 = (2, dy, 0): |cross| = dy, |e12| |e13| = 2 in double
        W = np.array([[-1, 0, 5], [0, 0, 5], [1, dy, 5], [0.3, -0.4, 6]], np.float32)
        return K, W, _pixels(K, W)
    if name in ("danger_cylinder", "near_cylinder"):
        rad, th = 1.5, np.radians([0.0, 100.0, 220.0])
        W = np.array([[rad * np.cos(a), rad * np.sin(a), 5.0] for a in th] + [[0.3, -0.2, 6.0]], np.float32)
        k = 1.0 if name == "danger_cylinder" else 1.0 + 1e-4
        C = np.array([rad * k * np.cos(np.radians(300.0)), rad * k * np.sin(np.radians(300.0)), 0.0])
        return K, W, _pixels(K, W.astype(np.float64) - C)
    if name == "biquadratic":
        K = K_WIDE
        uv = np.array([[220, 240], [320, 140], [420, 340], [330, 250]], np.float32)
        Q = bearings(K, uv) * np.array([3.0, 4.0, 5.0, 4.0])[:, None]
        return K, Q.astype(np.float32), uv
    if name in ("tie_behind", "behind_one"):
        W = np.array([[-1.0, -0.5, 4.0], [1.2, -0.3, 5.0], [0.1, 0.9, 4.5]], np.float32)
        uv = _pixels(K, W)
        sols = p3p(K, W, uv)
        (_, Ra, ta), (_, Rb, tb) = sols[0], sols[1]
        rng = np.random.default_rng(0)
        for _ in range(100000):
            X = rng.uniform(-8, 8, 3).astype(np.float32).astype(np.float64)
            za, zb = (Ra @ X + ta)[2], (Rb @ X + tb)[2]
            if za < -0.5 and (zb < -0.5 if name == "tie_behind" else zb > 0.5):
                break
        h = np.asarray(K, np.float64) @ (Ra @ X + ta)
        return K, np.vstack([W, X]).astype(np.float32), np.vstack([uv, h[:2] / h[2]]).astype(np.float32)
    raise KeyError(name)


def embedded(K, world4, uv4, seed, n=12, rows=480, cols=640):
    """an n-pair problem whose hypothesis 0 (of 1, seed) draws the sample in its order, the other pairs inliers of the
    restatement's hypothesis of it (or of the identity when it is invalid), inside the image: (world, meas, pairs)"""
    idx = samples4(seed, 1, n)[0][0]
    r = hypothesis(K, world4, uv4)
    R_, t_ = (np.eye(3), np.zeros(3)) if r is None else r
    rng = np.random.default_rng(seed)
    world = np.zeros((n, 3), np.float32)
    meas = np.zeros((n, 2), np.float32)
    rest = [i for i in range(n) if i not in idx]
    Q = np.stack([rng.uniform(-0.6, 0.6, len(rest)), rng.uniform(-0.5, 0.5, len(rest)), np.ones(len(rest))], 1)
    Q *= rng.uniform(2, 8, len(rest))[:, None]
    world[rest] = ((Q - t_) @ R_).astype(np.float32)                      # R^T (Q - t)
    meas[rest] = _pixels(K, world[rest].astype(np.float64) @ R_.T + t_)
    world[idx], meas[idx] = world4, uv4
    return world, meas, np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
