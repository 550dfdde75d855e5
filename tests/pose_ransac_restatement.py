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


def hypothesis(K, world4, uv4):
    """the hypothesis of one 4-point sample: (R, t) in float64, or None when invalid"""
    world4 = np.asarray(world4, np.float64)
    if degenerate(world4[:3]):
        return None
    K64 = np.asarray(K, np.float32).astype(np.float64)
    best = None
    for v, R, t in p3p(K, world4[:3], uv4[:3]):
        q = R @ world4[3] + t
        h = K64 @ q
        err = np.sum((h[:2] / h[2] - uv4[3]) ** 2) if q[2] > 0 else np.inf
        if not np.isfinite(err) and err != np.inf:
            err = np.inf
        if best is None or err < best[0] or (err == best[0] and v < best[1]):
            best = (err, v, R, t)
    return None if best is None else (best[2], best[3])


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
