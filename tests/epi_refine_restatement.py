"""float64 numpy restatement of vo_refine_transform, written from the text of include/vo_hip.h alone: the Sampson residual
of a relative pose over 2D-2D pairs, its analytic Jacobian in the 5 parameters (rotation, translation direction on the
sphere), Huber weights, plain Gauss-Newton, the accept rule and the status words.  Test support: no part of the product."""
import numpy as np

OK, FEW_PAIRS, SINGULAR, COST_ROSE, BAD_INPUT, BAD_INDEX = 0, 1, 2, 3, 4, 5
STATUS_NAMES = {0: "OK", 1: "FEW_PAIRS", 2: "SINGULAR", 3: "COST_ROSE", 4: "BAD_INPUT", 5: "BAD_INDEX"}


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def tangent_basis(th):
    """b1 = normalise(th x e_k), k the axis of the smallest |th_k| (lowest k on ties), b2 = th x b1"""
    k = int(np.argmin(np.abs(th)))          # argmin returns the first of equal minima
    e = np.zeros(3)
    e[k] = 1.0
    b1 = np.cross(th, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return b1, np.cross(th, b1)


def rot_exp(w):
    """exp([w]x) = I + A W + B W^2, A = sin(a)/a, B = 2 sin^2(a/2)/a^2 (series below a^2 = 1e-16)"""
    a2 = float(w @ w)
    if a2 < 1e-16:
        A, B = 1.0 - a2 / 6.0, 0.5 - a2 / 24.0
    else:
        a = np.sqrt(a2)
        s = np.sin(0.5 * a)
        A, B = np.sin(a) / a, 2.0 * s * s / a2
    W = skew(w)
    return np.eye(3) + A * W + B * (W @ W)


def fundamental(Kinv, R, th):
    """F = K^-T R^T [th]x^T K^-1: x1^T F x2 = 0 for a true pair (x1 reference pixel, x2 current pixel)"""
    return Kinv.T @ (skew(th) @ R).T @ Kinv


def fundamental_derivatives(Kinv, R, th):
    """dF/d(parameter) at zero: three rotation components (R <- exp([w]x) R), then a and b (th + a b1 + b b2)"""
    b1, b2 = tangent_basis(th)
    dE = [skew(th) @ skew(np.eye(3)[k]) @ R for k in range(3)] + [skew(b1) @ R, skew(b2) @ R]
    return [Kinv.T @ d.T @ Kinv for d in dE]


def sampson(F, x1, x2):
    """(e, s2, a, b): e = x1^T F x2, a = F x2, b = F^T x1, s2 = a0^2 + a1^2 + b0^2 + b1^2; x1, x2 (n, 3) homogeneous"""
    a = x2 @ F.T
    b = x1 @ F
    e = np.einsum("ij,ij->i", x1, a)
    return e, a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2, a, b


def residuals(Kinv, R, th, x1, x2):
    """r (pixels) and the mask of usable pairs (denominator > 0, r finite)"""
    with np.errstate(all="ignore"):
        e, s2, _, _ = sampson(fundamental(Kinv, R, th), x1, x2)
        r = e / np.sqrt(s2)
        ok = (s2 > 0) & np.isfinite(r)
    return np.where(ok, r, 0.0), ok


def jacobian(Kinv, R, th, x1, x2):
    """(r, J (n, 5), ok): analytic d r / d(w0, w1, w2, a, b) at zero"""
    with np.errstate(all="ignore"):
        e, s2, a, b = sampson(fundamental(Kinv, R, th), x1, x2)
        s = np.sqrt(s2)
        r = e / s
        ok = (s2 > 0) & np.isfinite(r)
        J = np.zeros((len(x1), 5))
        for p, G in enumerate(fundamental_derivatives(Kinv, R, th)):
            da = x2 @ G.T
            db = x1 @ G
            de = np.einsum("ij,ij->i", x1, da)
            ds = (a[:, 0] * da[:, 0] + a[:, 1] * da[:, 1] + b[:, 0] * db[:, 0] + b[:, 1] * db[:, 1]) / s
            J[:, p] = (de - r * ds) / s
    return np.where(ok, r, 0.0), np.where(ok[:, None], J, 0.0), ok


def huber_weights(r, huber_px):
    if not huber_px > 0:
        return np.ones_like(r)
    ar = np.abs(r)
    return np.where(ar <= huber_px, 1.0, huber_px / np.where(ar > 0, ar, 1.0))


def apply_step(R, th, d):
    b1, b2 = tangent_basis(th)
    t = th + d[3] * b1 + d[4] * b2
    return rot_exp(np.asarray(d[:3], float)) @ R, t / np.sqrt(t @ t)


def solve_ldlt(H, g):
    """delta with H delta = -g by LDL^T without pivoting; None when a pivot is <= 1e-12 x the largest diagonal of H (or NaN)"""
    n = len(g)
    lim = 1e-12 * np.max(np.diag(H))
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        D[j] = H[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        if not D[j] > lim:
            return None
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / D[j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = -g[i] - sum(L[i, k] * y[k] for k in range(i))
    z = y / D
    x = np.zeros(n)
    for i in reversed(range(n)):
        x[i] = z[i] - sum(L[k, i] * x[k] for k in range(i + 1, n))
    return x


def accumulate(Kinv, R, th, x1, x2, huber_px):
    r, J, ok = jacobian(Kinv, R, th, x1, x2)
    w = huber_weights(r, huber_px) * ok
    return (J * w[:, None]).T @ J, J.T @ (w * r), float(np.sum(w * r * r)), int(ok.sum())


def cost_of(K, X, pairs, p1, p2, huber_px=0.0, mask=None):
    """sum w r^2 of the pose X (4x4) over the (masked) pairs with valid indices"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    if mask is not None:
        pairs = pairs[np.asarray(mask, bool)]
    X = np.asarray(X, np.float64)
    t = X[:3, 3]
    Kinv = np.linalg.inv(np.asarray(K, np.float32).astype(np.float64))
    x1 = np.concatenate([np.asarray(p1, np.float32)[pairs[:, 0]].astype(np.float64), np.ones((len(pairs), 1))], axis=1)
    x2 = np.concatenate([np.asarray(p2, np.float32)[pairs[:, 1]].astype(np.float64), np.ones((len(pairs), 1))], axis=1)
    r, ok = residuals(Kinv, X[:3, :3], t / np.sqrt(t @ t), x1, x2)
    return float(np.sum(huber_weights(r, huber_px) * ok * r * r))


def refine_transform(K, pairs, p1, p2, X_in, n_rounds=10, huber_px=0.0, mask=None, n_live=None):
    """(X_out (4x4 float64, or X_in itself when the refit is not accepted), stats dict).  K: the float camera matrix (3x3);
    p1, p2: pixel arrays (float32 values); pairs: (n, 2) indices; mask: one flag per position or None; n_live: live count
    or None (all)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    p1 = np.asarray(p1, np.float32).reshape(-1, 2)
    p2 = np.asarray(p2, np.float32).reshape(-1, 2)
    n = len(pairs) if n_live is None else max(0, min(int(n_live), len(pairs)))
    pairs = pairs[:n]
    take = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1)[:n].astype(bool)
    unmarked = int(n - take.sum())
    pairs = pairs[take]
    good = (pairs[:, 0] >= 0) & (pairs[:, 0] < len(p1)) & (pairs[:, 1] >= 0) & (pairs[:, 1] < len(p2))
    n_bad = int((~good).sum())
    pairs = pairs[good]
    x1 = np.concatenate([p1[pairs[:, 0]].astype(np.float64), np.ones((len(pairs), 1))], axis=1)
    x2 = np.concatenate([p2[pairs[:, 1]].astype(np.float64), np.ones((len(pairs), 1))], axis=1)
    Kinv = np.linalg.inv(np.asarray(K, np.float32).astype(np.float64))
    X_in = np.asarray(X_in)
    R = X_in[:3, :3].astype(np.float64)
    t = X_in[:3, 3].astype(np.float64)
    tn = float(np.sqrt(t @ t))
    bad_input = not (np.isfinite(tn) and tn > 0)
    with np.errstate(all="ignore"):
        th = t / tn
    H, g, cost0, used0 = accumulate(Kinv, R, th, x1, x2, huber_px)
    stats = dict(status=OK, rounds=0, n_used=used0, n_skipped=len(pairs) - used0 + unmarked, n_bad=n_bad,
                 cost_before=cost0, cost_after=cost0)
    if n_bad:
        stats["status"] = BAD_INDEX
    elif bad_input:
        stats["status"] = BAD_INPUT
    elif used0 < 8:
        stats["status"] = FEW_PAIRS
    if stats["status"] != OK:
        return X_in, stats
    cost, used = cost0, used0
    for _ in range(int(n_rounds)):
        d = solve_ldlt(H, g)
        if d is None:
            stats["status"] = SINGULAR
            return X_in, stats
        R, th = apply_step(R, th, d)
        stats["rounds"] += 1
        H, g, cost, used = accumulate(Kinv, R, th, x1, x2, huber_px)
    if used != used0 or not cost <= cost0:
        stats["status"] = COST_ROSE
        return X_in, stats
    stats["cost_after"] = cost
    X = np.eye(4)
    X[:3, :3] = R
    X[:3, 3] = tn * th
    return X, stats


def pose_errors(X, X_gt):
    """(rotation angle, angle between the translation directions) in radians"""
    X, X_gt = np.asarray(X, np.float64), np.asarray(X_gt, np.float64)
    dR = X[:3, :3] @ X_gt[:3, :3].T
    # atan2(sin, cos): an arccos alone cannot resolve angles below ~1e-4 when an input was rounded to float
    s = 0.5 * np.sqrt((dR[2, 1] - dR[1, 2]) ** 2 + (dR[0, 2] - dR[2, 0]) ** 2 + (dR[1, 0] - dR[0, 1]) ** 2)
    rot = float(np.arctan2(s, (np.trace(dR) - 1.0) / 2.0))
    a, b = X[:3, 3], X_gt[:3, 3]
    return rot, float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))
