"""Float64 NumPy restatement of vo_estimate_transform_ransac (include/vo_hip.h): the sampling rule, the minimal 8-point
solve, Sampson scoring and the selection -- written from the header's description, independently of ransac.hip -- plus
the plain 8-point pose (oracle's estimate_fundamental, E = K^T F K, the four candidates, a cheirality count) that the CPU
tests use as the refit."""
import numpy as np

from oracle import vo_pipeline as vp

M64 = 0xFFFFFFFFFFFFFFFF


def splitmix64(x):
    """vectorised over a uint64 array (wrapping arithmetic)"""
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(seed, n_hyp, n):
    """draw(h, j) for h < n_hyp, j < 64: (n_hyp, 64) int64"""
    h = np.arange(n_hyp, dtype=np.uint64)[:, None]
    j = np.arange(64, dtype=np.uint64)[None, :]
    r = splitmix64(np.uint64(int(seed) & M64) ^ ((h << np.uint64(20)) | j)) >> np.uint64(32)
    with np.errstate(over="ignore"):
        return ((r * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def samples(seed, n_hyp, n):
    """(idx (n_hyp, 8), valid (n_hyp,)): the first 8 distinct draws of every hypothesis"""
    d = draws(seed, n_hyp, n)
    idx = np.zeros((n_hyp, 8), np.int64)
    valid = np.zeros(n_hyp, bool)
    for h in range(n_hyp):
        _, first = np.unique(d[h], return_index=True)
        first = np.sort(first)
        if len(first) >= 8:
            idx[h] = d[h, first[:8]]
            valid[h] = True
    return idx, valid


def image_maxima(p):
    """the per-axis maxima normalize() scales an image by: over ALL its points, starting from 0, a value replacing the running
    maximum only when it is larger (so a NaN or a value <= 0 never does) -- float32 (max x, max y)"""
    p = np.asarray(p, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        q = np.where(p > 0, p, np.float32(0))
    return np.float32(q[:, 0].max(initial=0)), np.float32(q[:, 1].max(initial=0))


def normalised(p1, p2, maxima=None):
    """normalize() of both images as the library forms it: float32 maxima over ALL points, x / (max / 2) - 1 in float32
    (maxima: ((mx1, my1), (mx2, my2)) in place of the images' own)"""
    out, T = [], []
    for k, p in enumerate((np.asarray(p1, np.float32), np.asarray(p2, np.float32))):
        m = image_maxima(p) if maxima is None else tuple(np.float32(v) for v in maxima[k])
        mx, my = m[0] / np.float32(2), m[1] / np.float32(2)
        out.append(np.stack([p[:, 0] / mx - np.float32(1), p[:, 1] / my - np.float32(1)], 1).astype(np.float64))
        T.append(np.array([[np.float32(1) / mx, 0, -1], [0, np.float32(1) / my, -1], [0, 0, 1]], np.float64))
    return out[0], out[1], T[0], T[1]


def minimal_fits(pairs, p1, p2, idx, valid, with_conditioning=False):
    """F (n_hyp, 3, 3), unit Frobenius norm, rank 2; valid updated for singular systems (with_conditioning: also s7 / s0 of
    every 8 x 9 system)"""
    a, b, T1, T2 = normalised(p1, p2)
    pairs = np.asarray(pairs, np.int64)
    d1 = np.concatenate([a[pairs[idx, 0]], np.ones(idx.shape + (1,))], -1)          # (H, 8, 3)
    d2 = np.concatenate([b[pairs[idx, 1]], np.ones(idx.shape + (1,))], -1)
    A = np.einsum("hni,hnj->hnij", d1, d2).reshape(len(idx), 8, 9)
    with np.errstate(invalid="ignore"):
        _, s, Vt = np.linalg.svd(np.where(np.isfinite(A), A, 0.0))
        cond = np.where(np.isfinite(A).all((1, 2)), s[:, 7] / s[:, 0], 0.0)
    valid = valid & (s[:, 7] > 1e-12 * s[:, 0]) & np.isfinite(A).all((1, 2))
    Fa = Vt[:, 8].reshape(-1, 3, 3)
    U, s3, Vt3 = np.linalg.svd(Fa)
    s3[:, 2] = 0
    F = T1.T @ (U * s3[:, None, :]) @ Vt3 @ T2
    F /= np.linalg.norm(F.reshape(-1, 9), axis=1)[:, None, None]
    return (F, valid, cond) if with_conditioning else (F, valid)


def sampson_sq(F, pairs, p1, p2):
    """d^2 of every pair under every F: (n_hyp, n)"""
    pairs = np.asarray(pairs, np.int64)
    x1 = np.concatenate([np.asarray(p1, np.float64)[pairs[:, 0]], np.ones((len(pairs), 1))], 1)
    x2 = np.concatenate([np.asarray(p2, np.float64)[pairs[:, 1]], np.ones((len(pairs), 1))], 1)
    Fx2 = np.einsum("hij,nj->hni", F, x2)
    Ftx1 = np.einsum("hji,nj->hni", F, x1)
    e = np.einsum("ni,hni->hn", x1, Fx2)
    den = Fx2[..., 0] ** 2 + Fx2[..., 1] ** 2 + Ftx1[..., 0] ** 2 + Ftx1[..., 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return e * e / den


def ransac(pairs, p1, p2, threshold_px=1.0, n_hyp=2048, seed=0, chunk=256):
    """(counts (-1 invalid), winner, mask of the winner)"""
    pairs = np.asarray(pairs, np.int64)
    idx, valid = samples(seed, n_hyp, len(pairs))
    F, valid = minimal_fits(pairs, p1, p2, idx, valid)
    counts = np.zeros(n_hyp, np.int64)
    thr2 = float(threshold_px) ** 2
    for h0 in range(0, n_hyp, chunk):
        d2 = sampson_sq(F[h0:h0 + chunk], pairs, p1, p2)
        counts[h0:h0 + chunk] = (d2 < thr2).sum(1)
    counts[~valid] = -1
    win = int(np.argmax(counts))                  # first maximum: ties to the lowest h
    mask = sampson_sq(F[win:win + 1], pairs, p1, p2)[0] < thr2
    return counts, win, mask, F


def pose_8point(K, pairs, p1, p2, F=None):
    """plain normalised 8-point fit on all the pairs (or the given F) -> the candidate with the most pairs in front of both
    cameras (X = pose of the first camera in the frame of the second, float64)"""
    pairs = np.asarray(pairs, np.int64)
    if F is None:
        F = vp.estimate_fundamental(pairs, np.asarray(p1, np.float32), np.asarray(p2, np.float32))
    K = np.asarray(K, np.float64)
    E = K.T @ F @ K
    X1, X2 = vp.essential_to_pair(E)
    iK = np.linalg.inv(K)
    d1 = np.concatenate([np.asarray(p1, np.float64)[pairs[:, 0]], np.ones((len(pairs), 1))], 1) @ iK.T
    d2 = np.concatenate([np.asarray(p2, np.float64)[pairs[:, 1]], np.ones((len(pairs), 1))], 1) @ iK.T
    best, n_best = np.eye(4), -1
    for X in (X1, X2):
        for sgn in (1.0, -1.0):
            R, t = X[:3, :3], sgn * X[:3, 3]
            # R (l1 d1) + t = l2 d2, least squares per pair
            a = d1 @ R.T
            aa, bb, ab = (a * a).sum(1), (d2 * d2).sum(1), (a * d2).sum(1)
            at, bt = a @ t, d2 @ t
            det = aa * bb - ab * ab
            with np.errstate(divide="ignore", invalid="ignore"):
                l1 = (-at * bb + ab * bt) / det
                l2 = (aa * bt - ab * at) / det
            n = int(((l1 > 0) & (l2 > 0)).sum())
            if n > n_best:
                best, n_best = np.eye(4), n
                best[:3, :3], best[:3, 3] = R, t
    return best


def fundamental(pairs, p1, p2, maxima=None):
    """vp.estimate_fundamental in float64 with the maxima of image_maxima (or the given ones) and the thin SVD of A: the same
    fit at any size, and on images that hold NaN or negative coordinates"""
    pairs = np.asarray(pairs, np.int64)
    m = [image_maxima(p) for p in (p1, p2)] if maxima is None else maxima
    pts, T = [], []
    for p, (mx, my) in zip((p1, p2), m):
        p = np.asarray(p, np.float32).astype(np.float64)
        hx, hy = float(mx) / 2, float(my) / 2
        pts.append(np.stack([p[:, 0] / hx - 1, p[:, 1] / hy - 1], 1))
        T.append(np.array([[1 / hx, 0, -1], [0, 1 / hy, -1], [0, 0, 1]]))
    d1 = np.concatenate([pts[0][pairs[:, 0]], np.ones((len(pairs), 1))], 1)
    d2 = np.concatenate([pts[1][pairs[:, 1]], np.ones((len(pairs), 1))], 1)
    A = np.einsum("ni,nj->nij", d1, d2).reshape(len(pairs), 9)
    Fa = np.linalg.svd(A, full_matrices=len(A) < 9)[2][8].reshape(3, 3)
    U, s, Vt = np.linalg.svd(Fa)
    return T[0].T @ (U @ np.diag([s[0], s[1], 0]) @ Vt) @ T[1]


def estimate_transform(o, K, pairs, p1, p2, maxima=None):
    """vp.estimate_transform (the four candidates of E = K^T F K, the first with the most pairs the oracle triangulates) on
    fundamental()'s F: float32 X"""
    pairs = np.ascontiguousarray(pairs, np.int32)
    F = fundamental(pairs, p1, p2, maxima)
    E = np.asarray(K, np.float64).T @ F @ np.asarray(K, np.float64)
    best, n_best = np.eye(4, dtype=np.float32), 0
    for X in vp.essential_to_pair(E):
        for sgn in (1.0, -1.0):
            Xt = X.copy(); Xt[:3, 3] *= sgn
            Xt = Xt.astype(np.float32)
            n = len(o.triangulate(K, Xt, pairs, np.asarray(p1, np.float32), np.asarray(p2, np.float32), want_pairs=False)[0])
            if n > n_best:
                best, n_best = Xt, n
    return best


def sampson_band(F, pairs, p1, p2, threshold_px, delta, c_float=16):
    """d^2 of every pair under every F (n_hyp, n) and whether it lies in the band around thr^2 where a float evaluation may
    decide either way: |d^2 - thr^2| <= delta thr^2 + c_float 2^-24 (2 |e| S_e + d^2 S_den) / den, S_e the sum of the absolute
    terms of e = x1^T F x2 and S_den that of den's (2 sum |a_k| (|F| |x|)_k) -- the first-order float error of d^2, large for
    a pair near an epipole, where e and den both cancel"""
    pairs = np.asarray(pairs, np.int64)
    x1 = np.concatenate([np.asarray(p1, np.float64)[pairs[:, 0]], np.ones((len(pairs), 1))], 1).T.copy()     # (3, n)
    x2 = np.concatenate([np.asarray(p2, np.float64)[pairs[:, 1]], np.ones((len(pairs), 1))], 1).T.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Fx2, Ftx1 = F @ x2, F.transpose(0, 2, 1) @ x1                                                  # sampson_sq's terms
        aF = np.abs(F)
        sx2, stx1 = aF @ np.abs(x2), aF.transpose(0, 2, 1) @ np.abs(x1)
        e = (x1[None] * Fx2).sum(1)
        s_e = (np.abs(x1)[None] * sx2).sum(1)
        den = Fx2[:, 0] ** 2 + Fx2[:, 1] ** 2 + Ftx1[:, 0] ** 2 + Ftx1[:, 1] ** 2
        s_den = 2 * (np.abs(Fx2[:, 0]) * sx2[:, 0] + np.abs(Fx2[:, 1]) * sx2[:, 1] + np.abs(Ftx1[:, 0]) * stx1[:, 0] +
                     np.abs(Ftx1[:, 1]) * stx1[:, 1])
        d2 = e * e / den
        thr2 = float(threshold_px) ** 2
        band = np.abs(d2 - thr2) <= delta * thr2 + c_float * 2.0 ** -24 * (2 * np.abs(e) * s_e + d2 * s_den) / den
    return d2, band


def sampson_bands(F, valid, pairs, p1, p2, threshold_px, delta, chunk=64):
    """per hypothesis: (exact count, lower bound, upper bound) -- the pairs with d^2 < thr^2, those below it outside
    sampson_band's band, and those below it or inside the band; -1 for an invalid hypothesis"""
    thr2 = float(threshold_px) ** 2
    out = np.full((3, len(F)), -1, np.int64)
    for h0 in range(0, len(F), chunk):
        d2, band = sampson_band(F[h0:h0 + chunk], pairs, p1, p2, threshold_px, delta)
        with np.errstate(invalid="ignore"):
            below = d2 < thr2
            out[0, h0:h0 + chunk] = below.sum(1)
            out[1, h0:h0 + chunk] = (below & ~band).sum(1)
            out[2, h0:h0 + chunk] = (below | band).sum(1)
    out[:, ~valid] = -1
    return out


def pose_errors(X, X_ref):
    """(rotation angle between the two, rad; angle between the translation directions, rad)"""
    X, X_ref = np.asarray(X, np.float64), np.asarray(X_ref, np.float64)
    c = (np.trace(X[:3, :3].T @ X_ref[:3, :3]) - 1) / 2
    t, tr = X[:3, 3], X_ref[:3, 3]
    ct = t @ tr / (np.linalg.norm(t) * np.linalg.norm(tr))
    return float(np.arccos(np.clip(c, -1, 1))), float(np.arccos(np.clip(ct, -1, 1)))


def corrupt(pairs, n2, frac, seed=1):
    """a copy of the pairs with `frac` of the second indices replaced at random; returns (pairs, corrupted?)"""
    rng = np.random.default_rng(seed)
    out = np.array(pairs, np.int32, copy=True)
    bad = rng.uniform(size=len(out)) < frac
    out[bad, 1] = rng.integers(0, n2, int(bad.sum()))
    return out, bad & (out[:, 1] != np.asarray(pairs)[:, 1])
