"""voe_map_align* and voe_map_merge* restated in float64 NumPy from include/vo_map_align.h alone (not from the kernels): the
lookup as vo_map_lookup defines it, the sample rule of vo_hip.h, Umeyama's closed form with np.linalg.svd, the scoring, the
refits with their guard, the status and the statistics; and the merge of both policies through the map of oracle/vo_pipeline.

WHAT THE DEVICE MAY DO DIFFERENTLY, AND THE MEASURES FOR IT.

(1) The predicate.  The header scores in float32: r_i = fma(M_i0, a0, fma(M_i1, a1, fma(M_i2, a2, t_i))) - b_i and
d2 = fma(r_0, r_0, fma(r_1, r_1, r_2 r_2)), inlier iff d2 < thr2.  Here d2 is taken in double from the float32 model.  With
u = eps32 = 2^-24 (the unit roundoff of float32) every fma and the subtraction round once, so with the magnitude
    m_i = |M_i0 a0| + |M_i1 a1| + |M_i2 a2| + |t_i| + |b_i|
the computed r_i lies within 4 u m_i of the exact one (four roundings, each of a partial result bounded by m_i; second order in
u left out, far below the rest).  The device's float32 model may be ONE float32 ulp away from the one here in each of its 12
numbers (its double solve rounds differently and may fall on the other side of a float32 boundary): an ulp of x is at most
2 u |x|, which moves r_i by at most 2 u (|M_i0 a0| + |M_i1 a1| + |M_i2 a2| + |t_i|) <= 2 u m_i.  So e_i = 6 u m_i bounds
|r_i(device) - r_i(here)|, and the three roundings of d2 add at most 3 u of its magnitude:
    band = sum_i (2 |r_i| e_i + e_i^2) + 4 u sum_i (|r_i| + e_i)^2.
A pair is IN THE BAND of a model when |d2 - thr2| <= band: only such a pair can be classed differently.  A NaN is in no band
(it is an outlier on both sides).  The CPU test asserts that no pair lies in the band of the winner, of any refit or of any
hypothesis whose count comes within its own band population of the winner's, and that at most 10 % of the valid hypotheses
have a pair in theirs; the GPU test then compares masks and statuses exactly and a count within its band population.

(2) The order of the double sums.  `reverse` sums every mean and moment over the pairs in the opposite order; the spread of S,
scale and rms between the two orders is what profiles/map_align_budget.json records per case.

(3) The a-priori bound (apriori() below) of what ANY order of summation in double can move.  With u64 = 2^-53 and m terms, a
sum's error is at most m u64 times the sum of the magnitudes (Higham 2002, (4.4), for any order).  The centroids move by at most
rho_c = m u64 max|a| (or |b|); the centred terms are exact differences of nearby numbers plus that shift, and the shift enters the
moments only through sum(da) ~ 0, so the moments Sigma and var_a move relatively by at most rho = m u64 (1 + 2 g) with
g = max(|ca|, |cb|) / the rms extent of the centred set (the cancellation of a scene far from its origin: the `far` case).  The singular values
move by at most |dSigma|_F <= rho |Sigma|_F (Weyl), c = tr(D S) / var_a by dc <= (3 rho |Sigma|_F + rho tr) / var_a, the
rotation by |dR|_F <= 2 |dSigma|_F / (s1 + s2) (the polar factor's perturbation bound, Higham 2008, Thm 8.9, with the two
smallest singular values; s2 = 0 on a plane), M = c R by dM <= c |dR|_F + dc, and t = cb - M ca by dt <= dM sqrt(3) |ca|
+ rho_c (1 + c).  The svd itself is backward stable: its own error is of the size of 10 u64 |Sigma|_F, added to |dSigma|_F.
rms: per pair r is formed in double from float32 numbers, within 5 u64 m_i of exact, and the mean of the squares moves by
m u64 relatively, so d(rms) <= 5 u64 sqrt(3) max m_i + m u64 rms.  The GPU ceiling is 4 x the spread + 2 x this bound (for S one
float32 ulp more): reasoning written down before any device value was seen, none goes into the budget file.

(4) Rounding boundaries.  A double that lies within the ceiling of the midpoint between two float32 numbers may round to either:
`rounding_margin` is the smallest distance of a model's numbers to such a midpoint (M and t apart: their bounds differ); the CPU
test asserts that it stays above twice the a-priori bound for every refit, so that the refit's float32 model is expected bit for
bit and rms needs no ulp of its own (a minimal model is covered by the band's ulp)."""
import numpy as np

OK, FEW_MATCHES, NO_HYPOTHESIS, FEW_INLIERS = range(4)
STATUS = ("OK", "FEW_MATCHES", "NO_HYPOTHESIS", "FEW_INLIERS")
TAKE_SRC, KEEP_DST = 0, 1
MAX_REFITS = 16
EPS32, U64 = 2.0 ** -24, 2.0 ** -53
DEFAULT = dict(seed=1, n_hypotheses=64, with_scale=1, n_refits=1, min_inliers=3, threshold=0.05)
MASK64 = (1 << 64) - 1


# ---- the sample rule (vo_hip.h) ----
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, h, j, n):
    return (((splitmix64((seed ^ ((h << 20) | j)) & MASK64)) >> 32) * n) >> 32


def sample(seed, h, n):
    """the first 3 distinct draws within j < 64, or None"""
    if n < 3:
        return None
    s = []
    for j in range(64):
        v = draw(seed, h, j, n)
        if v not in s:
            s.append(v)
            if len(s) == 3:
                return s
    return None


# ---- the lookup (vo_map_lookup: the entry update() would have found; -0 == +0, a NaN equals nothing) ----
def _keys(app):
    a = np.ascontiguousarray(np.asarray(app, np.float32).reshape(-1, 10) + np.float32(0.0))      # -0 -> +0
    return [None if np.isnan(r).any() else r.tobytes() for r in a]


def lookup(map_app, query_app):
    """(pairs (k, 2) int32 = (query, entry) in query order, entries (n,) int32 or -1)"""
    table = {}
    for e, k in enumerate(_keys(map_app)):
        if k is not None and k not in table:
            table[k] = e
    ent = np.array([-1 if k is None else table.get(k, -1) for k in _keys(query_app)], np.int32).reshape(-1)
    hit = np.nonzero(ent >= 0)[0]
    return np.stack([hit, ent[hit]], 1).astype(np.int32).reshape(-1, 2), ent


# ---- Umeyama ----
def umeyama(a, b, with_scale=True, reverse=False):
    """(M (3, 3) = c R, t (3,), c, s (3,)) in float64, or None: the header's solve on the rows of a and b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if reverse:
        a, b = a[::-1], b[::-1]
    m = len(a)
    with np.errstate(all="ignore"):
        ca, cb = a.sum(0) / m, b.sum(0) / m
        da, db = a - ca, b - cb
        Sg = (db[:, :, None] * da[:, None, :]).sum(0) / m
        var_a = (da * da).sum(1).sum() / m
        if not (var_a > 0 and np.isfinite(var_a)) or not np.isfinite(Sg).all():
            return None
        U, s, Vt = np.linalg.svd(Sg)
        if not (s[1] > 1e-9 * s[0]):
            return None
        d = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
        R = U @ np.diag([1.0, 1.0, d]) @ Vt
        c = (s[0] + s[1] + d * s[2]) / var_a if with_scale else 1.0
        if not c > 0:
            return None
        M = c * R
        t = cb - M @ ca
    if not (np.isfinite(M).all() and np.isfinite(t).all() and np.isfinite(c)):
        return None
    return M, t, float(c), s, dict(ca=ca, cb=cb, var_a=var_a, Sg=Sg, m=m, da=da, db=db)


def rounded(M, t):
    return np.asarray(M, np.float64).astype(np.float32), np.asarray(t, np.float64).astype(np.float32)


def rounding_margin(x):
    """the smallest distance of the numbers to a midpoint between two neighbouring float32 numbers"""
    x = np.asarray(x, np.float64).ravel()
    f = x.astype(np.float32)
    up, dn = np.nextafter(f, np.float32(np.inf)).astype(np.float64), np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    return float(np.minimum(np.abs(x - (f + up) / 2), np.abs(x - (f + dn) / 2)).min())


# ---- scoring ----
def residuals(M32, t32, a, b):
    """(d2 (n,), band (n,), magnitude (n, 3)) of the float32 model on the pairs, in double"""
    M, t = np.asarray(M32, np.float64), np.asarray(t32, np.float64)
    with np.errstate(all="ignore"):
        r = ((M[None, :, 0] * a[:, None, 0] + M[None, :, 1] * a[:, None, 1]) + M[None, :, 2] * a[:, None, 2] + t[None, :]) - b
        d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        mag = np.abs(M)[None, :, :] @ np.abs(a)[:, :, None]
        mag = mag[:, :, 0] + np.abs(t)[None, :] + np.abs(b)
        e = 6 * EPS32 * mag
        band = (2 * np.abs(r) * e + e * e).sum(1) + 4 * EPS32 * ((np.abs(r) + e) ** 2).sum(1)
    return d2, band, mag


def classify(M32, t32, a, b, thr2):
    """(inlier mask, in-band mask, d2)"""
    d2, band, _ = residuals(M32, t32, a, b)
    with np.errstate(all="ignore"):
        return d2 < thr2, np.abs(d2 - thr2) <= band, d2


def _sum(x, reverse):
    return float((x[::-1] if reverse else x).sum())


def apriori(sol, c, s, a, b, M32, t32, rms):
    """the a-priori bound of the docstring for one solve over the rows a, b: dict(S, scale, rms)"""
    m = sol["m"]
    ext = np.sqrt(min((sol["da"] ** 2).sum() / m, (sol["db"] ** 2).sum() / m))
    g = max(np.abs(sol["ca"]).max(), np.abs(sol["cb"]).max()) / ext
    rho = m * U64 * (1 + 2 * g)
    rho_c = m * U64 * max(np.abs(a).max(), np.abs(b).max())
    nS = np.linalg.norm(sol["Sg"])
    dSg = (rho + 10 * U64) * nS
    dc = (3 * dSg + rho * (s[0] + s[1] + s[2])) / sol["var_a"]
    dR = 2 * dSg / (s[1] + s[2])
    dM = c * dR + dc
    dt = dM * np.sqrt(3) * np.abs(sol["ca"]).max() + rho_c * (1 + c)
    _, _, mag = residuals(M32, t32, a, b)
    return dict(S=float(max(dM, dt)), M=float(dM), t=float(dt), scale=float(dc), rms=float(5 * U64 * np.sqrt(3) * mag.max() + m * U64 * rms))


def run(case, reverse=False):
    """the alignment of case = dict(dst_pts, dst_app, src_pts, src_app, params): every output of the header, the bands and margins"""
    p = dict(DEFAULT, **case.get("params", {}))
    H, seed = int(p["n_hypotheses"]), int(p["seed"])
    thr2 = float(np.float32(p["threshold"]) * np.float32(p["threshold"]))
    pairs, _ = lookup(case["dst_app"], case["src_app"])
    n = len(pairs)
    a = np.asarray(case["src_pts"], np.float32).reshape(-1, 3)[pairs[:, 0]].astype(np.float64)
    b = np.asarray(case["dst_pts"], np.float32).reshape(-1, 3)[pairs[:, 1]].astype(np.float64)
    counts = np.full(H, -1, np.int32)
    band_pop = np.zeros(H, np.int64)
    models, scales, rank_ratio = {}, {}, []
    for h in range(H):
        s3 = sample(seed, h, n)
        if s3 is None:
            continue
        if np.isfinite(a[s3]).all() and np.isfinite(b[s3]).all():
            sv = np.linalg.svd((b[s3] - b[s3].mean(0)).T @ (a[s3] - a[s3].mean(0)), compute_uv=False)
            if sv[0] > 0:
                rank_ratio.append(sv[1] / sv[0])
        sol = umeyama(a[s3], b[s3], p["with_scale"])
        if sol is None:
            continue
        M32, t32 = rounded(sol[0], sol[1])
        if not (np.isfinite(M32).all() and np.isfinite(t32).all()):
            continue
        models[h], scales[h] = (M32, t32), sol[2]
        inl, inb, _ = classify(M32, t32, a, b, thr2)
        counts[h], band_pop[h] = int(inl.sum()), int(inb.sum())
    n_valid = len(models)
    out = dict(pairs=pairs, n_matches=n, counts=counts, band_pop=band_pop, n_valid=n_valid, a=a, b=b, thr2=thr2,
               rank_ratio=np.array(rank_ratio), budget=None)
    win = int(np.flatnonzero(counts == counts.max())[0]) if n_valid else -1
    win_cnt = int(counts[win]) if win >= 0 else 0
    band_models, margins = [], []
    kept, have_ref, cnt_cur, fin, scale_fin, ref_sol = False, False, 0, None, 1.0, None
    if win >= 0:
        cur, ref, scale_ref = models[win], None, None
        band_models.append(int(band_pop[win]))
        done = False
        for _ in range(int(p["n_refits"])):
            inl, inb, _ = classify(cur[0], cur[1], a, b, thr2)
            cnt_cur = int(inl.sum())
            band_models[-1] = int(inb.sum())
            if cnt_cur < 3:
                done = True
                break
            sol = umeyama(a[inl], b[inl], p["with_scale"], reverse)
            if sol is not None:
                rank_ratio.append(sol[3][1] / sol[3][0])
            if sol is None or not all(np.isfinite(x).all() for x in rounded(sol[0], sol[1])):
                done = True
                break
            ref, scale_ref, have_ref = rounded(sol[0], sol[1]), sol[2], True
            ref_sol = (sol, a[inl], b[inl])
            margins.append((rounding_margin(sol[0]), rounding_margin(sol[1])))
            cur = ref
            band_models.append(0)
        if not done and have_ref:
            inl, inb, _ = classify(cur[0], cur[1], a, b, thr2)
            cnt_cur, band_models[-1] = int(inl.sum()), int(inb.sum())
        kept = have_ref and cnt_cur >= win_cnt
        fin, scale_fin = (ref, scale_ref) if kept else (models[win], scales[win])
    n_fin = cnt_cur if kept else win_cnt
    need = max(int(p["min_inliers"]), 3)
    status = FEW_MATCHES if n < 3 else NO_HYPOTHESIS if win < 0 else FEW_INLIERS if n_fin < need else OK
    S = np.eye(4, dtype=np.float32)
    mask = np.zeros(n, bool)
    rms, scale = 0.0, 1.0
    if status == OK:
        S[:3, :3], S[:3, 3] = fin
        mask, _, d2 = classify(fin[0], fin[1], a, b, thr2)
        rms, scale = float(np.sqrt(_sum(d2[mask], reverse) / n_fin)), scale_fin
        if kept:
            out["budget"] = apriori(ref_sol[0][4], ref_sol[0][2], ref_sol[0][3], ref_sol[1], ref_sol[2], fin[0], fin[1], rms)
        else:
            s3 = sample(seed, win, n)
            sol = umeyama(a[s3], b[s3], p["with_scale"])
            out["budget"] = apriori(sol[4], sol[2], sol[3], a[s3], b[s3], fin[0], fin[1], rms)
            _, _, mag = residuals(fin[0], fin[1], a[mask], b[mask])
            out["budget"]["rms"] = float(5 * U64 * np.sqrt(3) * mag.max() + n_fin * U64 * rms)
    else:
        kept, n_fin = False, 0
    out.update(S=S, mask=mask, status=status, n_inliers=n_fin, best_hypothesis=win, best_count=win_cnt, refit_kept=int(kept), scale=scale,
               rms=rms, band_models=band_models, margins=margins, rank_ratio=np.array(rank_ratio),
               stats=dict(status=status, n_matches=n, n_inliers=n_fin, best_hypothesis=win, best_count=win_cnt, n_valid=n_valid,
                          refit_kept=int(kept)))
    return out


# ---- the merge, through the oracle's map (PointCloudVector<3>::update) ----
def apply_S(S, pts):
    """vo_map_update's transform in float32: p' = t + (M0 p0 + (M1 p1 + M2 p2)) per row (Eigen's 3-term inner product, vo_math.h dot3)"""
    if S is None:
        return np.asarray(pts, np.float32).copy()
    S = np.asarray(S, np.float32)
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for i in range(3):
            out[:, i] = S[i, 3] + (S[i, 0] * p[:, 0] + (S[i, 1] * p[:, 1] + S[i, 2] * p[:, 2]))
    return out


def merge(case, S, policy):
    """dict(pts, app of dst afterwards, remap, stats): TAKE_SRC is update of all of src's rows, KEEP_DST update of the misses"""
    from oracle import vo_pipeline as vp
    dp, da = np.asarray(case["dst_pts"], np.float32).reshape(-1, 3), np.asarray(case["dst_app"], np.float32).reshape(-1, 10)
    sp, sa = np.asarray(case["src_pts"], np.float32).reshape(-1, 3), np.asarray(case["src_app"], np.float32).reshape(-1, 10)
    _, ent = lookup(da, sa)
    rows = np.arange(len(sa)) if policy == TAKE_SRC else np.nonzero(ent < 0)[0]
    m = vp.Map()
    m.update([r for r in dp], [r for r in da])                 # (dst's arrays are a map's: update builds them again)
    moved = apply_S(S, sp[rows])
    m.update([r for r in moved], [r for r in sa[rows]])
    pts, app = np.array(m.pts, np.float32).reshape(-1, 3), np.array(m.app, np.float32).reshape(-1, 10)
    _, remap = lookup(app, sa)
    return dict(pts=pts, app=app, remap=remap, rows=rows,
                stats=dict(n_src=len(sa), n_shared=int((ent >= 0).sum()), n_appended=len(pts) - len(dp), n_dst_after=len(pts)))


def similarity_pose(T, S):
    """T' = [R_T R^T | c t_T - R_T R^T t] in double"""
    T, S = np.asarray(T, np.float64), np.asarray(S, np.float64)
    c = np.cbrt(np.linalg.det(S[:3, :3]))
    R = S[:3, :3] / c
    out = np.eye(4)
    out[:3, :3] = T[:3, :3] @ R.T
    out[:3, 3] = c * T[:3, 3] - out[:3, :3] @ S[:3, 3]
    return out
