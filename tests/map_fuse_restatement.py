"""NumPy brute force of voe_map_fuse* (include/vo_hip.h, FUSE: rules 1-11).  Every entry meets every entry; d2 is the float32
left-to-right sum of NEAREST's rule 1 and g2 the float32 sum ((dx dx + dy dy) + dz dz) (np.float32 arrays: every product and every
sum rounds to float32, nothing is fused).  There is no grid here: the device's index must not show.  `compare` is what the GPU test
uses; `margins` evaluates the same decisions in float64 for the hygiene of the cases; `FAULTS` are planted against `compare`."""
import numpy as np

import map_nearest_restatement as N

VERDICT = ("NOT_FINITE", "ALONE", "NOT_MUTUAL", "CONFLICT", "SURVIVOR", "ABSORBED")
NOT_FINITE, ALONE, NOT_MUTUAL, CONFLICT, SURVIVOR, ABSORBED = range(6)
STATUS = ("OK", "NOTHING_FUSED")
OK, NOTHING_FUSED = range(2)
FAULTS = ("tie_to_higher", "le_for_lt_xyz", "le_for_lt_app", "no_xyz_gate", "chains_followed", "veto_ignored", "higher_survives",
          "position_ignored", "rows_left", "remap_minus_one")


def gap2(pts, dtype=np.float32):
    """(M, M) squared distances of the points: ((dx dx + dy dy) + dz dz), every step in `dtype`"""
    P = np.asarray(pts, dtype).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (P[None, :, k] - P[:, None, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def finite(pts, app):
    return np.isfinite(np.asarray(pts, np.float32).reshape(-1, 3)).all(axis=1) & np.isfinite(np.asarray(app, np.float32).reshape(-1, 10)).all(axis=1)


def partners(pts, app, radius_xyz, radius, dtype=np.float32, fault=None):
    """rules 1 and 2: (partner, d2, g2 per entry, the candidate matrix, n_gated).  The radii are the float32 values they are; their
    squares are products in `dtype`."""
    pts, app = np.asarray(pts, np.float32).reshape(-1, 3), np.asarray(app, np.float32).reshape(-1, 10)
    M = len(pts)
    if M == 0:
        return np.zeros(0, np.int64), np.zeros(0, dtype), np.zeros(0, dtype), np.zeros((0, 0), bool), 0
    fin = finite(pts, app)
    r2 = dtype(np.float32(radius)) * dtype(np.float32(radius))
    x2 = dtype(np.float32(radius_xyz)) * dtype(np.float32(radius_xyz))
    D = N.dist2(app, app, dtype)                              # [a, b] = sum_k (b_k - a_k)^2
    G = gap2(pts, dtype)
    both = fin[:, None] & fin[None, :] & ~np.eye(M, dtype=bool)
    with np.errstate(invalid="ignore"):
        near = (G <= x2) if fault == "le_for_lt_xyz" else (G < x2)      # a NaN compares false
        if fault == "no_xyz_gate":
            near = np.ones_like(near)
        like = (D <= r2) if fault == "le_for_lt_app" else (D < r2)
    gated = int((near & both).sum())
    cand = near & like & both
    t = np.where(cand, D, np.inf)
    j = M - 1 - np.argmin(t[:, ::-1], axis=1) if fault == "tie_to_higher" else np.argmin(t, axis=1)      # the first of equal minima: the lowest index
    has = cand.any(axis=1)
    rows = np.arange(M)
    return np.where(has, j, -1), np.where(has, t[rows, j], np.inf).astype(dtype), np.where(has, G[rows, j], np.inf).astype(dtype), cand, gated


def live(frames, n_rows, n_max, f):
    return min(len(frames[f]), n_max) if n_rows is None else max(0, min(int(n_rows[f]), n_max))


def run(pts, app, frames, n_rows, n_max, radius_xyz, radius, position=1, veto=0, dry_run=0, fault=None):
    """frames: None (no frames) or a list of (>= n_rows[f], 10) arrays (rows behind n_rows[f] are not live; n_rows None: every row
    given is live).  Returns dict(partner, dist2, gap2, verdict, remap: (M,); map_pts, map_app: the map afterwards; ent: the exact
    lookup of the rows BEFORE the call, (F, n_max) or None; app: the frames' arrays after the call, or None; stats)."""
    pts, app = np.asarray(pts, np.float32).reshape(-1, 3), np.asarray(app, np.float32).reshape(-1, 10)
    M = len(pts)
    partner, d2, g2, _, gated = partners(pts, app, radius_xyz, radius, fault=fault)
    fin = finite(pts, app)
    ent = N.lookup(app, frames, n_rows, n_max) if frames is not None else None
    seen = [set() for _ in range(M)]                          # the frames with a live row that hits the entry
    if ent is not None:
        for f in range(len(frames)):
            for e in ent[f][ent[f] >= 0]:
                seen[e].add(f)
    verdict = np.zeros(M, np.int32)
    n_conflicts = 0
    for a in range(M):
        b = int(partner[a])
        if not fin[a]:
            verdict[a] = NOT_FINITE
        elif b < 0:
            verdict[a] = ALONE
        elif partner[b] != a:
            verdict[a] = ABSORBED if fault == "chains_followed" else NOT_MUTUAL
        elif veto and frames is not None and fault != "veto_ignored" and seen[a] & seen[b]:
            verdict[a] = CONFLICT
            n_conflicts += a < b
        else:
            lower = (a < b) != (fault == "higher_survives")
            verdict[a] = SURVIVOR if lower else ABSORBED
    keep = verdict != ABSORBED
    new = (np.cumsum(keep) - 1).astype(np.int32)
    remap = np.where(keep, new, -1).astype(np.int32)
    for a in np.nonzero(~keep)[0]:
        if fault != "remap_minus_one":
            remap[a] = new[partner[a]]
    moved = pts.copy()
    if position == 1:
        for a in np.nonzero(verdict == SURVIVOR)[0]:
            b = partner[a]
            if fault != "position_ignored":                   # (the sum of two float32 is exact in double: the midpoint rounds once)
                moved[a] =((pts[a].astype(np.float64) + pts[b].astype(np.float64)) * 0.5).astype(np.float32)
    n_rewritten = 0
    out = None
    if frames is not None:
        out = [np.asarray(a, np.float32).reshape(-1, 10).copy() for a in frames]
        for f in range(len(frames)):
            for i in range(live(frames, n_rows, n_max, f)):
                e = ent[f, i]
                if e >= 0 and verdict[e] == ABSORBED:
                    n_rewritten += 1
                    if not dry_run and fault != "rows_left":
                        out[f][i] = app[partner[e]]
    n_after = int(keep.sum())
    changes = n_after != M and not dry_run
    stats = dict(status=OK if n_after != M else NOTHING_FUSED, n_before=M, n_after=n_after, n_pairs=int((verdict == SURVIVOR).sum()),
                 n_conflicts=int(n_conflicts), n_rows_rewritten=n_rewritten, by_verdict=[int((verdict == k).sum()) for k in range(6)], n_gated=gated)
    return dict(partner=partner.astype(np.int32), dist2=d2.astype(np.float32), gap2=g2.astype(np.float32), verdict=verdict, remap=remap,
                map_pts=moved[keep] if changes else pts.copy(), map_app=app[keep] if changes else app.copy(), ent=ent, app=out, stats=stats)


def compare(ref, got):
    """byte for byte: the list of what differs (empty: equal).  `got` may leave out map_pts / map_app / app."""
    bad = []
    for k in ("partner", "dist2", "gap2", "verdict", "remap", "map_pts", "map_app"):
        if k not in got:
            continue
        a, b = np.ascontiguousarray(ref[k]), np.ascontiguousarray(got[k])
        if a.tobytes() != b.tobytes():
            where = np.argwhere(a.view(np.int32) != b.view(np.int32)) if a.shape == b.shape else [("shape", a.shape, b.shape)]
            bad.append((k, where[:4].tolist() if hasattr(where, "tolist") else where))
    if "app" in got:
        ra, ga = ref["app"] or [], got["app"] or []
        if len(ra) != len(ga) or any(np.asarray(a).tobytes() != np.asarray(b).tobytes() for a, b in zip(ra, ga)):
            bad.append(("app", [f for f, (a, b) in enumerate(zip(ra, ga)) if np.asarray(a).tobytes() != np.asarray(b).tobytes()][:4]))
    if ref["stats"] != got["stats"]:
        bad.append(("stats", ref["stats"], got["stats"]))
    return bad


def margins(pts, app, radius_xyz, radius):
    """the decisions of rules 1 and 2 in float32 and in float64 (the radii as the float32 values they are): the list of (entry,
    what) where the two evaluations decide differently -- a gate, a candidate set or a partner (hence a tie)"""
    p32, _, _, c32, n32 = partners(pts, app, radius_xyz, radius, np.float32)
    p64, _, _, c64, n64 = partners(pts, app, radius_xyz, radius, np.float64)
    diff = [(int(a), "candidates") for a in np.nonzero((c32 != c64).any(axis=1))[0]] if len(p32) else []
    diff += [(int(a), "partner") for a in np.nonzero(p32 != p64)[0]]
    if n32 != n64:
        diff.append((-1, "n_gated"))
    return diff
