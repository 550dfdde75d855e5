"""NumPy brute force of voe_map_guided* (include/vo_hip.h, GUIDED: rules 1-7).  Every row meets every entry.  The projection is
project_point of vo_math.h restated in float32 (np.float32 arrays: every product and every sum rounds to float32, nothing is fused;
three-term sums as x0 + (x1 + x2)), the pixel gate the unfused left-to-right sum of rule 2, the distance NEAREST's rule 1
(tests/map_nearest_restatement.py).  `compare` is what the GPU test uses; `margins` evaluates the same decisions in float64 for the
hygiene of the cases; `FAULTS` are planted against `compare`."""
import numpy as np

import map_nearest_restatement as N

STATUS = N.STATUS
MATCHED, NO_ENTRY, AMBIGUOUS, DISPLACED, NAN_ROW, NOT_LIVE = range(6)
QNAN = N.QNAN
FAULTS = ("gate_le_for_lt", "z_gate_ignored", "tie_to_higher", "second_outside_gate", "image_gate_applied", "le_for_lt", "second_beyond_radius")
CHUNK = 256


def project(K, T, P, z_near, z_far, dtype=np.float32, fault=None, image=(480, 640)):
    """rule 1 for every point of P (M, 3) under T (4x4, p_cam = T p_map) and K (3x3): (u, v, in_view), every step in `dtype`"""
    K, T, P = np.asarray(K, np.float32).astype(dtype), np.asarray(T, np.float32).astype(dtype), np.asarray(P, np.float32).astype(dtype).reshape(-1, 3)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        pc = [T[i, 3] + (T[i, 0] * x + (T[i, 1] * y + T[i, 2] * z)) for i in range(3)]      # pose_apply: t + dot3
        ph = [K[i, 0] * pc[0] + (K[i, 1] * pc[1] + K[i, 2] * pc[2]) for i in range(3)]      # mat3_vec: dot3
        inv = dtype(1) / ph[2]
        u, v = ph[0] * inv, ph[1] * inv
        z_ok = ~((pc[2] > dtype(z_far)) | (pc[2] < dtype(z_near)))
        view = (pc[2] > 0) & z_ok
        if fault == "z_gate_ignored":
            view = np.ones(len(P), bool)
        if fault == "image_gate_applied":
            rows, cols = image
            view = view & ~((u < 0) | (u > dtype(cols - 1))) & ~((v < 0) | (v > dtype(rows - 1)))
    return u, v, view


def gate2(u, v, quv, dtype=np.float32):
    """(n, M) g2 of rule 2: (u_e - u_row)^2 + (v_e - v_row)^2, unfused, left to right"""
    quv = np.asarray(quv, np.float32).astype(dtype).reshape(-1, 2)
    with np.errstate(all="ignore"):
        du = u[None, :] - quv[:, None, 0]
        dv = v[None, :] - quv[:, None, 1]
        return du * du + dv * dv


def best_two(quv, q, u, v, view, E, rp2, r2, dtype=np.float32, fault=None):
    """per row: best candidate (-1: none), its d2 and g2, whether another candidate exists, the smallest d2 of the others, and the
    number of gated entries"""
    n, M = len(q), len(E)
    bi, bd, bg = np.full(n, -1, np.int64), np.full(n, np.inf, dtype), np.full(n, np.inf, dtype)
    has2, d2nd, ng = np.zeros(n, bool), np.full(n, np.inf, dtype), np.zeros(n, np.int64)
    if M == 0:
        return bi, bd, bg, has2, d2nd, ng
    for a in range(0, n, CHUNK):
        g2 = gate2(u, v, quv[a:a + CHUNK], dtype)
        s = N.dist2(q[a:a + CHUNK], E, dtype)
        with np.errstate(invalid="ignore"):
            gated = view[None, :] & ((g2 <= rp2) if fault == "gate_le_for_lt" else (g2 < rp2))      # a NaN compares false
            near = (s <= r2) if fault == "le_for_lt" else (s < r2)
        inside = gated & near
        t = np.where(inside, s, np.inf)
        any_ = inside.any(axis=1)
        j = (M - 1 - np.argmin(t[:, ::-1], axis=1)) if fault == "tie_to_higher" else np.argmin(t, axis=1)      # the first of equal minima
        rows = np.arange(len(t))
        bi[a:a + CHUNK] = np.where(any_, j, -1)
        bd[a:a + CHUNK] = np.where(any_, t[rows, j], np.inf)
        bg[a:a + CHUNK] = np.where(any_, g2[rows, j], np.inf)
        if fault == "second_outside_gate":
            others = np.where(near, s, np.inf)
        elif fault == "second_beyond_radius":
            others = np.where(gated & ~np.isnan(s), s, np.inf)
        else:
            others = t.copy()
        others[rows, j] = np.inf
        m2 = others.min(axis=1)
        has2[a:a + CHUNK] = any_ & np.isfinite(m2)
        d2nd[a:a + CHUNK] = m2
        ng[a:a + CHUNK] = gated.sum(axis=1)
    return bi, bd, bg, has2, d2nd, ng


def _live(a, n_rows, f, n_max):
    return min(len(a), n_max) if n_rows is None else max(0, min(int(n_rows[f]), n_max))


def run(map_pts, map_app, K, frames, poses, n_rows, n_max, radius_px, radius, ratio=0.0, unique=0, z_near=0, z_far=10, fault=None, image=(480, 640)):
    """frames: list of (uv (>= n_rows[f], 2), app (>= n_rows[f], 10)); poses: list of 4x4.  Returns dict(entry, status, dist2, pix2:
    (F, n_max); app: list of the frames' appearance arrays after the call; stats)."""
    P = np.asarray(map_pts, np.float32).reshape(-1, 3)
    E = np.asarray(map_app, np.float32).reshape(-1, 10)
    F = len(frames)
    rp = np.float32(radius_px)
    rp2 = np.float32(rp * rp)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    rr = np.float32(np.float32(ratio) * np.float32(ratio))
    entry = np.full((F, n_max), -1, np.int32)
    status = np.full((F, n_max), NOT_LIVE, np.int32)
    d2 = np.full((F, n_max), np.inf, np.float32)
    g2 = np.full((F, n_max), np.inf, np.float32)
    out = []
    n_in_view = n_gated = 0
    for f, (quv, a) in enumerate(frames):
        a = np.asarray(a, np.float32).reshape(-1, 10)
        quv = np.asarray(quv, np.float32).reshape(-1, 2)
        n = _live(a, n_rows, f, n_max)
        q = a[:n]
        u, v, view = project(K, poses[f], P, z_near, z_far, fault=fault, image=image)
        n_in_view += int(view.sum())
        nan = np.isnan(q).any(axis=1)
        bi, bd, bg, has2, d2nd, ng = best_two(quv[:n], q, u, v, view, E, rp2, r2, fault=fault)
        n_gated += int(ng.sum())
        st = np.where(nan, NAN_ROW, np.where(bi < 0, NO_ENTRY, MATCHED)).astype(np.int32)
        if ratio != 0:
            with np.errstate(invalid="ignore", over="ignore"):
                amb = has2 & ~(bd < (rr * d2nd).astype(np.float32))
            st[(st == MATCHED) & amb] = AMBIGUOUS
        if unique:
            for e in np.unique(bi[st == MATCHED]):
                rows = np.nonzero((st == MATCHED) & (bi == e))[0]
                keep = rows[np.lexsort((rows, bd[rows].view(np.uint32)))[0]]      # smallest d2, ties to the lowest row
                st[rows[rows != keep]] = DISPLACED
        status[f, :n] = st
        entry[f, :n] = np.where(st == MATCHED, bi, -1)
        has = (st == MATCHED) | (st == AMBIGUOUS) | (st == DISPLACED)
        d2[f, :n] = np.where(has, bd, np.inf)
        g2[f, :n] = np.where(has, bg, np.inf)
        o = a.copy()
        for i in range(n):
            if st[i] == MATCHED:
                o[i] = E[bi[i]]
            elif st[i] in (AMBIGUOUS, DISPLACED):
                o[i, 0] = QNAN
        out.append(o)
    live = status != NOT_LIVE
    stats = dict(n_frames=F, n_entries=len(E), n_live=int(live.sum()), n_matched=int((status == MATCHED).sum()),
                 n_no_entry=int((status == NO_ENTRY).sum()), n_ambiguous=int((status == AMBIGUOUS).sum()),
                 n_displaced=int((status == DISPLACED).sum()), n_nan=int((status == NAN_ROW).sum()), n_in_view=n_in_view, n_gated=n_gated)
    return dict(entry=entry, status=status, dist2=d2, pix2=g2, app=out, stats=stats)


def compare(ref, got):
    """byte for byte: the list of what differs (empty: equal)"""
    bad = []
    for k in ("entry", "status", "dist2", "pix2"):
        if np.asarray(ref[k]).tobytes() != np.asarray(got[k]).tobytes():
            where = np.argwhere(np.asarray(ref[k]).view(np.int32) != np.asarray(got[k]).view(np.int32))
            bad.append((k, where[:4].tolist()))
    if len(ref["app"]) != len(got["app"]) or any(np.asarray(a).tobytes() != np.asarray(b).tobytes() for a, b in zip(ref["app"], got["app"])):
        bad.append(("app", [f for f, (a, b) in enumerate(zip(ref["app"], got["app"])) if np.asarray(a).tobytes() != np.asarray(b).tobytes()][:4]))
    if ref["stats"] != got["stats"]:
        bad.append(("stats", ref["stats"], got["stats"]))
    return bad


def margins(map_pts, map_app, K, frames, poses, n_rows, n_max, radius_px, radius, ratio=0.0, unique=0, z_near=0, z_far=10):
    """the decisions of rules 1-4 in float32 and in float64 (the inputs, radius_px, radius and ratio as the float32 values they
    are): the list of (frame, row or -1, what) where the two evaluations decide differently"""
    P = np.asarray(map_pts, np.float32).reshape(-1, 3)
    E32 = np.asarray(map_app, np.float32).reshape(-1, 10)
    diff, per = [], {}
    for dt in (np.float32, np.float64):
        rp2 = dt(np.float32(radius_px)) * dt(np.float32(radius_px))
        r2 = dt(np.float32(radius)) * dt(np.float32(radius))
        rr = dt(np.float32(ratio)) * dt(np.float32(ratio))
        res = []
        for f, (quv, a) in enumerate(frames):
            a = np.asarray(a, np.float32).reshape(-1, 10)
            quv = np.asarray(quv, np.float32).reshape(-1, 2)
            n = _live(a, n_rows, f, n_max)
            u, v, view = project(K, poses[f], P, z_near, z_far, dtype=dt)
            bi, bd, bg, has2, d2nd, ng = best_two(quv[:n].astype(dt), a[:n].astype(dt), u, v, view, E32.astype(dt), rp2, r2, dtype=dt)
            with np.errstate(invalid="ignore", over="ignore"):
                amb = has2 & ~(bd < rr * d2nd) if ratio != 0 else np.zeros(n, bool)
            ok = (bi >= 0) & ~amb & ~np.isnan(a[:n]).any(axis=1)
            keep = np.zeros(n, bool)
            for e in np.unique(bi[ok]):
                rows = np.nonzero(ok & (bi == e))[0]
                keep[rows[np.lexsort((rows, bd[rows]))[0]]] = True
            res.append((view, bi, ng, amb, keep if unique else ok))
        per[dt] = res
    for f, (a, b) in enumerate(zip(per[np.float32], per[np.float64])):
        if (a[0] != b[0]).any():
            diff.append((f, -1, "view"))
        for what, x, y in zip(("best", "gated", "ratio", "unique"), a[1:], b[1:]):
            for i in np.nonzero(np.asarray(x) != np.asarray(y))[0]:
                diff.append((f, int(i), what))
    return diff
