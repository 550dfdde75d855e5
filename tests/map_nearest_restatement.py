"""NumPy brute force of voe_map_nearest* (include/vo_hip.h, NEAREST: rules 1-7).  Every row meets every entry; the distance is
the float32 left-to-right sum of the rule (np.float32 arrays: every product and every sum rounds to float32, nothing is fused).
`compare` is what the GPU test uses; `margins` evaluates the same decisions in float64 for the hygiene of the cases; `FAULTS`
are planted against `compare`."""
import numpy as np

STATUS = ("MATCHED", "NO_ENTRY", "AMBIGUOUS", "DISPLACED", "NAN_ROW", "NOT_LIVE")
MATCHED, NO_ENTRY, AMBIGUOUS, DISPLACED, NAN_ROW, NOT_LIVE = range(6)
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
FAULTS = ("tie_to_higher", "le_for_lt", "second_beyond_radius")
CHUNK = 128


def dist2(q, E, dtype=np.float32):
    """(n, M) squared distances: the sum over components 0..9 of (e_k - q_k)^2, left to right, every step in `dtype`"""
    q, E = np.asarray(q, dtype).reshape(-1, 10), np.asarray(E, dtype).reshape(-1, 10)
    with np.errstate(invalid="ignore", over="ignore"):
        d = E[None, :, 0] - q[:, None, 0]
        s = d * d
        for k in range(1, 10):
            d = E[None, :, k] - q[:, None, k]
            s = s + d * d
    return s


def best_two(q, E, r2, dtype=np.float32, fault=None):
    """per row: best entry (-1: none), its d2, whether another entry lies within the radius, and the smallest d2 of the others"""
    n, M = len(q), len(E)
    bi, bd = np.full(n, -1, np.int64), np.full(n, np.inf, dtype)
    has2, d2nd = np.zeros(n, bool), np.full(n, np.inf, dtype)
    if M == 0:
        return bi, bd, has2, d2nd
    for a in range(0, n, CHUNK):
        s = dist2(q[a:a + CHUNK], E, dtype)
        with np.errstate(invalid="ignore"):
            inside = (s <= r2) if fault == "le_for_lt" else (s < r2)      # a NaN compares false
        t = np.where(inside, s, np.inf)
        any_ = inside.any(axis=1)
        if fault == "tie_to_higher":
            j = M - 1 - np.argmin(t[:, ::-1], axis=1)
        else:
            j = np.argmin(t, axis=1)                          # the first of equal minima: the lowest entry index
        rows = np.arange(len(t))
        bi[a:a + CHUNK] = np.where(any_, j, -1)
        bd[a:a + CHUNK] = np.where(any_, t[rows, j], np.inf)
        others = (np.where(np.isnan(s), np.inf, s) if fault == "second_beyond_radius" else t).copy()
        others[rows, j] = np.inf
        m2 = others.min(axis=1)
        has2[a:a + CHUNK] = any_ & np.isfinite(m2)
        d2nd[a:a + CHUNK] = m2
    return bi, bd, has2, d2nd


def run(map_app, frames, n_rows, n_max, radius, ratio=0.0, unique=0, fault=None):
    """frames: list of (>= n_rows[f], 10) arrays (rows behind n_rows[f] are not live), n_rows None: every row given is live.
    Returns dict(entry, status, dist2: (F, n_max); app: list of the frames' arrays after the call; stats)."""
    E = np.asarray(map_app, np.float32).reshape(-1, 10)
    F = len(frames)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    rr = np.float32(np.float32(ratio) * np.float32(ratio))
    entry = np.full((F, n_max), -1, np.int32)
    status = np.full((F, n_max), NOT_LIVE, np.int32)
    d2 = np.full((F, n_max), np.inf, np.float32)
    out = []
    for f, a in enumerate(frames):
        a = np.asarray(a, np.float32).reshape(-1, 10)
        n = min(len(a), n_max) if n_rows is None else max(0, min(int(n_rows[f]), n_max))
        q = a[:n]
        nan = np.isnan(q).any(axis=1)
        bi, bd, has2, d2nd = best_two(q, E, r2, fault=fault)
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
                 n_displaced=int((status == DISPLACED).sum()), n_nan=int((status == NAN_ROW).sum()))
    return dict(entry=entry, status=status, dist2=d2, app=out, stats=stats)


def compare(ref, got):
    """byte for byte: the list of what differs (empty: equal)"""
    bad = []
    for k in ("entry", "status", "dist2"):
        if np.asarray(ref[k]).tobytes() != np.asarray(got[k]).tobytes():
            where = np.argwhere(np.asarray(ref[k]).view(np.int32) != np.asarray(got[k]).view(np.int32))
            bad.append((k, where[:4].tolist()))
    if len(ref["app"]) != len(got["app"]) or any(np.asarray(a).tobytes() != np.asarray(b).tobytes() for a, b in zip(ref["app"], got["app"])):
        bad.append(("app", [f for f, (a, b) in enumerate(zip(ref["app"], got["app"])) if np.asarray(a).tobytes() != np.asarray(b).tobytes()][:4]))
    if ref["stats"] != got["stats"]:
        bad.append(("stats", ref["stats"], got["stats"]))
    return bad


def lookup(map_app, frames, n_rows, n_max):
    """the exact lookup restated: per position the FIRST entry that compares equal under == on ten floats, or -1"""
    E = np.asarray(map_app, np.float32).reshape(-1, 10)
    ent = np.full((len(frames), n_max), -1, np.int32)
    for f, a in enumerate(frames):
        a = np.asarray(a, np.float32).reshape(-1, 10)
        n = min(len(a), n_max) if n_rows is None else max(0, min(int(n_rows[f]), n_max))
        for i in range(n):
            if len(E):
                hit = np.nonzero((E == a[i]).all(axis=1))[0]
                if len(hit):
                    ent[f, i] = hit[0]
    return ent


def margins(map_app, frames, n_rows, n_max, radius, ratio=0.0, unique=0):
    """the decisions of rules 2-4 in float32 and in float64 (the radius and the ratio as the float32 values they are): the list of
    (frame, row, what) where the two evaluations decide differently"""
    E32 = np.asarray(map_app, np.float32).reshape(-1, 10)
    r = np.float32(radius)
    diff = []
    per = {}
    for dt in (np.float32, np.float64):
        r2 = dt(r) * dt(r)
        rr = dt(np.float32(ratio)) * dt(np.float32(ratio))
        res = []
        for f, a in enumerate(frames):
            a = np.asarray(a, np.float32).reshape(-1, 10)
            n = min(len(a), n_max) if n_rows is None else max(0, min(int(n_rows[f]), n_max))
            bi, bd, has2, d2nd = best_two(a[:n].astype(dt), E32.astype(dt), r2, dtype=dt)
            with np.errstate(invalid="ignore", over="ignore"):
                inside = (dist2(a[:n], E32, dt) < r2).sum(axis=1) if len(E32) else np.zeros(n, int)
                amb = has2 & ~(bd < rr * d2nd) if ratio != 0 else np.zeros(n, bool)
            ok = (bi >= 0) & ~amb & ~np.isnan(a[:n]).any(axis=1)
            keep = np.zeros(n, bool)
            for e in np.unique(bi[ok]):
                rows = np.nonzero(ok & (bi == e))[0]
                keep[rows[np.lexsort((rows, bd[rows]))[0]]] = True
            res.append((bi, inside, amb, keep if unique else ok))
        per[dt] = res
    for f, (a, b) in enumerate(zip(per[np.float32], per[np.float64])):
        for what, x, y in zip(("best", "inside", "ratio", "unique"), a, b):
            for i in np.nonzero(np.asarray(x) != np.asarray(y))[0]:
                diff.append((f, int(i), what))
    return diff
