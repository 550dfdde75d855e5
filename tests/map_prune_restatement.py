"""NumPy restatement of voe_map_prune* (include/vo_hip.h, PRUNE), written from the header's rules, in float64 on the observation
lists of tests/map_refine_restatement.py (R.observation_lists) with the per-observation terms of tests/map_cull_restatement.py
(Cu.observation_terms), which also hands out the a-priori rounding bounds dsq, dz of |e|^2 and of the camera z (first order in
eps = 2^-53, from the magnitudes alone; two correct implementations lie within TWICE the bound of one another).

MARGINAL.  Every decision the rules take on a floating point number is reported as marginal when another correct evaluation
could take it the other way, i.e. when the two sides lie within twice the bound:
    z > 0                       |z| <= 2 dz
    sq > max_err_px^2           |sq - thr| <= 2 dsq
    sq > rel_floor_px^2         the same
    sq > rel_factor^2 med       |sq - f2 med| <= 2 (dsq + f2 dsq_med + eps f2 med)
    the median's rank           another eligible observation of the landmark lies within 2 (dsq + dsq_med) of med
    the duplicate winner        another member of the run that passed rule 3 lies within 2 (dsq + dsq_winner) of the winner
Observations with BIT-EQUAL inputs -- the same entry, the same frame (hence pose) and the same pixel bits -- give the same bits
in any one implementation: that is an exact tie, not a marginal one, and the rules send it to the lowest key.
`fault` plants a mistake, to show that the tests see it."""
import numpy as np

import map_cull_restatement as Cu
import map_localise_restatement as M
import map_refine_restatement as R

KEPT, NOT_LIVE, MISS, NOT_FINITE, BEHIND, DUPLICATE, HIGH_ERROR, RELATIVE, LANDMARK_AT_FAULT, FRAME_AT_FAULT = range(10)
STATUS = ("KEPT", "NOT_LIVE", "MISS", "NOT_FINITE", "BEHIND", "DUPLICATE", "HIGH_ERROR", "RELATIVE", "LANDMARK_AT_FAULT", "FRAME_AT_FAULT")
FAULTS = ("upper_median", "guard_ge", "dup_by_key", "frame_guard_first")
EPS = 2.0 ** -53
QNAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]
DEFAULT = dict(max_err_px=0.0, rel_factor=0.0, rel_floor_px=0.0, rel_min_obs=3, unique=1, max_share_landmark=1000, max_share_frame=1000)


def eligible(s):
    return (s == KEPT) | ((s >= HIGH_ERROR) & (s <= FRAME_AT_FAULT))


def soft(s):
    return (s == HIGH_ERROR) | (s == RELATIVE)


def pruned(s):
    return (s >= NOT_FINITE) & (s <= RELATIVE)


def guard_fires(n_soft, n_el, share, fault=None):
    """rules 7 and 8, in Python's unbounded integers"""
    a, b = int(n_soft) * 1000, int(share) * int(n_el)
    return a >= b if fault == "guard_ge" else a > b


def prune(K, map_pts, map_app, frames, poses, max_err_px=0.0, rel_factor=0.0, rel_floor_px=0.0, rel_min_obs=3, unique=1,
          max_share_landmark=1000, max_share_frame=1000, n_rows=None, n_max=None, alt=False, fault=None):
    """The whole call.  frames: [(uv, app)]; poses: one 4x4 per frame (p_cam = T p_map), taken as the float32 the device call is
    given.  A frame with fewer than n_max rows counts as padded with NaN appearance rows, which find nothing: live rows all the same
    when n_rows is None or says so.  Returns dict(status, entry (F, n_max) int32, sq, b_sq (F, n_max) float64: |e|^2 (+inf where there is no
    observation) and its bound, z, b_z: the camera z likewise, app_out: one (rows, 10) float32 array per frame, landmarks: dict of (M,) arrays n_obs, n_el,
    n_soft, n_pruned, at_fault, med_sq, b_med, frames: dict of (F,) arrays n_obs, n_el, n_soft, at_fault, stats,
    marginal: [(what, entry, key)], ties: the exact ties met)."""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    pts = np.asarray(map_pts, np.float32).reshape(-1, 3)
    app = np.asarray(map_app, np.float32).reshape(-1, 10)
    Mn, F = len(pts), len(frames)
    T = np.stack([np.asarray(X, np.float32).astype(np.float64).reshape(4, 4) for X in poses])
    lists, n_max, ents = R.observation_lists(app, frames, n_rows, n_max)
    uvs = [np.asarray(uv, np.float32).reshape(-1, 2) for uv, _ in frames]
    apps = [np.asarray(a, np.float32).reshape(-1, 10) for _, a in frames]
    thr = float(np.float32(max_err_px)) ** 2
    f2 = float(np.float32(rel_factor)) ** 2
    floor2 = float(np.float32(rel_floor_px)) ** 2
    status = np.full((F, n_max), NOT_LIVE, np.int32)
    entry = np.full((F, n_max), -1, np.int32)
    sq_out = np.full((F, n_max), np.inf)
    b_sq = np.zeros((F, n_max))
    z_out, b_z = np.full((F, n_max), np.inf), np.zeros((F, n_max))
    for f in range(F):
        live = n_max if n_rows is None else max(0, min(int(n_rows[f]), n_max))      # (rows a frame does not bring are NaN rows: MISS when live)
        status[f, :live] = MISS
    lm = dict(n_obs=np.zeros(Mn, np.int32), n_el=np.zeros(Mn, np.int32), n_soft=np.zeros(Mn, np.int32), n_pruned=np.zeros(Mn, np.int32),
              at_fault=np.zeros(Mn, np.int32), med_sq=np.zeros(Mn), b_med=np.zeros(Mn))
    marginal, ties = [], []
    st_flat, sq_flat, b_flat, ent_flat = status.reshape(-1), sq_out.reshape(-1), b_sq.reshape(-1), entry.reshape(-1)
    z_flat, bz_flat = z_out.reshape(-1), b_z.reshape(-1)
    soft_of = {}                                                    # entry -> keys that rule 6 made soft

    def same_inputs(k1, k2):
        fa, ia, fb, ib = k1 // n_max, k1 % n_max, k2 // n_max, k2 % n_max
        return fa == fb and uvs[fa][ia].tobytes() == uvs[fb][ib].tobytes()

    for e in range(Mn):
        keys = np.array(lists.get(e, []), np.int64)
        n = len(keys)
        lm["n_obs"][e] = n
        if n == 0:
            continue
        f, i = keys // n_max, keys % n_max
        uv = np.stack([uvs[a][b] for a, b in zip(f, i)])
        sq, z, _, dsq, dz, _ = Cu.observation_terms(K, T[f, :3, :3], T[f, :3, 3], uv, pts[e].astype(np.float64), alt)
        st = np.full(n, KEPT, np.int32)
        finite = np.isfinite(sq) & np.isfinite(z)
        st[~finite] = NOT_FINITE
        with np.errstate(all="ignore"):
            st[finite & ~(z > 0)] = BEHIND
            for k in np.nonzero(finite & (np.abs(z) <= 2 * dz))[0]:
                marginal.append(("z", e, int(keys[k])))
        # rule 4: runs of one frame
        if unique:
            a = 0
            while a < n:
                b = a
                while b + 1 < n and f[b + 1] == f[a]:
                    b += 1
                run = [k for k in range(a, b + 1) if st[k] == KEPT]
                if len(run) > 1:
                    w = min(run, key=(lambda k: k) if fault == "dup_by_key" else (lambda k: (sq[k], k)))
                    for k in run:
                        if k == w:
                            continue
                        st[k] = DUPLICATE
                        if sq[k] == sq[w] and same_inputs(int(keys[k]), int(keys[w])):
                            ties.append(("duplicate", e, int(keys[k])))
                        elif abs(sq[k] - sq[w]) <= 2 * (dsq[k] + dsq[w]):
                            marginal.append(("duplicate", e, int(keys[k])))
                a = b + 1
        el = np.nonzero(st == KEPT)[0]
        n_el = len(el)
        lm["n_el"][e] = n_el
        rel = f2 > 0 and n_el >= rel_min_obs and n_el >= 1
        med = dmed = 0.0
        if rel:
            order = sorted(el, key=lambda k: (sq[k], k))
            m = order[n_el // 2 if fault == "upper_median" else (n_el - 1) // 2]
            med, dmed = float(sq[m]), float(dsq[m])
            lm["med_sq"][e], lm["b_med"][e] = med, dmed
            for k in el:
                if k == m or (sq[k] == med and same_inputs(int(keys[k]), int(keys[m]))):
                    continue
                if abs(sq[k] - med) <= 2 * (dsq[k] + dmed):
                    marginal.append(("median", e, int(keys[k])))
        for k in el:
            if thr > 0:
                if abs(sq[k] - thr) <= 2 * dsq[k]:
                    marginal.append(("max_err", e, int(keys[k])))
                if sq[k] > thr:
                    st[k] = HIGH_ERROR
                    continue
            if rel:
                if abs(sq[k] - f2 * med) <= 2 * (dsq[k] + f2 * dmed + EPS * f2 * med):
                    marginal.append(("relative", e, int(keys[k])))
                if abs(sq[k] - floor2) <= 2 * dsq[k]:
                    marginal.append(("floor", e, int(keys[k])))
                if sq[k] > f2 * med and sq[k] > floor2:
                    st[k] = RELATIVE
        n_soft = int(soft(st).sum())
        lm["n_soft"][e] = n_soft
        soft_of[e] = [int(keys[k]) for k in np.nonzero(soft(st))[0]]
        st_flat[keys] = st
        sq_flat[keys] = sq
        b_flat[keys] = np.where(finite, dsq, 0.0)
        z_flat[keys] = z
        bz_flat[keys] = np.where(finite, dz, 0.0)
        ent_flat[keys] = e

    def landmark_guard():
        for e, ks in soft_of.items():
            still = [k for k in ks if soft(st_flat[k])]
            n_s = len(ks) if fault != "frame_guard_first" else len(still)
            if guard_fires(n_s, lm["n_el"][e], max_share_landmark, fault):
                lm["at_fault"][e] = 1
                st_flat[still] = LANDMARK_AT_FAULT

    fr = dict(n_obs=np.zeros(F, np.int32), n_el=np.zeros(F, np.int32), n_soft=np.zeros(F, np.int32), at_fault=np.zeros(F, np.int32))

    def frame_guard():
        for f in range(F):
            s = status[f]
            fr["n_obs"][f] = int(((s != NOT_LIVE) & (s != MISS)).sum())
            fr["n_el"][f] = int(eligible(s).sum())
            fr["n_soft"][f] = int(soft(s).sum())
            if guard_fires(fr["n_soft"][f], fr["n_el"][f], max_share_frame, fault):
                fr["at_fault"][f] = 1
                s[soft(s)] = FRAME_AT_FAULT

    if fault == "frame_guard_first":
        frame_guard(); landmark_guard()
    else:
        landmark_guard(); frame_guard()
    for e in range(Mn):
        ks = np.array(lists.get(e, []), np.int64)
        lm["n_pruned"][e] = int(pruned(st_flat[ks]).sum()) if len(ks) else 0
    keep = (status == KEPT) | (status == LANDMARK_AT_FAULT) | (status == FRAME_AT_FAULT)
    entry[~keep] = -1
    app_out = []
    for f in range(F):
        a = apps[f].copy()
        rows = min(len(a), n_max)
        cut = pruned(status[f, :rows])
        a[:rows][cut, 0] = QNAN
        app_out.append(a)
    by = [int((status == k).sum()) for k in range(10)]
    stats = dict(n_frames=F, n_entries=Mn, by_status=by, n_landmarks_at_fault=int(lm["at_fault"].sum()), n_frames_at_fault=int(fr["at_fault"].sum()),
                 n_obs=int(sum(by) - by[NOT_LIVE] - by[MISS]), n_pruned=int(sum(by[NOT_FINITE:RELATIVE + 1])))
    return dict(status=status, entry=entry, sq=sq_out, b_sq=b_sq, z=z_out, b_z=b_z, app_out=app_out, landmarks=lm, frames=fr, stats=stats, marginal=marginal,
                ties=ties, n_max=n_max)


def lookup_contract(map_app, res, n_rows=None):
    """rule 11: the exact lookup on app_out returns entry at every position of every frame"""
    tab = M.table(map_app)
    n_max = res["n_max"]
    for f, a in enumerate(res["app_out"]):
        live = len(a) if n_rows is None else max(0, min(int(n_rows[f]), len(a), n_max))
        ent = M.lookup(map_app, a[:n_max], n_live=live, tab=tab)[0]
        want = res["entry"][f, : len(ent)]
        if not np.array_equal(ent, want) or (res["entry"][f, len(ent):] != -1).any():
            return False
    return True
