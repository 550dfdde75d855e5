"""NumPy restatement of voe_map_loops* (include/vo_map_loops.h), written from the header's rules.

Rules 1-6 are integers: the hits come from the lookup of tests/map_localise_restatement.py through
tests/map_refine_restatement.observation_lists (the entry per live row of every frame), the reference frame is the minimum key,
the histogram counts entries (not rows), candidates, suppression and ranking are the header's text with its three tie orders.
Rule 7 is the composition of tests/pose_ransac_restatement.py that tests/map_localise_restatement.py uses (P3P RANSAC winner,
Gauss-Newton PICP from it on its inliers), in float64.  Rule 8 is float64 from the float32 inputs widened.  `fault` plants a
mistake, to show that the comparison of the GPU test (compare(), below) sees it."""
import numpy as np

import map_refine_restatement as R
import pose_ransac_restatement as P

STATUS = ("OK", "FEW_MATCHES", "NO_CONSENSUS", "FEW_INLIERS", "NOT_FINITE", "EMPTY")
OK, FEW_MATCHES, NO_CONSENSUS, FEW_INLIERS, NOT_FINITE, EMPTY = range(6)
FAULTS = ("band_off_by_one", "gap_le", "rows_counted", "tie_reversed", "cj_for_ci")
DEFAULT = dict(gap=50, ref_window=5, min_shared=12, separation=3, max_loops=8, threshold_px=2.0, n_hypotheses=64, seed=0,
               kernel_threshold=10000.0, n_iters=50, min_inliers=6, w_loop=(1.0, 1.0, 1.0))


# ---- rules 2-5: integers ----
def reference_frames(ents, n_max, size):
    """ref(e): the frame of the smallest key f * n_max + row over the hits; -1 for an entry no row sees"""
    big = np.iinfo(np.int64).max
    key = np.full(size, big, np.int64)
    for f, ent in enumerate(ents):
        rows = np.nonzero(ent >= 0)[0]
        np.minimum.at(key, ent[rows], f * n_max + rows)
    return np.where(key == big, -1, key // max(n_max, 1)).astype(np.int32)


def histogram(ents, ref, fault=None):
    """hist[j][r]: the entries frame j sees whose reference frame is r -- two rows on one entry count once"""
    F = len(ents)
    hist = np.zeros((F, F), np.int64)
    for j, ent in enumerate(ents):
        hit = ent[ent >= 0]
        if fault != "rows_counted":
            hit = np.unique(hit)
        np.add.at(hist[j], ref[hit], 1)
    return hist.astype(np.int32)


def band(i, ref_window, fault=None):
    """the reference frames of the band of i: [lo, i]"""
    return max(i - ref_window - (1 if fault == "band_off_by_one" else 0), 0), i


def candidates(hist, gap, ref_window, min_shared, fault=None):
    """(F, 2) int32: (i, c) of every frame's candidate, (-1, 0) where it has none"""
    F = len(hist)
    prefix = np.concatenate([np.zeros((F, 1), np.int64), np.cumsum(hist.astype(np.int64), 1)], 1)
    out = np.tile(np.array([-1, 0], np.int32), (F, 1))
    for j in range(F):
        best = None
        for i in range(0, min(max(j - gap + (1 if fault == "gap_le" else 0), 0), F)):
            lo, hi = band(i, ref_window, fault)
            c = int(prefix[j, hi + 1] - prefix[j, lo])
            if c < min_shared:
                continue
            if best is None or c > best[1] or (fault == "tie_reversed" and c == best[1]):      # c descending, i ascending
                best = (i, c)
        if best is not None:
            out[j] = best
    return out


def choose(cand, separation, max_loops, fault=None):
    """(survivors in rank order [(i, j, c)], slots: the first max_loops of them)"""
    F = len(cand)
    rev = fault == "tie_reversed"
    surv = []
    for j in range(F):
        i, c = int(cand[j, 0]), int(cand[j, 1])
        if i < 0:
            continue
        keep = True
        for o in range(max(j - separation, 0), min(j + separation, F - 1) + 1):
            if o == j or cand[o, 0] < 0:
                continue
            co = int(cand[o, 1])
            if co > c or (co == c and ((o < j) != rev)):
                keep = False
        if keep:
            surv.append((i, j, c))
    surv.sort(key=lambda s: (-s[2], -s[1] if rev else s[1]))  # c descending, j ascending
    return surv, surv[:max_loops]


# ---- rule 6 ----
def slot_pairs(ent_j, ref, i, ref_window, fault=None, seen_by=None):
    """the rows of frame j, ascending, whose entry lies in the band of i (seen_by: a boolean per entry instead of the band -- the
    variant the header argues against, for the CPU test that measures why)"""
    rows = np.nonzero(ent_j >= 0)[0]
    if seen_by is not None:
        return rows[seen_by[ent_j[rows]]]
    lo, hi = band(i, ref_window, fault)
    r = ref[ent_j[rows]]
    return rows[(r >= lo) & (r <= hi)]


# ---- rule 7 ----
def measure(K, cam, world, uv, rows, thr_px, n_hyp, seed, thr, n_iters):
    """the two public calls on one slot's problem: dict(ransac_status, ransac_inliers, num_inliers (None where the RANSAC fell
    back: the plain solve from the identity is the device's business), T float64 rounded to float32, margins)"""
    n = len(rows)
    pairs = np.stack([rows, np.arange(n)], 1).astype(np.int64).reshape(-1, 2)
    out = dict(ransac_status=0, ransac_inliers=n, num_inliers=None, T=np.eye(4), margins=dict(count=None, pairs=0, tie=0), mask=np.ones(n, bool))
    if n < 4:
        out["ransac_status"] = 1
        return out
    T, valid, _ = P.hypotheses(K, world, uv, pairs, n_hyp, seed)
    if not valid.any():
        out["ransac_status"] = 2
        return out
    bands = np.full((n_hyp, 3), -1, np.int64)
    for h in np.nonzero(valid)[0]:
        bands[h] = P.error_bands(K, T[h], world, uv, pairs, thr_px, 0.5, *cam)
    win = int(np.argmax(bands[:, 0]))
    count = int(bands[win, 0])
    # a marginal decision: a pair of the winner between the bands, or another hypothesis whose upper band reaches the winner
    out["margins"] = dict(count=count, pairs=int(bands[win, 2] - bands[win, 1]),
                          tie=int((bands[:win, 2] >= bands[win, 1]).sum() + (bands[win + 1:, 2] > bands[win, 1]).sum()))
    if count < 6:
        out["ransac_status"] = 3
        return out
    mask = P.inliers(K, T[win], world, uv, pairs, thr_px, *cam)
    handed = pairs[mask]
    Ts = P.picp(K, T[win], world, uv, handed, thr, n_iters, *cam)
    out.update(ransac_inliers=len(handed), mask=mask, T=np.asarray(Ts, np.float64).astype(np.float32).astype(np.float64))
    if np.isfinite(Ts).all():
        out["num_inliers"] = int(P.inliers(K, Ts, world, uv, handed, np.sqrt(thr), *cam).sum())
    return out


# ---- rule 8 ----
def inv3(Mx):
    """the adjugate over the determinant"""
    Mx = np.asarray(Mx, np.float64)
    adj = np.array([[Mx[1, 1] * Mx[2, 2] - Mx[1, 2] * Mx[2, 1], Mx[0, 2] * Mx[2, 1] - Mx[0, 1] * Mx[2, 2], Mx[0, 1] * Mx[1, 2] - Mx[0, 2] * Mx[1, 1]],
                    [Mx[1, 2] * Mx[2, 0] - Mx[1, 0] * Mx[2, 2], Mx[0, 0] * Mx[2, 2] - Mx[0, 2] * Mx[2, 0], Mx[0, 2] * Mx[1, 0] - Mx[0, 0] * Mx[1, 2]],
                    [Mx[1, 0] * Mx[2, 1] - Mx[1, 1] * Mx[2, 0], Mx[0, 1] * Mx[2, 0] - Mx[0, 0] * Mx[2, 1], Mx[0, 0] * Mx[1, 1] - Mx[0, 1] * Mx[1, 0]]])
    return adj / np.linalg.det(Mx)


def edge_Z(S_i, T, S_j=None, fault=None):
    """(Z (4, 4) float64, the largest term summed into every entry (4, 4)): Z = [c_i R | c_i t] S_i^-1 from the float32 S_i and
    the float32 solved pose T, widened"""
    S_i = np.asarray(S_i, np.float32).astype(np.float64)
    T = np.asarray(T, np.float32).astype(np.float64)
    src = np.asarray(S_j, np.float32).astype(np.float64) if fault == "cj_for_ci" else S_i
    c = np.cbrt(np.linalg.det(src[:3, :3]))
    A, at = c * T[:3, :3], c * T[:3, 3]
    Mi = inv3(S_i[:3, :3])
    u = Mi @ S_i[:3, 3]
    Z, big = np.eye(4), np.zeros((4, 4))
    Z[:3, :3] = A @ Mi
    Z[:3, 3] = at - A @ u
    big[:3, :3] = np.abs(A[:, :, None] * Mi[None, :, :]).max(1)
    big[:3, 3] = np.maximum(np.abs(at), np.abs(A * u[None, :]).max(1))
    big[3, 3] = 1.0
    return Z, big


def run(K, cam, map_pts, map_app, frames, S, n_rows=None, n_max=None, fault=None, seen_by_i=False, forced=None, **params):
    """the whole call.  frames: [(uv, app)]; S: (F, 4, 4).  Returns dict(ref_frame, hist, cand, survivors, edges (L, 2) int32,
    Z (L, 4, 4) float64 (as float32 widened), weights (L, 3) float32, slots: one dict per slot -- i, j, c, rows (the pairs' rows),
    n_pairs, world, ransac_status, ransac_inliers, num_inliers, status, T, margins --, stats).  forced: [(i, j)] that fill the slots
    instead of the chosen survivors, and seen_by_i: the pairs of a slot are frame j's rows on ANY entry frame i sees -- both for the
    CPU test that measures why the band is the rule, neither has a counterpart in the library."""
    p = dict(DEFAULT, **params)
    map_pts = np.asarray(map_pts, np.float32).reshape(-1, 3)
    S32 = np.asarray(S, np.float32).reshape(-1, 4, 4)
    F, size = len(frames), len(map_pts)
    _, n_max, ents = R.observation_lists(map_app, frames, n_rows=n_rows, n_max=n_max)
    ref = reference_frames(ents, n_max, size)
    hist = histogram(ents, ref, fault)
    cand = candidates(hist, p["gap"], p["ref_window"], p["min_shared"], fault)
    surv, taken = choose(cand, p["separation"], p["max_loops"], fault)
    if forced is not None:
        taken = [(i, j, int(hist[j, band(i, p["ref_window"])[0]:i + 1].sum())) for i, j in forced][:p["max_loops"]]
    L = p["max_loops"]
    edges = np.full((L, 2), -1, np.int32)
    Z = np.tile(np.eye(4), (L, 1, 1))
    weights = np.zeros((L, 3), np.float32)
    slots = []
    for l in range(L):
        if l >= len(taken):
            slots.append(dict(i=-1, j=-1, c=0, rows=np.zeros(0, np.int64), n_pairs=0, ransac_status=1, ransac_inliers=0, num_inliers=None,
                              status=EMPTY, T=np.eye(4), margins=None, world=np.zeros((0, 3), np.float32)))
            continue
        i, j, c = taken[l]
        seen = None
        if seen_by_i:
            seen = np.zeros(size, bool)
            seen[ents[i][ents[i] >= 0]] = True
        rows = slot_pairs(ents[j], ref, i, p["ref_window"], fault, seen)
        world = map_pts[ents[j][rows]]
        s = dict(i=i, j=j, c=c, rows=rows, n_pairs=len(rows), world=world, ransac_status=0, ransac_inliers=len(rows), num_inliers=None, T=np.eye(4),
                 margins=None)
        edges[l] = (i, j)
        uv = np.asarray(frames[j][0], np.float32).reshape(-1, 2)
        s.update(measure(K, cam, world, uv, rows, p["threshold_px"], p["n_hypotheses"], p["seed"], p["kernel_threshold"], p["n_iters"]))
        if s["n_pairs"] < 6:
            s["status"] = FEW_MATCHES
        elif s["ransac_status"] != 0:
            s["status"] = NO_CONSENSUS
        elif not np.isfinite(s["T"]).all():
            s["status"] = NOT_FINITE
        elif s["num_inliers"] is None or s["num_inliers"] < p["min_inliers"]:
            s["status"] = NOT_FINITE if s["num_inliers"] is None else FEW_INLIERS
        else:
            s["status"] = OK
            Zl, _ = edge_Z(S32[i], s["T"], S32[j], fault)
            if np.isfinite(Zl).all():
                Z[l] = Zl.astype(np.float32).astype(np.float64)
                weights[l] = np.asarray(p["w_loop"], np.float32)
            else:
                s["status"] = NOT_FINITE
        slots.append(s)
    stats = dict(n_frames=F, n_entries=size, n_candidates=int((cand[:, 0] >= 0).sum()), n_survivors=len(surv), n_slots=len(taken),
                 n_ok=sum(s["status"] == OK for s in slots))
    return dict(ref_frame=ref, hist=hist, cand=cand, survivors=surv, edges=edges, Z=Z, weights=weights, slots=slots, stats=stats, S=S32,
                params=p, n_max=n_max)


# ---- the comparison of the GPU test ----
def as_got(run_):
    """a restatement run in the shape compare() takes: what the device call and the problems' read-back give"""
    s = run_["slots"]
    return dict(ref_frame=run_["ref_frame"], hist=run_["hist"], cand=run_["cand"], edges=run_["edges"], Z=run_["Z"].astype(np.float32),
                weights=run_["weights"], stats=run_["stats"], rows=[x["rows"] for x in s], world=[x["world"] for x in s],
                T=[np.asarray(x["T"], np.float32) for x in s],
                loops=[dict(i=x["i"], j=x["j"], c=x["c"], n_pairs=x["n_pairs"], ransac_status=x["ransac_status"], ransac_inliers=x["ransac_inliers"],
                            num_inliers=-1 if x["num_inliers"] is None else x["num_inliers"], status=x["status"]) for x in s])


def compare(ref, got, log=None):
    """every difference between a device result `got` and the restatement `ref`, as a list of strings: the integers byte for byte
    (the solver's inlier count only where the RANSAC did not fall back: behind a fallback it belongs to the plain solve from the
    identity, which the GPU test holds against the explicit public sequence instead), the gathered points byte for byte, Z of
    every OK slot against rule 8 evaluated from the result's own float32 pose within one float32 ulp at the largest term"""
    bad = []
    for k in ("ref_frame", "hist", "cand", "edges"):
        if not np.array_equal(np.asarray(ref[k], np.int64), np.asarray(got[k], np.int64)):
            bad.append(k)
    if ref["stats"] != {k: int(got["stats"][k]) for k in ref["stats"]}:
        bad.append("stats %s != %s" % (got["stats"], ref["stats"]))
    worst = 0.0
    for l, s in enumerate(ref["slots"]):
        g = got["loops"][l]
        for k in ("i", "j", "c", "n_pairs", "ransac_status", "ransac_inliers", "status"):
            if int(g[k]) != int(s[k]):
                bad.append("slot %d: %s %d != %d" % (l, k, int(g[k]), int(s[k])))
        if s["ransac_status"] == 0 and s["num_inliers"] is not None and int(g["num_inliers"]) != s["num_inliers"]:
            bad.append("slot %d: num_inliers %d != %d" % (l, int(g["num_inliers"]), s["num_inliers"]))
        if not np.array_equal(np.asarray(got["rows"][l], np.int64), s["rows"]):
            bad.append("slot %d: the pairs' rows" % l)
        elif np.asarray(got["world"][l], np.float32).tobytes() != np.asarray(s["world"], np.float32).tobytes():
            bad.append("slot %d: the gathered points" % l)
        Zg = np.asarray(got["Z"][l], np.float32)
        w_want = np.asarray(ref["params"]["w_loop"], np.float32) if s["status"] == OK else np.zeros(3, np.float32)
        if np.asarray(got["weights"][l], np.float32).tobytes() != w_want.tobytes():
            bad.append("slot %d: weights" % l)
        if int(g["status"]) != OK or s["status"] != OK:
            if Zg.tobytes() != np.eye(4, dtype=np.float32).tobytes():
                bad.append("slot %d: Z of a slot that is not OK is not the identity" % l)
            continue
        Zr, big = edge_Z(ref["S"][s["i"]], got["T"][l])
        ulp = np.spacing(big.astype(np.float32)).astype(np.float64)
        d = np.abs(Zg.astype(np.float64) - Zr) / ulp
        worst = max(worst, float(d.max()))
        if not (d <= 1.0).all() or Zg[3].tobytes() != np.array([0, 0, 0, 1], np.float32).tobytes():
            bad.append("slot %d: Z is %.3g ulp of its largest term off rule 8" % (l, d.max()))
    if log is not None:
        log["z_ulp"] = worst
    return bad
