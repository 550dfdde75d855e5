"""The named cases of voe_map_loops* that the CPU and the GPU test share: the smallest scenes at which the kernels can go wrong.

A case is a dict: K, cam, map_pts (M, 3) -- the DRIFTED map: every entry where the drifted similarity of its reference frame puts
it --, map_app (M, 10), frames [(uv, app)], n_rows (or None), S (F, 4, 4) the drifted chain, gt (F, 4, 4), dup_rows (rows of the map
entered TWICE by the update that builds it, so that the host's bound of the size lies above the size the device holds), params
(the keyword arguments of map_loops_restatement.run / vo.Map.loops).

The scenes are made by hand: the cameras jitter around one place and look at one box of landmarks, so every landmark projects
into every frame and WHICH frame sees WHICH landmark is the case's choice alone.  Frame r creates new[r] landmarks; a frame sees
its own, those of the `recent` frames before it and what the case adds: the loops.  Pixels are exact projections under the ground
truth, so a measured slot has every pair as an inlier to a thousandth of a pixel and a scrambled one has none: no decision of a
case is marginal, which tests/test_map_loops_cpu.py asserts."""
import numpy as np

import map_loops_restatement as L
import map_refine_restatement as R
import pose_graph_cases as Cc

K = np.array([[300.0, 0, 320], [0, 300, 240], [0, 0, 1]], np.float32)
CAM = (480, 640, 0, 30)
FRAME_COUNTS = (1, 2, 3, 255, 256, 257, 513)                  # the edges of the prefix sum's runs and of the histogram's rows


def _project(G, p):
    q = p @ G[:3, :3].T + G[:3, 3]
    h = q @ K.astype(np.float64).T
    return (h[:, :2] / h[:, 2:3]).astype(np.float32)


def build(F, new, sees, seed, n_max, drift=0.002, params=None, dup_rows=0, edit=None):
    """new[r]: landmarks frame r creates (their entries are consecutive, in frame order); sees[f]: the entries frame f sees, in
    row order; edit(frames, app, rng): the case's own changes to the frames (a list of [uv, app] arrays), returns n_rows or None"""
    rng = np.random.default_rng(seed)
    M = int(np.sum(new))
    gt = np.array([Cc._sim(1.0, 0.03 * rng.standard_normal(3), 0.2 * rng.standard_normal(3)) for _ in range(F)])
    S = [gt[0].copy()]
    for k in range(F - 1):
        S.append(Cc._sim(np.exp(drift), 0.0005 * rng.standard_normal(3), 0.0005 * rng.standard_normal(3)) @ gt[k + 1] @ np.linalg.inv(gt[k]) @ S[-1])
    S = np.array(S, np.float32)
    pts = np.stack([rng.uniform(-1.5, 1.5, M), rng.uniform(-1.0, 1.0, M), rng.uniform(5.0, 9.0, M)], 1)
    app = rng.uniform(-1, 1, (M, 10)).astype(np.float32)
    frames = []
    for f in range(F):
        ids = np.asarray(sees[f], np.int64)
        frames.append([_project(gt[f], pts[ids]).reshape(-1, 2), app[ids].reshape(-1, 10).copy()])
    n_rows = edit(frames, app, rng) if edit else None
    frames = [(uv, a) for uv, a in frames]
    # the drifted map: every seen entry where S of its reference frame puts it
    assert max(len(a) for _, a in frames) <= n_max
    _, _, ents = R.observation_lists(app, frames, n_rows=n_rows, n_max=n_max)
    ref = L.reference_frames(ents, n_max, M)
    drifted = pts.copy()
    for e in np.nonzero(ref >= 0)[0]:
        r = ref[e]
        q = gt[r][:3, :3] @ pts[e] + gt[r][:3, 3]
        Sr = S[r].astype(np.float64)
        drifted[e] = np.linalg.solve(Sr[:3, :3], q - Sr[:3, 3])
    return dict(K=K, cam=CAM, map_pts=drifted.astype(np.float32), map_app=app, frames=frames, n_rows=n_rows, n_max=n_max, S=S, gt=gt, dup_rows=dup_rows,
                params=dict(L.DEFAULT, **(params or {})), ref=ref)


def _ids(new):
    off = np.concatenate([[0], np.cumsum(new)])
    return [list(range(off[r], off[r + 1])) for r in range(len(new))]


def _base(F, new, recent):
    ids = _ids(new)
    return ids, [[e for r in range(max(f - recent, 0), f + 1) for e in ids[r]] for f in range(F)]


def small13():
    """n_max 13, frames of 3 .. 13 rows: a band that reaches below frame 0 with an i tie inside it (slot OK), a slot of 5 pairs
    (FEW_MATCHES), a slot whose pixels are scrambled (NO_CONSENSUS), more slots than survivors (EMPTY), a host bound above the size"""
    F, new = 20, [3] * 20
    ids, sees = _base(F, new, 0)
    sees[15] += ids[0] + ids[1] + ids[2]                       # c(2) = c(3) = 9 -> i = 2, whose band [-1, 2] reaches below frame 0
    sees[17] += ids[8] + ids[9][:2]                            # c(9) = c(10) = c(11) = 5 -> i = 9: five pairs
    sees[18] += ids[10] + ids[11] + ids[12]                    # 9 entries, pixels scrambled below

    def edit(frames, app, rng):
        frames[18][0][:] = np.stack([rng.uniform(0, 639, len(frames[18][0])), rng.uniform(0, 479, len(frames[18][0]))], 1).astype(np.float32)
        for f in (15, 17, 18):                                 # rows in no particular order
            order = rng.permutation(len(frames[f][0]))
            frames[f][0], frames[f][1] = frames[f][0][order], frames[f][1][order]
        return None
    return build(F, new, sees, 13, 13, params=dict(gap=5, ref_window=3, min_shared=4, separation=0, max_loops=5), dup_rows=2, edit=edit)


def content64(max_loops=4):
    """n_max 64, band of one frame (ref_window 0): equal counts that every order rule must break, a plateau wider than the
    separation, a frame at exactly the gap, two rows of one frame on one entry, a NaN appearance row, a frame with no hit, garbage
    behind the live rows"""
    F, new = 24, [9] * 24
    ids, sees = _base(F, new, 1)
    sees[10] += ids[2]                                         # survivor (2, 10, 9): ties with (4, 20, 9) in c -> j ascending
    for j in range(13, 18):
        sees[j] += ids[1][:8]                                  # a plateau of c = 8 over 13 .. 17, separation 2: only 13 keeps
    sees[20] += ids[4] + ids[5]                                # c(4) = c(5) = 9 -> i ascending: 4
    sees[21] += ids[5]                                         # c = 9 like 20, within the separation: j' < j wins
    sees[22] += ids[16]                                        # i = j - gap exactly: NOT a candidate (i < j - gap)

    def edit(frames, app, rng):
        uv, a = frames[20]
        k = len(a) - 18 + 2                                    # a row on an entry of frame 4's
        frames[20][0], frames[20][1] = np.concatenate([uv, uv[k:k + 1]]), np.concatenate([a, a[k:k + 1]])      # ... twice
        nan = rng.uniform(-1, 1, (1, 10)).astype(np.float32)
        nan[0, 3] = np.nan
        frames[20][0], frames[20][1] = np.concatenate([frames[20][0], [[5.0, 5.0]]]).astype(np.float32), np.concatenate([frames[20][1], nan])
        frames[7][1][:] = rng.uniform(-1, 1, frames[7][1].shape).astype(np.float32)      # frame 7 hits nothing: its own entries go unseen
        n_rows = np.array([len(a) for _, a in frames], np.int32)
        frames[21][0] = np.concatenate([frames[21][0], frames[20][0][-12:-2]])           # garbage behind the live rows: rows that WOULD hit
        frames[21][1] = np.concatenate([frames[21][1], frames[20][1][-12:-2]])
        return n_rows
    return build(F, new, sees, 64, 64, params=dict(gap=6, ref_window=0, min_shared=5, separation=2, max_loops=max_loops), edit=edit)


def frame_count(F):
    """F frames of 2 .. 4 rows: every 7th frame, the last one and those around 256 see two entries of a frame two behind"""
    new = [2] * F
    ids, sees = _base(F, new, 0)
    for j in sorted(set(range(2, F, 7)) | {F - 1, 255, 256, 257, 258} if F > 2 else {F - 1}):
        if 2 <= j < F:
            sees[j] = sees[j] + ids[j - 2]
        elif j == 1 and F == 2:
            sees[1] = sees[1] + ids[0]
    return build(F, new, sees, 500 + F, 4, params=dict(gap=0 if F <= 2 else 1, ref_window=1, min_shared=1, separation=1, max_loops=min(4, F)))


def no_candidate():
    c = small13()
    c["params"] = dict(c["params"], gap=len(c["frames"]))
    return c


CASES = {"small13": small13, "content64": content64, "one_loop": lambda: content64(max_loops=1), "no_candidate": no_candidate}
CASES.update({"frames%d" % F: (lambda F=F: frame_count(F)) for F in FRAME_COUNTS})

_CASE, _REF = {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = CASES[name]()
    return _CASE[name]


def run(c, **kw):
    return L.run(c["K"], c["cam"], c["map_pts"], c["map_app"], c["frames"], c["S"], n_rows=c["n_rows"], n_max=c["n_max"], **dict(c["params"], **kw))


def reference(name, fault=None):
    """the restatement's run of a case (computed once, shared, never changed)"""
    if (name, fault) not in _REF:
        _REF[(name, fault)] = run(case(name), fault=fault)
    return _REF[(name, fault)]
