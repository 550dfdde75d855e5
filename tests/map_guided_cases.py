"""The cases of tests/test_gpu_map_guided.py: the smallest shapes at which voe_map_guided* can go wrong, each with what it is there
for, and their references (tests/map_guided_restatement.py), computed once.

A case: dict(map_pts (M, 3), map_app (M, 10), K (3, 3), frames [(uv (rows, 2), app (rows, 10))], poses [4x4], n_rows (list or None),
n_max, radius_px, radius, ratio, unique, z_near, z_far, dup_rows, capacity, dyadic).
DYADIC cases are the deliberate ties and boundaries: the focal lengths are powers of two, the poses hold only 0, 1 and a dyadic
translation, depths are powers of two and pixels multiples of 1/8, appearance coordinates multiples of 2^-13, so every projection,
difference, square and sum is exact in float32 AND in float64 and the two evaluations agree although the decisions are at equality.
Every other case takes no decision that float32 and float64 evaluate differently (tests/test_map_guided_cpu.py asserts both)."""
import functools

import numpy as np

import map_guided_restatement as G
from map_nearest_cases import ROW_COUNTS_14

K_REF = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]], np.float32)


def _case(map_pts, map_app, frames, poses, K=K_REF, n_max=None, n_rows=None, radius_px=8.0, radius=0.1, ratio=0.0, unique=0, z_near=0, z_far=10,
          dup_rows=0, capacity=0, dyadic=False):
    frames = [(np.asarray(p, np.float32).reshape(-1, 2), np.asarray(a, np.float32).reshape(-1, 10)) for p, a in frames]
    if n_max is None:
        n_max = max([len(a) for _, a in frames] + [0])
    return dict(map_pts=np.asarray(map_pts, np.float32).reshape(-1, 3), map_app=np.asarray(map_app, np.float32).reshape(-1, 10),
                K=np.asarray(K, np.float32), frames=frames, poses=[np.asarray(T, np.float32) for T in poses], n_rows=n_rows, n_max=n_max,
                radius_px=radius_px, radius=radius, ratio=ratio, unique=unique, z_near=z_near, z_far=z_far, dup_rows=dup_rows,
                capacity=capacity, dyadic=dyadic)


def _pose(rng, rot=0.05, trans=0.3):
    """a small rigid motion: rotation vector U(-rot, rot)^3 (Rodrigues), translation U(-trans, trans)^3"""
    w = rng.uniform(-rot, rot, 3)
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + (np.sin(th) / th) * Wx + ((1 - np.cos(th)) / th ** 2) * Wx @ Wx if th > 0 else np.eye(3)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.uniform(-trans, trans, 3)
    return T


def _scene(M, rows, seed, classes=0, close_pairs=0, stray=0.1, box=(4.0, 3.0, 1.0, 12.0), push=(0.01, 0.005), motion=(0.3, 0.05), **kw):
    """M points in front of the camera (some beyond z_far = 10), appearances U(-1, 1)^10 -- or `classes` classes of near-copies
    (N(0, 0.002) apart) --, close_pairs entries 1 cm and 0.012 in appearance beside another (second candidates inside the gate).
    Per frame a true pose, rows drawn WITH replacement among the entries in view (so several rows meet one entry: unique), pixels
    pushed by N(0, 0.3), appearances by N(0, 0.005), a tenth of the rows strays; the prior is the true pose pushed by `push`."""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-box[0], box[0], M), rng.uniform(-box[1], box[1], M), rng.uniform(box[2], box[3], M)], axis=1)
    if classes:
        E = rng.uniform(-1, 1, (classes, 10))[np.arange(M) % classes] + rng.normal(0, 0.002, (M, 10))
    else:
        E = rng.uniform(-1, 1, (M, 10))
    for j in range(min(close_pairs, M // 2)):
        d = rng.normal(0, 1, 10)
        E[M - 1 - j] = E[j] + 0.012 * d / np.linalg.norm(d)
        P[M - 1 - j] = P[j] + rng.normal(0, 0.01, 3)
    P, E = P.astype(np.float32), E.astype(np.float32)
    frames, poses = [], []
    for n in rows:
        T = _pose(rng, motion[1], motion[0])
        prior = _pose(rng, push[1], push[0]) @ T
        u, v, view = G.project(K_REF, T, P, 0, 10, dtype=np.float64)
        seen = np.nonzero(view & (u > 0) & (u < 639) & (v > 0) & (v < 479))[0] if M else np.zeros(0, int)
        if len(seen) == 0:
            uv, app = rng.uniform(0, 480, (n, 2)), rng.uniform(-1, 1, (n, 10))
        else:
            idx = seen[rng.integers(0, len(seen), n)]
            uv = np.stack([u[idx], v[idx]], axis=1) + rng.normal(0, 0.3, (n, 2))
            app = E[idx] + rng.normal(0, 0.005, (n, 10))
            k = rng.random(n) < stray
            uv[k] = rng.uniform(0, 480, (int(k.sum()), 2))
            app[k] = rng.uniform(-1, 1, (int(k.sum()), 10))
        frames.append((uv, app))
        poses.append(prior)
    return _case(P, E, frames, poses, **kw)


# ---- the dyadic case ----
K_DYADIC = np.array([[512.0, 0, 256], [0, 512.0, 256], [0, 0, 1]], np.float32)


def _dyadic(ratio, unique):
    """radius_px 8, radius 0.25, z_near 1, z_far 4, frame 0 under the identity, frame 1 under a translation of 1/4 along x.  Groups
    40 px apart along u at v = 104; component 1 of the appearance carries the group, the geometry lies along component 0 (and 5)."""
    P, E, Q0, Q1 = [], [], [], []
    app = lambda g, x, y=0.0: [x, 4.0 * g, 0, 0, 0, y, 0, 0, 0, 0]
    cu = lambda g: 40.0 * g + 24.0

    def ent(u, v, z, a):                                      # the point that projects to (u, v) at depth z under the identity: exact
        P.append([(u - 256.0) * z / 512.0, (v - 256.0) * z / 512.0, z]); E.append(a)

    def row(Q, u, v, a):
        Q.append(([u, v], a))

    # g0: the entry exactly radius_px from the row (g2 == 64 must not gate); g1: 1/8 px inside
    ent(cu(0) + 8.0, 104.0, 2.0, app(0, 0.0625)); row(Q0, cu(0), 104.0, app(0, 0.0))
    ent(cu(1) + 7.875, 104.0, 2.0, app(1, 0.0625)); row(Q0, cu(1), 104.0, app(1, 0.0))
    # g2: two gated entries at exactly equal d2 (entries 2 and 3: the lowest index wins; with a ratio the row is ambiguous)
    ent(cu(2) + 2.0, 104.0, 2.0, app(2, 0.0625)); ent(cu(2) - 1.0, 105.0, 2.0, app(2, -0.0625)); row(Q0, cu(2), 104.0, app(2, 0.0))
    # g3: best d2 = 2^-8 inside the gate, an entry with d2 = 2^-6 OUTSIDE it (16 px away): counted, 2^-8 < 0.25 * 2^-6 is false and
    #     the row would be ambiguous at ratio 0.5; it does not count
    ent(cu(3) + 1.0, 104.0, 2.0, app(3, 0.0625)); ent(cu(3) + 16.0, 104.0, 2.0, app(3, -0.125)); row(Q0, cu(3), 104.0, app(3, 0.0))
    # g4: the same second entry INSIDE the gate: ambiguous at ratio 0.5 (the ratio exactly at equality)
    ent(cu(4) + 1.0, 104.0, 2.0, app(4, 0.0625)); ent(cu(4) - 4.0, 104.0, 2.0, app(4, -0.125)); row(Q0, cu(4), 104.0, app(4, 0.0))
    # g5 .. g9: depth exactly at z_near (in view), at z_far (in view), 0 (never), 8 (beyond z_far) and 1/2 (in front of z_near)
    for g, z in ((5, 1.0), (6, 4.0), (7, 0.0), (8, 8.0), (9, 0.5)):
        ent(cu(g) + 1.0, 104.0, z, app(g, 0.0625)); row(Q0, cu(g), 104.0, app(g, 0.0))
    # g10: an entry whose pixel lies outside the image (u = -4); the row 2 px beside it: matched (the image gate is not applied)
    ent(-4.0, 104.0, 2.0, app(10, 0.0625)); row(Q0, -2.0, 104.0, app(10, 0.0))
    # g11: the appearance exactly at the radius (d2 == r2 must miss), gated
    ent(cu(11) + 1.0, 104.0, 2.0, app(11, 0.25)); row(Q0, cu(11), 104.0, app(11, 0.0))
    # g12: three rows on one entry, two of them tied in d2, the third closer; g13: two tied rows alone (the lower row keeps it)
    ent(cu(12), 200.0, 2.0, app(12, 0.0)); ent(cu(13), 200.0, 2.0, app(13, 0.0))
    row(Q0, cu(12) + 1.0, 200.0, app(12, 0.0625)); row(Q0, cu(12) - 1.0, 200.0, app(12, -0.0625)); row(Q0, cu(12), 201.0, app(12, 0.0, 0.03125))
    row(Q0, cu(13), 199.0, app(13, 0.0, 0.0625)); row(Q0, cu(13) + 2.0, 200.0, app(13, -0.0625))
    # g14: best at 0.125 (1 + 2^-9), a gated entry just outside the radius: it does not count (counted, the row would be ambiguous)
    ent(cu(14) + 1.0, 200.0, 2.0, app(14, 0.125 * (1 + 2.0 ** -9))); ent(cu(14) - 1.0, 200.0, 2.0, app(14, -0.25 * (1 + 2.0 ** -10)))
    row(Q0, cu(14), 200.0, app(14, 0.0))
    # frame 1, moved 1/4 along x: at depth 2 every pixel moves by 512 * 0.25 / 2 = 64.  The same entries again (uniqueness is per
    # frame), and the gate's boundary once more under the translation
    row(Q1, cu(12) + 64.0, 200.0, app(12, 0.0625)); row(Q1, cu(13) + 65.0, 200.0, app(13, 0.0625))
    row(Q1, cu(0) + 64.0, 104.0, app(0, 0.0)); row(Q1, cu(1) + 64.0, 104.0, app(1, 0.0))
    T1 = np.eye(4)
    T1[0, 3] = 0.25
    fr = lambda Q: (np.array([p for p, _ in Q]), np.array([a for _, a in Q]))
    return _case(P, E, [fr(Q0), fr(Q1)], [np.eye(4), T1], K=K_DYADIC, radius_px=8.0, radius=0.25, ratio=ratio, unique=unique, z_near=1, z_far=4,
                 dyadic=True)


def _one_cell(seed=11):
    """2000 entries whose projections fall within 6 px of one pixel (a box narrower than R: one cell holds them), 30 classes"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(3, 6, 2000)
    uv = np.array([300.0, 200.0]) + rng.uniform(-3, 3, (2000, 2))
    P = np.stack([(uv[:, 0] - 320) * z / 500, (uv[:, 1] - 240) * z / 500, z], axis=1).astype(np.float32)
    E = (rng.uniform(-1, 1, (30, 10))[np.arange(2000) % 30] + rng.normal(0, 0.02, (2000, 10))).astype(np.float32)
    frames = []
    for n in (40, 7):
        idx = rng.integers(0, 2000, n)
        frames.append((uv[idx] + rng.normal(0, 0.2, (n, 2)), E[idx] + rng.normal(0, 0.002, (n, 10))))
    return _case(P, E, frames, [np.eye(4), np.eye(4)], ratio=0.5, unique=1)


def _far_outside(seed=13):
    """entries that project far outside the rows' box, under identity priors so that a depth stays what the map holds: a quarter
    of them at pixels around 1e6 and beyond, some at a depth so small (2e-38, still a normal float32) that the reciprocal is 5e37 and
    the pixel infinite, some at x = 3e38; the rows see the rest"""
    c = _scene(1200, [150, 90], seed, ratio=0.8, unique=1, motion=(0.0, 0.0), push=(0.0, 0.0))
    P = c["map_pts"].copy()
    P[0::4, 0] *= 1e4                                         # x of several thousand metres: pixels around 1e6
    P[1::16, 2] = 2e-38
    P[2::64, 0] = 3e38
    return dict(c, map_pts=P)


def _nan_pose(seed=14):
    """three frames, the middle one's prior holds a NaN: all its live rows are NO_ENTRY, its neighbours are untouched"""
    c = _scene(500, [60, 60, 60], seed, ratio=0.8, unique=1)
    poses = [T.copy() for T in c["poses"]]
    poses[1][1, 2] = np.nan
    return dict(c, poses=poses)


def _special(seed=15):
    """NaN, infinity and +-0 in rows and pixels (and in two entries)"""
    c = _scene(40, [12, 12], seed, stray=0.0, ratio=0.8, unique=1)
    P, E = c["map_pts"].copy(), c["map_app"].copy()
    (uv, app), second = c["frames"][0], c["frames"][1]
    uv, app = uv.copy(), app.copy()
    app[0, 3] = np.nan                                        # NAN_ROW
    app[1, 5] = np.inf                                        # an infinity in the row: NO_ENTRY
    uv[2, 0] = np.nan                                         # the pixel: gates nothing
    uv[3, 1] = np.inf
    uv[4] = [-np.inf, np.inf]
    ref = G.run(P, E, c["K"], [(uv, app)], c["poses"][:1], None, 12, 8.0, 0.1)
    e5, e6 = int(ref["entry"][0, 5]), int(ref["entry"][0, 6])
    assert e5 >= 0 and e6 >= 0 and e5 != e6
    E[e5] = 0.0
    E[e5, [1, 4]] = -0.0                                      # an entry of zeros, two of them negative ...
    app[5] = 0.0                                              # ... met by a row of +0 (it takes the entry's bytes)
    E[e6, 2] = np.nan                                         # an entry with a NaN is never matched
    P[int(ref["entry"][0, 7])] = [np.nan, 0.0, 5.0]           # nor one whose point holds a NaN
    return dict(c, map_pts=P, map_app=E, frames=[(uv, app), second])


CASES = {
    "empty_map": lambda: _scene(0, [5, 2], 1, ratio=0.8, unique=1),
    "one_entry": lambda: _case([[0.1, 0.1, 5.0]], np.full((1, 10), 0.5), [(np.array([[330.0, 250.0], [331.0, 251.0], [350.0, 250.0], [330.0, 250.0]]),
                                                                          np.array([[0.5] * 10, [0.51] * 10, [0.5] * 9 + [0.51], [0.5] * 9 + [0.7]]))],
                               [np.eye(4)], ratio=0.8, unique=1),
    "zero_rows": lambda: _scene(50, [3, 3], 2, n_rows=[0, 2], ratio=0.8),
    "n_max_1": lambda: _scene(70, [1, 1, 1], 3, stray=0.0, unique=1),
    "frames14": lambda: _scene(3000, ROW_COUNTS_14, 4, close_pairs=400, ratio=0.8, unique=1),
    "frames3_plain": lambda: _scene(300, [300, 17, 128], 7, close_pairs=30),
    "bound_above_size": lambda: _scene(300, [100, 64], 8, close_pairs=20, ratio=0.8, unique=1, dup_rows=50),
    "one_cell": _one_cell,
    "far_outside": _far_outside,
    "nan_pose": _nan_pose,
    "special": _special,
    "classes": lambda: _scene(1000, [200, 150], 9, classes=50, box=(1.5, 1.1, 3.0, 6.0), radius_px=16.0, ratio=0.8),
    "two_groups": lambda: _scene(300, [5, 3, 6, 4, 5, 2, 6], 10, ratio=0.8, unique=1, capacity=1 << 21),
    "all_in_view": lambda: _scene(600, [200, 50], 16, close_pairs=40, box=(3.0, 2.0, 2.0, 8.0), ratio=0.8, unique=1),
    "dyadic": lambda: _dyadic(0.5, 0),
    "dyadic_plain": lambda: _dyadic(0.0, 0),
    "dyadic_unique": lambda: _dyadic(0.5, 1),
}
DYADIC = ("dyadic", "dyadic_plain", "dyadic_unique")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def run(c, fault=None, **kw):
    c = dict(c, **kw)
    return G.run(c["map_pts"], c["map_app"], c["K"], c["frames"], c["poses"], c["n_rows"], c["n_max"], c["radius_px"], c["radius"], c["ratio"],
                 c["unique"], c["z_near"], c["z_far"], fault=fault)


@functools.lru_cache(maxsize=None)
def reference(name, fault=None):
    return run(case(name), fault=fault)


def groups(c):
    """how many frame groups the call runs on this case: GUIDED_GROUP_BYTES over (12-byte record + 8-byte claim word) per entry of
    the capacity and the two cell tables (visual-odometry_amd/csrc/map_guided.hip, guided_group)"""
    cap = max(c["capacity"], 1024)
    per = 20 * cap + 2 * 4 * (64 * 64 + 1)
    g = max(1, min((128 << 20) // per, len(c["frames"])))
    return -(-len(c["frames"]) // g)
