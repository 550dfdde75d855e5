"""vo_map_update[_dev] (csrc/map.hip) where its table, its scan and its captured form can go wrong without random data noticing:
cloud sizes at the wave and workgroup edges, more than 1024 workgroups in the scan, live-row counts at and beyond their limits,
classes of equal 32-bit tags and probe chains over the table's end (tests/map_update_cases.py), replayed captures, and a map
that overflows.  Every case compares entries, appearance bits and points byte for byte against oracle.vo_pipeline.Map (the
literal double loop too while the map stays small) and looks every member up against tests/map_localise_restatement.py."""
import ctypes as C
import time

import numpy as np
import pytest

import map_localise_restatement as R
import map_update_cases as U
from map_refine_dev import RefineDev
from oracle import vo_pipeline as P

pytestmark = pytest.mark.gpu

LITERAL_MAX = 600                                             # the O(N M) double loop only below this many entries
ROT = np.array([[0, -1, 0, 0.5], [1, 0, 0, -2], [0, 0, 1, 1], [0, 0, 0, 1]], np.float32)


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    print(f"\n[time] {request.node.name}: {time.perf_counter() - t0:.2f} s")


class Ref:
    """the dictionary map and, while it is small, the literal double loop beside it"""

    def __init__(self, literal=True):
        self.dic = P.Map()
        self.lit = ([], []) if literal else None

    def update(self, pts, app):
        pts = np.asarray(pts, np.float32).reshape(-1, 3); app = np.asarray(app, np.float32).reshape(-1, 10)
        self.dic.update(list(pts), list(app))
        if self.lit is not None:
            if len(self.dic.pts) > LITERAL_MAX:
                self.lit = None
            else:
                P.literal_update(self.lit[0], self.lit[1], list(pts), list(app))

    @property
    def pts(self):
        return np.array(self.dic.pts, np.float32).reshape(-1, 3)

    @property
    def app(self):
        return np.array(self.dic.app, np.float32).reshape(-1, 10)


def _same(m, ref):
    """the device map equals the reference, byte for byte; returns its bytes"""
    p, a = m.read()
    assert len(p) == len(ref.dic.pts), (len(p), len(ref.dic.pts))
    assert a.tobytes() == ref.app.tobytes()                    # bits: the FIRST occurrence's row stays
    assert p.tobytes() == ref.pts.tobytes()                    # the LAST occurrence's point
    if ref.lit is not None:
        assert p.tobytes() == np.array(ref.lit[0], np.float32).tobytes() and a.tobytes() == np.array(ref.lit[1], np.float32).tobytes()
    return p.tobytes() + a.tobytes()


def _lookups(m, map_app, map_pts, queries):
    """vo_map_lookup of the queries (and of rows nobody entered) against the restatement: entries, pairs, points"""
    q = np.concatenate([np.asarray(queries, np.float32).reshape(-1, 10), np.full((3, 10), 0.123, np.float32) * np.arange(1, 4, dtype=np.float32)[:, None]])
    pairs, ent, xyz = m.lookup(q, want_points=True)
    ent_ref, pairs_ref, xyz_ref = R.lookup(map_app, q, map_pts)
    assert np.array_equal(ent, ent_ref)
    assert np.array_equal(pairs, pairs_ref)
    assert xyz.tobytes() == np.ascontiguousarray(xyz_ref, np.float32).tobytes()
    return ent


def _moved(o32, T, pts):
    return o32.transform_points(T, pts) if (T is not None and len(pts)) else pts


# ---- 1. tile edges ----------------------------------------------------------------------------------------------------------
EDGES = (0, 63, 64, 255, 256)


def _edge_cloud(rng, n, known, variant):
    """n rows, about half of them classes of `known` (if any).  variant 0: a class whose first occurrence is row 0 and whose last
    is row n-1, one at rows 63 and 64 (a wave edge), one at rows 255 and 256 (a workgroup edge).  variant 1: NaN rows at 0, 63,
    64, 255, 256 and n-1, and the same classes one row further in (1 .. n-2, 62 / 65, 254 / 257)."""
    app = rng.uniform(-1, 1, (n, 10)).astype(np.float32)
    if len(known):
        take = rng.random(n) < 0.5
        app[take] = known[rng.choice(len(known), int(take.sum()), replace=len(known) < n)]
    d = variant
    spans = [(0 + d, n - 1 - d), (63 - d, 64 + d), (255 - d, 256 + d)]
    held = []
    for a, b in spans:
        if 0 <= a < b < n:
            app[a] = app[b] = rng.uniform(-1, 1, 10).astype(np.float32)
            held.append((a, b))
    nans = []
    if variant == 1:
        nans = sorted({i for i in EDGES + (n - 1,) if i < n})
        app[nans, rng.integers(0, 10, len(nans))] = np.nan
    pts = rng.normal(0, 3, (n, 3)).astype(np.float32)
    return pts, app, held, nans


def _tile_edge_case(vo, m, o32, rng, n):
    base_p, base_a = rng.normal(0, 3, (1000, 3)).astype(np.float32), rng.uniform(-1, 1, (1000, 10)).astype(np.float32)
    for onto in (0, 1000):
        for T in (None, ROT):
            for variant in (0, 1):
                m.clear()
                ref = Ref()
                if onto:
                    m.update(base_p, base_a); ref.update(base_p, base_a)
                pts, app, held, nans = _edge_cloud(rng, n, base_a[:onto], variant)
                if variant == 0 and n >= 2:
                    assert held[0] == (0, n - 1) and (n < 65 or (63, 64) in held) and (n < 257 or (255, 256) in held)
                if variant == 1:
                    assert np.isnan(app[[i for i in EDGES + (n - 1,) if i < n]]).any(axis=1).all()
                m.update(pts, app, T)
                ref.update(_moved(o32, T, pts), app)
                _same(m, ref)
                for a, b in held:                               # one entry per spanning class, holding row b's point
                    assert (ref.app == app[a]).all(axis=1).sum() == 1
                assert len(ref.dic.pts) >= onto + len(nans)      # every NaN row was appended
                _lookups(m, ref.app, ref.pts, app)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2049])
def test_tile_edges(vo, ctx, o32, n):
    m = vo.Map(ctx)
    _tile_edge_case(vo, m, o32, np.random.default_rng(1000 + n), n)
    m.close()


# ---- 2. the scan's carry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [262145, 262145 + 3 * 256])
def test_scan_carry_over_1024_workgroups(vo, ctx, n):
    """map_scan_kernel takes 1024 workgroup counts per pass: 262 145 rows are 1025 workgroups, the last of one row -- a new class,
    whose entry index is the carry.  262 913 rows put three whole workgroups and one row behind the boundary, so that runs of
    workgroups where every row is new and runs with no new class lie on BOTH sides of it."""
    rng = np.random.default_rng(n)
    nb = (n + 255) // 256
    assert nb > 1024
    wg = np.arange(n) // 256
    new = rng.random(n) < 0.6
    all_new = [(40, 48), (1008, 1016), (1024, 1025), (1026, 1027)]
    none_new = [(300, 310), (1016, 1024), (1025, 1026)]
    for a, b in all_new:
        new[(wg >= a) & (wg < b)] = True
    for a, b in none_new:
        new[(wg >= a) & (wg < b)] = False
    new[0] = True
    new[n - 1] = True                                          # the last row's entry index is M + everything before it
    new_idx = np.nonzero(new)[0]
    before = np.searchsorted(new_idx, np.arange(n))            # new rows in front of row i
    label = np.arange(n)
    dup = np.nonzero(~new)[0]
    label[dup] = new_idx[(rng.random(len(dup)) * before[dup]).astype(np.int64)]
    far = dup[(wg[dup] >= 1016)]
    label[far[::2]] = new_idx[(rng.random(len(far[::2])) * 1000).astype(np.int64)]      # reaching back to the first workgroups
    assert (label[dup] < dup).all() and new[label].all()
    assert (wg[label[far]] < 8).any() and (wg[far] >= 1016).all()              # duplicates at the boundary of rows far in front of it
    base = rng.uniform(-1, 1, (n, 10)).astype(np.float32)
    app = base[label]
    app[new_idx[5::5000], 3] = np.nan                          # a few NaN rows among the new ones
    pts = rng.normal(0, 2, (n, 3)).astype(np.float32)
    assert 0.55 < new.mean() < 0.65
    counts = np.bincount(wg, weights=new, minlength=nb)
    assert (counts[1008:1016] == 256).all() and (counts[1016:1024] == 0).all() and counts[nb - 1] == 1
    m = vo.Map(ctx, capacity=n)
    ref = Ref(literal=False)
    m.update(pts, app); ref.update(pts, app)
    assert abs(len(ref.dic.pts) - int(new.sum())) < 200        # (a copy of a row that was given a NaN is a class of its own)
    _same(m, ref)
    n2 = 1025
    app2 = rng.uniform(-1, 1, (n2, 10)).astype(np.float32)
    app2[::2] = ref.app[rng.choice(len(ref.app), len(app2[::2]), replace=False)]      # half of them known (a NaN entry's copy is new again)
    pts2 = rng.normal(0, 2, (n2, 3)).astype(np.float32)
    m.update(pts2, app2); ref.update(pts2, app2)
    _same(m, ref)
    sample = np.concatenate([app[n - 600:], app[:300], app2])
    _lookups(m, ref.app, ref.pts, sample)
    m.close()


# ---- 3. the live-row count in device memory ------------------------------------------------------------------------------
def test_device_row_counts_at_their_edges(vo, ctx, o32):
    rng = np.random.default_rng(3)
    n_max = 700
    base_p, base_a = rng.normal(0, 3, (300, 3)).astype(np.float32), rng.uniform(-1, 1, (300, 10)).astype(np.float32)
    m = vo.Map(ctx)
    d_p, d_a, d_n, d_T = ctx.alloc(12 * n_max), ctx.alloc(40 * n_max), ctx.alloc(16), ctx.to_device(np.ascontiguousarray(ROT.T))
    for count, live in ((0, 0), (1, 1), (699, 699), (700, 700), (705, 700), (-3, 0)):
        app = rng.uniform(-1, 1, (n_max, 10)).astype(np.float32)
        app[::3] = base_a[rng.integers(0, 300, len(app[::3]))]                   # known classes, with other points
        app[10::50, 6] = np.nan
        # behind the live count: known classes with other points, new classes, NaN rows -- none may reach the map
        tail = app[live:]
        assert live >= 699 or ((tail[:, None, :] == base_a[None, :, :]).all(2).any() and np.isnan(tail).any() and len(tail) > 100)
        pts = rng.normal(0, 3, (n_max, 3)).astype(np.float32)
        m.clear()
        ref = Ref()
        m.update(base_p, base_a); ref.update(base_p, base_a)
        ctx.h2d(d_p, pts); ctx.h2d(d_a, app); ctx.h2d(d_n, np.array([count], np.int32))
        m.update_dev(d_p, d_a, n_max, d_n, d_T)
        ref.update(_moved(o32, ROT, pts[:live]), app[:live])
        assert len(m) == len(ref.dic.pts)                       # the size, read back after each value
        _same(m, ref)
        if live == 0:
            assert len(m) == 300
        _lookups(m, ref.app, ref.pts, app)
    for d in (d_p, d_a, d_n, d_T):
        ctx.free(d)
    m.close()


# ---- 4. equal tags, one home slot, chains over the table's end ----------------------------------------------------------
def _members(rng):
    fams = [U.tag_family(rng, 6) for _ in range(8)]
    chain, wrap = U.slot_chain(rng, 40), U.wrap_chain(rng, 36)
    for f in fams:                                             # what the rows were built for, on the rows in hand
        U.check_family(f)
    U.check_chain(chain); U.check_chain(wrap, wrap=True)
    return fams, chain, wrap


def _scenario(vo, ctx, kind, seed):
    rng = np.random.default_rng(seed)
    fams, chain, wrap = _members(rng)
    mem = np.concatenate(fams + [chain, wrap])
    K = len(mem)
    U.check_zero_flip(mem, U.flip_zeros(mem))
    first_half = np.concatenate([f[:3] for f in fams] + [chain[::2], wrap[::2]])
    second_half = np.concatenate([f[3:] for f in fams] + [chain[1::2], wrap[1::2]])
    fresh = lambda k: rng.uniform(-1, 1, (k, 10)).astype(np.float32)
    P3 = lambda k: rng.normal(0, 3, (k, 3)).astype(np.float32)
    sh = lambda rows: rows[rng.permutation(len(rows))]
    clouds = []
    if kind == "one_cloud":
        clouds = [sh(np.concatenate([mem, fresh(50), U.nan_copy(mem[::7])]))]
    elif kind == "three_updates":
        parts = np.array_split(sh(mem), 3)
        clouds = [sh(np.concatenate([p, fresh(20)])) for p in parts]
    elif kind == "half_known":
        clouds = [sh(first_half), sh(np.concatenate([second_half, first_half[::2], fresh(30)]))]
    elif kind == "repeats":
        clouds = [sh(np.concatenate([mem, U.flip_zeros(mem), mem, U.nan_copy(mem[::5])])), sh(np.concatenate([U.flip_zeros(mem), mem]))]
    elif kind == "growth":                                     # capacity 1024 -> grown and re-hashed between the halves of every family
        clouds = [sh(np.concatenate([first_half, fresh(880)])), sh(np.concatenate([second_half, fresh(700), U.nan_copy(mem[::9])])),
                  sh(np.concatenate([U.flip_zeros(mem), mem, fresh(10)]))]
    m = vo.Map(ctx, capacity=1024)
    ref = Ref()
    for app in clouds:
        pts = P3(len(app))
        m.update(pts, app); ref.update(pts, app)
        out = _same(m, ref)
    n_nan = int(sum(U.has_nan(c).sum() for c in clouds))
    n_fresh = {"one_cloud": 50, "three_updates": 60, "half_known": 30, "repeats": 0, "growth": 1590}[kind]
    assert len(ref.dic.pts) == K + n_fresh + n_nan              # one entry per member: an equal tag is not an equal class
    if kind == "growth":
        assert len(ref.dic.pts) > 1024
    ent = _lookups(m, ref.app, ref.pts, np.concatenate([mem, U.flip_zeros(mem), U.nan_copy(mem)]))
    assert len(set(ent[:K].tolist())) == K and (ent[:K] >= 0).all() and np.array_equal(ent[:K], ent[K:2 * K]) and (ent[2 * K:3 * K] == -1).all()
    m.close()
    return out


@pytest.mark.parametrize("kind", ["one_cloud", "three_updates", "half_known", "repeats", "growth"])
def test_equal_tags_and_probe_chains(vo, ctx, kind):
    runs = [_scenario(vo, ctx, kind, seed=44) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]                        # min / max over cloud indices decide, not the order of arrival


# ---- 5. - 7. captured updates -------------------------------------------------------------------------------------------
class Captured:
    """one vo_map_update_dev on fixed device buffers (cloud, live count, isometry), captured after one eager call has sized the
    map's scratch; launch() rewrites the buffers in place and replays"""

    def __init__(self, vo, c, m, n_max, with_T=True):
        self.c, self.m, self.lib, self.n_max = c, m, c.lib, n_max
        self.d_p, self.d_a, self.d_n = c.alloc(12 * n_max), c.alloc(40 * n_max), c.alloc(16)
        self.d_T = c.alloc(64) if with_T else None
        self.g = None

    def write(self, pts, app, count, T=None):
        pts = np.asarray(pts, np.float32); app = np.asarray(app, np.float32)
        assert pts.shape == (self.n_max, 3) and app.shape == (self.n_max, 10)
        self.c.h2d(self.d_p, pts); self.c.h2d(self.d_a, app); self.c.h2d(self.d_n, np.array([count], np.int32))
        if self.d_T:
            self.c.h2d(self.d_T, np.ascontiguousarray(np.asarray(T, np.float32).T))

    def eager(self, m=None):
        (self.m if m is None else m).update_dev(self.d_p, self.d_a, self.n_max, self.d_n, self.d_T)
        self.c.synchronize()

    def capture(self):
        assert self.lib.vo_ctx_begin_capture(self.c.h) == 0
        try:
            rc = self.lib.vo_map_update_dev(self.m.h, C.c_void_p(self.d_p), C.c_void_p(self.d_a), C.c_int(self.n_max), C.c_void_p(self.d_n),
                                            C.c_void_p(self.d_T) if self.d_T else None)
        finally:
            g = C.c_void_p()
            assert self.lib.vo_ctx_end_capture(self.c.h, C.byref(g)) == 0
        assert rc == 0, self.lib.vo_last_error()
        self.g = g

    def launch(self):
        assert self.lib.vo_graph_launch(self.g) == 0
        self.c.synchronize()

    def close(self):
        if self.g:
            self.lib.vo_graph_destroy(self.g)
        for d in (self.d_p, self.d_a, self.d_n, self.d_T):
            if d:
                self.c.free(d)


def test_captured_update_replays_as_the_eager_sequence(vo, o32):
    c = vo.Context(0)
    rng = np.random.default_rng(5)
    n_max = 400
    m, twin = vo.Map(c, capacity=4096), vo.Map(c, capacity=4096)
    ref = Ref(literal=False)
    cap = Captured(vo, c, m, n_max)
    seen = np.zeros((0, 10), np.float32)

    def step(run):
        nonlocal seen
        app = rng.uniform(-1, 1, (n_max, 10)).astype(np.float32)
        if len(seen):
            app[::3] = seen[rng.integers(0, len(seen), len(app[::3]))]
        app[7::90, 1] = np.nan
        pts = rng.normal(0, 3, (n_max, 3)).astype(np.float32)
        count = int(rng.integers(250, n_max + 1))
        T = vo.synth.random_isometry(rng, 0.3, 0.5).astype(np.float32)
        cap.write(pts, app, count, T)
        run()
        cap.eager(twin)                                        # the same buffers, eagerly, on the twin
        ref.update(_moved(o32, T, pts[:count]), app[:count])
        _same(m, ref)
        p, a = m.read(); tp, ta = twin.read()
        assert p.tobytes() == tp.tobytes() and a.tobytes() == ta.tobytes()
        seen = np.concatenate([seen, app[:count]])

    step(cap.eager)
    cap.capture()
    assert len(m) == len(ref.dic.pts)                           # a capture records, it does not run
    for _ in range(5):
        step(cap.launch)
    _lookups(m, ref.app, ref.pts, seen[-500:])
    # growth inside a capture is still refused, and the context stays usable
    small = vo.Map(c, capacity=1024)
    pts, app = rng.normal(0, 1, (600, 3)).astype(np.float32), rng.uniform(-1, 1, (600, 10)).astype(np.float32)
    small.update(pts, app)
    lib = c.lib
    assert lib.vo_ctx_begin_capture(c.h) == 0
    try:
        assert lib.vo_map_update_dev(small.h, C.c_void_p(cap.d_p), C.c_void_p(cap.d_a), C.c_int(400), None, None) == 0
        assert lib.vo_map_update_dev(small.h, C.c_void_p(cap.d_p), C.c_void_p(cap.d_a), C.c_int(400), None, None) == -6
    finally:
        g = C.c_void_p()
        assert lib.vo_ctx_end_capture(c.h, C.byref(g)) == 0
    assert len(small) == 600
    lib.vo_graph_destroy(g)
    small.update(pts[:10], app[:10])
    assert len(small) == 600
    cap.close(); small.close(); m.close(); twin.close()
    c.close()


def _refine_case(rng, map_pts, map_app, seen):
    """two cameras that see the entries `seen` exactly (pixels = projections): every other entry is UNSEEN"""
    K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], np.float32)
    poses = [np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)]
    poses[1][0, 3] = 0.5
    frames = []
    for T in poses:
        pc = map_pts[seen].astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]
        uv = (pc @ K.T.astype(np.float64))
        frames.append(((uv[:, :2] / uv[:, 2:3]).astype(np.float32), map_app[seen]))
    return dict(K=K, frames=frames, poses=poses, map_pts=map_pts, map_app=map_app, n_rows=None,
                params=dict(n_rounds=3, min_obs=2, huber_px=0.0, damping=0.0))


def test_host_acts_on_the_true_size_after_replays(vo, o32):
    """the host's bound of the size counts a captured update once, whatever the graph's replays add: an eager update afterwards
    must ask the device (and grow), and vo_map_transform / vo_map_refine_batch_dev must reach every entry"""
    c = vo.Context(0)
    rng = np.random.default_rng(6)
    m = vo.Map(c, capacity=1024)
    ref = Ref(literal=False)
    cap = Captured(vo, c, m, 300, with_T=False)

    def fresh():
        pts = rng.normal(0, 1, (300, 3)).astype(np.float32)
        pts[:, 2] = rng.uniform(3, 6, 300).astype(np.float32)          # in front of the refinement's cameras
        return pts, rng.uniform(-1, 1, (300, 10)).astype(np.float32)

    for k, run in enumerate((cap.eager, None, cap.launch, cap.launch)):
        if run is None:
            cap.capture()
            continue
        pts, app = fresh()
        cap.write(pts, app, 300)
        run()
        ref.update(pts, app)
    assert _read_dev(c, m, 1024)[2] == 900                     # (read from the device arrays: vo_map_size would refresh the host's bound)
    pts, app = fresh()
    cap.write(pts, app, 300)
    cap.eager()                                                # 900 + 300 > 1024: the map grows, nothing is dropped
    ref.update(pts, app)
    assert len(m) == 1200
    _same(m, ref)
    _lookups(m, ref.app, ref.pts, ref.app[::3])
    # a second map in the same state, read by nothing that refreshes the host's bound: 1200 entries in a map of capacity 4096
    m2 = vo.Map(c, capacity=4096)
    cap2 = Captured(vo, c, m2, 300, with_T=False)
    ref2 = Ref(literal=False)
    for k, run in enumerate((cap2.eager, None, cap2.launch, cap2.launch, cap2.launch)):
        if run is None:
            cap2.capture()
            continue
        pts, app = fresh()
        cap2.write(pts, app, 300)
        run()
        ref2.update(pts, app)
    H = vo.synth.random_isometry(rng, 0.02, 0.05).astype(np.float32)
    lib = c.lib
    assert lib.vo_map_transform(m2.h, np.ascontiguousarray(H.T).ctypes.data_as(C.c_void_p)) == 0      # the host knows of 600 entries
    moved = o32.transform_points(H, ref2.pts)
    seen = np.arange(5, 1200, 7)                               # entries on both sides of the stale bound
    case = _refine_case(rng, moved, ref2.app, seen)
    r = RefineDev(vo, c, case, m=m2)
    r.clear_out()
    assert r.call(status=True, xyz=False) == 0, lib.vo_last_error()
    c.synchronize()
    st, _, raw = r.results()
    assert len(st) == 1200 and (st != -7).all()                 # a status for every entry
    is_seen = np.zeros(1200, bool); is_seen[seen] = True
    assert (st[~is_seen] == 1).all()                            # VO_MAP_REFINE_UNSEEN
    assert (st[is_seen] != 1).all() and (st[is_seen] != 2).all()      # two observations each, min_obs 2: refined, behind the bound too
    assert r.stats(raw)["n_entries"] == 1200
    p2, a2 = m2.read()
    assert len(p2) == 1200 and a2.tobytes() == ref2.app.tobytes()
    unseen = ~is_seen
    assert p2[unseen].tobytes() == moved[unseen].tobytes()      # vo_map_transform moved every entry
    r.close(); cap.close(); cap2.close(); m.close(); m2.close()
    c.close()


def _read_dev(c, m, cap):
    """the map's device arrays through vo_map_dev_ptrs, whole: (points (cap, 3), appearances (cap, 10), size)"""
    d_p, d_a, d_s = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert c.lib.vo_map_dev_ptrs(m.h, C.byref(d_p), C.byref(d_a), C.byref(d_s)) == 0
    p = np.zeros((cap, 3), np.float32); a = np.zeros((cap, 10), np.float32); s = np.zeros(4, np.int32)
    c.d2h(p, d_p.value); c.d2h(a, d_a.value); c.d2h(s, d_s.value)
    return p, a, int(s[0])


def test_overflowing_replays_cut_the_map_and_count_what_they_drop(vo, o32):
    """A captured update cannot grow the map; what does not fit is dropped, counted, and leaves nothing behind that a later
    update or lookup could mistake for an entry.  ONE cloud buffer of 400 rows serves every launch, so every index the kernels
    form lies in memory this test owns.  (The parent's defect was a read outside the cloud when the NEXT cloud is smaller than
    the one that overflowed; this test is built not to provoke that read and is not claimed to have found it.)"""
    c = vo.Context(0)
    lib = c.lib
    rng = np.random.default_rng(7)
    CAP, N = 1024, 400
    m = vo.Map(c, capacity=CAP)
    dic = P.Map()
    cap = Captured(vo, c, m, N, with_T=False)
    fresh = lambda k: rng.uniform(-1, 1, (k, 10)).astype(np.float32)
    dropped_total, overflows, dropped_rows = 0, 0, np.zeros((0, 10), np.float32)
    plans = ["eager", "capture", "fresh", "overflow", "again", "known", "again"]
    for plan in plans:
        if plan == "capture":
            cap.capture()
            continue
        known = np.array(dic.app, np.float32).reshape(-1, 10)
        known = known[~U.has_nan(known)] if len(known) else known
        if plan in ("eager", "fresh"):
            app = fresh(N)
        elif plan == "overflow":
            app = np.concatenate([fresh(300), known[rng.choice(len(known), 100, replace=False)]])[rng.permutation(N)]
        elif plan == "again":                                   # what was dropped comes again (dropped and counted again), with known and new rows
            k = min(len(dropped_rows), 80)
            app = np.concatenate([dropped_rows[:k], known[rng.choice(len(known), N - k - 30, replace=False)], fresh(28), U.nan_copy(fresh(2))])
            app = app[rng.permutation(N)]
        else:
            app = known[rng.choice(len(known), N, replace=False)]
        pts = rng.normal(0, 3, (N, 3)).astype(np.float32)
        cap.write(pts, app, N)
        (cap.eager if plan == "eager" else cap.launch)()
        full = P.Map(); full.pts, full.app, full.idx = list(dic.pts), list(dic.app), dict(dic.idx)
        full.update(list(pts), list(app))
        cut = U.cut_update(dic, pts, app, CAP)
        if cut:
            overflows += 1
            dropped_rows = np.array(full.app[CAP:], np.float32).reshape(-1, 10)
            dropped_rows = dropped_rows[~U.has_nan(dropped_rows)]
        dropped_total += cut
        p, a, size = _read_dev(c, m, CAP)
        want_p, want_a = np.array(dic.pts, np.float32).reshape(-1, 3), np.array(dic.app, np.float32).reshape(-1, 10)
        assert size == len(want_p) <= CAP
        assert a[:size].tobytes() == want_a.tobytes() and p[:size].tobytes() == want_p.tobytes()
        n = C.c_int()
        rc = lib.vo_map_size(m.h, C.byref(n))
        assert n.value == size
        if dropped_total:
            assert rc == -5 and (b"%d entries were dropped" % dropped_total) in lib.vo_last_error(), lib.vo_last_error()
        else:
            assert rc == 0
        # lookups find exactly the entries below the capacity: the dropped classes are found by nobody
        q = np.concatenate([app, dropped_rows[:100], want_a[::5]])
        ent = _lookups(m, want_a, want_p, q)
        if cut:
            assert (ent[len(app):len(app) + min(len(dropped_rows), 100)] == -1).all()
    assert overflows >= 2 and 0 < dropped_total < 512, (overflows, dropped_total)
    m.clear()
    assert len(m) == 0
    _tile_edge_case(vo, m, o32, np.random.default_rng(1257), 257)
    cap.close(); m.close()
    c.close()
