"""Every `_dev` call of the device map where the host's bound of the size is NOT the size (tests/map_states.py: slack_1,
slack_300, replayed, overflowed), on the window of tests/map_state_cases.py.

Each call runs on the state's map and on its twin -- a map of the same context holding the same entries, built by one eager
update, whose bound IS its size -- with identical frame, pose and parameter buffers:
  exact against the float64 restatement   every integer output, entry for entry (tests/test_map_states_cpu.py shows that no
                                          decision of these cases is marginal and that entries on both sides of the smaller
                                          bound decide);
  bytes against the twin                  every output, and the map afterwards (points, appearances, the size; the base and rows
                                          of the last update too where the call writes them);
  array ends                              every output array is as long as the TRUE size, with a guard of 64 elements behind it
                                          that must come back untouched: nothing in [size, bound) is ever written.  (The two
                                          arrays of voe_map_align_dev / voe_map_merge_dev that include/vo_map_align.h sizes by
                                          voe_map_size_bound(src) are that long, and hold 0 / -1 beyond the size as it says.)
The host's bound is asserted before the call (by the builder) and after it.

The capture in front of an update (the last test) is the per-frame graph { window call ; vo_map_update_dev }: the call must see
the map as each replay finds it.  It did not before MapBound::launch_bound (visual-odometry_amd/csrc/map_checks.h).

Every index these tests make the kernels form lies in memory the test owns; the guards are read back, not overrun.  No graph is
launched after a map's arrays have moved (the two growths here, the grow and the merge on the full `overflowed` map, are eager
and the last thing done to their maps)."""
import ctypes as C
import time

import numpy as np
import pytest

import map_align_restatement as A
import map_covis_restatement as Cv
import map_state_cases as S
import map_states as MS
from map_states import Outs, Win, i32

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    print(f"\n[time] {request.node.name}: {time.perf_counter() - t0:.2f} s")


def _struct(cls, raw, k=0):
    s = cls()
    C.memmove(C.byref(s), np.ascontiguousarray(raw).ctypes.data + k * C.sizeof(cls), C.sizeof(cls))
    return s.as_dict()


def _ints(d, *drop):
    return {k: v for k, v in d.items() if not isinstance(v, float) and k not in drop}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: the bytes of '{k}' differ between the state's map and its twin"


def _same_map(ma, mb, what, words=1):
    assert ma[0].tobytes() == mb[0].tobytes(), f"{what}: the points afterwards differ"
    assert ma[1].tobytes() == mb[1].tobytes(), f"{what}: the appearances afterwards differ"
    assert np.array_equal(ma[2][:words], mb[2][:words]), (what, ma[2], mb[2])


class Pair:
    """the state's map and its twin, the window in device memory, and one run of a call on both"""

    def __init__(self, vo, ctx, state):
        self.vo, self.ctx, self.state, self.c = vo, ctx, state, S.case(state)
        self.size = self.c["kept"]
        self.st = MS.build(vo, ctx, state, self.c["map_pts"], self.c["map_app"])
        self.tw = MS.build_exact(vo, ctx, *S.cut(self.c))
        self.win = Win(vo, ctx, self.c)
        self.outs = []

    def run(self, call, what, bound_after=None, twin_bound_after=None, words=1, rows_after=None):
        """call(map, outs) on both; returns (outputs of the state's map, its content afterwards)"""
        res = []
        for s, after in ((self.st, bound_after), (self.tw, twin_bound_after)):
            o = Outs(self.ctx)
            self.outs.append(o)
            call(s.m, o)
            out = o.read()
            s.check_bound(after)
            res.append((out, MS.content(self.ctx, s.m, rows_after or s.cap)))
        _same(res[0][0], res[1][0], what)
        _same_map(res[0][1], res[1][1], what, words)
        return res[0]

    def close(self):
        for o in self.outs:
            o.close()
        self.win.close(); self.st.close(); self.tw.close()


@pytest.fixture
def pair(vo, ctx, request):
    p = Pair(vo, ctx, request.param)
    yield p
    p.close()


states = pytest.mark.parametrize("pair", S.STATES, indirect=True)


@states
def test_lookup(pair):
    out, _ = pair.run(lambda m, o: pair.win.lookup(m, o, pair.size), "lookup")
    F, n = pair.win.F, pair.win.n_max
    cnt, ent = i32(out["counts"]), i32(out["entries"]).reshape(F, n)
    pairs, xyz = i32(out["pairs"]).reshape(F, n, 2), out["xyz"].view(np.float32).reshape(F, n, 3)
    for f, (e_ref, p_ref, x_ref) in enumerate(S.reference(pair.state, "lookup")):
        k = len(p_ref)
        assert cnt[f] == k and np.array_equal(ent[f], e_ref) and np.array_equal(pairs[f, :k], p_ref)
        assert xyz[f, :k].tobytes() == np.ascontiguousarray(x_ref, np.float32).tobytes()
        assert MS.untouched(out["pairs"].reshape(F, n, 8)[f, k:]) and MS.untouched(out["xyz"].reshape(F, n, 12)[f, k:])
    if pair.state == "overflowed":                            # the dropped classes are in the frames, and they are misses
        dropped = {r.tobytes() for r in pair.c["map_app"][1024:]}
        hit = [ent[f, i] for f, (_, a) in enumerate(pair.c["frames"]) for i in range(n) if a[i].tobytes() in dropped]
        assert len(hit) >= 100 and all(e == -1 for e in hit)


@states
def test_localise(pair):
    out, _ = pair.run(lambda m, o: pair.win.localise(m, o, pair.size), "localise")
    n_ok = 0
    for f, (e_ref, p_ref, _) in enumerate(S.reference(pair.state, "lookup")):
        st = _struct(pair.vo.MapLocaliseStats, out["stats"], f)
        assert st["n_rows"] == S.ROWS and st["n_hits"] == len(p_ref)
        n_ok += st["status"] == 0
    assert n_ok == pair.win.F                                  # (the scene is clean: every frame localises, on either map)


@states
def test_refine(pair):
    p0 = S.cut(pair.c)[0]
    # with an array for the points the map keeps every byte and the array takes every entry's point, refined or not
    out, (pts, _, _) = pair.run(lambda m, o: pair.win.refine(m, o, pair.size, S.REFINE, xyz=True), "refine into an array")
    ref = S.reference(pair.state, "refine")
    ok = ref["status"] == 0
    xyz = out["xyz"].view(np.float32).reshape(-1, 3)
    assert np.array_equal(i32(out["status"]), ref["status"]) and pts.tobytes() == p0.tobytes() and xyz[~ok].tobytes() == p0[~ok].tobytes()
    # in place
    out, (pts, _, _) = pair.run(lambda m, o: pair.win.refine(m, o, pair.size, S.REFINE), "refine")
    assert np.array_equal(i32(out["status"]), ref["status"])
    st = _struct(pair.vo.MapRefineStats, out["stats"])
    assert _ints(st) == _ints(ref["stats"]), (st, ref["stats"])
    assert xyz[ok].tobytes() == pts[ok].tobytes() and pts[~ok].tobytes() == p0[~ok].tobytes()
    assert (pts[ok] != p0[ok]).any(1).sum() >= 20               # the map moved


@states
def test_refine_poses(pair):
    out, _ = pair.run(lambda m, o: pair.win.refine_poses(m, o, pair.size, S.POSES), "refine_poses")
    ref = S.reference(pair.state, "poses")
    assert np.array_equal(i32(out["status"]), ref["status"])
    st = _struct(pair.vo.MapPoseRefineStats, out["stats"])
    assert _ints(st) == _ints(ref["stats"]), (st, ref["stats"])
    assert out["T"].tobytes() == pair.win.T0.tobytes()          # the poses that came in


@states
def test_adjust(pair):
    out, _ = pair.run(lambda m, o: pair.win.adjust(m, o, pair.size, S.ADJUST), "adjust")
    ref = S.run("adjust", pair.c)
    assert np.array_equal(i32(out["pose_status"]), ref["pose_status"]) and np.array_equal(i32(out["point_status"]), ref["point_status"])
    for k, sw in enumerate(ref["sweeps"]):
        assert _ints(_struct(pair.vo.MapPoseRefineStats, out["stats"][96 * k:])) == _ints(sw["poses"])
        assert _ints(_struct(pair.vo.MapRefineStats, out["stats"][96 * k + 48:])) == _ints(sw["points"])


@states
def test_bundle(pair):
    out, _ = pair.run(lambda m, o: pair.win.bundle(m, o, pair.size, S.BUNDLE), "bundle")
    ref = S.reference(pair.state, "bundle")
    assert np.array_equal(i32(out["pose_status"]), ref["pose_status"]) and np.array_equal(i32(out["point_status"]), ref["point_status"])
    st = _struct(pair.vo.MapBundleStats, out["stats"])
    assert _ints(st) == _ints(ref["stats"]), (st, ref["stats"])
    for k, rd in enumerate(ref["rounds"]):
        got = _struct(pair.vo.MapBundleRound, out["rounds"], k)
        assert (got["accepted"], got["cg_iterations"]) == (rd["accepted"], rd["cg_iterations"])


def _cull_ints(pair, out, ref):
    ent = out["entry"].view(pair.vo.MAP_CULL_ENTRY_DTYPE)
    assert np.array_equal(i32(out["verdict"]), ref["verdict"]) and np.array_equal(i32(out["remap"]), ref["remap"])
    assert np.array_equal(ent["verdict"], ref["verdict"]) and np.array_equal(ent["n_obs"], ref["n_obs"]) and np.array_equal(ent["n_frames"], ref["n_frames"])
    st = _struct(pair.vo.MapCullStats, out["stats"])
    assert st == ref["stats"], (st, ref["stats"])


@states
def test_cull_dry(pair):
    out, (pts, app, _) = pair.run(lambda m, o: pair.win.cull(m, o, pair.size, S.CULL, dry_run=True), "cull (dry run)")
    _cull_ints(pair, out, S.reference(pair.state, "cull"))
    p0, a0 = S.cut(pair.c)
    assert pts.tobytes() == p0.tobytes() and app.tobytes() == a0.tobytes()


@states
def test_cull(pair, vo, ctx):
    out, (pts, app, hdr) = pair.run(lambda m, o: pair.win.cull(m, o, pair.size, S.CULL), "cull", words=3)
    ref = S.reference(pair.state, "cull")
    _cull_ints(pair, out, ref)
    assert pts.tobytes() == ref["points"].tobytes() and app.tobytes() == ref["app"].tobytes() and hdr[0] == ref["stats"]["n_kept"]
    # afterwards every lookup returns remap[the entry it returned before], on both maps (and the bound still holds)
    before = S.reference(pair.state, "lookup")
    after, _ = pair.run(lambda m, o: pair.win.lookup(m, o, pair.size), "lookup after the cull", words=3)
    ent = i32(after["entries"]).reshape(pair.win.F, pair.win.n_max)
    for f, (e_ref, _, _) in enumerate(before):
        assert np.array_equal(ent[f], np.where(e_ref >= 0, ref["remap"][np.maximum(e_ref, 0)], -1))
    c, st = pair.c, pair.st
    if pair.state == "overflowed":
        assert MS.header(ctx, st.m)[3] == 176                   # the count of what was dropped for lack of room stays
        # every dropped class: found by nobody
        q = c["map_app"][1024:]
        o = Outs(ctx); pair.outs.append(o)
        d_q = ctx.to_device(q)
        assert ctx.lib.vo_map_lookup_dev(st.m.h, C.c_void_p(d_q), C.c_int(len(q)), None, C.c_void_p(o.new("pairs", len(q), 8)),
                                         C.c_void_p(o.new("count", 1, 4)), None, None, C.c_void_p(o.new("entries", len(q), 4))) == 0
        got = o.read()
        ctx.free(d_q)
        assert (i32(got["entries"]) == -1).all() and i32(got["count"])[0] == 0
        # the cull rebuilt the table: the overflow's markers are gone, and an eager update that sends 50 dropped classes again
        # appends 50 entries (eager: the map asks the device for its size; the host's bound stays the capacity)
        n0 = ref["stats"]["n_kept"]
        st.m.update(np.arange(150, dtype=np.float32).reshape(50, 3), q[:50])
        p2, a2, h2 = MS.content(ctx, st.m, 1024)
        assert h2[0] == n0 + 50 and a2[n0:].tobytes() == q[:50].tobytes() and p2[:n0].tobytes() == ref["points"].tobytes()
        st.check_bound()
    if pair.state == "replayed":
        # the map a cull leaves is the map an eager update of the survivors builds: both take the same further update -- a
        # dropped class, a kept class with a new point, a class neither has seen -- and agree in content and in every lookup
        keep = ref["keep"]
        other = vo.Map(ctx)
        try:
            other.update(c["map_pts"][:900][keep], c["map_app"][:900][keep])
            rows = np.stack([c["map_app"][np.nonzero(~keep)[0][0]], c["map_app"][np.nonzero(keep)[0][-1]], np.linspace(0.1, 0.9, 10).astype(np.float32)])
            pts3 = np.arange(9, dtype=np.float32).reshape(3, 3)
            for m in (st.m, other):
                m.update(pts3, rows)
            a, b = MS.content(ctx, st.m, 1024), MS.content(ctx, other, 1024)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2][0] == b[2][0] == int(keep.sum()) + 2
            oa, ob = Outs(ctx), Outs(ctx)
            pair.outs += [oa, ob]
            pair.win.lookup(st.m, oa, 0); pair.win.lookup(other, ob, 0)
            _same(oa.read(), ob.read(), "lookups after the cull and an update")
            # one more replay of the captured update (300 rows: 100 survivors, 100 dropped classes, 100 new) lands where
            # oracle.vo_pipeline.Map says
            from oracle import vo_pipeline as P
            rng = np.random.default_rng(9)
            buf_a = np.concatenate([c["map_app"][:900][keep][:100], c["map_app"][:900][~keep][-100:], rng.uniform(-1, 1, (100, 10)).astype(np.float32)])
            buf_p = rng.normal(0, 2, (300, 3)).astype(np.float32)
            dic = P.Map()
            dic.update(list(a[0]), list(a[1]))
            dic.update(list(buf_p), list(buf_a))
            st.captured.write(buf_p, buf_a, 300)
            st.captured.launch()
            p3, a3, h3 = MS.content(ctx, st.m, 1024)
            assert h3[0] == len(dic.pts) <= 1024 and h3[3] == 0
            assert p3.tobytes() == np.array(dic.pts, np.float32).tobytes() and a3.tobytes() == np.array(dic.app, np.float32).tobytes()
            st.check_bound()
        finally:
            other.close()


def _grow_ints(pair, out, ref, dry):
    F, n = pair.win.F, pair.win.n_max
    st = _struct(pair.vo.MapGrowStats, out["stats"])
    want = dict(ref["stats"])                                   # (n_after: as it would be, under dry_run -- the header)
    assert st == want, (st, want)
    assert np.array_equal(i32(out["rows"]).reshape(F, n), ref["rows"])
    tr = out["tracks"].view(pair.vo.MAP_GROW_TRACK_DTYPE)[: st["n_tracks"]]
    for k in ("verdict", "n_obs", "n_frames", "entry", "first_key", "refined"):
        assert np.array_equal(tr[k], ref[k]), k
    assert not out["tracks"][80 * st["n_tracks"]:].any()         # the records beyond the tracks keep their zeros


@states
def test_grow_dry(pair):
    def call(m, o):
        assert pair.win.grow(m, o, pair.size, S.GROW, dry_run=True) == 0, pair.ctx.lib.vo_last_error()
    out, (pts, app, _) = pair.run(call, "grow (dry run)")
    _grow_ints(pair, out, S.reference(pair.state, "grow"), True)
    p0, a0 = S.cut(pair.c)
    assert pts.tobytes() == p0.tobytes() and app.tobytes() == a0.tobytes()


@states
def test_grow(pair):
    """real: the host counts `room` = max_added more.  On the full `overflowed` map the arrays have to grow, on the host, eagerly
    (map_reserve): the capacity doubles, and the bound of a map whose update was captured is the capacity."""
    room = S.GROW["max_added"]

    def call(m, o):
        assert pair.win.grow(m, o, pair.size, S.GROW) == 0, pair.ctx.lib.vo_last_error()
    after = dict(slack_1=301 + room, slack_300=600 + room, replayed=1024, overflowed=2048)[pair.state]
    out, (pts, app, hdr) = pair.run(call, "grow", bound_after=after, twin_bound_after=pair.size + room, words=3, rows_after=pair.size + room)
    ref = S.reference(pair.state, "grow")
    _grow_ints(pair, out, ref, False)
    assert hdr[0] == ref["stats"]["n_after"] and app.tobytes() == ref["app"].tobytes()
    assert pts[: pair.size].tobytes() == S.cut(pair.c)[0].tobytes()
    if pair.state == "overflowed":
        assert hdr[3] == 176


@states
def test_covis_and_window(pair):
    def call(m, o):
        pair.win.covis(m, o, pair.size, S.N_WORDS)
        pair.win.window(m, o, S.N_WORDS, S.WINDOW)
    out, _ = pair.run(call, "covisibility and window")
    ref = S.reference(pair.state, "covis")
    F = pair.win.F
    bits = out["bits"].view(np.uint32).reshape(F, S.N_WORDS)
    assert np.array_equal(bits, ref["bits"]) and np.array_equal(i32(out["counts"]).reshape(F, F), ref["counts"])
    assert _struct(pair.vo.MapCovisStats, out["stats"]) == ref["stats"]
    w = Cv.window(ref["bits"], n_max=pair.win.n_max, **S.WINDOW)
    assert np.array_equal(i32(out["role"]), w["role"]) and np.array_equal(i32(out["n_rows"]), w["n_rows"])
    assert np.array_equal(out["fixed"], w["fixed"]) and np.array_equal(i32(out["order"]), w["order"])
    assert np.array_equal(out["union"].view(np.uint32), w["union"]) and _struct(pair.vo.MapWindowStats, out["wstats"]) == w["stats"]
    assert w["stats"]["n_free"] == S.WINDOW["k_free"] and w["stats"]["n_fixed"] == S.WINDOW["k_fixed"]


@states
def test_transform(pair, o32):
    H = pair.vo.synth.random_isometry(np.random.default_rng(11), 0.02, 0.05).astype(np.float32)
    _, (pts, app, _) = pair.run(lambda m, o: m.transform(H), "transform")
    p0, a0 = S.cut(pair.c)
    assert pts.tobytes() == o32.transform_points(H, p0).tobytes() and app.tobytes() == a0.tobytes()


@pytest.mark.parametrize("state_is", ["dst", "src"])
@states
def test_align_and_merge(pair, vo, ctx, state_is):
    """the state's map once as dst and once as src of voe_map_align_dev and voe_map_merge_dev (TAKE_SRC with the state as src,
    KEEP_DST with it as dst), against a second small map.  pairs, mask and remap are [voe_map_size_bound(src)] as the header
    says: beyond src's size the mask is 0 and the remap -1, and the guard behind the bound is untouched."""
    ref = S.align_reference(pair.state, state_is)
    case = S.align_case(pair.state, state_is)
    policy = 1 if state_is == "dst" else 0
    mref = A.merge(case, ref["S"], policy)
    op, oa = S.other_map(pair.state)
    res, others = [], []
    try:
        for s in (pair.st, pair.tw):
            other = MS.build_exact(vo, ctx, op, oa)
            others.append(other)
            dst, src = (s, other) if state_is == "dst" else (other, s)
            n_max, n_src = src.m.size_bound(), (len(op) if state_is == "dst" else pair.size)
            o = Outs(ctx); pair.outs.append(o)
            MS.align(vo, ctx, dst.m, src.m, o, n_max, S.ALIGN)
            MS.merge(vo, ctx, dst.m, src.m, o, n_max, ref["S"], policy)
            out = o.read()
            if state_is == "src":
                s.check_bound()                                 # src keeps every byte, and the host learns nothing about it
            elif s is pair.tw:
                s.check_bound(pair.size + n_max)                # dst: the host counts src's bound more ...
            else:                                               # ... and the full map has grown, on the host, to twice its capacity
                s.check_bound(dict(slack_1=301 + n_max, slack_300=600 + n_max, replayed=1024, overflowed=2048)[pair.state])
            n = int(i32(out["n_matches"])[0])
            mask, remap = out.pop("mask"), i32(out.pop("remap"))
            pairs = i32(out.pop("pairs")).reshape(-1, 2)
            assert not mask[n_src:].any() and (remap[n_src:] == -1).all() and MS.untouched(pairs[n:].view(np.uint8))
            out.update(mask=mask[:n_src], remap=remap[:n_src], pairs=pairs[:n])
            res.append((out, MS.content(ctx, dst.m, len(mref["pts"]) + 8), MS.content(ctx, src.m, n_src)))
        (a, da, sa), (b, db, sb) = res
        _same(a, b, "align and merge")
        _same_map(da, db, "dst after the merge", 3); _same_map(sa, sb, "src after the merge")
        assert int(i32(a["n_matches"])[0]) == ref["n_matches"] and np.array_equal(a["pairs"], ref["pairs"])
        st = _struct(vo.MapAlignStats, a["stats"])
        assert _ints(st) == _ints(ref["stats"]), (st, ref["stats"])
        assert np.array_equal(a["mask"][: ref["n_matches"]].astype(bool), ref["mask"]) and np.array_equal(i32(a["counts"]), ref["counts"])
        assert np.array_equal(a["remap"], mref["remap"]) and _struct(vo.MapMergeStats, a["mstats"]) == mref["stats"]
        assert da[1].tobytes() == mref["app"].tobytes() and da[2][0] == len(mref["pts"])
        assert da[0].tobytes() == mref["pts"].tobytes()
    finally:
        for x in others:
            x.close()


# ---- the host forms on a map that has dropped rows ------------------------------------------------------------------------------
def test_host_forms_refuse_a_map_that_dropped_rows(vo, ctx):
    c = S.case("overflowed")
    st = MS.build(vo, ctx, "overflowed", c["map_pts"], c["map_app"])
    cam = vo.Camera(*MS.CAM, c["K"])
    try:
        for form in (lambda: st.m.refine(cam, c["frames"], c["poses"], **S.REFINE),
                     lambda: st.m.cull(cam, c["frames"], c["poses"], **S.CULL),
                     lambda: st.m.adjust(cam, c["frames"], c["poses"], c["fixed"], **S.ADJUST),
                     lambda: st.m.bundle(cam, c["frames"], c["poses"], c["fixed"], **S.BUNDLE),
                     lambda: st.m.covisibility(c["frames"]),
                     lambda: len(st.m)):
            with pytest.raises(vo.VoError) as e:
                form()
            assert e.value.code == -5 and "176 entries were dropped" in str(e.value), str(e.value)
        p, a, h = st.content()                                  # and nothing happened to the map
        assert h[0] == 1024 and h[3] == 176 and p.tobytes() == c["map_pts"][:1024].tobytes() and a.tobytes() == c["map_app"][:1024].tobytes()
    finally:
        st.close()


# ---- a window call captured IN FRONT of an update ------------------------------------------------------------------------------
def _captured_call(win, call):
    if call == "refine":
        return lambda m, o: win.refine(m, o, 900, S.REFINE), "status"
    if call == "refine_poses":
        return lambda m, o: win.refine_poses(m, o, 900, S.POSES), None
    if call == "bundle":
        return lambda m, o: win.bundle(m, o, 900, S.BUNDLE), "point_status"
    return lambda m, o: win.cull(m, o, 900, S.CULL), "verdict"


@pytest.mark.parametrize("call", ["refine", "refine_poses", "bundle", "cull"])
def test_a_call_captured_in_front_of_an_update_sees_the_map_each_replay_finds(vo, ctx, call):
    """The per-frame graph { window call ; vo_map_update_dev(300-row buffer) } on a map of capacity 1024 that holds rows [0, 300),
    after one eager warm-up call; three replays with rows [300, 600), [600, 900) and 100 rows the map knows.  After each replay
    the call's outputs and the map equal what the same eager sequence gives on a twin whose bound is its size (refreshed by
    len() before every call) and which held what the map held WHEN THAT REPLAY BEGAN: 300, 600 and 900 entries (fewer after
    the cull's drops).  The output arrays are 900 long -- their pointers are fixed in the graph -- and what lies at or above
    the size of the moment must come back untouched."""
    lib = ctx.lib
    c = S.case("replayed")
    pts, app = c["map_pts"], c["map_app"]
    m, twin = vo.Map(ctx, capacity=1024), vo.Map(ctx, capacity=4096)
    win = Win(vo, ctx, c)
    cap = MS.Captured(vo, ctx, m, 300, with_T=False)
    om, ot = Outs(ctx), Outs(ctx)
    fn, per_entry = _captured_call(win, call)
    g = C.c_void_p()
    try:
        for x in (m, twin):
            x.update(pts[:300], app[:300])
        fn(m, om); fn(twin, ot)                                # the eager warm-up, on both (the cull's drops too)
        _same(om.read(), ot.read(), "warm-up")
        om.refill()
        cap.write(pts[300:600], app[300:600], 300)
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        try:
            fn(m, om)
            rc = lib.vo_map_update_dev(m.h, C.c_void_p(cap.d_p), C.c_void_p(cap.d_a), C.c_int(300), C.c_void_p(cap.d_n), None)
        finally:
            assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0
        assert rc == 0, lib.vo_last_error()
        assert m.size_bound() == 1024
        work = []
        buffers = [(pts[300:600], app[300:600], 300), (pts[600:900], app[600:900], 300), (pts[:300], app[:300], 100)]
        for k, (bp, ba, count) in enumerate(buffers):
            size0 = MS.header(ctx, m)[0]
            cap.write(bp, ba, count)
            om.refill()
            assert lib.vo_graph_launch(g) == 0
            got = om.read()
            assert len(twin) == size0                           # the twin's bound is its size when its call runs
            ot.refill()
            fn(twin, ot)
            cap.eager(twin)
            want = ot.read()
            _same(got, want, f"replay {k + 1} on {size0} entries")
            _same_map(MS.content(ctx, m, 1024), MS.content(ctx, twin, 1024), f"the map after replay {k + 1}", 3)
            if per_entry:
                per = got[per_entry].reshape(900, -1)
                assert MS.untouched(per[size0:]) and not MS.untouched(per[:size0])
                work.append(int((i32(per[:size0].copy()).ravel()[300:] == 0).sum()))      # OK / KEPT entries at or above the capture's bound()
            else:
                work.append(_struct(vo.MapPoseRefineStats, got["stats"])["n_obs"])
        print(f"{call}: per replay {work}")
        if per_entry:
            assert work[0] == 0 and work[1] >= 20 and work[2] >= 20, work      # entries the capture's bound() would have skipped
        else:
            assert work[0] < work[1] < work[2], work               # observations of entries beyond it
        assert m.size_bound() == 1024
    finally:
        if g.value:
            lib.vo_graph_destroy(g)
        om.close(); ot.close(); cap.close(); win.close(); m.close(); twin.close()
