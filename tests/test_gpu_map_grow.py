"""voe_map_grow[_batch_dev] on the GPU: every case of tests/map_grow_cases.py against the float64 restatement
(tests/map_grow_restatement.py), the map afterwards against a map built by update, equal bytes (three calls, with and without the
optional outputs, the host form, capture and replay, dry_run and NOTHING_ADDED), the cull's own bytes for every appended entry,
and many tracks whose answer is known by construction.

Against float64: the call status, the verdicts, n_obs, n_frames, entry, first_key, refined, the rows and the counts are equal
exactly (tests/test_map_grow_cpu.py shows that no case takes a marginal decision).  The point and the four score statistics lie
within a ceiling per track: 4 x the spread profiles/map_grow_budget.json records for the case between the forward and the
reversed order of summation, plus twice the restatement's a-priori rounding bound (its docstring derives it from eps = 2^-53,
the magnitudes of the terms and the conditioning of A).  No device value went into either.  The point's ceiling is that of the
DOUBLE point and lies far below a float32 ulp, so the stored float32 must be the restatement's own -- except on the tracks the
restatement flags `rounding` from its own numbers alone (the double point lies within 8 bounds of the midpoint of two
neighbouring float32): there either neighbour is a correct rounding -- the stored coordinates may lie one float32 ulp further
apart than the ceiling -- and the statistics are compared only where the stored bits agree."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import map_cull_restatement as Q
import map_grow_cases as Gc
import map_grow_restatement as G
from map_grow_dev import GrowDev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = json.load(open(os.path.join(ROOT, "profiles", "map_grow_budget.json")))["cases"]
STATS = ("mean_sq_px", "max_sq_px", "min_z", "cos_parallax")


def _live_frames(c):
    if c["n_rows"] is None:
        return c["frames"]
    return [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], c["n_rows"])]


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _compare(name, d, got):
    rows, tr, raw = got
    ref = Gc.reference(name)
    st = d.gstats(raw)
    assert st == ref["stats"], (name, st, ref["stats"])
    n = len(tr)
    assert n == min(ref["stats"]["n_tracks"], d.track_cap)
    for k in ("verdict", "n_obs", "n_frames", "entry", "first_key", "refined"):
        assert np.array_equal(tr[k], ref[k][:n]), (name, k, tr[k].tolist()[:20], ref[k][:20].tolist())
    assert not tr["reserved"].any() and not tr["reserved2"].any()
    assert np.array_equal(rows, ref["rows"]), name
    scored = Gc.scored(ref)[:n]
    rest = ~scored
    assert not tr["xyz"][rest].any() and (tr["cos_parallax"][rest] == 1.0).all()
    for k in STATS[:3]:
        assert (tr[k][rest] == 0.0).all(), k
    ceil = Gc.ceilings(name, BUDGET[name])
    dist = np.abs(tr["xyz"].astype(np.float64) - ref["xyz"][:n].astype(np.float64))
    ulp = np.spacing(np.abs(ref["xyz"][:n])).astype(np.float64)
    either = ref["rounding"][:n]
    firm = scored & ~either
    bad = np.nonzero(firm & (dist > ceil[0][:n, None]).any(1))[0]
    assert len(bad) == 0, (name, "xyz", bad[:5].tolist(), tr["xyz"][bad[:5]].tolist(), ref["xyz"][bad[:5]].tolist(), ceil[0][bad[:5]].tolist())
    # (two doubles within the ceiling of one another, rounded to either side of a midpoint: the ceiling and one ulp apart at most)
    assert (dist[scored & either] <= ceil[0][:n][scored & either, None] + ulp[scored & either]).all(), (name, "xyz of a track at a float32 midpoint")
    same_bits = scored & (dist == 0).all(1) & (ref["verdict"][:n] != G.NOT_FINITE)
    assert same_bits[firm & (ref["verdict"][:n] != G.NOT_FINITE)].all()
    worst = [float(np.max(dist[firm] / np.maximum(ceil[0][:n][firm, None], 1e-300), initial=0.0))]
    for k, cl in zip(STATS, ceil[1:]):
        dd = np.abs(tr[k][same_bits] - ref[k][:n][same_bits])
        ratio = np.where(dd == 0, 0.0, dd / np.maximum(cl[:n][same_bits], 1e-300))
        worst.append(float(ratio.max(initial=0.0)))
        assert (ratio <= 1.0).all(), (name, k, tr[k][same_bits][ratio > 1][:5].tolist(), ref[k][:n][same_bits][ratio > 1][:5].tolist())
    print(f"{name}: status {G.STATUS[st['status']]}, {st['n_open']} open rows in {st['n_tracks']} tracks, {st['n_added']} added to {st['n_before']}, by verdict "
          f"{st['by_verdict'][:9]}; {int(either[scored].sum())} tracks at a float32 midpoint; point / mean / max / z / cos at "
          + ", ".join(f"{w:.3g}" for w in worst) + " of their ceilings")


def _added_rows(c, tr):
    """(points, appearances) of the ADDED tracks in track order, from the device's records and the case's frames"""
    n_max = max([len(a) for _, a in c["frames"]] + [1])
    t = np.nonzero(tr["verdict"] == G.ADDED)[0]
    app = [np.asarray(c["frames"][k // n_max][1], np.float32).reshape(-1, 10)[k % n_max] for k in tr["first_key"][t]]
    return tr["xyz"][t].copy(), (np.stack(app) if len(t) else np.zeros((0, 10), np.float32))


@pytest.mark.parametrize("name", list(Gc.CASES))
def test_against_float64_and_every_form(vo, ctx, name):
    c, ref = Gc.case(name), Gc.reference(name)
    d = GrowDev(vo, ctx, c)
    other = vo.Map(ctx)
    try:
        pts0, app0, hist0 = d.map_state()
        ent0 = d.lookups()
        changes = ref["stats"]["status"] == G.OK and not c["params"]["dry_run"]
        runs, after = [], []
        for _ in range(3):                                    # three calls from the same start: the same bytes
            d.reset(); d.clear_grow_out()
            assert d.grow() == 0, ctx.lib.vo_last_error()
            runs.append(d.grow_results())
            after.append(d.map_state())
        for r, s in zip(runs[1:], after[1:]):
            assert _same(r, runs[0]) and _same(s, after[0])
        _compare(name, d, runs[0])
        rows, tr, raw = runs[0]
        pts1, app1, hist1 = after[0]
        assert hist1.tobytes() == hist0.tobytes()
        if changes:
            # the map afterwards: the old entries, then the ADDED tracks in track order; byte for byte the map that an update of
            # the reported rows into the map before the call builds
            xyz, app = _added_rows(c, tr)
            assert pts1.tobytes() == np.concatenate([pts0, xyz]).tobytes() and app1.tobytes() == np.concatenate([app0, app]).tobytes()
            assert len(d.m) == d.M + len(xyz) == ref["stats"]["n_after"]
            other.clear(); other.update(pts0, app0); other.update(xyz, app)
            assert _same(other.read(), (pts1, app1))
            look = d.lookups()
            assert np.array_equal(look, np.where(rows >= 0, rows, -1))
            # a second grow of the result adds nothing and leaves every byte (where no track was left out for lack of room)
            if ref["stats"]["by_verdict"][G.NO_ROOM] == 0:
                d.clear_grow_out()
                assert d.grow() == 0
                ctx.synchronize()
                st2 = d.gstats()
                assert st2["status"] in (G.NO_OPEN_ROWS, G.NOTHING_ADDED) and st2["n_added"] == 0 and st2["n_before"] == st2["n_after"] == len(pts1)
                assert _same(d.map_state(), after[0]) and np.array_equal(d.lookups(), look)
        else:                                                 # dry_run, NOTHING_ADDED, NO_OPEN_ROWS: the map, its table (probed by every class) and its size as before
            assert pts1.tobytes() == pts0.tobytes() and app1.tobytes() == app0.tobytes() and len(d.m) == d.M
            assert np.array_equal(d.lookups(), ent0)
        # without the optional outputs: the same map and statistics
        d.reset(); d.clear_grow_out()
        assert d.grow(outputs=False) == 0
        ctx.synchronize()
        assert d.read(d.d_gstats, 96, np.uint8).tobytes() == raw.tobytes() and _same(d.map_state(), after[0])
        assert (d.read(d.d_rows, d.rows, np.int32) == -7).all()
        # fewer records than tracks: the first ones, and nothing behind them
        if ref["stats"]["n_tracks"] >= 2:
            cap = ref["stats"]["n_tracks"] // 2
            d.reset(); d.clear_grow_out()
            assert d.grow(track_cap=cap) == 0
            ctx.synchronize()
            got = d.read(d.d_tracks, 80 * d.track_cap, np.uint8)
            assert got[: 80 * cap].tobytes() == tr.view(np.uint8)[: 80 * cap].tobytes() and (got[80 * cap:].view(np.int32) == -7).all()
            assert _same(d.map_state(), after[0])
        # the host form from the same start
        d.reset()
        h = d.m.grow(d.cam, _live_frames(c), c["poses"], **c["params"])
        cap = h["rows"].shape[1]                              # (the host form's n_max is the longest LIVE frame: its keys count in that)
        assert np.array_equal(h["rows"], rows[:, :cap]) and (rows[:, cap:] == -1).all() and h["stats"] == d.gstats(raw)
        mine = tr.copy()
        mine["first_key"] = tr["first_key"] // d.n_max * cap + tr["first_key"] % d.n_max
        assert h["tracks"].tobytes() == mine.tobytes()
        assert _same(d.map_state(), after[0])
    finally:
        other.close()
        d.close()


@pytest.mark.parametrize("name", ["room_one_below", "lists"])
def test_dry_run_writes_what_the_real_call_writes(vo, ctx, name):
    c = Gc.case(name)
    d = GrowDev(vo, ctx, c)
    try:
        start, ent0 = d.map_state(), d.lookups()
        d.clear_grow_out()
        assert d.grow(dry_run=True) == 0
        dry = d.grow_results()
        assert _same(d.map_state(), start) and len(d.m) == d.M and np.array_equal(d.lookups(), ent0)
        d.clear_grow_out()
        assert d.grow(dry_run=False) == 0
        assert _same(d.grow_results(), dry) and len(d.m) > d.M
    finally:
        d.close()


@pytest.mark.parametrize("name", ["lists", "example_refined", "sequence_noisy", "verdicts"])
def test_a_dry_run_cull_reports_the_same_bytes_for_every_appended_entry(vo, ctx, name):
    """one device function scores both (map_score.h), compiled with -ffp-contract=off: KEPT, and the same bytes of n_obs, n_frames and
    the four statistics as the track's record"""
    c = Gc.case(name)
    d = GrowDev(vo, ctx, c)
    try:
        d.clear_grow_out()
        assert d.grow() == 0, ctx.lib.vo_last_error()
        _, tr, raw = d.grow_results()
        st = d.gstats(raw)
        added = np.nonzero(tr["verdict"] == G.ADDED)[0]
        assert len(added) == st["n_added"] > 0
        dd = GrowDev(vo, ctx, dict(c, map_pts=np.zeros((st["n_after"], 3), np.float32)), m=d.m)      # the cull's output arrays at the grown size
        try:
            dd.clear_cull_out()
            assert dd.cull() == 0, ctx.lib.vo_last_error()
            ctx.synchronize()
            verdict, remap, ent, craw = dd.cull_results(st["n_after"])
            e = ent[tr["entry"][added]]
            assert (e["verdict"] == Q.KEPT).all(), e["verdict"].tolist()
            for k in ("n_obs", "n_frames") + STATS:
                assert e[k].tobytes() == tr[k][added].tobytes(), k
        finally:
            dd.close()
    finally:
        d.close()


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c = Gc.case("lists")
    d = GrowDev(vo, ctx, c)
    try:
        d.clear_grow_out()
        assert d.grow() == 0
        eager, eager_map = d.grow_results(), d.map_state()
        g = C.c_void_p()
        d.reset(); d.clear_grow_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.grow()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        assert lib.vo_graph_launch(g) == 0                    # the first replay adds
        assert _same(d.grow_results(), eager) and _same(d.map_state(), eager_map)
        assert lib.vo_graph_launch(g) == 0                    # the second leaves every byte
        ctx.synchronize()
        st = d.gstats()
        assert st["status"] == G.NOTHING_ADDED and st["n_added"] == 0 and st["n_before"] == len(eager_map[0])      # (the row seen once stays open)
        assert _same(d.map_state(), eager_map)
        assert lib.vo_graph_destroy(g) == 0
        # frames wider than any call has sized: refused inside a capture before anything is enqueued
        big = GrowDev(vo, ctx, c, n_max=4096, m=d.m)
        try:
            assert lib.vo_ctx_begin_capture(ctx.h) == 0
            assert big.grow() == -6 and b"capture" in lib.vo_last_error()
            assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
            if g.value:
                assert lib.vo_graph_destroy(g) == 0
        finally:
            big.close()
    finally:
        d.close()


def test_a_capture_that_would_have_to_grow_the_map_is_refused(vo, ctx):
    lib = ctx.lib
    c = Gc.case("grows_past_capacity")
    d = GrowDev(vo, ctx, c)
    try:
        assert d.grow(dry_run=True) == 0                      # sizes the workspaces; the map keeps its 1024 entries of room
        ctx.synchronize()
        start = d.map_state()
        g = C.c_void_p()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.grow()
        msg = lib.vo_last_error()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
        if g.value:
            assert lib.vo_graph_destroy(g) == 0
        assert rc == -6 and b"grow inside a graph capture" in msg, msg
        assert _same(d.map_state(), start)
    finally:
        d.close()


def test_many_tracks_known_by_construction(vo, ctx):
    """65 537 tracks: 257 blocks of 256 ranks.  Every second landmark is seen by one frame alone (FEW_OBS), the others by three:
    the verdicts, the entries, the rows and the map's size are known without the restatement; the points land on the truth to
    what the float32 pixels allow (a pixel is good to 2^-15 px = half an ulp below 512, the depth-to-pixel gain is below
    z^2 / (f b) = 49 / 500 per px over the 1 m baseline: 3e-6, asserted with a factor 4)."""
    c, verdict, _ = Gc.many_tracks()
    n = len(verdict)
    d = GrowDev(vo, ctx, c)
    try:
        d.clear_grow_out()
        assert d.grow() == 0, ctx.lib.vo_last_error()
        rows, tr, raw = d.grow_results()
        st = d.gstats(raw)
        full = verdict == G.ADDED
        assert st["n_tracks"] == n and st["n_added"] == int(full.sum()) == 32769 and st["n_after"] == 32769 and st["status"] == G.OK
        assert np.array_equal(tr["verdict"], verdict) and np.array_equal(tr["first_key"], np.arange(n))
        entry = np.where(full, np.cumsum(full) - 1, -1)
        assert np.array_equal(tr["entry"], entry) and np.array_equal(tr["n_obs"], np.where(full, 3, 1))
        assert np.array_equal(rows[0], np.where(full, entry, -2 - np.arange(n)))
        err = np.abs(tr["xyz"][full].astype(np.float64) - c["truth"][full].astype(np.float64)).max()
        print(f"{n} tracks, {st['n_added']} added; largest distance of a coordinate to the truth {err:.3g}")
        assert err < 4 * 3e-6 + 7 * 2.0 ** -24
        pts, app, _ = d.map_state()
        assert len(d.m) == 32769 and app.tobytes() == c["truth_app"][full].tobytes() and pts.tobytes() == tr["xyz"][full].tobytes()
    finally:
        d.close()


def test_refusals(vo, ctx):
    d = GrowDev(vo, ctx, Gc.case("verdicts"))
    try:
        start = d.map_state()
        nan, inf = float("nan"), float("inf")
        for bad in (dict(min_obs=1), dict(min_frames=1), dict(n_rounds=-1), dict(huber_px=-1.0), dict(damping=nan), dict(max_rms_px=-1.0),
                    dict(max_rms_px=nan), dict(max_err_px=-0.5), dict(max_err_px=inf), dict(min_parallax_deg=-1.0), dict(min_parallax_deg=nan),
                    dict(min_parallax_deg=180.0), dict(max_added=-1), dict(track_cap=-1), dict(track_cap=0), dict(d_tracks=d.d_tracks + 4),
                    dict(F=0), dict(F=65536), dict(n_max=-1), dict(uv_stride=1), dict(app_stride=1), dict(K=None), dict(prm=None), dict(d_T=None),
                    dict(d_stats=None), dict(d_stats=d.d_gstats + 4), dict(d_uv=None), dict(d_app=d.d_app + 4), dict(K=np.zeros(9, np.float32))):
            assert d.grow(**bad) == -1, bad
            assert b"voe_map_grow_batch_dev" in ctx.lib.vo_last_error(), bad
        assert d.grow(m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        assert _same(d.map_state(), start) and len(d.m) == d.M
    finally:
        d.close()


def test_bundle_after_cull_and_grow_on_the_example_data(vo, ctx):
    """the 40 pushed landmarks of map_cull_cases' 'example_pushed' are culled, grown back from the frames, and the map is handed to
    vox_map_bundle: its cost per observation is no higher than the bundle's on the untouched world.dat by more than the distance the
    float64 restatement finds between the two maps' start costs (profiles/map_grow_budget.json: downstream; 9.4e-6 against 8.5e-6
    px^2 -- the grown points fit the pixels, world.dat is the truth rounded to float32), with a margin of 2 for float32 storage."""
    import map_cull_cases as Cc
    from map_cull_dev import CullDev
    rec = json.load(open(os.path.join(ROOT, "profiles", "map_grow_budget.json")))["downstream"]
    figure = abs(rec["grown_cost_per_observation"] - rec["world_cost_per_observation"])
    cc, c = Cc.case("example_pushed"), Gc.case("example_after_cull")
    fixed = [True] + [False] * (len(cc["frames"]) - 1)
    d = CullDev(vo, ctx, dict(cc, map_pts=np.asarray(cc["truth"], np.float32)))
    try:
        _, _, _, _, world = d.m.bundle(d.cam, cc["frames"], cc["poses"], fixed, n_rounds=3)
    finally:
        d.close()
    d = CullDev(vo, ctx, cc)
    try:
        h = d.m.cull(d.cam, cc["frames"], cc["poses"], **cc["params"])
        assert h["stats"]["n_kept"] == 960
        g = d.m.grow(d.cam, cc["frames"], cc["poses"], **c["params"])
        assert g["stats"]["status"] == G.OK and g["stats"]["n_added"] == 40 and len(d.m) == 1000
        pts, app = d.m.read()
        key = {a.tobytes(): k for k, a in enumerate(c["truth_app"])}
        dist = max(np.linalg.norm(pts[e].astype(np.float64) - c["truth"][key[app[e].tobytes()]]) for e in range(960, 1000))
        _, _, _, _, grown = d.m.bundle(d.cam, cc["frames"], cc["poses"], fixed, n_rounds=3)
        a, b = world["cost_after"] / world["n_obs"], grown["cost_after"] / grown["n_obs"]
        print(f"40 landmarks culled and grown back, at most {dist:.3g} from world.dat; vox_map_bundle, 3 rounds: on world.dat status {world['status']}, "
              f"{world['cost_before'] / world['n_obs']:.4g} -> {a:.4g} px^2 per observation over {world['n_obs']}; on the grown map status {grown['status']}, "
              f"{grown['cost_before'] / grown['n_obs']:.4g} -> {b:.4g} over {grown['n_obs']} (the restatement's start costs differ by {figure:.3g})")
        assert grown["n_obs"] == world["n_obs"] == rec["world_observations"] and dist < 5.3e-4 * 1.03
        assert b <= a + 2 * figure
    finally:
        d.close()


def test_grow_map_app_on_the_example_data():
    """apps/bin/grow_map checks itself: exit 0 iff something was added and the largest distance of an added point to world.dat
    stays under its default bound"""
    import subprocess
    exe = os.path.join(ROOT, "apps", "bin", "grow_map")
    assert os.path.exists(exe), "apps/bin/grow_map is missing: build() makes it"
    data = os.path.join(ROOT, "tests", "golden", "example_data", "data")
    for args, want in ((["--from-empty"], "ADDED 462"), (["--from-empty", "--min-frames=2", "--parallax=0"], "ADDED 491"), (["--drop=60", "--seed=3"], "ADDED 60")):
        r = subprocess.run([exe, data] + args, capture_output=True, text=True, timeout=120)
        print(r.stdout[-1500:])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        assert want in r.stdout and "the added landmarks lie where world.dat has them" in r.stdout
