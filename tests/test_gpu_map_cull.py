"""voe_map_cull[_batch_dev] on the GPU: every case of tests/map_cull_cases.py against the float64 restatement
(tests/map_cull_restatement.py), the compaction at its block edges, the map afterwards against a map built by update, equal
bytes (three calls, with and without the optional outputs, the host form, capture and replay, dry_run and NOTHING_DROPPED) and
the joint adjustment downstream of a cull.

Against float64: the call status, the verdicts, n_obs, n_frames, the remap and the counts are equal exactly (tests/
test_map_cull_cpu.py shows that no case takes a marginal decision).  mean_sq_px, max_sq_px, min_z and cos_parallax lie within a
ceiling per entry: 4 x the spread profiles/map_cull_budget.json records for the case (mean_sq_px: forward against reversed order
of summation; the others: one expression order against another) plus twice the restatement's a-priori rounding bound of the
statistic, which is derived from eps = 2^-53 and the magnitudes of the terms (the docstring of the restatement).  No device
value went into either; tests/test_map_cull_cpu.py re-measures the spreads and shows planted faults 10^12 ceilings away."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import map_cull_cases as Cc
import map_cull_restatement as Q
from map_cull_dev import CullDev, remapped

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = json.load(open(os.path.join(ROOT, "profiles", "map_cull_budget.json")))["cases"]


def _live_frames(c):
    if c["n_rows"] is None:
        return c["frames"]
    return [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], c["n_rows"])]


def _compare(name, d, got):
    verdict, remap, ent, raw = got
    ref = Cc.reference(name)
    st = d.cstats(raw)
    assert st == ref["stats"], (name, st, ref["stats"])
    assert np.array_equal(verdict, ref["verdict"]), (name, verdict.tolist(), ref["verdict"].tolist())
    assert np.array_equal(remap, ref["remap"]) and np.array_equal(ent["verdict"], verdict) and not ent["reserved"].any()
    assert np.array_equal(ent["n_obs"], ref["n_obs"]) and np.array_equal(ent["n_frames"], ref["n_frames"])
    ok = (ref["n_obs"] > 0) & (ref["verdict"] != Q.NOT_FINITE)
    unseen = ref["n_obs"] == 0
    for k, want in (("mean_sq_px", 0.0), ("max_sq_px", 0.0), ("min_z", 0.0), ("cos_parallax", 1.0)):
        assert (ent[k][unseen] == want).all(), k
    worst = []
    for k, ceil in zip(("mean_sq_px", "max_sq_px", "min_z", "cos_parallax"), Cc.ceilings(name, BUDGET[name])):
        dist = np.abs(ent[k][ok] - ref[k][ok])
        ratio = np.where(dist == 0, 0.0, dist / np.maximum(ceil[ok], 1e-300))
        worst.append(float(ratio.max(initial=0.0)))
        bad = np.nonzero(ok)[0][ratio > 1.0]
        assert len(bad) == 0, (name, k, bad[:5].tolist(), ent[k][bad[:5]].tolist(), ref[k][bad[:5]].tolist(), ceil[bad[:5]].tolist())
    print(f"{name}: status {('OK', 'NOTHING_DROPPED')[st['status']]}, kept {st['n_kept']} of {st['n_before']}, by verdict {st['by_verdict']}; "
          f"mean / max / z / cos at {worst[0]:.3g}, {worst[1]:.3g}, {worst[2]:.3g}, {worst[3]:.3g} of their ceilings")


@pytest.mark.parametrize("name", list(Cc.CASES))
def test_against_float64_and_every_form(vo, ctx, name):
    c, ref = Cc.case(name), Cc.reference(name)
    d = CullDev(vo, ctx, c)
    try:
        pts0, app0, hist0 = d.map_state()
        ent0 = d.lookups()
        keep = ref["keep"]
        changes = ref["stats"]["status"] == Q.OK and not c["params"]["dry_run"]
        runs, after = [], []
        for _ in range(3):                                    # three calls from the same start: the same bytes
            d.reset(); d.clear_cull_out()
            assert d.cull() == 0, ctx.lib.vo_last_error()
            runs.append(d.cull_results())
            after.append(d.map_state())
        for r, s in zip(runs[1:], after[1:]):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0])) and all(a.tobytes() == b.tobytes() for a, b in zip(s, after[0]))
        _compare(name, d, runs[0])
        # the map afterwards: the old arrays under the keep mask, bit for bit; the history isometry as it was; no row counted as
        # dropped for lack of room (len() would fail); every lookup returns remap[the entry it returned before]
        pts1, app1, hist1 = after[0]
        if changes:
            assert pts1.tobytes() == pts0[keep].tobytes() and app1.tobytes() == app0[keep].tobytes() and len(d.m) == int(keep.sum())
            assert np.array_equal(d.lookups(), remapped(ent0, ref["remap"]))
        else:                                                 # dry_run, NOTHING_DROPPED: the map, its table (probed by every class) and its size as before
            assert pts1.tobytes() == pts0.tobytes() and app1.tobytes() == app0.tobytes() and len(d.m) == d.M
            assert np.array_equal(d.lookups(), ent0)
        assert hist1.tobytes() == hist0.tobytes()
        # a second cull of the result drops nothing and leaves every byte
        if changes:
            d.clear_cull_out()
            assert d.cull() == 0
            v2, r2, e2, raw2 = d.cull_results(int(keep.sum()))
            st2 = d.cstats(raw2)
            assert st2["status"] == Q.NOTHING_DROPPED and st2["n_before"] == st2["n_kept"] == int(keep.sum())
            assert np.array_equal(r2, np.arange(int(keep.sum()))) and np.array_equal(v2, ref["verdict"][keep])
            assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), after[0]))
            assert np.array_equal(d.lookups(), remapped(ent0, ref["remap"]))
        # without the optional outputs: the same map and statistics
        d.reset(); d.clear_cull_out()
        assert d.cull(outputs=False) == 0
        assert d.read(d.d_cstats, 48, np.uint8).tobytes() == runs[0][3].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), after[0]))
        assert (d.read(d.d_verdict, d.M, np.int32) == -7).all() and (d.read(d.d_remap, d.M, np.int32) == -7).all()
        # the host form from the same start
        d.reset()
        h = d.m.cull(d.cam, _live_frames(c), c["poses"], **c["params"])
        assert h["verdict"].tobytes() == runs[0][0].tobytes() and h["remap"].tobytes() == runs[0][1].tobytes()
        assert h["entries"].tobytes() == runs[0][2].tobytes() and h["stats"] == d.cstats(runs[0][3])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), after[0]))
    finally:
        d.close()


SIZES = (1, 255, 256, 257, 65537)                             # 65 537 entries: 257 blocks of 256


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("pattern", Cc.PATTERNS)
def test_compaction(vo, ctx, size, pattern):
    """the survivors are known by construction (the frame holds exactly their rows, the call drops the unseen)"""
    c, keep = Cc.compaction(size, pattern)
    d = CullDev(vo, ctx, c)
    probe = CullDev(vo, ctx, dict(c, frames=[(np.zeros((size, 2), np.float32), c["map_app"])]), m=d.m)      # every class of the old map
    try:
        pts0, app0, hist0 = d.map_state()
        assert np.array_equal(probe.lookups()[0], np.arange(size))
        d.clear_cull_out()
        assert d.cull() == 0, ctx.lib.vo_last_error()
        verdict, remap, ent, raw = d.cull_results()
        st = d.cstats(raw)
        n_kept = int(keep.sum())
        want = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        assert np.array_equal(remap, want) and np.array_equal(verdict, np.where(keep, Q.KEPT, Q.UNSEEN))
        assert st == dict(status=Q.NOTHING_DROPPED if keep.all() else Q.OK, n_before=size, n_kept=n_kept, n_obs=n_kept,
                          by_verdict=[n_kept, size - n_kept, 0, 0, 0, 0, 0, 0])
        assert np.array_equal(ent["n_obs"], keep.astype(np.int32)) and np.array_equal(ent["n_frames"], keep.astype(np.int32))
        assert len(d.m) == n_kept
        pts1, app1, hist1 = d.map_state()
        assert pts1.tobytes() == pts0[keep].tobytes() and app1.tobytes() == app0[keep].tobytes() and hist1.tobytes() == hist0.tobytes()
        assert np.array_equal(probe.lookups()[0], want)       # the rebuilt table finds every survivor at its new index and no dropped class
        # an update works afterwards (also on the map of size 0): a dropped class comes back at the end, a kept one is overwritten
        new_pts = np.array([[9, 9, 9], [8, 8, 8]], np.float32)
        rows = np.stack([app0[np.nonzero(~keep)[0][0]] if not keep.all() else np.full(10, 0.5, np.float32),
                         app0[np.nonzero(keep)[0][-1]] if keep.any() else np.full(10, 0.25, np.float32)])
        d.m.update(new_pts, rows)
        pts2, app2, _ = d.map_state()
        assert len(pts2) == n_kept + (2 if not keep.any() else 1)
        assert pts2[n_kept].tobytes() == new_pts[0].tobytes() and app2[n_kept].tobytes() == rows[0].tobytes()
        if keep.any():
            assert pts2[n_kept - 1].tobytes() == new_pts[1].tobytes() and pts2[: n_kept - 1].tobytes() == pts1[: n_kept - 1].tobytes()
    finally:
        probe.close()
        d.close()


@pytest.mark.parametrize("name", ["precedence", "lists", "example_pushed"])
def test_the_map_afterwards_is_the_map_an_update_builds(vo, ctx, name):
    """a second map made by clear() + update(survivors); both maps then take the same further update -- a dropped class, a kept
    class with a new point, a NaN row, a class neither has seen -- and agree in read() and in every lookup, bit for bit"""
    c, ref = Cc.case(name), Cc.reference(name)
    keep = ref["keep"]
    d = CullDev(vo, ctx, c)
    other = vo.Map(ctx)
    probe = None
    try:
        assert d.cull() == 0
        other.clear()
        other.update(c["map_pts"][keep], c["map_app"][keep])
        seen_dropped = [j for j in np.nonzero(~keep)[0] if not np.isnan(c["map_app"][j]).any()]
        rows = np.stack([c["map_app"][seen_dropped[0]], c["map_app"][np.nonzero(keep)[0][-1]], np.full(10, np.nan, np.float32),
                         np.linspace(0.1, 0.9, 10).astype(np.float32), c["map_app"][seen_dropped[0]]])
        pts = np.arange(15, dtype=np.float32).reshape(5, 3)
        for m in (d.m, other):
            m.update(pts, rows)
        a, b = d.m.read(), other.read()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[0]) == int(keep.sum()) + 3
        assert d.m.history().tobytes() == other.history().tobytes()
        mine = d.lookups()
        probe = CullDev(vo, ctx, c, m=other)
        assert np.array_equal(mine, probe.lookups())
        for q in (rows, c["map_app"]):
            assert np.array_equal(d.m.lookup(q)[1], other.lookup(q)[1])
    finally:
        if probe is not None:
            probe.close()
        other.close()
        d.close()


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c = Cc.case("lists")
    d = CullDev(vo, ctx, c)
    try:
        d.clear_cull_out()
        assert d.cull() == 0
        eager, eager_map = d.cull_results(), d.map_state()
        g = C.c_void_p()
        d.reset(); d.clear_cull_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.cull()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        for _ in range(2):                                    # replayed on a restored map
            d.reset(); d.clear_cull_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(d.cull_results(), eager))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), eager_map))
        # replayed once more on the culled map: NOTHING_DROPPED, every byte stays
        assert lib.vo_graph_launch(g) == 0
        ctx.synchronize()
        assert d.cstats(d.read(d.d_cstats, 48, np.uint8))["status"] == Q.NOTHING_DROPPED
        assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), eager_map))
        assert lib.vo_graph_destroy(g) == 0
        # frames wider than any call has sized: refused inside a capture before anything is enqueued
        big = CullDev(vo, ctx, c, n_max=4096, m=d.m)
        try:
            assert lib.vo_ctx_begin_capture(ctx.h) == 0
            assert big.cull() == -6 and b"capture" in lib.vo_last_error()
            assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
            if g.value:
                assert lib.vo_graph_destroy(g) == 0
        finally:
            big.close()
    finally:
        d.close()


def test_refusals(vo, ctx):
    d = CullDev(vo, ctx, Cc.case("precedence"))
    try:
        start = d.map_state()
        nan, inf = float("nan"), float("inf")
        for bad in (dict(min_obs=0), dict(min_frames=0), dict(max_rms_px=-1.0), dict(max_rms_px=nan), dict(max_err_px=-0.5), dict(max_err_px=inf),
                    dict(min_parallax_deg=-1.0), dict(min_parallax_deg=nan), dict(min_parallax_deg=180.0), dict(min_parallax_deg=inf),
                    dict(F=0), dict(F=65536), dict(n_max=-1), dict(uv_stride=1), dict(app_stride=1), dict(K=None), dict(prm=None), dict(d_T=None),
                    dict(d_stats=None), dict(d_stats=d.d_cstats + 4), dict(d_entry=d.d_entry + 4), dict(d_uv=None), dict(d_app=d.d_app + 4),
                    dict(K=np.zeros(9, np.float32))):
            assert d.cull(**bad) == -1, bad
            assert b"voe_map_cull_batch_dev" in ctx.lib.vo_last_error(), bad
        assert d.cull(m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), start)) and len(d.m) == d.M
        assert d.cull(min_parallax_deg=179.0) == 0            # (allowed)
    finally:
        d.close()


def test_bundle_after_the_cull_on_the_example_data(vo, ctx):
    """the 40 pushed landmarks of 'example_pushed' spoil a joint adjustment; after the cull vox_map_bundle is OK and ends at a lower
    cost per observation.  Both final costs are printed, and the pushed landmarks' share of the first."""
    c, ref = Cc.case("example_pushed"), Cc.reference("example_pushed")
    fixed = [True] + [False] * (len(c["frames"]) - 1)
    d = CullDev(vo, ctx, c)
    try:
        _, _, _, _, with_them = d.m.bundle(d.cam, c["frames"], c["poses"], fixed, n_rounds=3)
        d.reset()
        h = d.m.cull(d.cam, c["frames"], c["poses"], **c["params"])
        assert h["stats"]["status"] == Q.OK and h["stats"]["n_kept"] == 960
        _, _, _, _, without = d.m.bundle(d.cam, c["frames"], c["poses"], fixed, n_rounds=3)
        share = float((ref["mean_sq_px"] * ref["n_obs"])[~ref["keep"]].sum())
        a, b = with_them["cost_after"] / with_them["n_obs"], without["cost_after"] / without["n_obs"]
        print(f"vox_map_bundle, 3 rounds: without the cull status {with_them['status']}, cost {with_them['cost_before']:.6g} -> {with_them['cost_after']:.6g} "
              f"over {with_them['n_obs']} observations ({a:.4g} each; the pushed landmarks' share of the start {share:.6g}); after the cull status "
              f"{without['status']}, cost {without['cost_before']:.6g} -> {without['cost_after']:.6g} over {without['n_obs']} ({b:.4g} each)")
        assert without["status"] == 0 and b < a
    finally:
        d.close()


def test_cull_map_app_on_the_example_data():
    """apps/bin/cull_map checks itself: exit 0 iff exactly the pushed landmarks were dropped and every lookup afterwards returns
    remap[the entry it returned before]"""
    import subprocess
    exe = os.path.join(ROOT, "apps", "bin", "cull_map")
    assert os.path.exists(exe), "apps/bin/cull_map is missing: build() makes it"
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "example_data", "data")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "HIGH_ERROR 40" in r.stdout and "kept 960 of 1000" in r.stdout and "exactly the pushed landmarks were dropped" in r.stdout
