"""voe_map_fuse* on the GPU: every case of tests/map_fuse_cases.py against the brute force of tests/map_fuse_restatement.py, byte for
byte and without a tolerance anywhere -- every output is an integer, a copied float or a once-rounded midpoint.  Per case: three calls
from a restored map give the same bytes; the map afterwards is the reference's (entries, size, header, every survivor found by the
exact lookup at its new index, no absorbed appearance found); rule 7's contract, with d_app_out separate and in place; dry_run and
NOTHING_FUSED leave every byte of map, table, header and rows; without the optional outputs.  Then: host form = device form; capture
and replay, and the refusal of a capture that would have to grow a workspace; refusals through the device; and the experiment on the
example data through the public stack, a cull dry run and a bundle evaluation on the fused map and the rewritten rows included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_fuse_cases as Fc
import map_fuse_restatement as Fr
import map_nearest_restatement as N
import map_refine_restatement as R
from map_fuse_dev import GUARD, FuseDev, remapped, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _map_as_the_reference(d, ref, state):
    pts, app, hdr, look = state
    n = ref["stats"]["n_after"] if not d.case["dry_run"] else d.M
    assert hdr[0] == n and hdr[3] == 0
    if n:
        assert pts.tobytes() == ref["map_pts"].tobytes() and app.tobytes() == ref["map_app"].tobytes()
    E = d.case["map_app"]
    q = E[~np.isnan(E).any(axis=1)]
    want = N.lookup(ref["map_app"], [q], None, len(q))[0] if len(q) else np.zeros(0, np.int32)
    assert np.array_equal(look, want)                         # the rebuilt table: every survivor at its new index, no absorbed appearance


@pytest.mark.parametrize("name", list(Fc.CASES))
def test_fuse_against_the_restatement(vo, ctx, name):
    c, ref = Fc.case(name), Fc.reference(name)
    d = FuseDev(vo, ctx, c)
    try:
        if c["dup_rows"]:                                     # the host's bound lies above the size the device holds
            assert d.m.size_bound() == d.M + c["dup_rows"] > d.M
        start = d.map_state()
        changes = ref["stats"]["status"] == Fr.OK and not c["dry_run"]
        runs, after = [], []
        for _ in range(3):                                    # three calls from a restored map: the same bytes
            d.reset(); d.clear_out()
            assert d.call() == 0, ctx.lib.vo_last_error()
            runs.append(d.outputs())
            after.append(d.map_state())
        assert all(same(r, runs[0]) for r in runs[1:]) and all(same(s, after[0]) for s in after[1:])
        got = d.got(runs[0])
        print(f"{name}: {got['stats']}")
        bad = Fr.compare(ref, got)
        assert bad == [], bad
        assert d.rows_as_expected(ref, runs[0])
        _map_as_the_reference(d, ref, after[0])
        if not changes:                                       # dry_run, NOTHING_FUSED: map, table, header keep every byte
            assert same(after[0], start)
        # rule 7's contract: the exact lookup of the rows after the call = remap[the lookup before the call]
        if d.has_frames:
            if c["dry_run"]:
                assert np.array_equal(d.lookup_entries(d.d_app), ref["ent"])
            else:
                assert np.array_equal(d.lookup_entries(d.d_out), remapped(ref["ent"], ref["remap"]))
            # in place (d_app_out == d_app): the same bytes, and the same contract
            d_copy = d.alloc(d.app.nbytes)
            d.reset(); d.clear_out(d_out=d_copy, in_place=True)
            assert d.call(d_app=d_copy, d_out=d_copy) == 0, ctx.lib.vo_last_error()
            inplace = d.outputs(d_out=d_copy)
            assert same(inplace[:5] + inplace[6:], runs[0][:5] + runs[0][6:]) and d.rows_as_expected(ref, inplace)
            assert np.array_equal(d.lookup_entries(d_copy), remapped(ref["ent"], ref["remap"]) if not c["dry_run"] else ref["ent"])
            assert same(d.map_state(), after[0])
        # without the optional outputs: the same map and statistics, the optional arrays untouched
        d.reset(); d.clear_out()
        assert d.call(d_partner=None, d_dist2=None, d_gap2=None, d_verdict=None, d_remap=None, d_out=None) == 0, ctx.lib.vo_last_error()
        bare = d.outputs()
        assert bare[6].tobytes() == runs[0][6].tobytes() and all((bare[k][: d.S] == GUARD).all() for k in range(5))
        assert same(d.map_state(), after[0])
        # a second fuse of the result finds what the restatement finds on the reference's map
        if changes and not d.has_frames:
            d.clear_out()
            assert d.call() == 0
            again = Fr.run(ref["map_pts"], ref["map_app"], None, None, 0, c["radius_xyz"], c["radius"], c["position"])
            o = d.outputs()
            k = again["stats"]["n_before"]
            assert o[3][:k].tobytes() == again["verdict"].tobytes() and o[4][:k].tobytes() == again["remap"].tobytes()
    finally:
        d.close()


@pytest.mark.parametrize("name", ["dyadic", "special", "frames", "frames_no_veto", "frames_dry_run", "together", "size_0", "zero_rows"])
def test_host_form_equals_device_form(vo, ctx, name):
    c, ref = Fc.case(name), Fc.reference(name)
    d = FuseDev(vo, ctx, c)
    try:
        d.clear_out()
        assert d.call() == 0, ctx.lib.vo_last_error()
        got, state = d.got(), d.map_state()
        d.reset()
        live = None if c["frames"] is None else [a[: Fr.live(c["frames"], c["n_rows"], c["n_max"], f)] for f, a in enumerate(c["frames"])]
        h = d.m.fuse(c["radius_xyz"], c["radius"], frames=live, position=c["position"], veto_shared_frame=bool(c["veto"]), dry_run=bool(c["dry_run"]))
        assert h["stats"] == got["stats"]
        for k in ("partner", "dist2", "gap2", "verdict", "remap"):
            assert h[k].tobytes() == got[k].tobytes(), k
        if live is not None:
            for f, a in enumerate(live):
                assert h["app"][f].tobytes() == ref["app"][f][: len(a)].tobytes(), f
        assert same(d.map_state(), state)
        assert d.m.size_bound() == ref["stats"]["n_after" if not c["dry_run"] else "n_before"]      # the host's bound follows the call
    finally:
        d.close()


def test_capture_and_replay_and_the_refusal_of_a_growing_capture(vo, ctx):
    lib = ctx.lib
    c, ref = Fc.case("frames"), Fc.reference("frames")
    d, fresh = FuseDev(vo, ctx, c), FuseDev(vo, ctx, c)
    try:
        g = C.c_void_p()
        d.clear_out()
        assert d.call() == 0                                  # the eager call sizes the workspaces
        eager, eager_map = d.outputs(), d.map_state()
        d.reset(); d.clear_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        # a map on which no call has sized the workspaces: refused before anything is enqueued, and the capture stays valid -- the
        # call on the sized map is captured behind the refusal and replays below
        rf = fresh.call()
        err = lib.vo_last_error().decode()
        rc = d.call()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        assert rf == -6 and "would have to grow inside a graph capture" in err and "voe_map_fuse_batch_dev" in err, (rf, err)
        for _ in range(2):                                    # replayed on a restored map
            d.reset(); d.clear_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            assert same(d.outputs(), eager) and same(d.map_state(), eager_map)
        # replayed once more on the fused map (launched for the capacity, the size read on the device): what the restatement finds
        # there -- the vetoed pairs are still seen together, nothing else is near --, and the map keeps every byte
        d.clear_out()
        assert lib.vo_graph_launch(g) == 0
        ctx.synchronize()
        o = d.outputs()
        again = Fr.run(ref["map_pts"], ref["map_app"], c["frames"], c["n_rows"], c["n_max"], c["radius_xyz"], c["radius"], c["position"], c["veto"])
        st = vo.MapFuseStats()
        C.memmove(C.byref(st), o[6].ctypes.data, 56)
        assert st.as_dict() == again["stats"] and again["stats"]["status"] == Fr.NOTHING_FUSED and again["stats"]["n_conflicts"] == ref["stats"]["n_conflicts"]
        assert same(d.map_state()[:3], eager_map[:3])
        assert lib.vo_graph_destroy(g) == 0
    finally:
        fresh.close()
        d.close()


def test_refusals_through_the_device_call(vo, ctx):
    """(every row of rule 11 with its message: tests/hostcheck/map_fuse_checks_check.cpp; here that the entry point asks)"""
    c = Fc.case("frames")
    d = FuseDev(vo, ctx, c)
    try:
        start = d.map_state()
        P = vo.MapFuseParams
        nan = float("nan")
        for bad in (dict(F=0), dict(F=65536), dict(n_max=-1), dict(d_app=None), dict(d_app=d.d_app + 4), dict(app_stride=1), dict(prm=None),
                    dict(d_stats=None), dict(prm=P(nan, 0.1, 1, 0, 0)), dict(prm=P(0.04, 0.0, 1, 0, 0)), dict(prm=P(0.04, 0.1, 2, 0, 0)),
                    dict(prm=P(0.04, 0.1, 1, 2, 0)), dict(prm=P(0.04, 0.1, 1, 0, -1)), dict(prm=P(0.04, 0.1, 1, 0, 0, (0, 1, 0))),
                    dict(F=0, d_app=None, d_n=None, prm=P(0.04, 0.1, 1, 1, 0), d_out=None), dict(F=0, d_app=None, d_n=None),
                    dict(d_partner=d.d_per_entry[0] + 2), dict(d_out=d.d_out + 4), dict(d_stats=d.d_stats + 4), dict(d_out=d.d_app + 40)):
            assert d.call(**bad) == -1, bad
            assert b"voe_map_fuse_batch_dev" in ctx.lib.vo_last_error(), bad
        assert d.call(m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        assert same(d.map_state(), start)
    finally:
        d.close()


# ---- the known answer through the public stack: the example world with repeated appearance and planted duplicates ----
def test_experiment_fuses_exactly_the_planted_pairs_and_the_map_calls_run_on_the_result(vo, ctx):
    E = R.example_problem()
    pts, app, ch = Fc.experiment()
    planted = {(int(a), 1000 + j) for j, a in enumerate(ch)}
    copy_of = {int(a): 1000 + j for j, a in enumerate(ch)}
    rng = np.random.default_rng(9)
    frames = []
    for (uv, _), ids in zip(E["frames"][::6], E["ids"][::6]):      # a row goes to either copy of its landmark
        e = np.array([copy_of[i] if i in copy_of and rng.random() < 0.5 else i for i in ids.astype(int)])
        frames.append((uv, app[e]))
    poses = E["poses"][::6]
    cam = vo.Camera(*E["cam"], E["K"], np.eye(4), ctx=ctx)
    m = vo.Map(ctx)
    try:
        m.update(pts, app)
        before = [m.lookup(a)[1] for _, a in frames]
        dry = m.fuse(0.04, 0.1, frames=frames, position=0, veto_shared_frame=True, dry_run=True)
        assert len(m) == 1300 and Fc.pairs_of(dry) == planted
        r = m.fuse(0.04, 0.1, frames=frames, position=0, veto_shared_frame=True)
        print("experiment:", r["stats"])
        assert Fc.pairs_of(r) == planted and r["stats"]["n_after"] == len(m) == 1000 and r["stats"]["n_conflicts"] == 0
        assert r["stats"]["n_rows_rewritten"] == sum(int((b >= 1000).sum()) for b in before) > 100
        ref = Fr.run(pts, app, [a for _, a in frames], None, max(len(a) for _, a in frames), 0.04, 0.1, 0, 1)
        assert Fr.compare(ref, {k: r[k] for k in ("partner", "dist2", "gap2", "verdict", "remap", "app", "stats")}) == []
        rewritten = [(uv, r["app"][f]) for f, (uv, _) in enumerate(frames)]
        for f, (_, a) in enumerate(rewritten):                # rule 7's contract, and every row is back at its world.dat id
            assert np.array_equal(m.lookup(a)[1], remapped(before[f], r["remap"]))
            assert np.array_equal(m.lookup(a)[1], E["ids"][::6][f].astype(int))
        # without the spatial gate appearance alone pairs wrongly (a fresh map: the fuse above changed this one)
        m.clear(); m.update(pts, app)
        loose = m.fuse(1e30, 0.1, dry_run=True)
        wrong = Fc.pairs_of(loose) - planted
        print(f"no spatial gate: {len(Fc.pairs_of(loose))} pairs, {len(wrong)} wrong")
        assert len(wrong) > 0
        m.fuse(0.04, 0.1, position=0)
        # the map calls downstream run to OK on the fused map and the rewritten rows
        cull = m.cull(cam, rewritten, poses, dry_run=True)
        assert cull["stats"]["n_before"] == 1000 and cull["stats"]["n_obs"] == sum(len(a) for _, a in rewritten)
        _, _, _, _, st = m.bundle(cam, rewritten, poses, [True] + [False] * (len(poses) - 1), n_rounds=0)
        assert st["status"] == 0 and st["n_obs"] == cull["stats"]["n_obs"], st
    finally:
        m.close()


def test_fuse_map_app_exits_zero():
    exe = os.path.join(ROOT, "apps", "bin", "fuse_map")
    assert os.path.exists(exe), "apps/bin/fuse_map is missing: build() makes it"
    r = subprocess.run([exe, R.M.DATA], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "exactly the planted pairs were fused" in r.stdout
