"""voe_map_nearest* on the GPU: every case of tests/map_nearest_cases.py against the brute force of
tests/map_nearest_restatement.py, byte for byte and without a tolerance (entry, status, distance, canonical rows, statistics).
Then: three calls give the same bytes and the map keeps every byte; the contract of rule 6 (the exact lookup of the canonical
rows returns the call's entries), also in place; the matched pairs against the library's own matcher; batched = single, host
form = device form; capture and replay and the refusal of a capture that would have to grow the workspace; and the known answers
through the public stack on the example data with every appearance pushed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_nearest_cases as Nc
import map_nearest_restatement as N
import map_refine_restatement as R
from map_nearest_dev import GUARD, NearestDev, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(Nc.CASES))
def test_nearest_against_the_restatement(vo, ctx, name):
    c, ref = Nc.case(name), Nc.reference(name)
    d = NearestDev(vo, ctx, c)
    try:
        if c["dup_rows"]:                                     # the host's bound lies above the size the device holds
            assert d.m.size_bound() == d.M + c["dup_rows"] > d.M
        start = d.map_state()
        runs = []
        for _ in range(3):                                    # three calls: the same bytes
            d.clear_out()
            assert d.call() == 0, ctx.lib.vo_last_error()
            runs.append(d.outputs())
        assert all(same(r, runs[0]) for r in runs[1:])
        got = d.got(runs[0])
        print(f"{name}: {got['stats']}")
        bad = N.compare(ref, got)
        assert bad == [], bad
        assert same(d.map_state(), start)                     # the map, its table and its header keep every byte
        # rule 6's contract: the exact lookup of the canonical rows returns the bytes of d_entry_out
        assert d.lookup_entries(d.d_out).tobytes() == runs[0][0][: d.F * d.n_max].tobytes()
        # in place (d_app_out == d_app): the same bytes, and the same contract
        d_copy = d.alloc(d.app.nbytes)
        d.clear_out(d_out=d_copy)
        assert d.call(d_app=d_copy, d_out=d_copy) == 0, ctx.lib.vo_last_error()
        inplace = d.outputs(d_out=d_copy)
        assert same(inplace, runs[0])
        assert d.lookup_entries(d_copy).tobytes() == runs[0][0][: d.F * d.n_max].tobytes()
        # without the optional outputs: the same entries, the optional arrays untouched
        d.clear_out()
        assert d.call(d_status=None, d_dist2=None, d_out=None, d_stats=None) == 0
        bare = d.outputs()
        assert bare[0].tobytes() == runs[0][0].tobytes() and (bare[1] == GUARD).all() and (bare[2] == GUARD).all() and (bare[4] == GUARD).all()
        assert bare[3][: d.app.size].tobytes() == d.app.tobytes()
        assert same(d.map_state(), start)
    finally:
        d.close()


@pytest.mark.parametrize("name", ["frames3_plain", "zero_rows", "dyadic_unique", "special"])
def test_batched_equals_single_and_host_equals_device(vo, ctx, name):
    c = Nc.case(name)
    d = NearestDev(vo, ctx, c)
    try:
        d.clear_out()
        assert d.call() == 0, ctx.lib.vo_last_error()
        whole = d.outputs()
        N_, v = d.n_max, lambda p: C.c_void_p(p) if p else None
        for f in range(d.F):                                  # frame f alone through voe_map_nearest_dev, into fresh arrays
            e, s, q, o, st = d.alloc(4 * N_), d.alloc(4 * N_), d.alloc(4 * N_), d.dev(d.app[f]), d.alloc(32)
            rc = ctx.lib.voe_map_nearest_dev(d.m.h, v(d.d_app + 40 * f * d.stride), C.c_int(N_), v(d.d_n + 4 * f), C.byref(d.prm), v(e), v(s), v(q), v(o), v(st))
            assert rc == 0, ctx.lib.vo_last_error()
            ctx.synchronize()
            sl = slice(f * N_, (f + 1) * N_)
            assert d.read(e, N_, np.int32).tobytes() == whole[0][sl].tobytes() and d.read(s, N_, np.int32).tobytes() == whole[1][sl].tobytes()
            assert d.read(q, N_, np.int32).tobytes() == whole[2][sl].tobytes()
            assert d.read(o, d.stride * 10, np.int32).tobytes() == whole[3][f * d.stride * 10: (f + 1) * d.stride * 10].tobytes()
        # the host form
        got = d.got(whole)
        live = [a[: d.n[f]] for f, a in enumerate(c["frames"])]
        h = d.m.nearest(live, c["radius"], c["ratio"], bool(c["unique"]))
        assert h["stats"] == got["stats"]
        for f in range(d.F):
            k = len(live[f])
            assert h["entry"][f].tobytes() == got["entry"][f, :k].tobytes() and h["status"][f].tobytes() == got["status"][f, :k].tobytes()
            assert h["dist2"][f].tobytes() == got["dist2"][f, :k].tobytes() and h["app"][f].tobytes() == got["app"][f][:k].tobytes()
    finally:
        d.close()


@pytest.mark.parametrize("name", ["frames14", "frames3_plain", "bound_above_size", "one_cell", "flat_grid", "outside_bounds", "dyadic_plain"])
def test_matched_pairs_equal_the_matchers(vo, ctx, name):
    """ratio 0, unique 0, the map at least as large as every frame: the MATCHED pairs are the pairs of vo_match_appearances(map's
    appearances, frame's appearances, radius) -- the larger set is its tree, equal sizes go to the first set, ties to the lowest
    index: an independent implementation already in the library"""
    c = dict(Nc.case(name), ratio=0.0, unique=0)
    d = NearestDev(vo, ctx, c)
    try:
        d.clear_out()
        assert d.call() == 0, ctx.lib.vo_last_error()
        got = d.got()
        for f, a in enumerate(c["frames"]):
            k = int(d.n[f])
            assert d.M >= k
            pairs = vo.compute_correspondences_images(c["map_app"], a[:k], radius=c["radius"], ctx=ctx) if k else np.zeros((0, 2), np.int32)
            mine = {(int(e), i) for i, e in enumerate(got["entry"][f, :k]) if e >= 0}
            assert {(int(p), int(q)) for p, q in pairs} == mine, (name, f)
    finally:
        d.close()


def test_capture_and_replay_and_the_refusal_of_a_growing_capture(vo, ctx):
    lib = ctx.lib
    c = Nc.case("bound_above_size")
    d, fresh = NearestDev(vo, ctx, c), NearestDev(vo, ctx, c)
    try:
        g = C.c_void_p()
        d.clear_out()
        assert d.call() == 0                                  # the eager call sizes the workspace
        eager = d.outputs()
        d.clear_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        # a map on which no call has sized the workspace: refused before anything is enqueued, and the capture stays valid --
        # the call on the sized map is captured behind the refusal and replays below
        rf = fresh.call()
        err = lib.vo_last_error().decode()
        rc = d.call()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        assert rf == -6 and "would have to grow inside a graph capture" in err and "unique 1" in err, (rf, err)
        for _ in range(2):
            d.clear_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            assert same(d.outputs(), eager)
        # a replay sees the map it finds: the rows that had no entry become entries, and the same graph matches them
        ref0 = Nc.reference("bound_above_size")
        stray = np.concatenate([a[: d.n[f]][ref0["status"][f, : d.n[f]] == N.NO_ENTRY] for f, a in enumerate(c["frames"])])
        assert len(stray) > 0 and len(np.unique(stray, axis=0)) == len(stray)
        d.m.update(np.zeros((len(stray), 3), np.float32), stray)
        d.clear_out()
        assert lib.vo_graph_launch(g) == 0
        ctx.synchronize()
        after = d.got()
        assert lib.vo_graph_destroy(g) == 0
        ref2 = N.run(np.concatenate([c["map_app"], stray]), c["frames"], c["n_rows"], c["n_max"], c["radius"], c["ratio"], c["unique"])
        assert N.compare(ref2, after) == [] and after["stats"]["n_no_entry"] == 0
    finally:
        fresh.close()
        d.close()


# ---- known answers through the public stack: the example data, every appearance pushed ----
@pytest.fixture(scope="module")
def example():
    E = R.example_problem()
    rng = np.random.default_rng(1)
    pushed = [(a + rng.normal(0, 0.005, a.shape)).astype(np.float32) for _, a in E["frames"]]
    return E, pushed


def test_example_canonical_rows_localise_bit_for_bit(vo, ctx, example):
    E, pushed = example
    cam = vo.Camera(*E["cam"], E["K"], np.eye(4), ctx=ctx)
    m = vo.Map(ctx)
    try:
        m.update(E["world_pts"], E["world_app"])
        assert sum(len(m.lookup(a)[0]) for a in pushed) == 0      # bit equality finds nothing
        r = m.nearest(pushed, 0.1, 0.8)
        n_rows = sum(len(a) for a in pushed)
        assert r["stats"]["n_matched"] == n_rows == r["stats"]["n_live"]
        for f, (_, a) in enumerate(E["frames"]):
            assert r["app"][f].tobytes() == np.asarray(a, np.float32).tobytes()
            assert r["entry"][f].tolist() == E["ids"][f].astype(int).tolist()
        clean = m.localise_batch(cam, E["frames"])
        canon = m.localise_batch(cam, [(uv, r["app"][f]) for f, (uv, _) in enumerate(E["frames"])])
        assert len(clean) == len(canon) == len(pushed)
        for (Ta, sa), (Tb, sb) in zip(clean, canon):
            assert Ta.tobytes() == Tb.tobytes() and sa == sb and sa["status"] == 0
    finally:
        m.close()


def test_example_tracks_from_a_dictionary_grow_like_the_clean_frames(vo, ctx, example):
    E, pushed = example
    cam = vo.Camera(*E["cam"], E["K"], np.eye(4), ctx=ctx)
    dic, g_clean, g_canon = vo.Map(ctx, 4096), vo.Map(ctx), vo.Map(ctx)
    try:
        for a in pushed:                                      # the dictionary, frame by frame
            r = dic.nearest([a], 0.1, 0.8)
            dic.update(np.zeros((len(a), 3), np.float32), r["app"][0])
        n_ids = len(np.unique(np.concatenate([np.asarray(i) for i in E["ids"]])))
        assert len(dic) == n_ids                              # one class per landmark seen: none split, none merged
        r = dic.nearest(pushed, 0.1, 0.8)
        assert r["stats"]["n_matched"] == r["stats"]["n_live"]
        F = len(pushed)
        a_ = g_clean.grow(cam, E["frames"][:F], E["poses"][:F])["stats"]
        b_ = g_canon.grow(cam, [(uv, r["app"][f]) for f, (uv, _) in enumerate(E["frames"])], E["poses"][:F])["stats"]
        assert a_["n_added"] == b_["n_added"] > 0
        pa, pb = g_clean.read()[0], g_canon.read()[0]
        assert len(pa) > 0 and pa.tobytes() == pb.tobytes()
        print("grown:", len(pa), "landmarks from", n_ids, "classes")
    finally:
        dic.close(); g_clean.close(); g_canon.close()


@pytest.mark.parametrize("mode", [[], ["--tracks"]])
def test_the_app_exits_zero(mode):
    exe = os.path.join(ROOT, "apps", "bin", "associate_map")
    r = subprocess.run([exe, R.M.DATA] + mode, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
