"""voe_map_guided* on the GPU: every case of tests/map_guided_cases.py against the brute force of tests/map_guided_restatement.py,
byte for byte and without a tolerance (entry, status, both distances, canonical rows, statistics).  Then: three calls give the same
bytes and the map keeps every byte; the contract of rule 6 (the exact lookup of the canonical rows returns the call's entries),
also in place; batched = single, host form = device form; capture and replay and the refusal of a capture that would have to grow
the workspace; voe_map_nearest as the limit of a window that gates everything in view; and the known answers through the public
stack on the example data with every appearance and every pose pushed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_guided_cases as Gc
import map_guided_restatement as G
import map_refine_restatement as R
from map_guided_dev import GUARD, GuidedDev, same
from map_nearest_dev import NearestDev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(Gc.CASES))
def test_guided_against_the_restatement(vo, ctx, name):
    c, ref = Gc.case(name), Gc.reference(name)
    d = GuidedDev(vo, ctx, c)
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
        bad = G.compare(ref, got)
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
        assert d.call(d_status=None, d_dist2=None, d_pix2=None, d_out=None, d_stats=None) == 0
        bare = d.outputs()
        assert bare[0].tobytes() == runs[0][0].tobytes() and all((bare[k] == GUARD).all() for k in (1, 2, 3, 5))
        assert bare[4][: d.app.size].tobytes() == d.app.tobytes()
        assert same(d.map_state(), start)
    finally:
        d.close()


@pytest.mark.parametrize("name", ["frames3_plain", "zero_rows", "dyadic_unique", "special", "nan_pose"])
def test_batched_equals_single_and_host_equals_device(vo, ctx, name):
    c = Gc.case(name)
    d = GuidedDev(vo, ctx, c)
    try:
        d.clear_out()
        assert d.call() == 0, ctx.lib.vo_last_error()
        whole = d.outputs()
        N_, v = d.n_max, lambda p: C.c_void_p(p) if p else None
        for f in range(d.F):                                  # frame f alone through voe_map_guided_dev, into fresh arrays
            e, s, q, g, st = d.alloc(4 * N_), d.alloc(4 * N_), d.alloc(4 * N_), d.alloc(4 * N_), d.alloc(48)
            o = d.dev(d.app[f])
            rc = ctx.lib.voe_map_guided_dev(d.m.h, d.K.ctypes.data_as(C.c_void_p), v(d.d_uv + 8 * f * d.stride), v(d.d_app + 40 * f * d.stride),
                                            C.c_int(N_), v(d.d_n + 4 * f), v(d.d_T + 64 * f), C.byref(d.prm), v(e), v(s), v(q), v(g), v(o), v(st))
            assert rc == 0, ctx.lib.vo_last_error()
            ctx.synchronize()
            sl = slice(f * N_, (f + 1) * N_)
            for k, p in enumerate((e, s, q, g)):
                assert d.read(p, N_, np.int32).tobytes() == whole[k][sl].tobytes(), (f, k)
            assert d.read(o, d.stride * 10, np.int32).tobytes() == whole[4][f * d.stride * 10: (f + 1) * d.stride * 10].tobytes()
        # the host form
        got = d.got(whole)
        live = [(p[: d.n[f]], a[: d.n[f]]) for f, (p, a) in enumerate(c["frames"])]
        cam = vo.Camera(480, 640, c["z_near"], c["z_far"], c["K"], np.eye(4), ctx=ctx)
        h = d.m.guided(cam, live, c["poses"], c["radius_px"], c["radius"], c["ratio"], bool(c["unique"]))
        assert h["stats"] == got["stats"]
        for f in range(d.F):
            k = len(live[f][1])
            for key in ("entry", "status", "dist2", "pix2"):
                assert h[key][f].tobytes() == got[key][f, :k].tobytes(), (f, key)
            assert h["app"][f].tobytes() == got["app"][f][:k].tobytes()
    finally:
        d.close()


def test_capture_and_replay_and_the_refusal_of_a_growing_capture(vo, ctx):
    lib = ctx.lib
    c = Gc.case("bound_above_size")
    d, fresh = GuidedDev(vo, ctx, c), GuidedDev(vo, ctx, c)
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
        # a replay sees the map it finds: the rows that had no entry become entries -- their points 5 in front of the prior's
        # camera on the ray of their pixel --, and the same graph (sized by the capacity) matches them
        ref0 = Gc.reference("bound_above_size")
        pts, apps = [], []
        for f, (uv, a) in enumerate(c["frames"]):
            for i in np.nonzero(ref0["status"][f, : d.n[f]] == G.NO_ENTRY)[0]:
                ray = np.linalg.inv(c["K"].astype(np.float64)) @ np.array([uv[i, 0], uv[i, 1], 1.0]) * 5.0
                pts.append((np.linalg.inv(c["poses"][f].astype(np.float64)) @ np.append(ray, 1.0))[:3])
                apps.append(a[i])
        pts, apps = np.array(pts, np.float32), np.array(apps, np.float32)
        assert len(apps) > 0 and len(np.unique(apps, axis=0)) == len(apps)
        d.m.update(pts, apps)
        d.clear_out()
        assert lib.vo_graph_launch(g) == 0
        ctx.synchronize()
        after = d.got()
        assert lib.vo_graph_destroy(g) == 0
        ref2 = Gc.run(c, map_pts=np.concatenate([c["map_pts"], pts]), map_app=np.concatenate([c["map_app"], apps]))
        assert G.compare(ref2, after) == [] and after["stats"]["n_no_entry"] == 0 and after["stats"]["n_entries"] == d.M + len(apps)
    finally:
        fresh.close()
        d.close()


def test_the_corner_the_window_adds_to_the_lookup_contract(vo, ctx):
    """rule 6 states it: a row that compares equal to an entry outside its window is NO_ENTRY, keeps its bytes, and is a hit of the
    exact lookup (one_entry with row 2 a copy of the entry, 20 px from its projection)"""
    c = Gc.case("one_entry")
    uv, app = c["frames"][0]
    app = app.copy()
    app[2] = c["map_app"][0]
    c = dict(c, frames=[(uv, app)])
    d = GuidedDev(vo, ctx, c)
    try:
        d.clear_out()
        assert d.call() == 0, ctx.lib.vo_last_error()
        got = d.got()
        assert G.compare(Gc.run(c), got) == [] and got["status"][0, 2] == G.NO_ENTRY and got["entry"][0, 2] == -1
        look = d.lookup_entries(d.d_out)
        assert look[0, 2] == 0 and (np.delete(look[0], 2) == np.delete(got["entry"][0], 2)).all()
    finally:
        d.close()


@pytest.mark.parametrize("ratio,unique", [(0.0, 0), (0.8, 1)])
def test_nearest_is_the_limit_of_a_window_that_gates_everything(vo, ctx, ratio, unique):
    """every entry of the case is in view of every frame and radius_px is so large that every one of them is gated: the candidates
    are NEAREST's, and entry, status, distance and canonical rows equal voe_map_nearest's on the same rows -- an independent
    implementation already in the library"""
    c = dict(Gc.case("all_in_view"), radius_px=1e7, ratio=ratio, unique=unique)
    rows = sum(len(a) for _, a in c["frames"])
    d = GuidedDev(vo, ctx, c)
    n = NearestDev(vo, ctx, dict(map_app=c["map_app"], frames=[a for _, a in c["frames"]], n_rows=None, n_max=c["n_max"], radius=c["radius"],
                                 ratio=ratio, unique=unique, dup_rows=0))
    try:
        d.clear_out(); n.clear_out()
        assert d.call() == 0 and n.call() == 0, ctx.lib.vo_last_error()
        a, b = d.got(), n.got()
        assert a["stats"]["n_in_view"] == d.F * d.M and a["stats"]["n_gated"] == rows * d.M
        assert a["stats"]["n_matched"] > rows // 2
        for k in ("entry", "status", "dist2"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a["app"], b["app"]))
        assert {k: a["stats"][k] for k in b["stats"]} == b["stats"]
    finally:
        d.close(); n.close()


# ---- known answers through the public stack: the example data, every appearance and every pose pushed ----
def test_example_canonical_rows_localise_from_the_prior_bit_for_bit(vo, ctx):
    E = R.example_problem()
    rng = np.random.default_rng(1)
    pushed = [(a + rng.normal(0, 0.005, a.shape)).astype(np.float32) for _, a in E["frames"]]
    priors = [(Gc._pose(rng, 0.005, 0.01) @ T).astype(np.float32) for T in E["poses"]]
    cam = vo.Camera(*E["cam"], E["K"], np.eye(4), ctx=ctx)
    m = vo.Map(ctx)
    try:
        m.update(E["world_pts"], E["world_app"])
        r = m.guided(cam, [(uv, pushed[f]) for f, (uv, _) in enumerate(E["frames"])], priors, 16.0, 0.1, 0.8)
        n_rows = sum(len(a) for a in pushed)
        print("example, 16 px:", r["stats"])
        assert r["stats"]["n_live"] == n_rows and r["stats"]["n_matched"] > 0.99 * n_rows
        mixed = []                                            # the clean frames, every row that is not MATCHED replaced by its pushed bytes
        for f, (uv, a) in enumerate(E["frames"]):
            ok = r["status"][f] == G.MATCHED
            assert r["entry"][f][ok].tolist() == E["ids"][f].astype(int)[ok].tolist()
            mixed.append((uv, np.where(ok[:, None], np.asarray(a, np.float32), pushed[f])))
        kw = dict(n_hypotheses=0, T0=priors)
        canon = m.localise_batch(cam, [(uv, r["app"][f]) for f, (uv, _) in enumerate(E["frames"])], **kw)
        clean = m.localise_batch(cam, mixed, **kw)
        assert len(clean) == len(canon) == len(pushed)
        for (Ta, sa), (Tb, sb) in zip(clean, canon):
            assert Ta.tobytes() == Tb.tobytes() and sa == sb and sa["status"] == 0
    finally:
        m.close()


def test_the_tracker_exits_zero():
    exe = os.path.join(ROOT, "apps", "bin", "track_map")
    r = subprocess.run([exe, R.M.DATA], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "took the fallback" in r.stdout
