"""voe_map_loops* on the GPU: every case of tests/map_loops_cases.py against the restatement (tests/map_loops_restatement.py).

Reference frames, histogram, candidates, edges, the slots' pair lists, counts and gathered points and the records' integers are
compared byte for byte.  Poses, inlier sets and solver statistics are held bit for bit against the explicit public sequence
vo_estimate_pose_ransac_batch_dev -> vo_picp_solve_batch_dev that the test runs on the call's own gathered arrays.  Z is held
against rule 8 evaluated in float64 from the device's own float32 pose: both sides compute in double from the same float32
inputs, so only the final rounding can differ -- one float32 ulp at the largest term summed into the entry
(profiles/map_loops_budget.json records the largest difference seen).  Then: three calls give the same bytes, the map keeps every
byte, d_ref_frame_out is a dry-run voe_map_apply_correction's, host form = device form, capture and replay, the refusal of a
capture that would have to grow a workspace, the outputs straight into voe_pose_graph_dev, and the app."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_loops_cases as Lc
import map_loops_restatement as L
import pose_graph_restatement as PG
from map_loops_dev import LoopsDev, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _explicit(vo, ctx, d, pr):
    """the two public calls on the gathered arrays: (T_start, inlier pairs, counts, status, T_solved, stats4)"""
    L_, N, p, cam = d.L, d.n_max, d.p, d.cam
    ptr = pr["ptr"]
    out = dict(T0=ctx.alloc(64 * L_), handed=ctx.alloc(8 * L_ * N), n=ctx.alloc(4 * L_), st=ctx.alloc(4 * L_), T=ctx.alloc(64 * L_), s4=ctx.alloc(16 * L_))
    try:
        prm = vo.RansacParams(p["n_hypotheses"], p["threshold_px"], p["seed"])
        vo.estimate_pose_ransac_batch_dev(ctx, L_, cam._rows, cam._cols, cam._z_near, cam._z_far, cam._K, ptr["world"], N, N, ptr["uv"], N, N, ptr["pairs"], N,
                                          ptr["n_pairs"], prm, out["T0"], out["handed"], out["n"], None, None, out["st"])
        Kc = np.ascontiguousarray(np.asarray(cam._K, np.float32).reshape(3, 3).T)
        rc = ctx.lib.vo_picp_solve_batch_dev(ctx.h, C.c_int(L_), C.c_int(cam._rows), C.c_int(cam._cols), C.c_int(cam._z_near), C.c_int(cam._z_far),
                                             Kc.ctypes.data_as(C.c_void_p), C.c_float(p["kernel_threshold"]), C.c_int(0), C.c_void_p(ptr["world"]), C.c_size_t(N),
                                             C.c_void_p(ptr["uv"]), C.c_size_t(N), C.c_void_p(out["handed"]), C.c_size_t(N), C.c_void_p(out["n"]),
                                             C.c_void_p(out["T0"]), C.c_int(p["n_iters"]), C.c_void_p(out["T"]), C.c_void_p(out["s4"]))
        assert rc == 0, ctx.lib.vo_last_error()
        ctx.synchronize()
        return dict(handed=d.read(out["handed"], (L_, N, 2), np.int32), n=d.read(out["n"], L_, np.int32), status=d.read(out["st"], L_, np.int32),
                    T=d.read(out["T"], (L_, 16), np.float32), s4=d.read(out["s4"], (L_, 4), np.float32))
    finally:
        for q in out.values():
            ctx.free(q)


@pytest.mark.parametrize("name", list(Lc.CASES))
def test_loops_against_the_restatement(vo, ctx, name):
    c, ref = Lc.case(name), Lc.reference(name)
    d = LoopsDev(vo, ctx, c)
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
        got, rec, pr = d.got()
        log = {}
        bad = L.compare(ref, got, log)
        print(f"{name}: {got['stats']}, statuses {[L.STATUS[int(r['status'])] for r in rec]}, Z within {log['z_ulp']:.3f} ulp of its largest term")
        assert bad == [], bad
        assert log["z_ulp"] <= 1.0
        # the pixels of every filled slot are frame j's, the counts are the records'
        for l, s in enumerate(ref["slots"]):
            assert pr["n_pairs"][l] == rec[l]["n_pairs"]
            if s["j"] >= 0:
                uv = np.full((d.n_max, 2), 1e9, np.float32)
                uv[: len(c["frames"][s["j"]][0])] = c["frames"][s["j"]][0]
                assert pr["uv"][l].tobytes() == uv.tobytes()
        # poses, inlier sets and statistics: the explicit public sequence on the call's own gathered arrays, bit for bit
        ex = _explicit(vo, ctx, d, pr)
        assert ex["T"].tobytes() == pr["T16"].tobytes() and ex["s4"].tobytes() == pr["solver_stats"].tobytes()
        assert ex["n"].tobytes() == pr["n_inliers"].tobytes() and ex["status"].tolist() == [int(r["ransac_status"]) for r in rec]
        for l in range(d.L):
            assert ex["handed"][l, : ex["n"][l]].tobytes() == pr["inlier_pairs"][l, : ex["n"][l]].tobytes()
            assert int(rec[l]["ransac_inliers"]) == ex["n"][l] and int(rec[l]["num_inliers"]) == int(ex["s4"][l, 2])
            assert rec[l]["chi_inliers"].tobytes() == ex["s4"][l, 0].tobytes() and rec[l]["chi_outliers"].tobytes() == ex["s4"][l, 1].tobytes()
        assert same(d.map_state(), start)                     # the map, its table and its header keep every byte
        # without the optional outputs: the same required ones, the optional arrays untouched
        d.clear_out()
        assert d.call(optional=False) == 0
        bare = d.outputs()
        assert same(bare[:4] + bare[6:], runs[0][:4] + runs[0][6:]) and (bare[4] == -7).all() and (bare[5] == -7).all()
        # d_ref_frame_out is what a dry-run voe_map_apply_correction on the same frames writes
        d_ref2, d_st2 = d.alloc(4 * d.M), d.alloc(16)
        ctx.h2d(d_ref2, np.full(d.M + 4, -7, np.int32))
        d.m.apply_correction_batch_dev(d.F, d.d_app, d.stride, d.n_max, d.d_n, d.d_S, d.d_S, True, d_ref2, d_st2)
        ctx.synchronize()
        assert d.read(d_ref2, d.M + 4, np.int32).tobytes() == runs[0][5].tobytes()
        assert same(d.map_state(), start)
        # the host form (it reads the size first: the bound becomes the size): the same bytes
        live = [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], c["n_rows"])] if c["n_rows"] is not None else c["frames"]
        p = c["params"]
        h = d.m.loops(d.cam, live, c["S"], n_max=d.n_max, **p)
        F, Ls, M = d.F, d.L, d.M
        assert h["edges"].tobytes() == runs[0][0][: 2 * Ls].tobytes() and h["weights"].tobytes() == runs[0][2][: 3 * Ls].tobytes()
        assert np.ascontiguousarray(h["Z"].transpose(0, 2, 1)).tobytes() == runs[0][1][: 16 * Ls].tobytes()
        assert h["loops"].tobytes() == runs[0][3][: 10 * Ls].tobytes() and h["hist"].tobytes() == runs[0][4][: F * F].tobytes()
        assert h["ref_frame"].tobytes() == runs[0][5][:M].tobytes() and h["stats"] == got["stats"]
        assert same(d.map_state(), start) and len(d.m) == d.M
    finally:
        d.close()


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c = Lc.case("content64")
    d, fresh = LoopsDev(vo, ctx, c), LoopsDev(vo, ctx, c)
    try:
        g = C.c_void_p()
        start = d.map_state()
        d.clear_out()
        assert d.call() == 0
        eager = d.outputs()
        d.clear_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        # a map on which no call has sized the workspaces: refused before anything is enqueued, and the capture stays valid --
        # the call on the sized map is captured behind the refusal and replays below
        rf = fresh.call()
        err = lib.vo_last_error()
        rc = d.call()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        assert rf == -6 and b"capture" in err
        for _ in range(2):
            d.clear_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            assert same(d.outputs(), eager)
        assert lib.vo_graph_destroy(g) == 0
        assert same(d.map_state(), start)
    finally:
        fresh.close()
        d.close()


def test_the_outputs_go_straight_into_the_pose_graph(vo, ctx):
    """the odometry edges of the case's drifted chain, then the call's three arrays as they lie on the device: every slot that is
    not OK reads EDGE_SKIPPED, every OK slot is live"""
    c, ref = Lc.case("small13"), Lc.reference("small13")
    d = LoopsDev(vo, ctx, c)
    try:
        F, Ls = d.F, d.L
        S = np.asarray(c["S"], np.float64)
        odo = np.array([(k, k + 1) for k in range(F - 1)], np.int32)
        Zo = np.array([S[k + 1] @ np.linalg.inv(S[k]) for k in range(F - 1)], np.float32)
        E = len(odo) + Ls
        d_edges, d_Z, d_w = d.alloc(8 * E), d.alloc(64 * E), d.alloc(12 * E)
        ctx.h2d(d_edges, odo)
        ctx.h2d(d_Z, np.ascontiguousarray(Zo.transpose(0, 2, 1)))
        ctx.h2d(d_w, np.ones((len(odo), 3), np.float32))
        n = len(odo)
        assert d.call(d_edges=d_edges + 8 * n, d_Z=d_Z + 64 * n, d_w=d_w + 12 * n) == 0, ctx.lib.vo_last_error()
        d_S, d_es, d_st = d.dev(d.read(d.d_S, (F, 16), np.float32)), d.alloc(4 * E), d.alloc(48)
        fixed = np.zeros(F, np.uint8)
        fixed[0] = 1
        vo.pose_graph_dev(ctx, F, d_S, E, d_edges, d_Z, d_w, d.dev(fixed), vo.PoseGraphParams(4, 4, 1e-6, 1e-4, 0.0, 1, 0), d_es, None, None, d_st)
        ctx.synchronize()
        es = d.read(d_es, E, np.int32)
        st = vo.PoseGraphStats()
        C.memmove(C.byref(st), d.read(d_st, 48, np.uint8).ctypes.data, 48)
        status = [s["status"] for s in ref["slots"]]
        assert not es[:n].any() and es[n:].tolist() == [0 if s == L.OK else PG.EDGE_SKIPPED for s in status]
        assert L.OK in status and L.EMPTY in status and L.FEW_MATCHES in status and L.NO_CONSENSUS in status
        assert st.n_live_edges == n + status.count(L.OK) and vo.POSE_GRAPH_STATUS[st.status] == "OK"
    finally:
        d.close()


def test_refusals(vo, ctx):
    c = Lc.case("small13")
    d = LoopsDev(vo, ctx, c)
    try:
        start = d.map_state()
        assert d.call() == 0
        for bad in (dict(F=0), dict(F=vo.MAP_COVIS_MAX_FRAMES + 1), dict(n_max=0), dict(n_max=-1), dict(app_stride=1), dict(uv_stride=1), dict(d_app=None),
                    dict(d_uv=None), dict(d_app=d.d_app + 4), dict(d_uv=d.d_uv + 4), dict(K=None), dict(K=np.zeros((3, 3))), dict(d_S=None), dict(d_S=d.d_S + 2),
                    dict(prm=None), dict(d_edges=None), dict(d_Z=None), dict(d_w=None), dict(d_rec=None), dict(d_stats=None), dict(d_rec=d.d_rec + 4),
                    dict(d_stats=d.d_stats + 4), dict(d_hist=d.d_hist + 2)):
            assert d.call(**bad) == -1, bad
            assert b"voe_map_loops_batch_dev" in ctx.lib.vo_last_error() or b"vo_map_lookup" in ctx.lib.vo_last_error(), bad
        for field, value in (("gap", -1), ("ref_window", -1), ("min_shared", 0), ("separation", -1), ("max_loops", 0), ("max_loops", d.F + 1), ("n_iters", 0),
                             ("min_inliers", -1)):
            prm = vo.MapLoopsParams.from_buffer_copy(bytes(d.prm))
            setattr(prm, field, value)
            assert d.call(prm=prm) == -1, field
        for w in ((-1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (float("nan"), 1.0, 1.0), (float("inf"), 1.0, 1.0)):
            prm = vo.MapLoopsParams.from_buffer_copy(bytes(d.prm))
            prm.w_loop = (C.c_float * 3)(*w)
            assert d.call(prm=prm) == -1, w
        for n_hyp, thr in ((0, 2.0), (65537, 2.0), (64, 0.0)):
            prm = vo.MapLoopsParams.from_buffer_copy(bytes(d.prm))
            prm.ransac.n_hypotheses, prm.ransac.threshold_px = n_hyp, thr
            assert d.call(prm=prm) == -1, (n_hyp, thr)
        assert d.call(m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        assert same(d.map_state(), start)
    finally:
        d.close()


def test_close_loop_from_map_on_the_example_data():
    """apps/bin/close_loop --from-map: the loop edges come from ONE voe_map_loops call on the drifted map and the drifted chain --
    no world.dat localisation, no host ranking; exit 0 iff the median camera-centre error falls below a fifth"""
    exe = os.path.join(ROOT, "apps", "bin", "close_loop")
    assert os.path.exists(exe), "apps/bin/close_loop is not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "example_data", "data"), "--from-map"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "the loop is closed" in r.stdout and "status OK" in r.stdout and "voe_map_loops" in r.stdout
