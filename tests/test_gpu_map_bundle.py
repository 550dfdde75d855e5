"""vox_map_bundle[_batch_dev] on the GPU: every case of tests/map_bundle_cases.py against the float64 restatement
(tests/map_bundle_restatement.py), two reductions to merged code, equal bytes (three calls, the host form, capture and replay,
what a status other than OK leaves, what held and few-observation items keep) and the descent on the example data against
vo_map_adjust_batch_dev.

The measure against float64: for a free frame the 6-vector taking T_64 (the restatement's pose before it was rounded) to the
stored float32 pose, in the frame's final float64 U_f, sqrt(d^T U d), in pixels; for a free landmark sqrt(d^T V_j d) likewise.
The ceiling per case is 4 x the distance between the restatement's forward-order and reversed-order runs, measured on the CPU
alone (profiles/map_bundle_budget.json; tests/test_map_bundle_cpu.py re-measures it), plus half an ulp of each stored float32
entry carried through |U_f| / |V_j|.  No device value went into it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import map_bundle_cases as Bc
import map_bundle_restatement as B
import map_pose_refine_cases as Cs
import map_pose_refine_restatement as P
import map_refine_cases as Rc
import map_refine_restatement as R
from map_bundle_dev import BundleDev
from map_pose_refine_dev import mats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = json.load(open(os.path.join(ROOT, "profiles", "map_bundle_budget.json")))["cases"]


def _live_frames(c):
    if c["n_rows"] is None:
        return c["frames"]
    return [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], c["n_rows"])]


def _compare(name, d, got, start16, start_pts):
    """the device's outputs of a case against the float64 restatement"""
    T16, pts, ps, qs, raw_rounds, raw_stats = got
    ref = Bc.reference(name)
    assert not ref["marginal"]
    st, rounds = d.bstats(raw_stats), d.rounds(raw_rounds)
    assert st["status"] == ref["status"], (name, vo_name(st["status"]), vo_name(ref["status"]))
    assert np.array_equal(ps, ref["pose_status"]) and np.array_equal(qs, ref["point_status"])
    for k in ("n_frames", "n_entries", "n_obs", "n_free_frames", "n_free_points", "n_accepted"):
        assert st[k] == ref["stats"][k], (name, k, st[k], ref["stats"][k])
    assert [r["accepted"] for r in rounds] == [r["accepted"] for r in ref["rounds"]], name
    assert [r["cg_iterations"] for r in rounds] == [r["cg_iterations"] for r in ref["rounds"]], name
    rel = lambda a, b: abs(a - b) <= 1e-9 * abs(b) or (a != a and b != b)
    for k, (r, q) in enumerate(zip(rounds, ref["rounds"])):
        print(f"{name} round {k}: cost {r['cost']:.12g} (float64 {q['cost']:.12g}), candidate {r['cost_candidate']:.12g} ({q['cost_candidate']:.12g}), "
              f"lambda {r['lambda_']:.3g}, {r['cg_iterations']} PCG iterations, residual {r['residual']:.3g} ({q['residual']:.3g}), accepted {r['accepted']}")
        assert rel(r["cost"], q["cost"]) and rel(r["cost_candidate"], q["cost_candidate"]) and rel(r["lambda_"], q["lambda_"]), (name, k)
    assert rel(st["cost_before"], ref["stats"]["cost_before"]), (name, st["cost_before"], ref["stats"]["cost_before"])
    T = mats(T16)
    wrote = ref["status"] == B.OK and ref["stats"]["n_accepted"] > 0
    assert wrote == (name in Bc.WRITES)
    free_f = (ref["pose_status"] == B.POSE_OK) & wrote
    free_p = (ref["point_status"] == B.POINT_OK) & wrote
    assert T16[~free_f].tobytes() == start16[~free_f].tobytes() and pts[~free_p].tobytes() == start_pts[~free_p].tobytes()      # bit for bit
    reach_f, reach_p = BUDGET[name]["reach_pose_px"], BUDGET[name]["reach_point_px"]
    worst = [0.0, 0.0, 0.0, 0.0]
    for f in np.nonzero(free_f)[0]:
        ceiling = 4 * reach_f + P.half_ulp_px(T[f], ref["U"][f])
        dist = P.h_norm(P.pose_delta(ref["T64"][f], T[f]), ref["U"][f])
        worst[0], worst[1] = max(worst[0], dist), max(worst[1], dist / ceiling)
        assert dist <= ceiling, (name, "frame", int(f), dist, ceiling)
        assert T16[f][[3, 7, 11, 15]].tobytes() == np.array([0, 0, 0, 1], np.float32).tobytes()
    for j in np.nonzero(free_p)[0]:
        ceiling = 4 * reach_p + B.half_ulp_point_px(pts[j], ref["V"][j])
        dist = B.point_norm(pts[j].astype(np.float64) - ref["P64"][j], ref["V"][j])
        worst[2], worst[3] = max(worst[2], dist), max(worst[3], dist / ceiling)
        assert dist <= ceiling, (name, "landmark", int(j), dist, ceiling)
    if wrote:
        # cost_after is the cost of the STORED float32 state: where it lies a float32 step from the restatement's, an observation's
        # residual moves by at most |J d| <= 2 x the half ulps carried through the blocks, a cost of |r|^2 by 2 sqrt(cost) s + s^2
        s2 = sum((2 * P.half_ulp_px(ref["poses"][f], ref["U"][f])) ** 2 for f in np.nonzero(free_f)[0])
        s2 += sum((2 * B.half_ulp_point_px(ref["points"][j], ref["V"][j])) ** 2 for j in np.nonzero(free_p)[0])
        floor = 2 * np.sqrt(ref["stats"]["cost_after"] * s2) + s2
        print(f"{name}: cost_after {st['cost_after']:.12g}, float64 {ref['stats']['cost_after']:.12g}, allowed {1e-9 * ref['stats']['cost_after'] + floor:.3g}")
        assert abs(st["cost_after"] - ref["stats"]["cost_after"]) <= 1e-9 * ref["stats"]["cost_after"] + floor
        assert st["cost_after"] <= st["cost_before"]
    else:
        assert rel(st["cost_after"], ref["stats"]["cost_after"])
    print(f"{name}: status {vo_name(st['status'])}, poses {worst[0]:.3g} px = {worst[1]:.3g} of the ceiling, points {worst[2]:.3g} px = {worst[3]:.3g} of the ceiling")


def vo_name(code):
    return ("OK", "NOT_FINITE", "BEHIND", "NOTHING_FREE", "NO_STEP", "COST_ROSE")[code]


@pytest.mark.parametrize("name", list(Bc.CASES))
def test_against_float64_and_every_form(vo, ctx, name):
    c = Bc.case(name)
    d = BundleDev(vo, ctx, c)
    try:
        pts0 = d.points()
        runs = []
        for _ in range(3):                                    # three calls from the same start: the same bytes
            d.reset_map(); d.reset_poses(); d.clear_bundle_out()
            assert d.bundle() == 0, ctx.lib.vo_last_error()
            runs.append(d.bundle_results())
        for r in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0]))
        _compare(name, d, runs[0], d.T0, pts0)
        if name not in Bc.WRITES:                             # compared against bytes read before the call
            assert runs[0][0].tobytes() == d.T0.tobytes() and runs[0][1].tobytes() == pts0.tobytes()
        # without the optional outputs: the same poses, map and statistics
        d.reset_map(); d.reset_poses()
        assert d.bundle(outputs=False) == 0
        again = d.bundle_results()
        assert again[0].tobytes() == runs[0][0].tobytes() and again[1].tobytes() == runs[0][1].tobytes() and again[5].tobytes() == runs[0][5].tobytes()
        # the host form from the same start
        d.reset_map()
        hT, hps, hqs, hrounds, hst = d.m.bundle(d.cam, _live_frames(c), c["poses"], c["fixed"], **c["params"])
        assert np.ascontiguousarray(hT.transpose(0, 2, 1)).reshape(-1, 16).tobytes() == runs[0][0].tobytes()
        assert d.points().tobytes() == runs[0][1].tobytes() and hps.tobytes() == runs[0][2].tobytes() and hqs.tobytes() == runs[0][3].tobytes()
        assert repr(hst) == repr(d.bstats(runs[0][5])) and repr(hrounds) == repr(d.rounds(runs[0][4]))      # (repr: a NaN cost equals itself)
    finally:
        d.close()


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c = Bc.case("huber_noisy")
    d = BundleDev(vo, ctx, c)
    try:
        d.clear_bundle_out()
        assert d.bundle() == 0
        eager = d.bundle_results()
        g = C.c_void_p()
        d.reset_map(); d.reset_poses(); d.clear_bundle_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.bundle()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        for _ in range(2):
            d.reset_map(); d.reset_poses(); d.clear_bundle_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(d.bundle_results(), eager))
        assert lib.vo_graph_destroy(g) == 0
        # frames wider than any call has sized: refused inside a capture before anything is enqueued
        big = BundleDev(vo, ctx, c, n_max=4096, m=d.m)
        try:
            assert lib.vo_ctx_begin_capture(ctx.h) == 0
            assert big.bundle() == -6 and b"capture" in lib.vo_last_error()
            assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
            if g.value:
                assert lib.vo_graph_destroy(g) == 0
        finally:
            big.close()
    finally:
        d.close()


def test_refusals(vo, ctx):
    d = BundleDev(vo, ctx, Bc.case("hand"))
    try:
        start = (d.read(d.d_T, (d.F, 16), np.float32), d.points())
        for bad in (dict(n_cg=0), dict(cg_tol=-1.0), dict(cg_tol=float("nan")), dict(lambda0=-1.0), dict(lambda0=float("inf")), dict(n_rounds=-1),
                    dict(min_obs_pose=2), dict(min_obs_point=1), dict(huber_px=float("nan")), dict(n_rounds=1025, n_cg=62), dict(n_rounds=65537, n_cg=1),
                    dict(F=0), dict(n_max=-1), dict(uv_stride=1), dict(K=None), dict(prm=None), dict(d_T=None), dict(d_stats=None),
                    dict(d_stats=d.d_bstats + 4), dict(K=np.zeros(9, np.float32))):
            assert d.bundle(**bad) == -1, bad
            assert b"vox_map_bundle_batch_dev" in ctx.lib.vo_last_error(), bad
        assert d.bundle(m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        assert d.read(d.d_T, (d.F, 16), np.float32).tobytes() == start[0].tobytes() and d.points().tobytes() == start[1].tobytes()
    finally:
        d.close()


def test_poses_alone_is_one_round_of_the_pose_half(vo, ctx):
    """poses alone free, lambda0 = 0, one round, n_cg = 8: S is block-diagonal and the preconditioner exact, so PCG takes ONE
    iteration, and every frame's pose equals vo_map_refine_poses_batch_dev(n_rounds = 1, damping = 0) under that test's own
    measure and ceiling (4 x the reach of the restatement's float32 mode + the half ulps, in the frame's H)"""
    c = dict(Bc.case("poses_alone"), params=dict(Bc.case("poses_alone")["params"], n_rounds=1, lambda0=0.0, n_cg=8))
    kw = dict(K=c["K"], map_pts=c["map_pts"], map_app=c["map_app"], frames=c["frames"], poses=c["poses"], fixed=c["fixed"], n_rounds=1, min_obs=3)
    ref, r32 = P.refine_poses(**kw), P.refine_poses(dtype=np.float32, **kw)
    free = np.nonzero(ref["status"] == P.OK)[0]
    assert len(free) == 2
    reach = max(P.h_norm(P.pose_delta(ref["T64"][f], r32["T64"][f]), ref["H"][f]) for f in free)
    d = BundleDev(vo, ctx, c)
    try:
        d.clear_bundle_out()
        assert d.bundle() == 0
        T16, _, ps, _, raw_rounds, raw_stats = d.bundle_results()
        assert d.bstats(raw_stats)["status"] == B.OK and d.rounds(raw_rounds)[0]["cg_iterations"] == 1 and d.rounds(raw_rounds)[0]["accepted"] == 1
        d.reset_poses()
        assert d.call(in_place=True, H=False, n_rounds=1, min_obs=3, huber_px=0.0, damping=0.0) == 0
        half = mats(d.read(d.d_T, (d.F, 16), np.float32))
        for f in free:
            ceiling = 4 * reach + P.half_ulp_px(mats(T16)[f], ref["H"][f])
            a = P.h_norm(P.pose_delta(ref["T64"][f], mats(T16)[f]), ref["H"][f])
            b = P.h_norm(P.pose_delta(ref["T64"][f], half[f]), ref["H"][f])
            print(f"frame {f}: the joint call {a:.3g} px, the pose half {b:.3g} px from float64; ceiling {ceiling:.3g} px")
            assert a <= ceiling and b <= ceiling
    finally:
        d.close()


def test_every_frame_held_is_one_round_of_the_point_half(vo, ctx):
    """every frame held, lambda0 = 0, one round: every point equals vo_map_refine_batch_dev(n_rounds = 1, damping = 0) under that
    test's measure and ceiling"""
    c = dict(Bc.case("every_frame_held"), params=dict(Bc.case("every_frame_held")["params"], n_rounds=1, lambda0=0.0))
    kw = dict(K=c["K"], map_pts=c["map_pts"], map_app=c["map_app"], frames=c["frames"], poses=c["poses"], n_rounds=1, min_obs=3)
    ref, r32 = R.refine(**kw), R.refine(dtype=np.float32, **kw)
    free = np.nonzero(ref["status"] == R.OK)[0]
    assert len(free) == 65
    reach = max(R.h_norm(r32["p64"][e] - ref["p64"][e], ref["H"][e]) for e in free)
    d = BundleDev(vo, ctx, c)
    try:
        d.clear_bundle_out()
        assert d.bundle() == 0
        _, pts, _, qs, raw_rounds, raw_stats = d.bundle_results()
        assert d.bstats(raw_stats)["status"] == B.OK and d.rounds(raw_rounds)[0]["cg_iterations"] == 0 and (qs == B.POINT_OK).all()
        d.reset_map()
        assert d.refine_points(1, 3, 0.0, 0.0) == 0
        half = d.points()
        for e in free:
            ceiling = 4 * reach + Rc.half_ulp_px(pts[e], ref["H"][e])
            a = R.h_norm(pts[e].astype(np.float64) - ref["p64"][e], ref["H"][e])
            b = R.h_norm(half[e].astype(np.float64) - ref["p64"][e], ref["H"][e])
            assert a <= ceiling and b <= ceiling, (int(e), a, b, ceiling)
    finally:
        d.close()


def test_example_data_two_rounds_beat_six_sweeps_of_the_alternation(vo, ctx):
    """the total cost recomputed (tests/map_pose_refine_restatement.py: total_cost) from the bytes read back: after 2 joint rounds
    it is below what vo_map_adjust_batch_dev leaves after 6 sweeps of 2 + 2 rounds from the same start; both run on the device"""
    c = Bc.case("example")
    obs = P.frame_observations(c["map_app"], c["frames"])
    d = BundleDev(vo, ctx, c)
    d_st = ctx.alloc(96 * 6 + 16)
    try:
        cost = lambda: P.total_cost(c["K"], d.points(), c["map_app"], c["frames"], mats(d.read(d.d_T, (d.F, 16), np.float32)), obs=obs)
        start = cost()
        assert d.bundle() == 0
        joint = cost()
        d.reset_map(); d.reset_poses()
        assert d.adjust(d_st, n_sweeps=6, pose_rounds=2, point_rounds=2, min_obs_pose=3, min_obs_point=3, huber_px=0.0, damping=0.0) == 0
        alternation = cost()
        print(f"total cost: start {start:.6g}, 2 joint rounds {joint:.6g}, 6 sweeps of the alternation {alternation:.6g}")
        assert joint < alternation < start
    finally:
        ctx.free(d_st)
        d.close()


def test_bundle_map_app_on_the_example_data():
    """apps/bin/bundle_map checks itself: exit 0 iff the joint call's status is OK and its final cost, evaluated on the host, is
    below the one vo_map_adjust reaches with its defaults from the same start"""
    import subprocess
    exe = os.path.join(ROOT, "apps", "bin", "bundle_map")
    assert os.path.exists(exe), "apps/bin/bundle_map is missing: build() makes it"
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "example_data", "data")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "status OK" in r.stdout and "119 free frames, 462 free landmarks" in r.stdout and "ends below the alternation" in r.stdout
    assert r.stdout.count("accepted\n") == 3
