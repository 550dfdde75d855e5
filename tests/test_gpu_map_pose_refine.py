"""vo_map_refine_poses[_batch_dev] on the GPU: every case of tests/map_pose_refine_cases.py against the float64 restatement
frame by frame, the optional arguments, in place against out of place, the host form, reproducibility, capture and replay,
refusals.

The measure against float64: d = the 6-vector taking T_64 (the restatement's pose before it was rounded) to T_gpu (the stored
float32 pose) -- the translation left and the small angles of R_gpu R_64^T -- in the frame's own final float64 H, sqrt(d^T H d),
in pixels.  Its ceiling is 4 x REACH32_PX[case] -- the largest value the restatement's float32 mode reaches on that case,
measured on the CPU alone (profiles/map_pose_refine_budget.json; tests/test_map_pose_refine_cpu.py re-measures it) -- plus half
an ulp of each stored pose entry carried through |H|.  No device value went into it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import map_pose_refine_cases as Cs
import map_pose_refine_restatement as P
from map_pose_refine_dev import PoseDev, colmajor16, mats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACH32_PX = {
    "example": 0.0008568, "edges": 0.0002585, "edges_no_row_counts": 0.0001379, "one_frame": 3.487e-05, "two_frames_one_held": 4.051e-05,
    "frames_257": 9.132e-05, "huber_noisy_damped": 5.898e-05, "failures": 4.147e-05, "cost_rose": 3.336e-05, "zero_rounds": 0.0,
}


def test_the_ceiling_is_the_recorded_one():
    rec = json.load(open(os.path.join(ROOT, "profiles", "map_pose_refine_budget.json")))
    assert rec["factor"] == 4 and {k: v["reach32_px"] for k, v in rec["cases"].items()} == REACH32_PX
    assert set(REACH32_PX) == set(Cs.CASES)


def _live_frames(c):
    if c["n_rows"] is None:
        return c["frames"]
    return [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], c["n_rows"])]


def _compare(name, T16, status, H, stats, start16):
    """the device's poses, statuses, information matrices and statistics of a case against the float64 restatement"""
    c, ref = Cs.case(name), Cs.reference(name)
    assert not ref["marginal"].any()
    assert np.array_equal(status, ref["status"]), (name, status.tolist(), ref["status"].tolist())
    T = mats(T16)
    worst, worst_px = 0.0, 0.0
    replaced = (status == P.OK) & (c["params"]["n_rounds"] > 0)
    for f in np.nonzero(replaced)[0]:
        ceiling = 4 * REACH32_PX[name] + P.half_ulp_px(T[f], ref["H"][f])
        d = P.h_norm(P.pose_delta(ref["T64"][f], T[f]), ref["H"][f])
        print(f"{name} frame {f}: {ref['n_obs'][f]} observations, H-norm distance to float64 {d:.3g} px, ceiling {ceiling:.3g} px")
        worst, worst_px = max(worst, d / ceiling), max(worst_px, d)
        assert d <= ceiling, (name, int(f), d, ceiling)
        assert T16[f][[3, 7, 11, 15]].tobytes() == np.array([0, 0, 0, 1], np.float32).tobytes()
    keep = ~replaced
    assert T16[keep].tobytes() == start16[keep].tobytes()       # bit for bit
    solved = np.isfinite(ref["H"]).all((1, 2))                  # the frames that solved at least once
    assert (H[~solved] == -7.0).all()                           # ... and nothing written for the others
    for f in np.nonzero(solved & (status == P.OK))[0]:
        Hd, Hr = H[f].reshape(6, 6).T, ref["H"][f]
        assert np.array_equal(Hd, Hd.T)
        assert np.abs(Hd - Hr).max() <= 1e-9 * np.abs(Hr).max(), (name, int(f), np.abs(Hd - Hr).max() / np.abs(Hr).max())
    assert stats["n_frames"] == len(status) and stats["n_obs"] == ref["stats"]["n_obs"]
    assert stats["by_status"] == ref["stats"]["by_status"]
    assert abs(stats["cost_before"] - ref["stats"]["cost_before"]) <= 1e-9 * abs(ref["stats"]["cost_before"])
    # cost_after is the cost of the STORED float32 pose.  Where the device's pose lies a float32 step d from the restatement's, a
    # frame's cost moves by at most 2 sqrt(cost) |J d| + |J d|^2 (its cost is |r|^2 and r moves by J d; the Huber cost grows no
    # faster), with |J d| <= one ulp of each entry carried through |H| = 2 x half_ulp_px.
    floor = 0.0
    for f in np.nonzero(ref["status"] == P.OK)[0]:
        if solved[f]:
            step = 2 * P.half_ulp_px(ref["poses"][f], ref["H"][f])
            floor += 2 * np.sqrt(ref["cost1"][f]) * step + step * step
    print(f"{name}: cost_before {stats['cost_before']:.9g} (float64 {ref['stats']['cost_before']:.9g}), cost_after {stats['cost_after']:.9g}, "
          f"float64 {ref['stats']['cost_after']:.9g}, allowed {1e-9 * abs(ref['stats']['cost_after']) + floor:.3g}")
    assert abs(stats["cost_after"] - ref["stats"]["cost_after"]) <= 1e-9 * abs(ref["stats"]["cost_after"]) + floor
    print(f"{name}: {int((status == P.OK).sum())} OK of {len(status)}, largest H-norm distance to float64 {worst_px:.3g} px = {worst:.3g} of the ceiling")


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_against_float64_and_every_form(vo, ctx, name):
    c = Cs.case(name)
    d = PoseDev(vo, ctx, c)
    try:
        pts0 = d.points()
        # out of place, three times: the input stays, the bytes repeat
        runs = []
        for _ in range(3):
            d.clear_out()
            assert d.call() == 0, ctx.lib.vo_last_error()
            runs.append(d.results())
            assert d.read(d.d_T, (d.F, 16), np.float32).tobytes() == d.T0.tobytes()
        for r in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0]))
        T16, status, H, raw = runs[0]
        _compare(name, T16, status, H, d.stats(raw), d.T0)
        assert d.points().tobytes() == pts0.tobytes()            # the map is read, never written
        # without the optional outputs
        d.clear_out()
        assert d.call(status=False, H=False) == 0, ctx.lib.vo_last_error()
        T2, s2, H2, raw2 = d.results()
        assert T2.tobytes() == T16.tobytes() and (s2 == -7).all() and (H2 == -7.0).all() and raw2.tobytes() == raw.tobytes()
        # in place
        d.clear_out()
        assert d.call(in_place=True) == 0, ctx.lib.vo_last_error()
        T3, s3, H3, raw3 = d.results(in_place=True)
        assert T3.tobytes() == T16.tobytes() and s3.tobytes() == status.tobytes() and H3.tobytes() == H.tobytes() and raw3.tobytes() == raw.tobytes()
        assert (d.read(d.d_Tout, (d.F, 16), np.float32) == -7.0).all()
        d.reset_poses()
        # the mask missing: a case with held frames frees them, a case without sees no difference
        if c["fixed"] is not None:
            d.clear_out()
            assert d.call(d_fixed=None) == 0
            s4 = d.results()[1]
            assert (s4 != P.FIXED).all() and np.array_equal(s4[~c["fixed"]], status[~c["fixed"]])
        # the host form (frames cut to their live rows: it pads by itself)
        hT, hs, hst, hH = d.m.refine_poses(d.cam, _live_frames(c), c["poses"], c["fixed"], want_H=True, **c["params"])
        assert colmajor16(hT).tobytes() == T16.tobytes() and hs.tobytes() == status.tobytes() and hst == d.stats(raw)
        solved = H[:, 0] != -7.0
        assert hH.reshape(-1, 36)[solved].tobytes() == H[solved].tobytes() and np.isnan(hH.reshape(-1, 36)[~solved]).all()
    finally:
        d.close()


def test_cost_rose_keeps_the_pose_and_is_counted(vo, ctx):
    """the one-round jump on the device: the decision is taken on the cost of the float32-rounded pose, the frame keeps its 64
    bytes, by_status[COST_ROSE] counts it and the sums hold the OK frame alone; with 20 rounds the same start converges (the restatement: 2.7e-7 from the truth)"""
    c, ref = Cs.case("cost_rose"), Cs.reference("cost_rose")
    assert ref["status"].tolist() == [P.COST_ROSE, P.OK] and ref["cost1"][0] > 10 * ref["cost0"][0]
    d = PoseDev(vo, ctx, c)
    try:
        d.clear_out()
        assert d.call(in_place=True) == 0, ctx.lib.vo_last_error()
        T, status, _, raw = d.results(in_place=True)
        st = d.stats(raw)
        assert status.tolist() == [P.COST_ROSE, P.OK] and st["by_status"] == [1, 0, 0, 0, 0, 1]
        assert T[0].tobytes() == d.T0[0].tobytes() and T[1].tobytes() != d.T0[1].tobytes()
        assert abs(st["cost_before"] - ref["cost0"][1]) <= 1e-9 * ref["cost0"][1]
        d.reset_poses(); d.clear_out()
        assert d.call(in_place=True, n_rounds=20) == 0
        T, status, _, _ = d.results(in_place=True)
        assert status.tolist() == [P.OK, P.OK] and np.abs(mats(T)[0].astype(np.float64) - c["truth"][0]).max() < 1e-5
    finally:
        d.close()


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c = Cs.case("huber_noisy_damped")
    d = PoseDev(vo, ctx, c)
    try:
        d.clear_out()
        assert d.call() == 0                                     # sizes the workspace
        eager = d.results()
        d.clear_out()
        g = C.c_void_p()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.call()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        for _ in range(2):
            d.clear_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            replay = d.results()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(replay, eager))
        assert lib.vo_graph_destroy(g) == 0
        # frames wider than any call has sized: refused inside a capture before anything is enqueued, the context stays usable
        big = PoseDev(vo, ctx, c, n_max=4096, m=d.m)
        try:
            assert lib.vo_ctx_begin_capture(ctx.h) == 0
            assert big.call() == -6 and b"capture" in lib.vo_last_error()
            assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
            if g.value:
                assert lib.vo_graph_destroy(g) == 0
            big.clear_out()
            assert big.call() == 0
            again = big.results()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, eager))
        finally:
            big.close()
    finally:
        d.close()


def test_refusals(vo, ctx):
    c = Cs.case("one_frame")
    d = PoseDev(vo, ctx, c)
    lib = ctx.lib
    try:
        assert d.call() == 0
        bad = lambda **kw: d.call(**kw) == -1
        assert d.call(m=None) == -1 and b"null map" in lib.vo_last_error()
        assert bad(F=0) and bad(F=65536) and bad(n_max=-1)
        assert bad(uv_stride=d.n_max - 1) and bad(app_stride=d.n_max - 1)
        assert bad(n_rounds=-1) and bad(n_rounds=65537) and d.call(n_rounds=0) == 0 and bad(min_obs=2) and b"at least 3" in lib.vo_last_error() and bad(min_obs=0)
        for x in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert bad(huber_px=x), x
            assert bad(damping=x), x
        assert bad(K=np.zeros(9, np.float32)) and b"singular" in lib.vo_last_error()
        assert bad(K=None) and bad(prm=None) and bad(d_T=None) and bad(d_Tout=None) and bad(d_stats=None) and bad(d_uv=None) and bad(d_app=None)
        assert bad(d_stats=d.d_stats + 4) and bad(d_uv=d.d_uv + 4) and bad(d_app=d.d_app + 4) and bad(d_H=d.d_H + 4)
        assert d.call() == 0 and d.call(huber_px=0.0, damping=0.0, n_rounds=0, min_obs=3) == 0
        with pytest.raises(vo.VoError):
            d.m.refine_poses(d.cam, c["frames"], c["poses"], min_obs=2)
    finally:
        d.close()
