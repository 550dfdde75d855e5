"""vo_map_adjust[_batch_dev] on the GPU: the contract (bit for bit the explicit loop of vo_map_refine_poses_batch_dev and
vo_map_refine_batch_dev), the descent (the total cost over all hit rows, recomputed by the restatement from the bytes read
back, does not rise from sweep to sweep) and a use (the example data pushed off comes most of the way back, as far as the float64
restatement says it does: alternation is a descent, not a fast one)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_pose_refine_cases as Cs
import map_pose_refine_restatement as P
import map_refine_restatement as R
from map_pose_refine_dev import PoseDev, mats

pytestmark = pytest.mark.gpu

SMALL = dict(n_sweeps=6, pose_rounds=2, point_rounds=2, min_obs_pose=3, min_obs_point=3, huber_px=0.0, damping=0.0)
_cases, _ref = {}, {}


def _case(name):
    if name not in _cases:
        _cases[name] = Cs.example_adjust() if name == "example" else Cs.hand_adjust()
    return _cases[name]


def _reference():
    """the restatement's 6 sweeps on the example case, computed once"""
    if "example" not in _ref:
        c = _case("example")
        _ref["example"] = P.adjust(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], c["fixed"], **SMALL)
    return _ref["example"]


def _sweep_stats(vo, d, d_stats, n):
    raw = d.read(d_stats, 96 * n, np.uint8)
    st = (vo.MapAdjustStats * n)()
    C.memmove(st, raw.ctypes.data, 96 * n)
    return raw, [dict(poses=s.poses.as_dict(), points=s.points.as_dict()) for s in st]


@pytest.mark.parametrize("name,prm", [("example", dict(SMALL, n_sweeps=3)), ("hand", dict(SMALL, n_sweeps=2, huber_px=1.0, damping=1e-3))])
def test_contract_the_composed_call_is_the_explicit_loop(vo, ctx, name, prm):
    c = _case(name)
    d = PoseDev(vo, ctx, c)
    n = prm["n_sweeps"]
    d_loop, d_comp = ctx.alloc(96 * n + 16), ctx.alloc(96 * n + 16)
    try:
        # the explicit loop of the two public calls, in place, statistics sweep by sweep
        for s in range(n):
            assert d.call(in_place=True, H=False, d_stats=d_loop + 96 * s, n_rounds=prm["pose_rounds"], min_obs=prm["min_obs_pose"],
                          huber_px=prm["huber_px"], damping=prm["damping"]) == 0, ctx.lib.vo_last_error()
            assert d.refine_points(prm["point_rounds"], prm["min_obs_point"], prm["huber_px"], prm["damping"], d_stats=d_loop + 96 * s + 48) == 0
        loop = (d.read(d.d_T, (d.F, 16), np.float32), d.points(), d.read(d.d_status, d.F, np.int32), d.read(d.d_pstatus, d.M, np.int32))
        loop_raw, loop_stats = _sweep_stats(vo, d, d_loop, n)
        # the composed call from the same start
        d.reset_map(); d.reset_poses()
        ctx.h2d(d.d_status, np.full(d.F + 4, -7, np.int32)); ctx.h2d(d.d_pstatus, np.full(d.M + 4, -7, np.int32))
        assert d.adjust(d_comp, **prm) == 0, ctx.lib.vo_last_error()
        comp = (d.read(d.d_T, (d.F, 16), np.float32), d.points(), d.read(d.d_status, d.F, np.int32), d.read(d.d_pstatus, d.M, np.int32))
        comp_raw, comp_stats = _sweep_stats(vo, d, d_comp, n)
        for a, b, what in zip(comp, loop, ("poses", "map", "pose statuses", "point statuses")):
            assert a.tobytes() == b.tobytes(), what
        assert comp_raw.tobytes() == loop_raw.tobytes() and comp_stats == loop_stats
        assert (comp[0] != d.T0).any() and (comp[1] != c["map_pts"]).any()
        held = np.asarray(c["fixed"], bool)
        assert (comp[2][held] == P.FIXED).all() and comp[0][held].tobytes() == d.T0[held].tobytes()
        for s in comp_stats:
            assert s["poses"]["cost_after"] <= s["poses"]["cost_before"] and s["points"]["cost_after"] <= s["points"]["cost_before"]
        # the host form from the same start: the same bytes again
        d.reset_map()
        live = c["frames"] if c["n_rows"] is None else [(uv[:k], a[:k]) for (uv, a), k in zip(c["frames"], c["n_rows"])]
        hT, hps, hqs, hsw = d.m.adjust(d.cam, live, c["poses"], c["fixed"], **prm)
        assert np.ascontiguousarray(hT.transpose(0, 2, 1)).reshape(-1, 16).tobytes() == comp[0].tobytes() and d.points().tobytes() == comp[1].tobytes()
        assert hps.tobytes() == comp[2].tobytes() and hqs.tobytes() == comp[3].tobytes() and hsw == comp_stats
        # refusals of the composition
        for bad in (dict(n_sweeps=0), dict(n_sweeps=65537), dict(pose_rounds=65537), dict(point_rounds=65537), dict(min_obs_pose=2), dict(min_obs_point=1), dict(pose_rounds=-1), dict(huber_px=float("nan"))):
            assert d.adjust(d_comp, **dict(prm, **bad)) == -1, bad
        assert d.adjust(None, **prm) == -1
    finally:
        ctx.free(d_loop); ctx.free(d_comp)
        d.close()


def test_descent_from_the_bytes_read_back(vo, ctx):
    """the total cost over ALL hit rows (the restatement's total_cost on the poses and points the device left) after 1, 2 and 3
    sweeps from the same start does not rise, within 1e-9 relative"""
    c = _case("example")
    obs = P.frame_observations(c["map_app"], c["frames"])
    costs = [P.total_cost(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], obs=obs)]
    d = PoseDev(vo, ctx, c)
    d_st = ctx.alloc(96 * 3 + 16)
    try:
        for n in (1, 2, 3):
            d.reset_map(); d.reset_poses()
            assert d.adjust(d_st, **dict(SMALL, n_sweeps=n)) == 0, ctx.lib.vo_last_error()
            T = mats(d.read(d.d_T, (d.F, 16), np.float32))
            costs.append(P.total_cost(c["K"], d.points(), c["map_app"], c["frames"], T, obs=obs))
    finally:
        ctx.free(d_st)
        d.close()
    print("total cost at the start and after 1, 2, 3 sweeps:", costs)
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-9)
    assert costs[3] < 0.05 * costs[0]


def test_use_the_example_data_comes_back_as_far_as_float64_says(vo, ctx):
    """6 sweeps of 2 rounds from points pushed by 0.02 and poses by 0.01 / 0.005 rad, frames 0 and 120 held: the median pose
    error (largest entry of T - T_gt) and the median point error (distance to world.dat over the OK landmarks) each match the
    restatement's within 1 %"""
    c, ref = _case("example"), _reference()
    m = vo.Map(ctx)
    try:
        m.update(c["map_pts"], c["map_app"])
        T, ps, qs, sweeps = m.adjust(vo.Camera(480, 640, 0, 10, c["K"]), c["frames"], c["poses"], c["fixed"], **SMALL)
        pts = m.read()[0]
    finally:
        m.close()
    assert np.array_equal(ps, ref["pose_status"]) and np.array_equal(qs, ref["point_status"])
    assert sweeps[-1]["points"]["by_status"] == [462, 464, 74, 0, 0, 0] and sweeps[-1]["poses"]["by_status"] == [119, 2, 0, 0, 0, 0]
    ok = qs == R.OK
    perr = lambda Ts: float(np.median([np.abs(np.asarray(Ts[f], np.float64) - c["truth"][f]).max() for f in range(len(Ts))]))
    qerr = lambda p: float(np.median(np.linalg.norm(p[ok].astype(np.float64) - c["truth_pts"][ok], axis=1)))
    p0, p1, pr = perr(c["poses"]), perr(T), perr(ref["poses"])
    q0, q1, qr = qerr(c["map_pts"]), qerr(pts), qerr(ref["points"])
    print(f"median pose error {p0:.4g} -> {p1:.4g} (float64: {pr:.4g}); median point error {q0:.4g} -> {q1:.4g} (float64: {qr:.4g})")
    assert p1 < p0 and q1 < q0
    assert abs(p1 - pr) <= 0.01 * pr and abs(q1 - qr) <= 0.01 * qr
    for s, r in zip(sweeps, ref["sweeps"]):
        assert s["poses"]["by_status"] == r["poses"]["by_status"] and s["points"]["by_status"] == r["points"]["by_status"]


def test_adjust_map_app_on_the_example_data():
    """apps/bin/adjust_map checks itself: exit 0 iff the total cost (evaluated on the host after every half-sweep of the explicit
    loop) never rose, both medians fell and the composed call left the bytes of the explicit loop"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "apps", "bin", "adjust_map")
    assert os.path.exists(exe), "apps/bin/adjust_map is missing: build() makes it"
    r = subprocess.run([exe, os.path.join(root, "tests", "golden", "example_data", "data")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "never rose" in r.stdout and "equals the explicit loop bit for bit" in r.stdout
    assert "OK 119 FIXED 2" in r.stdout and "OK 462 UNSEEN 464 FEW_OBS 74" in r.stdout
    costs = [float(x) for x in r.stdout.split("total cost:")[1].split("\n")[0].split("->")]
    assert len(costs) == 13 and all(b <= a for a, b in zip(costs, costs[1:])) and costs[-1] < 0.02 * costs[0]
