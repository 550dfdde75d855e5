"""CPU checks behind vo_map_refine*: the float64 restatement (tests/map_refine_restatement.py) on the example data, where the
answer is known -- world.dat pushed off by up to 0.3 comes back from the ground-truth poses --, the rules on hand-made scenes
of one to three landmarks, planted faults against the measure the GPU test uses, the cases of the GPU test (no marginal
landmark, the ceiling re-measured), and the ABI of the new entry points on a machine without a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import map_refine_cases as Cs
import map_refine_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vo_map_refine_batch_dev", "vo_map_refine")
K = Cs.K_HAND


def test_known_answer_on_the_example_data():
    """10 rounds, min_obs 3, no Huber, no damping: measured 5.25e-4 at most from world.dat (bound 1e-3)"""
    c, r = Cs.case("example"), Cs.reference("example")
    n = r["n_obs"]
    assert len(c["frames"]) == 121 and len(n) == 1000
    assert int((n > 0).sum()) == 536 and int(n.sum()) == 10012 and int((n == 1).sum()) == 45 and int((n == 2).sum()) == 29
    assert np.array_equal(r["status"] == R.OK, n >= 3) and int((n >= 3).sum()) == 462
    assert np.array_equal(r["status"] == R.UNSEEN, n == 0) and int((n == 0).sum()) == 464
    assert np.array_equal(r["status"] == R.FEW_OBS, (n == 1) | (n == 2)) and int(((n == 1) | (n == 2)).sum()) == 74
    ok = r["status"] == R.OK
    d = np.linalg.norm(r["points"][ok].astype(np.float64) - c["truth"][ok], axis=1)
    print("largest distance to world.dat:", d.max(), "; at >= 4 observations:", d[n[ok] >= 4].max())
    assert d.max() < 1e-3
    assert r["points"][~ok].tobytes() == c["map_pts"][~ok].tobytes()          # every other status leaves the 12 bytes alone
    assert r["stats"]["by_status"] == [462, 464, 74, 0, 0, 0] and r["stats"]["n_obs"] == 10012
    assert r["stats"]["cost_after"] < 1e-6 * r["stats"]["cost_before"]


def test_observation_lists_are_by_key():
    c = Cs.case("edges_257_frames")
    lists, n_max, ents = R.observation_lists(c["map_app"], c["frames"], c["n_rows"])
    assert n_max == max(len(a) for _, a in c["frames"])
    for e, keys in lists.items():
        assert keys == sorted(set(keys))
        for k in keys:
            assert ents[k // n_max][k % n_max] == e and k % n_max < c["n_rows"][k // n_max]
    two = [e for e, keys in lists.items() if len({k // n_max for k in keys}) < len(keys)]
    assert two, "the case holds a frame with two rows of one landmark: two observations"
    assert sorted(len(lists.get(e, [])) for e in range(11))[:3] == [0, 1, 2]


# ---- the rules on hand-made scenes: cameras along x looking along +z, every frame sees every landmark ----
def _poses(xs):
    out = []
    for x in xs:
        T = np.eye(4); T[0, 3] = -x
        out.append(T)
    return out


def _proj(T, p):
    q = K.astype(np.float64) @ (T[:3, :3] @ np.asarray(p, np.float64) + T[:3, 3])
    return q[:2] / q[2]


def _scene(start, truth, poses, uv_edit=None, **kw):
    app = np.random.default_rng(5).uniform(-1, 1, (len(start), 10)).astype(np.float32)
    frames = []
    for f, T in enumerate(poses):
        uv = np.array([_proj(T, p) for p in truth], np.float32)
        if uv_edit:
            uv_edit(f, uv)
        frames.append((uv, app))
    return R.refine(K, np.asarray(start, np.float32), app, frames, poses, **kw)


TRUTH = [[0.3, -0.2, 5.0], [-0.5, 0.4, 6.0]]
FOUR = _poses((-1, 0, 1, 2))


def test_rule_behind():
    r = _scene([[0.3, -0.2, -5.0], [-0.5, 0.4, 6.1]], TRUTH, FOUR, n_rounds=0)          # at the start
    assert r["status"].tolist() == [R.BEHIND, R.OK]
    r = _scene([[0.3, -0.2, -5.0], [-0.5, 0.4, 6.1]], TRUTH, FOUR)
    assert r["status"][0] in (R.BEHIND, R.NOT_FINITE) and r["status"][1] == R.OK       # (NOT_FINITE takes precedence if the rounds blow up)
    assert r["points"][0].tobytes() == np.array([0.3, -0.2, -5.0], np.float32).tobytes()
    # behind only in a round: one jump from far away lands behind the cameras
    r = _scene([[0.3, -0.2, 15.0]], TRUTH[:1], FOUR, n_rounds=1)
    assert r["status"].tolist() == [R.BEHIND]


def test_rule_cost_rose_by_a_one_round_jump():
    r = _scene([[0.3, -0.2, 9.0]], TRUTH[:1], FOUR, n_rounds=1)
    assert r["status"].tolist() == [R.COST_ROSE] and r["cost1"][0] > r["cost0"][0] and not r["marginal"][0]
    assert r["points"][0].tobytes() == np.array([0.3, -0.2, 9.0], np.float32).tobytes()
    assert _scene([[0.3, -0.2, 9.0]], TRUTH[:1], FOUR, n_rounds=10)["status"].tolist() == [R.OK]


def test_rule_not_finite():
    def nan_pixel(f, uv):
        if f == 2:
            uv[0, 1] = np.nan
    r = _scene([[0.3, -0.2, 5.2], [-0.5, 0.4, 6.1]], TRUTH, FOUR, uv_edit=nan_pixel)
    assert r["status"].tolist() == [R.NOT_FINITE, R.OK]
    assert r["points"][0].tobytes() == np.array([0.3, -0.2, 5.2], np.float32).tobytes()
    # two identical observations, no damping: H has rank 2, the third pivot is exactly 0 (the point on the optical axis)
    two = _poses((0, 0))
    r = _scene([[0.0, 0.0, 2.0]], [[0.0, 0.0, 2.0]], two, min_obs=2)
    assert r["status"].tolist() == [R.NOT_FINITE]
    assert _scene([[0.0, 0.0, 2.0]], [[0.0, 0.0, 2.0]], two, min_obs=2, damping=1.0)["status"].tolist() == [R.OK]


def test_rule_zero_rounds_evaluates_and_writes_nothing():
    start = [[0.3, -0.2, 5.2], [-0.5, 0.4, 6.1]]
    r = _scene(start, TRUTH, FOUR, n_rounds=0)
    assert r["status"].tolist() == [R.OK, R.OK] and r["points"].tobytes() == np.array(start, np.float32).tobytes()
    assert np.array_equal(r["cost0"], r["cost1"]) and (r["cost0"] > 1).all()
    assert r["stats"]["cost_before"] == r["stats"]["cost_after"] == r["cost0"][0] + r["cost0"][1]


def test_rule_huber_recovers_the_inlier_fit():
    eight = _poses(np.linspace(-1.5, 2.0, 8))

    def gross(f, uv):
        if f == 3:
            uv[0] += np.float32(150.0)
    plain = _scene([[0.3, -0.2, 5.2]], TRUTH[:1], eight, uv_edit=gross)
    huber = _scene([[0.3, -0.2, 5.2]], TRUTH[:1], eight, uv_edit=gross, huber_px=1.0, n_rounds=30)
    e_plain = np.linalg.norm(plain["points"][0] - np.array(TRUTH[0]))
    e_huber = np.linalg.norm(huber["points"][0] - np.array(TRUTH[0]))
    print("distance to the inlier fit: squared error", e_plain, ", Huber 1 px", e_huber)
    assert huber["status"].tolist() == [R.OK] and e_huber < 0.02 and e_huber < 0.1 * e_plain
    # the Huber cost is |e|^2 inside and huber (2 |e| - huber) outside
    H, b, cost, z = R.evaluate(K, np.eye(3)[None], np.zeros((1, 3)), np.array([_proj(np.eye(4), TRUTH[0]) + [3.0, 4.0]]), TRUTH[0], 2.0)
    assert abs(cost - 2.0 * (2 * 5.0 - 2.0)) < 1e-9


def test_rule_damping():
    start = np.array([[0.3, -0.2, 5.2]], np.float32)
    app = np.random.default_rng(5).uniform(-1, 1, (1, 10)).astype(np.float32)
    uv = np.array([_proj(T, TRUTH[0]) for T in FOUR], np.float32)
    Rm, t = np.stack([T[:3, :3] for T in FOUR]), np.stack([T[:3, 3] for T in FOUR])
    H, b, _, _ = R.evaluate(K, Rm, t, uv, start[0], 0.0)
    for lam in (0.0, 50.0):
        r = _scene(start, TRUTH[:1], FOUR, n_rounds=1, damping=lam)
        want = start[0].astype(np.float64) - np.linalg.solve(H + lam * np.eye(3), b)
        assert np.abs(r["p64"][0] - want).max() < 1e-9, lam
    assert np.abs(np.linalg.solve(H + 50.0 * np.eye(3), b) - np.linalg.solve(H, b)).max() > 1e-3


# ---- planted faults: the measure of the GPU test (H-norm distance to the float64 point against the ceiling) sees each ----
def test_planted_faults_are_seen():
    c, ref = Cs.case("example"), Cs.reference("example")
    budget = json.load(open(os.path.join(ROOT, "profiles", "map_refine_budget.json")))
    sub = np.nonzero(ref["status"] == R.OK)[0][:60]

    def worst(r):
        """(excess over the ceiling of the worst landmark, statuses that changed)"""
        over = 0.0
        for e in sub:
            if r["status"][e] == R.OK:
                ceil = 4 * budget["cases"]["example"]["reach32_px"] + Cs.half_ulp_px(r["points"][e], ref["H"][e])
                over = max(over, R.h_norm(r["points"][e].astype(np.float64) - ref["p64"][e], ref["H"][e]) / ceil)
        return over, int((r["status"][sub] != ref["status"][sub]).sum())

    kw = dict(only=sub)
    clean = R.refine(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], **kw)
    assert worst(clean)[0] <= 1.0 and worst(clean)[1] == 0
    for fault in R.FAULTS:
        over, changed = worst(R.refine(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], fault=fault, **kw))
        print(f"{fault}: {over:.3g} x the ceiling, {changed} statuses changed")
        assert over > 1.0 or changed > 0, fault


@pytest.mark.parametrize("name", list(Cs.CASES))
def test_gpu_cases_have_no_marginal_landmark_and_the_recorded_ceiling(name):
    r = Cs.reference(name)
    assert not r["marginal"].any()
    assert np.array_equal(Cs.reference(name, np.float32)["status"], r["status"])
    rec = json.load(open(os.path.join(ROOT, "profiles", "map_refine_budget.json")))["cases"][name]
    reach = Cs.float32_reach(name)
    print(name, "float32 mode reaches", reach, "px; recorded", rec["reach32_px"])
    assert rec["by_status"] == r["stats"]["by_status"] and rec["n_obs"] == r["stats"]["n_obs"]
    assert abs(reach - rec["reach32_px"]) <= 0.05 * rec["reach32_px"]         # (summation order of the numpy at hand)


def test_gpu_cases_cover_the_edges():
    n = Cs.reference("edges_257_frames")["n_obs"].tolist()
    assert sorted(n) == [0, 1, 2, 3, Cs.G - 1, Cs.G, Cs.G + 1, 63, 64, 65, 257] and len(Cs.case("edges_257_frames")["frames"]) == 257
    assert [len(Cs.case(k)["map_pts"]) for k in ("map_of_1", "map_of_255", "map_of_256", "map_of_257")] == [1, 255, 256, 257]
    assert len(Cs.case("frames_beyond_lds")["frames"]) == Cs.LDS_FRAMES + 1
    assert set(Cs.reference("one_frame")["status"].tolist()) <= {R.FEW_OBS, R.UNSEEN}
    assert sorted(set(Cs.reference("failures")["status"].tolist())) == [R.OK, R.UNSEEN, R.FEW_OBS, R.BEHIND, R.NOT_FINITE]
    assert Cs.reference("cost_rose")["status"].tolist() == [R.COST_ROSE, R.OK]
    src = open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "map_refine.hip")).read()
    assert re.search(r"constexpr int RG = (\d+);", src).group(1) == str(Cs.G)
    assert re.search(r"constexpr int REFINE_LDS_FRAMES = (\d+);", src).group(1) == str(Cs.LDS_FRAMES)


# ---- ABI ----
def _declared():
    txt = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", txt))


def test_new_symbols_are_declared_and_exported(vo):
    lib = vo.load_library()
    for n in NEW:
        assert n in _declared(), n
        assert hasattr(lib, n), n
    assert len(_declared()) == 100
    for n in ("MapRefineParams", "MapRefineStats", "MAP_REFINE_STATUS"):
        assert hasattr(vo, n)
    for n in ("refine", "refine_batch_dev"):
        assert hasattr(vo.Map, n)
    assert C.sizeof(vo.MapRefineParams) == 16 and C.sizeof(vo.MapRefineStats) == 48
    assert vo.MapRefineStats.cost_before.offset == 32 and vo.MapRefineStats.by_status.offset == 8
    assert vo.MAP_REFINE_STATUS == ("OK", "UNSEEN", "FEW_OBS", "BEHIND", "NOT_FINITE", "COST_ROSE")
    hdr = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    for k, name in enumerate(vo.MAP_REFINE_STATUS):
        assert re.search(r"#define VO_MAP_REFINE_%s\s+%d\b" % (name, k), hdr), name
    hpp = open(os.path.join(ROOT, "include", "vo", "localise.hpp")).read()
    assert "struct RefineOptions" in hpp and "void refine(" in hpp


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the failure path is not reachable")
def test_new_symbols_refuse_without_a_device(vo):
    """no context can exist here, hence no map: both entry points refuse the null handle"""
    lib = vo.load_library()
    z, i = None, C.c_int
    Kp = np.eye(3, dtype=np.float32).ctypes.data_as(C.c_void_p)
    prm, st = vo.MapRefineParams(10, 3, 0.0, 0.0), vo.MapRefineStats()
    assert lib.vo_map_refine_batch_dev(z, i(1), Kp, z, C.c_size_t(1), z, C.c_size_t(1), i(1), z, z, C.byref(prm), z, z, z) == -1
    assert b"null map" in lib.vo_last_error()
    assert lib.vo_map_refine(z, i(1), Kp, z, z, z, i(1), z, C.byref(prm), z, C.byref(st)) == -1
    assert b"null map" in lib.vo_last_error()
