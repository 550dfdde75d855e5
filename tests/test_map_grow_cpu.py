"""CPU checks behind voe_map_grow*: the ABI of the sixth extension header -- by the voe_ rule -- on a machine without a device, the
example-data claims re-measured by the float64 restatement (tests/map_grow_restatement.py), the cases of the GPU test (no marginal
decision, the budget re-measured), planted faults against the measure the GPU test uses, the map afterwards against an update,
and the host refusals under the host sanitizers."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import map_grow_cases as Gc
import map_grow_restatement as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "profiles", "map_grow_budget.json")


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---- ABI: the sixth header, by rule ----
def test_the_voe_rule_holds_with_the_sixth_header(vo):
    lib = vo.load_library()
    hip = _read("include", "vo_hip.h")
    assert hip.count('#include "vo_map_grow.h"') == 1 and hip.index('#include "vo_map_covis.h"') < hip.index('#include "vo_map_grow.h"')
    declared = {}
    for h in ["vo_hip.h"] + re.findall(r'^#include "([a-z0-9_]+\.h)"', hip, flags=re.M):
        for n in re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _read("include", h), flags=re.S)):
            declared[n] = h
    assert declared["voe_map_grow_batch_dev"] == declared["voe_map_grow"] == "vo_map_grow.h"
    for n in declared:
        assert hasattr(lib, n), f"{n} is declared in include/{declared[n]} but not exported"
    assert lib.vo_abi_version() == 1
    import shutil
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M)) == set(declared)      # unversioned, and nothing else
    assert "voe_" not in _read("visual-odometry_amd", "csrc", "vo_map_adjust.map")
    mk = _read("visual-odometry_amd", "csrc", "Makefile")
    assert "map_grow.hip" in mk and "vo_map_grow.h" in mk and "map_score.h" in mk and "vo_map_grow.h" in _read("apps", "Makefile")


def test_structs_verdicts_and_python_names(vo):
    assert C.sizeof(vo.MapGrowParams) == 40 and C.sizeof(vo.MapGrowTrack) == 80 and C.sizeof(vo.MapGrowStats) == 96
    assert vo.MapGrowTrack.xyz.offset == 32 and vo.MapGrowTrack.mean_sq_px.offset == 48 and vo.MapGrowTrack.cos_parallax.offset == 72
    assert vo.MapGrowParams.max_added.offset == 32 and vo.MapGrowParams.dry_run.offset == 36 and vo.MapGrowStats.by_verdict.offset == 36
    assert vo.MAP_GROW_TRACK_DTYPE.itemsize == 80
    assert [vo.MAP_GROW_TRACK_DTYPE.fields[k][1] for k, _ in vo.MapGrowTrack._fields_] == [getattr(vo.MapGrowTrack, k).offset for k, _ in vo.MapGrowTrack._fields_]
    assert vo.MAP_GROW_VERDICT == G.VERDICTS and vo.MAP_GROW_STATUS == G.STATUS
    hdr = _read("include", "vo_map_grow.h")
    for names in (vo.MAP_GROW_VERDICT, vo.MAP_GROW_STATUS):
        for k, name in enumerate(names):
            assert re.search(r"#define VOE_MAP_GROW_%s\s+%d\b" % (name, k), hdr), name
    src = _read("visual-odometry_amd", "csrc", "map_grow.hip")
    for k, name in enumerate(vo.MAP_GROW_VERDICT):
        assert re.search(r"GV_%s = %d\b" % (name, k), src), name
    assert "static_assert(sizeof(voe_map_grow_params) == 40 && sizeof(voe_map_grow_track) == 80 && sizeof(voe_map_grow_stats) == 96" in \
        _read("visual-odometry_amd", "csrc", "capi_map.hip")
    for n in ("grow", "grow_batch_dev"):
        assert hasattr(vo.Map, n)
    hpp = _read("include", "vo", "localise.hpp")
    assert "struct GrowOptions" in hpp and " grow(" in hpp and "grow_verdict_name" in hpp
    names = re.search(r"grow_verdict_name\(int verdict\) \{\s*static const char\* names\[\] = \{([^}]*)\}", hpp).group(1)
    assert tuple(re.findall(r'"([A-Z_]+)"', names)) == vo.MAP_GROW_VERDICT
    opt = re.search(r"struct GrowOptions \{(.*?)\};", hpp, flags=re.S).group(1)
    got = {k: v.rstrip("f") for k, v in re.findall(r"(\w+) = ([\w.]+);", opt)}
    assert {k: float(got[k]) if got[k] not in ("false", "true") else got[k] == "true" for k in G.DEFAULT} == G.DEFAULT
    import inspect
    d = {k: v.default for k, v in inspect.signature(vo.Map.grow).parameters.items() if v.default is not inspect.Parameter.empty}
    assert {k: d[k] for k in G.DEFAULT} == G.DEFAULT == dict(n_rounds=5, min_obs=3, min_frames=3, huber_px=0.0, damping=0.0, max_rms_px=2.0,
                                                              max_err_px=0.0, min_parallax_deg=2.0, max_added=0, dry_run=False)
    assert "atomicAdd(double" not in src and "atomicAdd(float" not in src and "cooperative" not in src.lower() and "unsafeAtomicAdd" not in src
    assert re.search(r"constexpr int GB = (\d+);", src).group(1) == "256" and re.search(r"constexpr int GG = (\d+);", src).group(1) == "16"
    # one device function scores a landmark for the cull and for the grow
    assert "score_list(" in src and "score_list(" in _read("visual-odometry_amd", "csrc", "map_cull.hip")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the failure path is not reachable")
def test_new_symbols_refuse_without_a_device(vo):
    lib = vo.load_library()
    z, i, s = None, C.c_int, C.c_size_t
    Kp = np.eye(3, dtype=np.float32).ctypes.data_as(C.c_void_p)
    prm, st = vo.MapGrowParams(5, 3, 3, 0.0, 0.0, 2.0, 0.0, 2.0, 0, 0), vo.MapGrowStats()
    assert lib.voe_map_grow_batch_dev(z, i(1), Kp, z, s(1), z, s(1), i(1), z, z, C.byref(prm), z, z, i(0), z) == -1
    assert b"null map" in lib.vo_last_error()
    assert lib.voe_map_grow(z, i(1), Kp, z, z, z, i(1), z, C.byref(prm), z, z, i(0), C.byref(st)) == -1
    assert b"null map" in lib.vo_last_error()


# ---- the example data: the claims, re-measured ----
def _distances(name):
    c, r = Gc.case(name), Gc.reference(name)
    key = {a.tobytes(): k for k, a in enumerate(c["truth_app"])}
    return np.array([np.linalg.norm(p.astype(np.float64) - c["truth"][key[a.tobytes()]].astype(np.float64)) for p, a in r["added_rows"]])


def test_example_data_from_an_empty_map():
    """poses and frames alone: 491 tracks of two or more frames, 462 of three or more -- the 462 well-seen landmarks -- land on
    world.dat; the recorded distances are what apps/grow_map's default bound is made of"""
    rec = json.load(open(BUDGET))["example"]
    two, three = Gc.reference("example_from_empty_two_views"), Gc.reference("example_from_empty")
    assert two["stats"]["n_added"] == 491 and three["stats"]["n_added"] == 462 and two["stats"]["n_tracks"] == 536
    assert three["stats"]["by_verdict"][G.FEW_OBS] == 536 - 462 and two["stats"]["n_open"] == two["stats"]["n_live"]
    import map_cull_cases as Cc
    import map_refine_restatement as R
    P = R.example_problem()
    seen = {P["world_app"][e].tobytes() for e in Cc.well_seen(P)}
    assert {a.tobytes() for _, a in three["added_rows"]} == seen
    for name, want in (("example_from_empty_two_views", (3.2e-5, 1.8e-3)), ("example_from_empty", (None, 5.3e-4))):
        d = _distances(name)
        rms = np.sqrt(Gc.reference(name)["mean_sq_px"][Gc.reference(name)["verdict"] == G.ADDED].max())
        print(f"{name}: {len(d)} added, distance to world.dat median {np.median(d):.3g}, largest {d.max():.3g}; largest reprojection rms {rms:.3g} px")
        # (0.006 px to the digit it was quoted with: this is the rms at the STORED float32 point, 0.00602, a hair above the double point's)
        assert abs(d.max() - want[1]) < 0.03 * want[1] and round(float(rms), 3) <= 0.006
        assert want[0] is None or abs(np.median(d) - want[0]) < 0.1 * want[0]
        assert abs(d.max() - rec[name]["largest"]) <= 1e-6 * d.max() and rec[name]["n_added"] == len(d)
    # the app's default bound: 2 x the largest recorded distance (the margin: float32 rounding of the stored point)
    app = _read("apps", "grow_map.cpp")
    bound = float(re.search(r"constexpr double DEFAULT_BOUND = ([0-9.e-]+);", app).group(1))
    assert abs(bound - 2 * rec["example_from_empty_two_views"]["largest"]) <= 0.01 * bound


@pytest.mark.parametrize("name", ["example_removed", "example_after_cull"])
def test_removed_landmarks_come_back(name):
    c, r = Gc.case(name), Gc.reference(name)
    who = c["removed"]
    assert r["stats"]["n_added"] == len(who) == r["stats"]["n_tracks"] and r["stats"]["n_before"] == 1000 - len(who)
    assert {a.tobytes() for _, a in r["added_rows"]} == {c["truth_app"][e].tobytes() for e in who}
    d = _distances(name)
    print(f"{name}: {len(who)} landmarks re-made, distance to world.dat median {np.median(d):.3g}, largest {d.max():.3g}")
    assert d.max() < 5.3e-4 * 1.03


# ---- the cases of the GPU test ----
@pytest.mark.parametrize("name", list(Gc.CASES))
def test_gpu_cases_take_no_marginal_decision_and_have_the_recorded_budget(name):
    r, rv = Gc.reference(name), Gc.reference(name, reverse=True)
    assert not r["marginal"].any() and not rv["marginal"].any()
    for k in ("verdict", "n_obs", "n_frames", "entry", "first_key", "refined", "rows", "rounding"):
        assert np.array_equal(r[k], rv[k]), k
    assert r["stats"] == rv["stats"]
    rec = json.load(open(BUDGET))["cases"][name]
    st = r["stats"]
    assert (rec["status"], rec["n_open"], rec["n_tracks"], rec["n_added"], rec["by_verdict"]) == (st["status"], st["n_open"], st["n_tracks"], st["n_added"], st["by_verdict"])
    assert rec["sum_n_obs_sq"] == r["sum_n_obs_sq"] and rec["n_rounding"] == int(r["rounding"].sum())
    got = Gc.spreads(name)
    print(name, got, "tracks at a float32 midpoint:", int(r["rounding"].sum()))
    for k, v in got.items():
        assert abs(v - rec[k]) <= 0.05 * rec[k] + 1e-18, k     # (the same numpy gives the same figure; another one may round otherwise)
    # the ceiling holds what it is derived for -- another order of summation -- with room: a quarter of it at most; it lies below
    # a sixteenth of a float32 ulp of the stored coordinate wherever the track is not flagged `rounding` and well conditioned
    sc = Gc.scored(r) & Gc.scored(rv)
    ceil = Gc.ceilings(name, rec)
    d = np.abs(r["p64"][sc] - rv["p64"][sc]).max(1)
    assert (d <= 0.25 * ceil[0][sc] + 1e-300).all()
    same = sc & (r["xyz"] == rv["xyz"]).all(1)
    assert same[sc & ~r["rounding"]].all()
    dm = np.abs(r["mean_sq_px"][same] - rv["mean_sq_px"][same])
    assert (dm <= 0.25 * ceil[1][same] + 1e-300).all()


def _track_of_landmark(name):
    """the track that carries every landmark of the scene (tracks are numbered by their smallest key, not by landmark)"""
    c, r = Gc.case(name), Gc.reference(name)
    n_max = r["rows"].shape[1]
    key = {a.tobytes(): k for k, a in enumerate(c["truth_app"])}
    lm = [key[np.asarray(c["frames"][k[0] // n_max][1], np.float32).reshape(-1, 10)[k[0] % n_max].tobytes()] for k in r["keys"]]
    return np.argsort(lm)


def test_rules_on_the_hand_made_scenes():
    v, t = Gc.reference("verdicts"), _track_of_landmark("verdicts")
    assert v["verdict"][t].tolist() == [G.BEHIND, G.HIGH_ERROR, G.LOW_PARALLAX, G.FEW_FRAMES, G.FEW_OBS, G.DEGENERATE, G.ADDED, G.ADDED, G.ADDED]
    assert v["n_obs"][t[3]] == 2 and v["n_frames"][t[3]] == 1 and v["n_obs"][t[2]] == 2 and v["min_z"][t[0]] < -1 and v["max_sq_px"][t[1]] > 100
    assert sorted(v["entry"][t[6:]].tolist()) == [0, 1, 2] and (v["entry"][t[:6]] == -1).all() and not v["xyz"][t[3:6]].any()
    assert v["refined"][t[6:]].tolist() == [1, 1, 1]
    ls = Gc.reference("lists")
    c = Gc.case("lists")
    assert sorted(ls["n_obs"].tolist()) == Gc.LISTS and set(Gc.OBS) <= set(Gc.LISTS) and ls["stats"]["n_hits"] == 21 and ls["stats"]["n_nan"] == 1
    assert ls["stats"]["by_verdict"][G.FEW_OBS] == 1 and ls["stats"]["n_added"] == len(Gc.LISTS) - 1
    assert (ls["n_frames"] <= ls["n_obs"]).all() and (ls["n_frames"] < ls["n_obs"]).any()      # two rows of one frame in a track
    assert 0 in c["n_rows"] and any(len(f[1]) > n for f, n in zip(c["frames"], c["n_rows"]))
    assert any(np.signbit(f[1][f[1] == 0]).any() for f in c["frames"])
    assert (np.diff(ls["first_key"]) > 0).all()                # tracks by ascending smallest key
    for name, n_room in (("room_equal", 0), ("room_one_below", 1), ("room_far_above", 0)):
        r = Gc.reference(name)
        assert r["stats"]["by_verdict"][G.NO_ROOM] == n_room and (r["verdict"][11 - n_room:] == G.NO_ROOM).all() and (r["verdict"][: 11 - n_room] == G.ADDED).all()
    a, d = Gc.reference("room_one_below"), Gc.reference("dry_run")
    assert d["stats"] == a["stats"] and np.array_equal(d["rows"], a["rows"]) and len(d["points"]) == 0 and len(a["points"]) == 10
    assert Gc.reference("frames_1")["stats"]["by_verdict"][G.FEW_OBS] == 6 and Gc.reference("no_open_rows")["stats"]["status"] == G.NO_OPEN_ROWS
    assert Gc.reference("grows_past_capacity")["stats"]["n_after"] == 1103 > 1024


@pytest.mark.parametrize("name", ["lists", "verdicts", "sequence_noisy", "example_after_cull", "room_one_below"])
def test_the_map_afterwards_is_the_map_an_update_builds(name):
    from oracle import vo_pipeline as vp
    c, r = Gc.case(name), Gc.reference(name)
    m = vp.Map()
    m.update(list(c["map_pts"]), list(c["map_app"]))
    m.update([p for p, _ in r["added_rows"]], [a for _, a in r["added_rows"]])
    assert np.array(m.pts, np.float32).reshape(-1, 3).tobytes() == r["points"].tobytes()
    assert np.array(m.app, np.float32).reshape(-1, 10).tobytes() == r["app"].tobytes()
    # and the numbering of the tracks is the one an update of ALL open rows, in key order, into an empty map gives its entries
    code, _, n_max = G.open_rows(c["map_app"], c["frames"], c["n_rows"])
    t = vp.Map()
    rows = [np.asarray(c["frames"][f][1], np.float32).reshape(-1, 10)[i] for f, i in zip(*np.nonzero(code == 0))]
    t.update([np.zeros(3, np.float32)] * len(rows), rows)
    first = [np.asarray(c["frames"][k[0] // n_max][1], np.float32).reshape(-1, 10)[k[0] % n_max] for k in r["keys"]]
    assert np.array(t.app, np.float32).reshape(-1, 10).tobytes() == np.array(first, np.float32).reshape(-1, 10).tobytes()


def test_planted_faults_are_seen():
    """centre_of_the_next_lane: observation k's ray meets the camera centre of observation k + 1 -- what a row rotation one lane off
    makes of the sums; tracks_by_last_key: the tracks numbered by their LAST key; rounded_before_the_rounds: p_lin stored as float32
    before the rounds start.  The first moves points by metres, the second permutes entries and rows.  The third CANNOT show after
    undamped rounds: Gauss-Newton forgets its start to second order, and five rounds from a start 3e-7 off end on the same double
    to the last bits (the figure of 'lists' is printed and not asserted).  It shows where a round keeps part of its start: the case
    'damped_round' takes ONE round under a damping of the size of H, which leaves about half of the start's rounding in the
    refined double -- thousands of ceilings -- and moves stored float32 coordinates.  That case is there for this."""
    rec = json.load(open(BUDGET))["cases"]
    for name in ("lists", "sequence_noisy"):
        ref = Gc.reference(name)
        ceil = Gc.ceilings(name, rec[name])[0]
        sc = Gc.scored(ref)
        r = Gc.run(Gc.case(name), fault="centre_of_the_next_lane")
        both = sc & Gc.scored(r)
        ratio = (np.abs(r["p64"][both] - ref["p64"][both]).max(1) / ceil[both]).max()
        flipped = int((r["verdict"] != ref["verdict"]).sum())
        print(f"{name}, centre_of_the_next_lane: {flipped} verdicts flipped, the point at {ratio:.3g} x the ceiling")
        assert ratio > 1e6 and flipped >= 1
        r = Gc.run(Gc.case(name), fault="tracks_by_last_key")
        assert not np.array_equal(r["first_key"], ref["first_key"]) and not np.array_equal(r["rows"], ref["rows"])
        assert sorted(r["first_key"].tolist()) == sorted(ref["first_key"].tolist())
    for name in ("lists", "damped_round"):
        ref, r = Gc.reference(name), Gc.run(Gc.case(name), fault="rounded_before_the_rounds")
        ok = (ref["refined"] == 1) & (r["refined"] == 1)
        ratio = (np.abs(r["p64"][ok] - ref["p64"][ok]).max(1) / Gc.ceilings(name, rec[name])[0][ok]).max()
        moved = int((r["xyz"][ok] != ref["xyz"][ok]).any(1).sum())
        print(f"{name}, rounded_before_the_rounds: the refined double point at {ratio:.3g} x the ceiling, {moved} of {int(ok.sum())} stored points differ")
        if name == "damped_round":
            assert ratio > 1e3 and moved >= 1


def test_many_tracks_case_is_what_it_says():
    c, verdict, _ = Gc.many_tracks(n=1025)
    r = Gc.run(c)
    assert np.array_equal(r["verdict"], verdict) and np.array_equal(r["first_key"], np.arange(1025)) and r["stats"]["n_added"] == 513
    assert np.abs(r["xyz"][verdict == G.ADDED].astype(np.float64) - c["truth"][verdict == G.ADDED]).max() < 4 * 3e-6 + 7 * 2.0 ** -24
    assert not r["marginal"].any()


# ---- the refusals that need no HIP, under the host sanitizers ----
def test_grow_refusals_under_the_host_sanitizers(tmp_path):
    """visual-odometry_amd/csrc/map_checks.h: map_grow_check and map_grow_room in a stand-alone program under AddressSanitizer and
    UBSan, each row against the code and the whole message"""
    exe = str(tmp_path / "map_grow_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "visual-odometry_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostcheck", "map_grow_checks_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("map_grow_checks_check: all ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("-> ok") >= 30 and "FAILED" not in r.stdout
