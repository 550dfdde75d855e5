"""CPU checks behind voe_map_cull*: the ABI of the third namespace -- pinned by RULE, not by list -- on a machine without a
device, the float64 restatement (tests/map_cull_restatement.py) on the example data and on the hand-made scenes, its planted
faults against the measure the GPU test uses, and the cases of the GPU test (no marginal decision, the budget re-measured)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import map_cull_cases as Cc
import map_cull_restatement as Q
import map_refine_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "profiles", "map_cull_budget.json")


# ---- ABI: the third namespace, by rule ----
def _included_headers():
    """the headers under include/ that vo_hip.h includes, itself first (one level: extension headers include vo_hip.h alone)"""
    txt = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    return ["vo_hip.h"] + re.findall(r'^#include "([a-z0-9_]+\.h)"', txt, flags=re.M)


def _declared_voe():
    out = {}
    for h in _included_headers():
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        for n in re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", txt):
            out[n] = h
    return out


def test_every_voe_symbol_exported_is_declared_and_every_declared_one_exported(vo):
    import shutil
    import subprocess
    lib = vo.load_library()
    declared = _declared_voe()
    assert {"voe_map_cull_batch_dev", "voe_map_cull"} <= set(declared) and declared["voe_map_cull"] == "vo_map_cull.h"
    for n in declared:
        assert hasattr(lib, n), f"{n} is declared in include/{declared[n]} but not exported"
    hip = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    assert hip.count('#include "vo_map_cull.h"') == 1 and hip.index('#include "vo_map_bundle.h"') < hip.index('#include "vo_map_cull.h"')
    assert lib.vo_abi_version() == 1
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M)) == set(declared)      # unversioned, and nothing else
        assert not re.findall(r" [A-Za-z] (voe_[a-z0-9_]+)@", out, flags=re.M)
    assert "voe_" not in open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "vo_map_adjust.map")).read()
    header = open(os.path.join(ROOT, "include", "vo_map_cull.h")).read()
    assert "OPENED BY RULE" in header and "every exported voe_ function is declared" in header


def test_structs_verdicts_and_python_names(vo):
    assert C.sizeof(vo.MapCullParams) == 28 and C.sizeof(vo.MapCullEntry) == 48 and C.sizeof(vo.MapCullStats) == 48
    assert vo.MapCullEntry.mean_sq_px.offset == 16 and vo.MapCullEntry.cos_parallax.offset == 40 and vo.MapCullParams.dry_run.offset == 24
    assert vo.MapCullStats.by_verdict.offset == 16 and vo.MAP_CULL_ENTRY_DTYPE.itemsize == 48
    assert [vo.MAP_CULL_ENTRY_DTYPE.fields[k][1] for k, _ in vo.MapCullEntry._fields_] == [getattr(vo.MapCullEntry, k).offset for k, _ in vo.MapCullEntry._fields_]
    assert vo.MAP_CULL_VERDICT == Q.VERDICTS and vo.MAP_CULL_STATUS == ("OK", "NOTHING_DROPPED")
    hdr = open(os.path.join(ROOT, "include", "vo_map_cull.h")).read()
    for k, name in enumerate(vo.MAP_CULL_VERDICT):
        assert re.search(r"#define VOE_MAP_CULL_%s\s+%d\b" % (name, k), hdr), name
    for k, name in enumerate(vo.MAP_CULL_STATUS):
        assert re.search(r"#define VOE_MAP_CULL_%s\s+%d\b" % (name, k), hdr), name
    assert (Q.KEPT, Q.UNSEEN, Q.FEW_OBS, Q.FEW_FRAMES, Q.NOT_FINITE, Q.BEHIND, Q.HIGH_ERROR, Q.LOW_PARALLAX) == tuple(range(8))
    for n in ("cull", "cull_batch_dev"):
        assert hasattr(vo.Map, n)
    hpp = open(os.path.join(ROOT, "include", "vo", "localise.hpp")).read()
    assert "struct CullOptions" in hpp and " cull(" in hpp
    src = open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "map_cull.hip")).read()
    assert "atomicAdd(double" not in src and "atomicAdd(float" not in src and "cooperative" not in src.lower() and "unsafeAtomicAdd" not in src
    assert re.search(r"constexpr int CB = (\d+);", src).group(1) == "256" and re.search(r"constexpr int CG = (\d+);", src).group(1) == "16"
    mk = open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "Makefile")).read()
    assert "map_cull.hip" in mk and "vo_map_cull.h" in mk and "vo_map_cull.h" in open(os.path.join(ROOT, "apps", "Makefile")).read()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the failure path is not reachable")
def test_new_symbols_refuse_without_a_device(vo):
    lib = vo.load_library()
    z, i, s = None, C.c_int, C.c_size_t
    Kp = np.eye(3, dtype=np.float32).ctypes.data_as(C.c_void_p)
    prm, st = vo.MapCullParams(3, 2, 2.0, 0.0, 0.0, 0, 0), vo.MapCullStats()
    assert lib.voe_map_cull_batch_dev(z, i(1), Kp, z, s(1), z, s(1), i(1), z, z, C.byref(prm), z, z, z, z) == -1
    assert b"null map" in lib.vo_last_error()
    assert lib.voe_map_cull(z, i(1), Kp, z, z, z, i(1), z, C.byref(prm), z, z, z, C.byref(st)) == -1
    assert b"null map" in lib.vo_last_error()


# ---- the restatement on the example data ----
def test_example_data_clean_drops_nothing_that_is_seen():
    r = Cc.reference("example_clean")
    seen = r["n_obs"] > 0
    assert int(seen.sum()) == 536 and int((r["n_obs"] >= 3).sum()) == 462 and len(seen) == 1000
    assert (r["verdict"][seen] == Q.KEPT).all() and (r["verdict"][~seen] == Q.UNSEEN).all() and r["keep"].all()
    assert r["stats"]["status"] == Q.NOTHING_DROPPED and r["stats"]["n_kept"] == 1000
    rms, worst, z = np.sqrt(r["mean_sq_px"][seen].max()), np.sqrt(r["max_sq_px"][seen].max()), r["min_z"][seen].min()
    print(f"clean example data: largest RMS {rms:.4g} px, largest single error {worst:.4g} px, smallest camera z {z:.4g}")
    assert rms < 1.0 / 5 and z > 0.1


def test_example_data_with_40_pushes_drops_exactly_those():
    c, r, clean = Cc.case("example_pushed"), Cc.reference("example_pushed"), Cc.reference("example_clean")
    who = c["pushed"]
    assert len(who) == 40 and len(set(who)) == 40 and (clean["n_obs"][who] >= 3).all()
    dropped = np.nonzero(~r["keep"])[0]
    assert np.array_equal(dropped, who) and (r["verdict"][who] == Q.HIGH_ERROR).all()
    others = np.setdiff1d(np.nonzero(r["n_obs"] > 0)[0], who)
    big, small = np.sqrt(r["mean_sq_px"][others].max()), np.sqrt(r["mean_sq_px"][who].min())
    print(f"seed {Cc.PUSH_SEED}: largest clean RMS {big:.4g} px (x{1 / big:.3g} below 1 px), smallest pushed RMS {small:.4g} px (x{small:.3g} above), "
          f"smallest z of a pushed landmark {r['min_z'][who].min():.3g}")
    assert big * 5 <= 1.0 and small >= 5.0 and r["min_z"][who].min() > 0
    assert r["stats"]["status"] == Q.OK and r["stats"]["n_kept"] == 960 and r["stats"]["by_verdict"][Q.HIGH_ERROR] == 40
    assert r["points"].tobytes() == c["map_pts"][r["keep"]].tobytes() and np.array_equal(r["remap"][r["keep"]], np.arange(960))


def test_parallax_case_is_chosen_from_the_data():
    """5 degrees: among the landmarks with >= 3 observations in >= 2 frames the nearest angle on either side lies well away"""
    r = Cc.reference("example_parallax")
    judged = np.isin(r["verdict"], (Q.KEPT, Q.LOW_PARALLAX))
    deg = Q.parallax_deg(r)[judged]
    below, above = deg[deg < 5.0], deg[deg >= 5.0]
    print(f"{judged.sum()} landmarks judged on parallax: smallest {deg.min():.3f} deg, {len(below)} under 5 deg (largest {below.max():.3f}), "
          f"smallest above {above.min():.3f}")
    assert int((r["verdict"] == Q.LOW_PARALLAX).sum()) == len(below) > 10 and len(above) > 300
    assert not r["marginal"].any() and deg.min() > 1.0
    assert r["stats"]["by_verdict"][Q.FEW_OBS] == 536 - 462


@pytest.mark.parametrize("name", ["example_pushed", "example_parallax", "lists", "precedence", "drop_unseen"])
def test_a_second_cull_of_the_result_drops_nothing(name):
    c, r = Cc.case(name), Cc.reference(name)
    assert r["stats"]["status"] == Q.OK
    again = Cc.run(dict(c, map_pts=r["points"], map_app=r["app"]))
    assert again["stats"]["status"] == Q.NOTHING_DROPPED and again["keep"].all() and again["stats"]["n_before"] == r["stats"]["n_kept"]
    # the survivors' statistics are what they were: the frames see them as before
    for k in ("n_obs", "n_frames", "mean_sq_px", "max_sq_px", "min_z", "cos_parallax"):
        assert again[k].tobytes() == r[k][r["keep"]].tobytes(), k


@pytest.mark.parametrize("name", ["example_pushed", "precedence", "drop_unseen"])
def test_the_survivors_are_the_map_an_update_from_empty_builds(name):
    from oracle import vo_pipeline as vp
    r = Cc.reference(name)
    m = vp.Map()
    m.update(list(r["points"]), list(r["app"]))
    assert np.array(m.pts, np.float32).reshape(-1, 3).tobytes() == r["points"].tobytes()
    assert np.array(m.app, np.float32).reshape(-1, 10).tobytes() == r["app"].tobytes()


def test_rules_on_the_hand_made_scenes():
    r = Cc.reference("precedence")
    assert r["verdict"].tolist() == [Q.UNSEEN, Q.UNSEEN, Q.FEW_OBS, Q.FEW_FRAMES, Q.NOT_FINITE, Q.NOT_FINITE, Q.BEHIND, Q.HIGH_ERROR, Q.LOW_PARALLAX,
                                     Q.KEPT, Q.KEPT, Q.KEPT]
    assert r["n_obs"][3] == 2 and r["n_frames"][3] == 1 and r["n_obs"][1] == 0
    assert r["mean_sq_px"][6] > 1.0 and r["min_z"][6] < -1      # BEHIND before HIGH_ERROR
    assert r["keep"].tolist() == [True, True] + [False] * 7 + [True] * 3 and r["remap"].tolist() == [0, 1] + [-1] * 7 + [2, 3, 4]
    off = Cc.reference("thresholds_off")
    assert off["verdict"].tolist() == [Q.UNSEEN, Q.UNSEEN, Q.KEPT, Q.KEPT, Q.NOT_FINITE, Q.NOT_FINITE, Q.BEHIND] + [Q.KEPT] * 5
    assert (off["cos_parallax"] == 1.0).all()                  # the pairs are not visited with the test off
    e = Cc.reference("max_err_alone")
    assert e["verdict"].tolist() == [Q.HIGH_ERROR, Q.KEPT, Q.HIGH_ERROR, Q.KEPT] and e["mean_sq_px"][2] > 1.0 > e["mean_sq_px"][1] * 100
    a, b, d = Cc.reference("lists"), Cc.reference("drop_unseen"), Cc.reference("dry_run")
    # landmark 8 is in all 257 frames: one of them is emptied, in another it has two rows
    assert a["n_obs"].tolist() == Cc.LISTS == [0, 1, 2, 3, 15, 16, 17, 33, 257] and a["n_frames"].tolist() == [0, 1, 2, 3, 15, 16, 17, 33, 256]
    c = Cc.case("lists")
    assert 0 in c["n_rows"] and any(len(f[1]) > n for f, n in zip(c["frames"], c["n_rows"]))
    assert any(np.signbit(f[1][f[1] == 0]).any() for f in c["frames"]) and not np.signbit(c["map_app"][c["map_app"] == 0]).any()
    assert a["verdict"].tolist() == [Q.UNSEEN, Q.FEW_OBS, Q.KEPT, Q.HIGH_ERROR, Q.KEPT, Q.KEPT, Q.HIGH_ERROR, Q.KEPT, Q.KEPT]
    assert np.array_equal(a["verdict"], b["verdict"]) and a["keep"][0] and not b["keep"][0] and b["stats"]["n_kept"] == a["stats"]["n_kept"] - 1
    assert np.array_equal(d["remap"], a["remap"]) and d["stats"] == a["stats"] and d["points"].tobytes() == Cc.case("lists")["map_pts"].tobytes()
    nr = Cc.reference("lists_no_row_counts")                  # the frames cut to their live rows, no counts: the same call
    assert Cc.case("lists_no_row_counts")["n_rows"] is None and nr["stats"] == a["stats"] and nr["mean_sq_px"].tobytes() == a["mean_sq_px"].tobytes()
    n = Cc.reference("nothing_dropped")
    assert n["stats"]["status"] == Q.NOTHING_DROPPED and n["keep"].all() and Q.UNSEEN in n["verdict"]
    assert Q.lane_tree_sum(np.arange(40.0)) == 780.0 and Q.lane_tree_sum([1e16, 1.0, -1e16] + [0.0] * 13 + [1.0]) == 0.0      # (1e16 + 1 in lane 0 first)


# ---- the measure of the GPU test: budget, ceilings, planted faults ----
def _within(name, other, budget):
    """the largest ratio of |other - reference| to the ceiling, per statistic, over the entries both judge finite"""
    a = Cc.reference(name)
    ok = (a["n_obs"] > 0) & (a["verdict"] != Q.NOT_FINITE) & (other["n_obs"] == a["n_obs"])
    out = []
    for k, ceil in zip(("mean_sq_px", "max_sq_px", "min_z", "cos_parallax"), Cc.ceilings(name, budget)):
        d = np.abs(other[k][ok] - a[k][ok])
        out.append(float(np.max(np.where(d == 0, 0.0, d / np.maximum(ceil[ok], 1e-300)), initial=0.0)))
    return out


@pytest.mark.parametrize("name", list(Cc.CASES))
def test_gpu_cases_take_no_marginal_decision_and_have_the_recorded_budget(name):
    r, rv, x = Cc.reference(name), Cc.reference(name, reverse=True), Cc.reference(name, alt=True)
    assert not r["marginal"].any() and not rv["marginal"].any() and not x["marginal"].any()
    for o in (rv, x):
        assert np.array_equal(o["verdict"], r["verdict"]) and np.array_equal(o["remap"], r["remap"]) and o["stats"] == r["stats"]
    rec = json.load(open(BUDGET))["cases"][name]
    for k in ("status", "n_before", "n_kept", "n_obs", "by_verdict"):
        assert rec[k] == r["stats"][k], k
    assert rec["sum_n_obs_sq"] == r["sum_n_obs_sq"]
    got = Cc.spreads(name)
    print(name, got)
    for k, v in got.items():
        assert abs(v - rec[k]) <= 0.05 * rec[k] + 1e-18, k     # (the same numpy gives the same figure; another one may round otherwise)
    # the ceiling holds what it is derived for: another order of summation, another order of every expression
    ratios = (_within(name, rv, rec), _within(name, x, rec))
    print(name, "reversed / other expressions, as fractions of the ceiling:", ratios)
    assert max(ratios[0]) <= 0.25 + 1e-12 and max(ratios[1]) <= 1.0


def test_planted_faults_are_seen():
    """Each fault flips a verdict of the 'lists' scene or leaves some statistic far above its ceiling.  pairs_k_le_l CANNOT: the
    pairs k == l add u_k . u_k = 1 (to rounding) to a MINIMUM over values that are all <= 1, so the minimum keeps its bits on
    every list of two or more rays, and a list of one is 1 by rule.  It is planted all the same and asserted to change nothing --
    the figure is printed -- so that nobody takes the tile loop's k != l test for the thing that a test protects; what protects it
    is the 16 x 16 tiling itself, which the list lengths 15 ... 257 of this scene cross (a pair left out or a ray of a dead lane
    let in moves cos_parallax by the angle between two cameras, the R_for_Rt figure below)."""
    name = "lists"
    rec = json.load(open(BUDGET))["cases"][name]
    ref = Cc.reference(name)
    for fault in Q.FAULTS:
        r = Cc.run(Cc.case(name), fault=fault)
        flipped = int((r["verdict"] != ref["verdict"]).sum())
        counts = int((r["n_obs"] != ref["n_obs"]).sum())
        ratios = _within(name, r, rec)
        print(f"{fault}: {flipped} verdicts flipped, {counts} observation counts differ, mean / max / z / cos at {ratios[0]:.3g}, {ratios[1]:.3g}, "
              f"{ratios[2]:.3g}, {ratios[3]:.3g} x the ceiling")
        if fault == "pairs_k_le_l":
            assert flipped == 0 and max(ratios) == 0.0
        elif fault == "dropped_last_observation":
            assert counts >= 7 and flipped >= 1                # (the landmark seen twice falls under min_obs)
        else:
            assert flipped >= 1 or max(ratios) > 1e6, fault
            assert max(ratios) > 1e6, fault


def test_compaction_cases_are_what_they_say():
    for size in (1, 255, 256, 257):
        for pattern in Cc.PATTERNS:
            c, keep = Cc.compaction(size, pattern)
            r = Cc.run(c)
            assert np.array_equal(r["keep"], keep) and not r["marginal"].any(), (size, pattern)
            assert set(r["verdict"][keep]) <= {Q.KEPT} and set(r["verdict"][~keep]) <= {Q.UNSEEN}
            assert r["stats"]["status"] == (Q.NOTHING_DROPPED if keep.all() else Q.OK)
    c, keep = Cc.compaction(65537, "every_second")
    assert len(keep) == 65537 == 256 * 256 + 1 and int(keep.sum()) == 32769 and len(c["frames"][0][1]) == 32769
