"""CPU checks behind voe_map_align* / voe_map_merge*: the voe_ rule with the new header, the records' sizes and offsets, the
refusal without a device, the float64 restatement (tests/map_align_restatement.py) on planted similarities, similarity_pose on
the example frames, and -- for every case of the GPU test -- the conditions its exact comparisons rest on (no pair in the band
of a model that decides, few hypotheses with a band at all, no refit near a float32 rounding boundary); it writes
profiles/map_align_budget.json, into which no device value goes."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import map_align_cases as Cc
import map_align_restatement as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"voe_map_size_bound", "voe_map_align_dev", "voe_map_align", "voe_map_merge_dev", "voe_map_merge"}


# ---- ABI ----
def test_the_voe_rule_holds_the_new_symbols(vo):
    import shutil
    import subprocess
    lib = vo.load_library()
    hip = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    assert hip.count('#include "vo_map_align.h"') == 1 and hip.index('#include "vo_map_cull.h"') < hip.index('#include "vo_map_align.h"')
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo_map_align.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", txt)) == NEW
    for n in NEW:
        assert hasattr(lib, n), n
    assert lib.vo_abi_version() == 1
    assert "voe_" not in open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "vo_map_adjust.map")).read()
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert NEW <= set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M))      # unversioned
    mk = open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "Makefile")).read()
    assert "map_align.hip" in mk and "vo_map_align.h" in mk and "vo_map_align.h" in open(os.path.join(ROOT, "apps", "Makefile")).read()
    src = open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "map_align.hip")).read()
    assert "atomicAdd(double" not in src and "atomicAdd(float" not in src and "unsafeAtomicAdd" not in src and "cooperative" not in src.lower()
    assert "ransac_score_body(AlignModel" in src and "ransac_select_best(" in src


def test_records_are_pinned(vo):
    P, S, M = vo.MapAlignParams, vo.MapAlignStats, vo.MapMergeStats
    assert C.sizeof(P) == 32 and C.sizeof(S) == 48 and C.sizeof(M) == 16
    assert [getattr(P, k).offset for k, _ in P._fields_] == [0, 8, 12, 16, 20, 24, 28]
    assert [getattr(S, k).offset for k, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert [getattr(M, k).offset for k, _ in M._fields_] == [0, 4, 8, 12]
    assert [k for k, _ in S._fields_] == ["status", "n_matches", "n_inliers", "best_hypothesis", "best_count", "n_valid", "refit_kept", "reserved",
                                          "scale", "rms"]
    hdr = open(os.path.join(ROOT, "include", "vo_map_align.h")).read()
    assert vo.MAP_ALIGN_STATUS == A.STATUS
    for k, name in enumerate(vo.MAP_ALIGN_STATUS):
        assert re.search(r"#define VOE_MAP_ALIGN_%s\s+%d\b" % (name, k), hdr), name
    assert re.search(r"#define VOE_MAP_MERGE_TAKE_SRC\s+0\b", hdr) and re.search(r"#define VOE_MAP_MERGE_KEEP_DST\s+1\b", hdr)
    assert re.search(r"#define VOE_MAP_ALIGN_MAX_REFITS\s+%d\b" % vo.MAP_ALIGN_MAX_REFITS, hdr) and vo.MAP_ALIGN_MAX_REFITS == A.MAX_REFITS
    assert (vo.MAP_MERGE_TAKE_SRC, vo.MAP_MERGE_KEEP_DST) == (A.TAKE_SRC, A.KEEP_DST)
    cap = open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "capi_map.hip")).read()
    assert "sizeof(voe_map_align_params) == 32 && sizeof(voe_map_align_stats) == 48 && sizeof(voe_map_merge_stats) == 16" in cap
    for n in ("align", "align_dev", "merge", "merge_dev", "size_bound"):
        assert hasattr(vo.Map, n)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the failure path is not reachable")
def test_new_symbols_refuse_without_a_device(vo):
    lib = vo.load_library()
    z = None
    prm, st, ms, n = vo.MapAlignParams(1, 64, 1, 1, 3, 0.05, 0), vo.MapAlignStats(), vo.MapMergeStats(), C.c_int()
    S = np.zeros(16, np.float32)
    for rc in (lib.voe_map_size_bound(z, C.byref(n)), lib.voe_map_align_dev(z, z, C.byref(prm), z, z, z, z, z, z),
               lib.voe_map_align(z, z, C.byref(prm), S.ctypes.data_as(C.c_void_p), z, z, z, z, C.byref(st)),
               lib.voe_map_merge_dev(z, z, z, C.c_int(0), z, z), lib.voe_map_merge(z, z, z, C.c_int(1), z, C.byref(ms))):
        assert rc == -1 and b"null map" in lib.vo_last_error()


# ---- the restatement ----
def test_sample_rule_and_lookup():
    assert A.splitmix64(0) == 0xE220A8397B1DCDAF                # the published first output of splitmix64 from state 0
    for n in (3, 4, 100):
        for h in range(20):
            s = A.sample(7, h, n)
            assert s is None or (len(set(s)) == 3 and all(0 <= v < n for v in s))
    assert A.sample(7, 0, 2) is None
    app = np.array([[0.0] * 10, [1.0] * 10, [np.nan] + [2.0] * 9, [0.0] * 9 + [3.0]], np.float32)
    q = np.array([[1.0] * 10, [-0.0] * 10, [np.nan] + [2.0] * 9, [5.0] * 10], np.float32)
    pairs, ent = A.lookup(app, q)
    assert ent.tolist() == [1, 0, -1, -1] and pairs.tolist() == [[0, 1], [1, 0]]


@pytest.mark.parametrize("with_scale", [1, 0])
def test_umeyama_recovers_planted_similarities(with_scale):
    rng = np.random.default_rng(5)
    for k in range(20):
        R = Cc.rotation(rng.normal(size=3), rng.uniform(0.1, 3.0))
        c, t = (rng.uniform(0.2, 5.0) if with_scale else 1.0), rng.normal(size=3) * 10
        a = rng.normal(size=(3 + k, 3))
        M, tt, cc, s, _ = A.umeyama(a, c * a @ R.T + t, with_scale)
        assert np.abs(M - c * R).max() < 1e-12 * c and np.abs(tt - t).max() < 1e-11 and abs(cc - c) < 1e-12 * c
        assert abs(np.linalg.det(M / cc) - 1) < 1e-12
    # a reflection is not a similarity: the best ROTATION comes back
    a = rng.normal(size=(10, 3))
    M, _, cc, _, _ = A.umeyama(a, a * np.array([1.0, 1.0, -1.0]), 1)
    assert abs(np.linalg.det(M / cc) - 1) < 1e-12
    assert A.umeyama(np.array([[0.0, 0, 0], [1, 2, 3], [2, 4, 6]]), a[:3], 1) is None       # collinear
    assert A.umeyama(np.ones((3, 3)), a[:3], 1) is None                                       # coincident


def test_similarity_pose_leaves_every_reprojection_of_the_example_frames_unchanged(vo):
    import map_refine_restatement as R
    P = R.example_problem()
    c, Rm, t = Cc.example()["truth"]
    S = np.eye(4); S[:3, :3] = c * Rm; S[:3, 3] = t
    K, world = np.asarray(P["K"], np.float64), np.asarray(P["world_pts"], np.float64)
    moved = world @ S[:3, :3].T + S[:3, 3]
    worst = 0.0
    for T in P["poses"]:
        T = np.asarray(T, np.float64)
        T2 = A.similarity_pose(T, S)
        assert np.abs(T2 - vo.similarity_pose(T, S)).max() < 1e-12
        assert np.abs(T2[:3, :3] @ T2[:3, :3].T - np.eye(3)).max() < 1e-12 and (T2[3] == [0, 0, 0, 1]).all()
        pc, pc2 = world @ T[:3, :3].T + T[:3, 3], moved @ T2[:3, :3].T + T2[:3, 3]
        assert np.abs(pc2 - c * pc).max() < 1e-12 * np.abs(c * pc).max()
        front = pc[:, 2] > 0.1
        q, q2 = pc[front] @ K.T, pc2[front] @ K.T
        worst = max(worst, np.abs(q[:, :2] / q[:, 2:] - q2[:, :2] / q2[:, 2:]).max())
    print(f"largest change of a projection over {len(P['poses'])} frames: {worst:.3g} px")
    assert worst < 1e-9                                         # double rounding of pixels of a few hundred


def test_example_case_is_what_the_issue_describes():
    c, r = Cc.case("example"), Cc.reference("example")
    assert r["n_matches"] == 950 and len(c["src_pts"]) == 950 and len(c["dst_pts"]) == 1000 and len(c["pushed_src"]) == 40
    clean = np.setdiff1d(np.arange(950), c["pushed_src"])
    assert r["status"] == A.OK and np.array_equal(np.nonzero(r["mask"])[0], clean) and r["n_inliers"] == 910 and r["n_valid"] == 64
    _, _, d2 = A.classify(r["S"][:3, :3], r["S"][:3, 3], r["a"], r["b"], r["thr2"])
    print(f"clean residuals <= {np.sqrt(d2[clean].max()):.3g}, pushed >= {np.sqrt(d2[c['pushed_src']].min()):.3g}, c off by {abs(r['scale'] - 2.7):.3g}")
    assert np.sqrt(d2[clean].max()) < 2e-6 and np.sqrt(d2[c["pushed_src"]].min()) > 0.2 and abs(r["scale"] - 2.7) < 1e-8
    assert not (np.abs(d2 - r["thr2"]) <= 1e-4 * r["thr2"]).any()


def test_hand_made_cases_are_what_they_say():
    ref = Cc.reference
    assert ref("collinear")["status"] == A.NO_HYPOTHESIS and ref("collinear")["n_matches"] == 60 and ref("collinear")["rank_ratio"].max() < 1e-12
    assert ref("coincident")["status"] == A.NO_HYPOTHESIS and ref("coincident")["n_valid"] == 0
    assert ref("disjoint")["status"] == A.FEW_MATCHES and ref("disjoint")["n_matches"] == 0
    assert ref("two")["status"] == A.FEW_MATCHES and ref("two")["n_matches"] == 2
    for n in ("collinear", "coincident", "disjoint", "two"):
        r = ref(n)
        assert (r["S"] == np.eye(4)).all() and not r["mask"].any() and r["n_inliers"] == 0 and r["scale"] == 1.0 and r["rms"] == 0.0
    p = ref("planar")
    assert p["status"] == A.OK and abs(np.linalg.det(p["S"][:3, :3].astype(np.float64) / p["scale"]) - 1) < 1e-5 and p["refit_kept"] == 1
    assert ref("rigid")["scale"] == 1.0 and ref("rigid")["n_inliers"] == 285
    # nan: the NaN point is a match but never an inlier, and the hypotheses that drew it are invalid; NaN appearances match nothing
    c, r = Cc.case("nan"), ref("nan")
    k = int(np.flatnonzero(r["pairs"][:, 0] == c["nan_point"])[0])
    assert not r["mask"][k] and r["n_matches"] == 58 and r["n_inliers"] == 57
    drew = [h for h in range(64) if k in A.sample(1, h, 58)]
    assert len(drew) >= 1 and (r["counts"][drew] == -1).all() and r["n_valid"] == 64 - len(drew)
    assert c["nan_app_src"] not in r["pairs"][:, 0] and c["nan_app_dst_of"] not in r["pairs"][:, 0] and c["signed_zero"] in r["pairs"][:, 0]
    t = ref("tie")
    assert (t["counts"] == t["counts"].max()).sum() >= 2 and t["best_hypothesis"] == int(np.flatnonzero(t["counts"] == 50)[0]) and t["refit_kept"] == 0
    n, n0 = ref("noisy"), A.run(dict(Cc.case("noisy"), params=dict(Cc.case("noisy")["params"], n_refits=0)))
    print(f"noisy: rms of the winner {n0['rms']:.4g}, of the refit {n['rms']:.4g}")
    assert n["refit_kept"] == 1 and n0["refit_kept"] == 0 and n["rms"] < n0["rms"] and n["n_inliers"] >= n0["n_inliers"]
    j = ref("refit_rejected")
    assert j["status"] == A.OK and j["refit_kept"] == 0 and j["n_inliers"] == 65 and len(j["margins"]) == 1      # a valid refit, not taken
    f = ref("far")
    assert f["status"] == A.OK and f["n_inliers"] == 480 and np.abs(f["S"][:3, 3]).max() > 900


# ---- the conditions of the GPU comparison, and the budget ----
ALL = list(Cc.CASES) + list(Cc.MERGE_CASES)


@pytest.mark.parametrize("name", ALL)
def test_no_marginal_decision(name):
    r, rv = Cc.reference(name), Cc.reference(name, True)
    valid = r["counts"] >= 0
    assert all(b == 0 for b in r["band_models"]) and all(b == 0 for b in rv["band_models"]), "a pair in the band of the winner or of a refit"
    if r["best_hypothesis"] >= 0:
        near = valid & (r["counts"] + r["band_pop"] >= r["best_count"])
        assert (r["band_pop"][near] == 0).all(), "a hypothesis that could overtake the winner has a pair in its band"
        assert int((r["band_pop"][valid] > 0).sum()) * 10 <= int(valid.sum())
    assert not ((r["rank_ratio"] > 1e-10) & (r["rank_ratio"] < 1e-8)).any(), "a solve near the rank test"
    for k in ("status", "n_inliers", "best_hypothesis", "refit_kept"):
        assert r[k] == rv[k]
    assert np.array_equal(r["mask"], rv["mask"])
    if r["budget"] is not None:
        for (mM, mt) in r["margins"]:
            assert mM > 2 * r["budget"]["M"] and mt > 2 * r["budget"]["t"], "a refit near a float32 rounding boundary"


def test_budget_file_is_written_from_the_restatement_alone():
    rec = {name: Cc.budget_record(name) for name in ALL}
    for name, v in rec.items():
        assert set(v["spread"]) == set(("S", "scale", "rms")) and all(np.isfinite(list(v["apriori"].values())))
        assert Cc.reference(name)["status"] != A.OK or v["apriori"]["scale"] > 0
    # the two-pass centring: the far scene's bound stays under a float32 ulp of its translation
    far = Cc.ceilings(rec["far"])
    print("far:", rec["far"]["spread"], rec["far"]["apriori"])
    assert far["S"] < np.spacing(np.float32(1000.0)) / 10
    doc = dict(note="per case: the statistics of the float64 restatement (tests/map_align_restatement.py), the spread of S, scale and rms "
                    "between forward and reversed summation, and the a-priori rounding bound of its docstring.  Written by "
                    "tests/test_map_align_cpu.py; no device value goes into it.  The GPU ceiling is 4 x spread + 2 x apriori (S: one float32 "
                    "ulp more).", cases=rec)
    os.makedirs(os.path.dirname(Cc.BUDGET), exist_ok=True)
    with open(Cc.BUDGET, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    assert Cc.load_budget().keys() == rec.keys()


def test_merge_restatement():
    c = Cc.case("miss_257")
    r = Cc.reference("miss_257")
    for policy in (A.TAKE_SRC, A.KEEP_DST):
        m = A.merge(c, r["S"], policy)
        assert m["stats"]["n_src"] == 557 and m["stats"]["n_shared"] == 300 and m["stats"]["n_appended"] == 257
        assert m["app"][:303].tobytes() == c["dst_app"].tobytes() and (m["remap"] >= 0).all()
        if policy == A.KEEP_DST:
            assert m["pts"][:303].tobytes() == c["dst_pts"].tobytes() and len(m["rows"]) == 257
            assert np.array_equal(m["remap"][m["rows"]], 303 + np.arange(257))
        else:
            moved = A.apply_S(r["S"], c["src_pts"])
            sh = r["pairs"]
            assert m["pts"][sh[:, 1]].tobytes() == moved[sh[:, 0]].tobytes()
