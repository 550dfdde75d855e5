"""CPU checks behind voe_map_fuse*: the ABI of declarations that live in vo_hip.h itself -- by the voe_ rule -- on a machine without a
device, struct sizes, offsets, verdict and status names (header = Python = C++), the host refusals under the host sanitizers, the
experiment on the example data with its appearances folded into classes and 300 planted duplicates (tests/map_fuse_restatement.py),
the hygiene of the GPU test's cases (no gate or tie decision differs between the float32 rules and a float64 evaluation; the dyadic
ties and boundaries are exact in both), what the cases cover, and planted faults against the comparison the GPU test uses."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import map_fuse_cases as Fc
import map_fuse_restatement as Fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("voe_map_fuse_batch_dev", "voe_map_fuse")


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---- ABI ----
def test_the_voe_rule_holds_with_the_fuse_calls_in_vo_hip_h(vo):
    lib = vo.load_library()
    hip = _read("include", "vo_hip.h")
    includes = re.findall(r'^#include "([a-z0-9_]+\.h)"', hip, flags=re.M)
    assert len(includes) == 8                                 # no ninth extension header
    declared = {}
    for h in ["vo_hip.h"] + includes:
        for n in re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _read("include", h), flags=re.S)):
            declared[n] = h
    assert all(declared[n] == "vo_hip.h" for n in NAMES)
    # at the end of the map section: behind the localisation and the refinement, in front of the extension headers
    assert (hip.index("/* LOCALISATION.") < hip.index("int vo_map_refine(") < hip.index("/* FUSE.") < hip.index("int voe_map_fuse_batch_dev(")
            < hip.index("int voe_map_fuse(") < hip.index('#include "vo_map_adjust.h"'))
    for n in declared:
        assert hasattr(lib, n), f"{n} is declared in include/{declared[n]} but not exported"
    assert lib.vo_abi_version() == 1
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M)) == set(declared)      # unversioned, and nothing else
        assert not re.search(r"map_fuse_layout|map_fuse_check|launch_map_fuse|launch_map_cull_compact", out)      # the helpers stay hidden
    assert "voe_" not in _read("visual-odometry_amd", "csrc", "vo_map_adjust.map")
    assert "map_fuse.hip" in _read("visual-odometry_amd", "csrc", "Makefile") and "bin/fuse_map" in _read("apps", "Makefile")
    # integer atomics only; the compaction and the rebuild are the cull's, shared and not copied
    src = re.sub(r"//.*", "", _read("visual-odometry_amd", "csrc", "map_fuse.hip"))
    assert "atomicAdd" in src and "atomicMin" in src and not re.search(r"atomic\w*\(\s*\(?\s*(float|double)", src)
    assert not re.search(r"\w+_(count|scan|scatter|copy|header)_kernel\b", src.replace("fuse_count_kernel", "")) and "stage_" not in src
    capi = _read("visual-odometry_amd", "csrc", "capi_map.hip")
    body = capi[capi.index("int voe_map_fuse_batch_dev("): capi.index("int voe_map_fuse(vo_map")]
    assert (body.index("launch_map_fuse(") < body.index("launch_map_cull_compact(") < body.index("launch_map_rehash(") < body.index("launch_map_fuse_finish("))
    assert "k.w.ctl + 2" in body and "hipMemcpy" not in body and "Synchronize" not in body      # behind the device flag; nothing is read back
    cull = _read("visual-odometry_amd", "csrc", "map_cull.hip")
    assert re.search(r"hipError_t launch_map_cull\(.*?return launch_map_cull_compact\(st, a\);", cull, flags=re.S)


def test_structs_verdicts_and_names_header_python_cpp(vo):
    P, S = vo.MapFuseParams, vo.MapFuseStats
    assert C.sizeof(P) == 32 and C.sizeof(S) == 56
    assert [(k, getattr(P, k).offset) for k, _ in P._fields_] == [("radius_xyz", 0), ("radius", 4), ("position", 8), ("veto_shared_frame", 12),
                                                                  ("dry_run", 16), ("reserved", 20)]
    assert [(k, getattr(S, k).offset) for k, _ in S._fields_] == [("status", 0), ("n_before", 4), ("n_after", 8), ("n_pairs", 12), ("n_conflicts", 16),
                                                                  ("n_rows_rewritten", 20), ("by_verdict", 24), ("n_gated", 48)]
    hdr = _read("include", "vo_hip.h")
    fields = re.search(r"typedef struct voe_map_fuse_stats\s*\{(.*?)\} voe_map_fuse_stats;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?:\[6\])?\s*[,;]", fields)) == tuple(k for k, _ in S._fields_)
    fields = re.search(r"typedef struct voe_map_fuse_params\s*\{(.*?)\} voe_map_fuse_params;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?:\[3\])?\s*;", fields)) == tuple(k for k, _ in P._fields_)
    assert vo.MAP_FUSE_VERDICT == Fr.VERDICT and vo.MAP_FUSE_STATUS == Fr.STATUS
    for k, name in enumerate(vo.MAP_FUSE_VERDICT):
        assert re.search(r"#define VOE_MAP_FUSE_%s\s+%d\b" % (name, k), hdr), name
    for k, name in enumerate(vo.MAP_FUSE_STATUS):
        assert re.search(r"#define VOE_MAP_FUSE_%s\s+%d\b" % (name, k), hdr), name
    for text in (_read("visual-odometry_amd", "csrc", "capi_map.hip"), _read("tests", "hostcheck", "map_fuse_checks_check.cpp")):
        assert "static_assert(sizeof(voe_map_fuse_params) == 32 && sizeof(voe_map_fuse_stats) == 56" in text
    loc = _read("include", "vo", "localise.hpp")
    names = re.search(r"fuse_verdict_name\(int verdict\) \{\s*static const char\* names\[\] = \{([^}]*)\}", loc).group(1)
    assert tuple(re.findall(r'"([A-Z_]+)"', names)) == vo.MAP_FUSE_VERDICT
    assert " fuse(" in loc and "struct FuseOptions" in loc
    assert hasattr(vo.Map, "fuse") and hasattr(vo.Map, "fuse_batch_dev")
    # the kernels' verdict numbers are the header's
    enum = re.search(r"enum \{ (FV_NOT_FINITE.*?) \};", _read("visual-odometry_amd", "csrc", "map_fuse.hip")).group(1)
    assert [(a[3:], int(b)) for a, b in re.findall(r"(FV_[A-Z_]+) = (\d)", enum)] == list(zip(Fr.VERDICT, range(6)))
    # what tests/map_fuse_cases.py:cells() restates
    assert "constexpr int FUSE_NC = 128;" in _read("visual-odometry_amd", "csrc", "vo_internal.h")


def test_map_fuse_refusals_under_the_host_sanitizers(tmp_path):
    """visual-odometry_amd/csrc/map_checks.h: map_fuse_check in a stand-alone program under AddressSanitizer and UBSan, each row
    against the code and the whole message"""
    exe = str(tmp_path / "map_fuse_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "visual-odometry_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostcheck", "map_fuse_checks_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("map_fuse_checks_check: all ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("-> ok") >= 78 and "FAILED" not in r.stdout


# ---- the experiment: repeated appearance, planted duplicates ----
def test_example_with_folded_appearances_needs_the_spatial_gate():
    """world.dat's appearances folded into 50 classes of 20 near-copies and 300 landmarks entered a second time (Fc.experiment).
    With radius 0.1 and radius_xyz 0.04 (world.dat's closest two landmarks are 0.051 apart) the rules pair exactly the 300 planted
    duplicates; with the spatial gate effectively off the mutual pairs of appearance alone are wrong."""
    pts, app, ch = Fc.experiment()
    planted = {(int(a), 1000 + j) for j, a in enumerate(ch)}
    d = np.sqrt(Fr.gap2(pts[:1000], np.float64) + np.eye(1000) * 1e9).min()
    assert 0.05 < d < 0.052
    r = Fr.run(pts, app, None, None, 0, 0.04, 0.1)
    pairs = Fc.pairs_of(r)
    print(f"both gates: {len(pairs)} pairs, {len(pairs - planted)} wrong; n_gated {r['stats']['n_gated']}")
    assert len(pairs) == 300 and pairs == planted and r["stats"]["n_after"] == 1000
    assert Fr.margins(pts, app, 0.04, 0.1) == []
    with np.errstate(over="ignore"):
        loose = Fr.run(pts, app, None, None, 0, 1e30, 0.1)
    lp = Fc.pairs_of(loose)
    print(f"no spatial gate: {len(lp)} pairs, {len(lp - planted)} wrong")      # 204 of 204 when this was written
    assert len(lp - planted) >= 1


# ---- the cases of the GPU test ----
@pytest.mark.parametrize("name", list(Fc.CASES))
def test_case_takes_no_marginal_decision(name):
    """both gates, the candidate sets and the partners (hence every tie) are the same in the float32 rules and in float64; in the
    DYADIC cases because both are exact there (the ties and boundaries are deliberate), in every other case because none is close"""
    c, ref = Fc.case(name), Fc.reference(name)
    assert Fc.margins(c) == []
    assert c["dyadic"] == (name in Fc.DYADIC)
    if c["dyadic"]:
        for a in (c["map_app"], c["map_pts"]):
            assert (a * 2.0 ** 27 == np.round(a * 2.0 ** 27)).all() and np.abs(a).max() < 64
        p32, d32, g32, _, _ = Fr.partners(c["map_pts"], c["map_app"], c["radius_xyz"], c["radius"], np.float32)
        p64, d64, g64, _, _ = Fr.partners(c["map_pts"], c["map_app"], c["radius_xyz"], c["radius"], np.float64)
        assert (p32 == p64).all() and np.isfinite(d64[p64 >= 0]).all()
    assert Fr.compare(ref, ref) == []


def test_the_cases_cover_what_they_are_there_for():
    st = {n: Fc.reference(n) for n in Fc.CASES}
    V = Fr.VERDICT
    d = st["dyadic"]
    assert [V[k] for k in d["verdict"]] == ["ALONE", "ALONE", "SURVIVOR", "ABSORBED", "ALONE", "ALONE", "SURVIVOR", "ABSORBED", "SURVIVOR", "ABSORBED",
                                           "NOT_MUTUAL", "SURVIVOR", "NOT_MUTUAL", "ABSORBED", "NOT_MUTUAL", "SURVIVOR", "ABSORBED", "SURVIVOR", "ABSORBED",
                                           "ALONE"]
    c = Fc.case("dyadic")
    x2, r2 = np.float32(c["radius_xyz"]) ** 2, np.float32(c["radius"]) ** 2
    G, D = Fr.gap2(c["map_pts"]), Fr.N.dist2(c["map_app"], c["map_app"])
    zero = np.float32(0)
    # on the radius: excluded; the offset one ulp inside the radius: a pair (its square then lies two ulps inside the radius's)
    assert G[0, 1] == x2 and c["map_pts"][3, 0] == np.nextafter(np.float32(c["radius_xyz"]), zero) and d["gap2"][2] == G[2, 3] < x2
    assert D[4, 5] == r2 and c["map_app"][7, 0] == np.nextafter(np.float32(c["radius"]), zero) and d["dist2"][6] == D[6, 7] < r2
    assert G[2, 3] == np.nextafter(np.nextafter(x2, zero), zero) and D[6, 7] == np.nextafter(np.nextafter(r2, zero), zero)
    assert D[8, 9] == D[8, 10] and d["partner"][8] == 9 and D[13, 11] == D[13, 12] and d["partner"][13] == 11      # ties: the lowest index
    assert d["partner"][14:17].tolist() == [15, 16, 15]       # the chain a -> b <-> c
    assert d["gap2"][17] == 0 and (c["map_pts"][:, 2] == 0).all()      # the same point; zero extent on z
    assert st["dyadic"]["map_pts"][2, 0] == np.float32((0.25 - 2.0 ** -26) / 2) and st["dyadic_keep"]["map_pts"][2, 0] == 0      # position 1 and 0
    # partners across a face, an edge and a corner of the device's grid
    c, r = Fc.case("grid"), st["grid"]
    cl = Fc.cells(c)
    s = np.nonzero(r["verdict"] == Fr.SURVIVOR)[0]
    across = np.bincount((cl[s] != cl[r["partner"][s]]).sum(axis=1), minlength=4)
    assert cl.max() >= 11 and (across[1:] >= 3).all(), across
    assert (Fc.cells(Fc.case("one_point")) == 0).all() and np.ptp(Fc.case("one_point")["map_pts"], axis=0).max() == 0
    assert st["one_point"]["stats"]["n_gated"] == 300 * 299 and st["one_point"]["stats"]["n_pairs"] == 60
    assert np.ptp(Fc.case("flat")["map_pts"][:, 2]) == 0 and Fc.cells(Fc.case("flat"))[:, :2].max() > 3
    c = Fc.case("clamped")
    assert np.ptp(c["map_pts"][:, 0]) / c["radius_xyz"] > 1000 * Fc.cells(c).max() and st["clamped"]["stats"]["n_pairs"] == 100
    for n in (0, 1, 255, 256, 257, 513):
        r = st[f"size_{n}"]
        assert r["stats"]["n_before"] == n
        if n > 1:
            ab = r["verdict"] == Fr.ABSORBED
            assert ab[1] and ab[-1] and np.diff(np.nonzero(ab)[0]).tolist().count(1) > 20      # first, last, and a run
    assert st["size_0"]["stats"]["status"] == st["size_1"]["stats"]["status"] == Fr.NOTHING_FUSED
    s = st["special"]
    assert [V[k] for k in s["verdict"][:6]] == ["NOT_FINITE"] * 6 and [V[k] for k in s["verdict"][24:30]] == ["ALONE"] * 6
    assert [V[k] for k in s["verdict"][30:32]] == ["NOT_FINITE"] * 2 and s["stats"]["n_pairs"] == 2 and (s["remap"] >= 0).all()
    # the frames: rows on survivors, on absorbed entries and on nothing, rows behind the count that would hit, the veto
    c, r = Fc.case("frames"), st["frames"]
    hit = r["ent"][r["ent"] >= 0]
    assert (r["verdict"][hit] == Fr.ABSORBED).any() and (r["verdict"][hit] == Fr.SURVIVOR).any() and (r["ent"][0, :100] == -1).any()
    assert c["n_rows"][1] < len(c["frames"][1]) and (Fr.N.lookup(c["map_app"], [c["frames"][1][c["n_rows"][1]:]], None, 40)[0] >= 0).any()
    assert r["stats"]["n_conflicts"] > 0 and st["frames_no_veto"]["stats"]["n_conflicts"] == 0
    assert st["frames_no_veto"]["stats"]["n_pairs"] == r["stats"]["n_pairs"] + r["stats"]["n_conflicts"]
    assert Fc.case("frames_no_count")["n_rows"] is None and st["frames_dry_run"]["map_app"].tobytes() == c["map_app"].tobytes()
    assert st["together"]["stats"]["status"] == Fr.NOTHING_FUSED and st["together"]["stats"]["n_conflicts"] == 12 == st["together_no_veto"]["stats"]["n_pairs"]
    assert st["nothing"]["stats"]["status"] == Fr.NOTHING_FUSED and (st["nothing"]["ent"] >= 0).all()
    assert Fc.case("bound_above_size")["dup_rows"] > 0 and Fc.case("zero_rows")["n_max"] == 0 and Fc.case("zero_rows")["frames"] is not None
    assert all((st[n]["remap"] >= 0).all() for n in Fc.CASES)      # rule 6: never -1
    assert {Fc.case(n)["position"] for n in Fc.CASES} == {0, 1}


@pytest.mark.parametrize("fault", Fr.FAULTS)
def test_every_planted_fault_is_seen_by_the_gpu_tests_comparison(fault):
    seen = [n for n in Fc.CASES if Fr.compare(Fc.reference(n), Fc.reference(n, fault=fault))]
    print(fault, "seen on", seen)
    assert seen
    if fault in ("tie_to_higher", "le_for_lt_xyz", "le_for_lt_app", "chains_followed"):
        assert set(seen) & set(Fc.DYADIC)
