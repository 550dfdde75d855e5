"""CPU checks behind voe_map_guided*: the ABI of declarations that live in vo_hip.h itself -- by the voe_ rule -- on a machine without
a device, struct sizes, offsets and status names (header = Python = C++), the host refusals under the host sanitizers, the float32
projection of the restatement against the oracle bit for bit, the experiment on the example data with its appearances folded into
classes (tests/map_guided_restatement.py against tests/map_nearest_restatement.py), the hygiene of the GPU test's cases (no decision
differs between the float32 rules and a float64 evaluation; the dyadic ties and boundaries are exact in both), and planted faults
against the comparison the GPU test uses."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import map_guided_cases as Gc
import map_guided_restatement as G
import map_nearest_restatement as N
import map_refine_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("voe_map_guided_batch_dev", "voe_map_guided_dev", "voe_map_guided")


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---- ABI ----
def test_the_voe_rule_holds_with_the_guided_calls_in_vo_hip_h(vo):
    lib = vo.load_library()
    hip = _read("include", "vo_hip.h")
    includes = re.findall(r'^#include "([a-z0-9_]+\.h)"', hip, flags=re.M)
    assert len(includes) == 8                                 # no ninth extension header
    declared = {}
    for h in ["vo_hip.h"] + includes:
        for n in re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _read("include", h), flags=re.S)):
            declared[n] = h
    assert all(declared[n] == "vo_hip.h" for n in NAMES)
    # behind NEAREST, in front of the localisation
    assert (hip.index("/* NEAREST.") < hip.index("int voe_map_nearest(") < hip.index("/* GUIDED.") < hip.index("int voe_map_guided_batch_dev(")
            < hip.index("int voe_map_guided_dev(") < hip.index("int voe_map_guided(") < hip.index("/* LOCALISATION."))
    for n in declared:
        assert hasattr(lib, n), f"{n} is declared in include/{declared[n]} but not exported"
    assert lib.vo_abi_version() == 1
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M)) == set(declared)      # unversioned, and nothing else
        assert not re.search(r"map_guided_layout|map_guided_check|launch_map_guided|launch_nearest_", out)      # the helpers stay hidden
    assert "voe_" not in _read("visual-odometry_amd", "csrc", "vo_map_adjust.map")
    assert "map_guided.hip" in _read("visual-odometry_amd", "csrc", "Makefile") and "bin/track_map" in _read("apps", "Makefile")
    # the map is never written: map_guided.hip holds its arrays as pointers to const; integer atomics only
    src = re.sub(r"//.*", "", _read("visual-odometry_amd", "csrc", "map_guided.hip"))
    internal = _read("visual-odometry_amd", "csrc", "vo_internal.h")
    args = re.search(r"struct MapGuidedArgs \{(.*?)\n\};", internal, flags=re.S).group(1)
    assert re.search(r"\bconst\s+float\s*\*\s*pts\s*;", args) and "const_cast" not in src
    assert "atomicAdd" in src and not re.search(r"atomic\w*\(\s*\(?\s*float", src)
    # the kernels nearest owns are shared, not copied
    assert re.search(r"\blaunch_nearest_unique\s*\(", src) and re.search(r"\blaunch_nearest_finish\s*\(", src)
    assert not re.search(r"\w+_(claim|resolve|finish)_kernel", src)


def test_structs_statuses_and_names_header_python_cpp(vo):
    P, S = vo.MapGuidedParams, vo.MapGuidedStats
    assert C.sizeof(P) == 32 and C.sizeof(S) == 48
    assert [(k, getattr(P, k).offset) for k, _ in P._fields_] == [("radius_px", 0), ("radius", 4), ("ratio", 8), ("unique", 12), ("z_near", 16),
                                                                  ("z_far", 20), ("reserved", 24)]
    assert [(k, getattr(S, k).offset) for k, _ in S._fields_][-3:] == [("n_nan", 28), ("n_in_view", 32), ("n_gated", 40)]
    assert [k for k, _ in S._fields_][:8] == [k for k, _ in vo.MapNearestStats._fields_]      # the eight counts, in the same order
    hdr = _read("include", "vo_hip.h")
    fields = re.search(r"typedef struct voe_map_guided_stats\s*\{(.*?)\} voe_map_guided_stats;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\b(n_[a-z_]+)\s*[,;]", fields)) == tuple(k for k, _ in S._fields_)
    fields = re.search(r"typedef struct voe_map_guided_params\s*\{(.*?)\} voe_map_guided_params;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?:\[2\])?\s*;", fields)) == tuple(k for k, _ in P._fields_)
    assert vo.MAP_GUIDED_STATUS == G.STATUS == vo.MAP_NEAREST_STATUS
    for k, name in enumerate(vo.MAP_GUIDED_STATUS):
        assert re.search(r"#define VOE_MAP_GUIDED_%s\s+%d\b" % (name, k), hdr), name
    for text in (_read("visual-odometry_amd", "csrc", "capi_map.hip"), _read("tests", "hostcheck", "map_guided_checks_check.cpp")):
        assert "static_assert(sizeof(voe_map_guided_params) == 32 && sizeof(voe_map_guided_stats) == 48" in text
    loc = _read("include", "vo", "localise.hpp")
    names = re.search(r"guided_status_name\(int status\) \{\s*static const char\* names\[\] = \{([^}]*)\}", loc).group(1)
    assert tuple(re.findall(r'"([A-Z_]+)"', names)) == vo.MAP_GUIDED_STATUS
    assert " guided(const Camera& camera" in loc and "struct GuidedOptions" in loc
    assert hasattr(vo.Map, "guided") and hasattr(vo.Map, "guided_batch_dev")
    # the kernels' status numbers are the header's
    enum = re.search(r"enum \{ (GS_MATCHED.*?) \};", _read("visual-odometry_amd", "csrc", "map_guided.hip")).group(1)
    assert [(a[3:], int(b)) for a, b in re.findall(r"(GS_[A-Z_]+) = (\d)", enum)] == list(zip(G.STATUS, range(6)))
    # what tests/map_guided_cases.py:groups() restates
    internal = _read("visual-odometry_amd", "csrc", "vo_internal.h")
    assert "constexpr int GUIDED_NC = 64;" in internal and "constexpr size_t GUIDED_GROUP_BYTES = (size_t)128 << 20;" in internal


def test_map_guided_refusals_under_the_host_sanitizers(tmp_path):
    """visual-odometry_amd/csrc/map_checks.h: map_guided_check in a stand-alone program under AddressSanitizer and UBSan, each row
    against the code and the whole message"""
    exe = str(tmp_path / "map_guided_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "visual-odometry_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostcheck", "map_guided_checks_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("map_guided_checks_check: all ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("-> ok") >= 75 and "FAILED" not in r.stdout


# ---- the projection ----
def test_the_float32_projection_is_the_oracles_bit_for_bit(o32):
    """rule 1 on the example data: wherever the oracle's projectPoint keeps a point (depth gate and image gate), the restatement has
    it in view at the same bits; and the points the restatement has in view and inside the image are exactly those"""
    from oracle.oracle import Camera as OCam
    E = R.example_problem()
    rows, cols, zn, zf = E["cam"]
    kept = 0
    for T in E["poses"][::4]:
        T = np.asarray(T, np.float32)
        uv_o, _ = o32.project_points(OCam(rows, cols, zn, zf, E["K"], T), E["world_pts"], keep_indices=True)
        u, v, view = G.project(E["K"], T, E["world_pts"], zn, zf)
        valid = uv_o[:, 0] != -1
        with np.errstate(invalid="ignore"):
            inside = view & ~((u < 0) | (u > np.float32(cols - 1))) & ~((v < 0) | (v > np.float32(rows - 1)))
        assert (valid == inside).all()
        assert np.stack([u, v], axis=1)[valid].astype(np.float32).tobytes() == uv_o[valid].astype(np.float32).tobytes()
        kept += int(valid.sum())
    assert kept > 1000


# ---- the experiment: repeated appearance ----
def test_example_with_folded_appearances_needs_the_pixel_gate():
    """The 1000 appearances of world.dat folded into 50 classes of 20 near-copies (N(0, 0.002) apart, default_rng(2)), every frame
    row its landmark's appearance pushed by N(0, 0.005), every pose pushed by U(-0.01, 0.01) and U(-0.005, 0.005) rad
    (default_rng(3)).  Appearance alone (radius 0.1, ratio 0.8) leaves more than 90 % of the rows AMBIGUOUS; gated to 8 px of the
    projection under the pushed pose more than 95 % go to their file id and fewer than 0.5 % to a wrong one."""
    E = R.example_problem()
    rng = np.random.default_rng(2)
    W = (rng.uniform(-1, 1, (50, 10))[np.arange(1000) % 50] + rng.normal(0, 0.002, (1000, 10))).astype(np.float32)
    assert len(E["world_app"]) == 1000
    rng = np.random.default_rng(3)
    frames = [(uv, (W[ids.astype(int)] + rng.normal(0, 0.005, (len(ids), 10))).astype(np.float32)) for (uv, _), ids in zip(E["frames"], E["ids"])]
    priors = [(Gc._pose(rng, 0.005, 0.01) @ T).astype(np.float32) for T in E["poses"]]
    n_max = max(len(a) for _, a in frames)
    rows = sum(len(a) for _, a in frames)
    ids = np.full((len(frames), n_max), -2, np.int64)
    for f, i in enumerate(E["ids"]):
        ids[f, : len(i)] = i
    _, _, zn, zf = E["cam"]

    def tally(r):
        right = int(((r["status"] == G.MATCHED) & (r["entry"] == ids)).sum())
        wrong = int(((r["status"] == G.MATCHED) & (r["entry"] != ids)).sum())
        return right, wrong, int((r["status"] == G.AMBIGUOUS).sum()), int((r["status"] == G.NO_ENTRY).sum())

    a = tally(N.run(W, [q for _, q in frames], None, n_max, 0.1, 0.8, 0))
    print(f"{rows} rows; appearance only (right, wrong, ambiguous, no candidate): {a}")
    assert rows == 10012 and a[2] > 0.90 * rows
    for px in (8.0, 16.0):
        r = G.run(E["world_pts"], W, E["K"], frames, priors, None, n_max, px, 0.1, 0.8, 0, zn, zf)
        g = tally(r)
        print(f"gated to {px:g} px: {g}; entries tested per row {r['stats']['n_gated'] / rows:.3f}")
        if px == 8.0:
            assert g[0] > 0.95 * rows and g[1] < 0.005 * rows


# ---- the cases of the GPU test ----
def _margins(c):
    return G.margins(c["map_pts"], c["map_app"], c["K"], c["frames"], c["poses"], c["n_rows"], c["n_max"], c["radius_px"], c["radius"], c["ratio"],
                     c["unique"], c["z_near"], c["z_far"])


@pytest.mark.parametrize("name", list(Gc.CASES))
def test_case_takes_no_marginal_decision(name):
    """in view, the pixel gate, `< r2`, best, tie, ratio and unique decide alike in the float32 rules and in float64; in the DYADIC
    cases because both are exact there (the ties and boundaries are deliberate), in every other case because no decision is close"""
    c, ref = Gc.case(name), Gc.reference(name)
    assert _margins(c) == []
    assert c["dyadic"] == (name in Gc.DYADIC)
    if c["dyadic"]:
        f = np.log2(np.diag(c["K"])[:2])
        assert (f == np.round(f)).all()                       # focal lengths: powers of two
        for a in [c["map_app"]] + [q for _, q in c["frames"]]:
            assert (a * 8192 == np.round(a * 8192)).all() and np.abs(a).max() < 64
        for T, (uv, _) in zip(c["poses"], c["frames"]):
            assert (uv * 8 == np.round(uv * 8)).all() and np.isin(T[:3, :3], (0.0, 1.0)).all()
            u64, v64, _ = G.project(c["K"], T, c["map_pts"], c["z_near"], c["z_far"], dtype=np.float64)
            u32, v32, _ = G.project(c["K"], T, c["map_pts"], c["z_near"], c["z_far"])
            ok = np.isfinite(u64)
            assert (u32[ok] == u64[ok]).all() and (v32[ok] == v64[ok]).all() and (u64[ok] * 8 == np.round(u64[ok] * 8)).all()
    assert G.compare(ref, ref) == []


def test_the_cases_cover_what_they_are_there_for():
    st = {n: Gc.reference(n) for n in Gc.CASES}
    S = G.STATUS
    assert st["empty_map"]["stats"]["n_entries"] == 0 and st["one_entry"]["stats"]["n_entries"] == 1
    assert Gc.case("zero_rows")["n_rows"][0] == 0 and Gc.case("n_max_1")["n_max"] == 1
    assert [len(a) for _, a in Gc.case("frames14")["frames"]] == Gc.ROW_COUNTS_14 and len(Gc.case("frames14")["map_app"]) == 3000
    assert all(st["frames14"]["stats"][k] > 0 for k in ("n_matched", "n_no_entry", "n_ambiguous", "n_displaced"))
    assert Gc.case("bound_above_size")["dup_rows"] > 0
    # one cell: every projection inside a box narrower than R
    c = Gc.case("one_cell")
    u, v, view = G.project(c["K"], c["poses"][0], c["map_pts"], 0, 10)
    assert view.all() and max(u.max() - u.min(), v.max() - v.min()) < 8.0 * 1.001 and st["one_cell"]["stats"]["n_gated"] > 40 * 1500
    # far outside: huge and infinite pixels among the entries in view, and rows that still find theirs
    c = Gc.case("far_outside")
    u, v, view = G.project(c["K"], c["poses"][0], c["map_pts"], 0, 10)
    assert (view & np.isinf(u)).sum() > 20 and (view & np.isfinite(u) & (np.abs(u) > 1e5)).sum() > 100 and st["far_outside"]["stats"]["n_matched"] > 100
    # the NaN pose: its frame is NO_ENTRY throughout, the neighbours are the frames they are alone
    c = Gc.case("nan_pose")
    assert np.isnan(c["poses"][1]).any() and (st["nan_pose"]["status"][1] == G.NO_ENTRY).all()
    for f in (0, 2):
        alone = Gc.run(c, frames=[c["frames"][f]], poses=[c["poses"][f]])
        assert alone["status"][0].tobytes() == st["nan_pose"]["status"][f].tobytes() and alone["stats"]["n_matched"] > 20
    s = st["special"]
    assert [S[k] for k in s["status"][0][:5]] == ["NAN_ROW", "NO_ENTRY", "NO_ENTRY", "NO_ENTRY", "NO_ENTRY"]
    assert S[s["status"][0][5]] == "MATCHED" and np.signbit(s["app"][0][5][[1, 4]]).all() and not np.signbit(Gc.case("special")["frames"][0][1][5]).any()
    assert S[s["status"][0][6]] == S[s["status"][0][7]] == "NO_ENTRY"      # the entry with a NaN, the point with a NaN
    # repeated appearance: appearance alone would call rows ambiguous that the gate decides, and the gate leaves some ambiguous
    c = Gc.case("classes")
    alone = N.run(c["map_app"], [a for _, a in c["frames"]], None, c["n_max"], c["radius"], c["ratio"], 0)
    both = (alone["status"] == N.AMBIGUOUS) & (st["classes"]["status"] == G.MATCHED)
    assert both.sum() > 200 and st["classes"]["stats"]["n_ambiguous"] > 10
    assert Gc.groups(Gc.case("two_groups")) >= 2 and len(Gc.case("two_groups")["map_app"]) == 300
    c = Gc.case("all_in_view")
    assert all(G.project(c["K"], T, c["map_pts"], 0, 10)[2].all() for T in c["poses"])
    d = st["dyadic"]
    assert [S[k] for k in d["status"][0][:12]] == ["NO_ENTRY", "MATCHED", "AMBIGUOUS", "MATCHED", "AMBIGUOUS", "MATCHED", "MATCHED", "NO_ENTRY",
                                                  "NO_ENTRY", "NO_ENTRY", "MATCHED", "NO_ENTRY"]
    assert d["pix2"][0][1] == np.float32(7.875 ** 2) and st["dyadic_plain"]["entry"][0][2] == 2      # the tie goes to the lower of 2 and 3
    assert d["dist2"][0][2] == np.float32(2.0 ** -8) and S[d["status"][0][17]] == "MATCHED"      # g14: the entry beyond the radius does not count
    u = st["dyadic_unique"]
    assert [S[k] for k in u["status"][0][12:17]] == ["DISPLACED", "DISPLACED", "MATCHED", "MATCHED", "DISPLACED"]
    assert u["entry"][0][14] == u["entry"][1][0] == 15 and u["entry"][0][15] == u["entry"][1][1] == 16      # the same entries in two frames
    assert [S[k] for k in d["status"][1][:4]] == ["MATCHED", "MATCHED", "NO_ENTRY", "MATCHED"]      # the gate's boundary under the translation


@pytest.mark.parametrize("fault", G.FAULTS)
def test_every_planted_fault_is_seen_by_the_gpu_tests_comparison(fault):
    """(frames14 is left out: its reference takes seconds, and nothing is planted that only it could show)"""
    seen = [n for n in Gc.CASES if n != "frames14" and G.compare(Gc.reference(n), Gc.reference(n, fault=fault))]
    print(fault, "seen on", seen)
    assert seen and set(seen) & set(Gc.DYADIC)
