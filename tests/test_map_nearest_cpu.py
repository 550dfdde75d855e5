"""CPU checks behind voe_map_nearest*: the ABI of declarations that live in vo_hip.h itself -- by the voe_ rule -- on a machine
without a device, struct sizes and status names (header = Python = C++), the host refusals under the host sanitizers, the example
experiment on the brute-force restatement (tests/map_nearest_restatement.py), the hygiene of the GPU test's cases (no decision
differs between the float32 rule and a float64 evaluation; the dyadic ties and boundaries are exact in both), and planted faults
against the comparison the GPU test uses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_nearest_cases as Nc
import map_nearest_restatement as N
import map_refine_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---- ABI ----
def test_the_voe_rule_holds_with_declarations_in_vo_hip_h(vo):
    lib = vo.load_library()
    hip = _read("include", "vo_hip.h")
    includes = re.findall(r'^#include "([a-z0-9_]+\.h)"', hip, flags=re.M)
    assert len(includes) == 8                                 # no ninth extension header
    declared = {}
    for h in ["vo_hip.h"] + includes:
        for n in re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _read("include", h), flags=re.S)):
            declared[n] = h
    assert declared["voe_map_nearest_batch_dev"] == declared["voe_map_nearest_dev"] == declared["voe_map_nearest"] == "vo_hip.h"
    # directly behind vo_map_lookup*, in front of the localisation; the comment says why the names may live here
    assert hip.index("int vo_map_lookup(") < hip.index("/* NEAREST.") < hip.index("int voe_map_nearest_batch_dev(") < hip.index("/* LOCALISATION.")
    assert "vo_hip.h is a declaring header of the voe_" in hip
    for n in declared:
        assert hasattr(lib, n), f"{n} is declared in include/{declared[n]} but not exported"
    assert lib.vo_abi_version() == 1
    import shutil
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M)) == set(declared)      # unversioned, and nothing else
        assert not re.search(r"map_nearest_layout|map_nearest_check|launch_map_nearest", out)            # the shared helpers stay hidden
    assert "voe_" not in _read("visual-odometry_amd", "csrc", "vo_map_adjust.map")
    assert "map_nearest.hip" in _read("visual-odometry_amd", "csrc", "Makefile") and "bin/associate_map" in _read("apps", "Makefile")
    # the map is never written: no kernel of map_nearest.hip stores through the map's arrays, which it holds as pointers to const
    src = re.sub(r"//.*", "", _read("visual-odometry_amd", "csrc", "map_nearest.hip"))
    assert "const float* app; const int* hdr;" in _read("visual-odometry_amd", "csrc", "vo_internal.h") and "const_cast" not in src
    assert "atomicMin" in src and not re.search(r"atomic\w*\(\s*\(?\s*float", src)      # integer atomics only


def test_structs_statuses_and_names_header_python_cpp(vo):
    assert C.sizeof(vo.MapNearestParams) == 16 and C.sizeof(vo.MapNearestStats) == 32
    assert [(k, getattr(vo.MapNearestParams, k).offset) for k, _ in vo.MapNearestParams._fields_] == [("radius", 0), ("ratio", 4), ("unique", 8), ("reserved", 12)]
    hdr = _read("include", "vo_hip.h")
    fields = re.search(r"typedef struct voe_map_nearest_stats\s*\{(.*?)\} voe_map_nearest_stats;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\b(n_[a-z_]+)\s*[,;]", fields)) == tuple(k for k, _ in vo.MapNearestStats._fields_)
    fields = re.search(r"typedef struct voe_map_nearest_params\s*\{(.*?)\} voe_map_nearest_params;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)\s*;", fields)) == tuple(k for k, _ in vo.MapNearestParams._fields_)
    assert vo.MAP_NEAREST_STATUS == N.STATUS
    for k, name in enumerate(vo.MAP_NEAREST_STATUS):
        assert re.search(r"#define VOE_MAP_NEAREST_%s\s+%d\b" % (name, k), hdr), name
    for text in (_read("visual-odometry_amd", "csrc", "capi_map.hip"), _read("tests", "hostcheck", "map_nearest_checks_check.cpp")):
        assert "static_assert(sizeof(voe_map_nearest_params) == 16 && sizeof(voe_map_nearest_stats) == 32" in text
    loc = _read("include", "vo", "localise.hpp")
    names = re.search(r"nearest_status_name\(int status\) \{\s*static const char\* names\[\] = \{([^}]*)\}", loc).group(1)
    assert tuple(re.findall(r'"([A-Z_]+)"', names)) == vo.MAP_NEAREST_STATUS
    assert " nearest(const std::vector<Vector10fVector>& appearances" in loc and "struct NearestOptions" in loc
    assert hasattr(vo.Map, "nearest") and hasattr(vo.Map, "nearest_batch_dev")
    # the kernels' status numbers are the header's
    enum = re.search(r"enum \{ (NS_MATCHED.*?) \};", _read("visual-odometry_amd", "csrc", "map_nearest.hip")).group(1)
    assert [(a[3:], int(b)) for a, b in re.findall(r"(NS_[A-Z_]+) = (\d)", enum)] == list(zip(N.STATUS, range(6)))


def test_map_nearest_refusals_under_the_host_sanitizers(tmp_path):
    """visual-odometry_amd/csrc/map_checks.h: map_nearest_check in a stand-alone program under AddressSanitizer and UBSan, each row
    against the code and the whole message"""
    exe = str(tmp_path / "map_nearest_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "visual-odometry_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostcheck", "map_nearest_checks_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("map_nearest_checks_check: all ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("-> ok") >= 55 and "FAILED" not in r.stdout


# ---- the example experiment on the restatement ----
@pytest.fixture(scope="module")
def example():
    E = R.example_problem()
    rng = np.random.default_rng(1)
    pushed = [(a + rng.normal(0, 0.005, a.shape)).astype(np.float32) for _, a in E["frames"]]
    return E, pushed


def test_example_world_rows_lie_far_apart():
    W = R.example_problem()["world_app"]
    d = np.sqrt(N.dist2(W, W, np.float64))
    np.fill_diagonal(d, np.inf)
    nearest = d.min(axis=1)
    print(f"{len(W)} rows, nearest neighbour: least {nearest.min():.4f}, median {np.median(nearest):.4f}")
    assert len(W) == 1000 and nearest.min() > 0.47 and np.median(nearest) > 1.0


def test_example_pushed_rows_all_match_their_file_id(example):
    """sigma 0.005, radius 0.1, ratio 0.8, default_rng(1): all 10 012 rows of the 121 frames are MATCHED to their file id, no
    second candidate lies within the radius, the canonical rows equal the clean rows byte for byte -- and bit equality, the only
    association the map calls had, hits nothing"""
    E, pushed = example
    W = E["world_app"]
    n_max = max(len(a) for a in pushed)
    r = N.run(W, pushed, None, n_max, 0.1, 0.8, 1)
    rows = sum(len(a) for a in pushed)
    assert len(pushed) == 121 and rows == 10012
    assert r["stats"]["n_matched"] == rows and r["stats"]["n_live"] == rows
    for f, (_, a) in enumerate(E["frames"]):
        assert r["entry"][f, : len(a)].tolist() == E["ids"][f].astype(int).tolist()
        assert r["app"][f].tobytes() == np.asarray(a, np.float32).tobytes()
        _, _, has2, _ = N.best_two(pushed[f], W, np.float32(0.1) * np.float32(0.1))
        assert not has2.any()
    assert (N.lookup(W, pushed[:8], None, n_max) == -1).all()      # bit equality of the same rows: nothing


def test_example_sequential_dictionary_has_one_class_per_landmark(example):
    """--tracks of apps/associate_map: the dictionary filled frame by frame ends with 536 classes for 536 distinct ids, none
    split; the largest accepted distance leaves more than a factor 2 to the radius"""
    E, pushed = example
    dic = np.zeros((0, 10), np.float32)
    owner = []                                                # the file id behind every class
    largest = 0.0
    for f, a in enumerate(pushed):
        r = N.run(dic, [a], None, len(a), 0.1, 0.8, 0)
        ids = E["ids"][f].astype(int)
        st, ent = r["status"][0], r["entry"][0]
        assert set(st.tolist()) <= {N.MATCHED, N.NO_ENTRY}
        for i in np.nonzero(st == N.MATCHED)[0]:
            assert owner[ent[i]] == ids[i]                    # never merged into another landmark's class
        if (st == N.MATCHED).any():
            largest = max(largest, float(np.sqrt(r["dist2"][0][st == N.MATCHED].max())))
        new = np.nonzero(st == N.NO_ENTRY)[0]                 # what map.update appends: the rows no entry equals, in order
        assert len(np.unique(a[new], axis=0)) == len(new)
        dic = np.concatenate([dic, a[new]])
        owner += ids[new].tolist()
    n_ids = len(np.unique(np.concatenate([i for i in E["ids"]])))
    print(f"{len(dic)} classes for {n_ids} ids, largest accepted distance {largest:.4f}")
    assert len(dic) == n_ids == 536 and len(set(owner)) == 536
    assert largest < 0.05


# ---- the cases of the GPU test ----
@pytest.mark.parametrize("name", list(Nc.CASES))
def test_case_takes_no_marginal_decision(name):
    """`< r2`, best, tie, ratio and unique decide alike in the float32 rule and in float64; in the DYADIC cases because both are
    exact there (the ties and boundaries are deliberate), in every other case because no decision is close"""
    c, ref = Nc.case(name), Nc.reference(name)
    assert N.margins(c["map_app"], c["frames"], c["n_rows"], c["n_max"], c["radius"], c["ratio"], c["unique"]) == []
    assert c["dyadic"] == (name in Nc.DYADIC)
    if c["dyadic"]:                                           # every coordinate a multiple of 2^-13 below 64: 20 bits, squares exact
        for a in [c["map_app"]] + c["frames"]:
            assert (a * 8192 == np.round(a * 8192)).all() and np.abs(a).max() < 64
    assert N.compare(ref, ref) == []


def test_the_cases_cover_what_they_are_there_for():
    st = {n: Nc.reference(n) for n in Nc.CASES}
    S = N.STATUS
    assert st["empty_map"]["stats"]["n_entries"] == 0 and st["one_entry"]["stats"]["n_entries"] == 1
    assert Nc.case("zero_rows")["n_rows"][0] == 0 and Nc.case("n_max_1")["n_max"] == 1
    assert [len(a) for a in Nc.case("frames14")["frames"]] == Nc.ROW_COUNTS_14 and len(Nc.case("frames14")["map_app"]) == 3000
    assert all(st["frames14"]["stats"][k] > 0 for k in ("n_matched", "n_no_entry", "n_ambiguous", "n_displaced"))
    assert Nc.case("bound_above_size")["dup_rows"] > 0
    E = Nc.case("one_cell")["map_app"]
    assert (E.max(axis=0) - E.min(axis=0)).max() < 0.1 * 1.001 and len(E) == 3000      # every spread below R: one cell
    E = Nc.case("flat_grid")["map_app"]
    assert ((E.max(axis=0) - E.min(axis=0)) > 0).sum() == 2 and st["flat_grid"]["stats"]["n_no_entry"] > 0
    c = Nc.case("outside_bounds")
    even, odd = c["map_app"][0::2], c["map_app"][1::2]
    assert len(c["map_app"]) > 2 * 2048 and (np.abs(odd).max(axis=1) > np.abs(even).max()).all()
    hit = st["outside_bounds"]["entry"][0]
    assert (hit[hit >= 0] % 2 == 1).sum() > 50                # rows matched to entries outside the sampled bounds
    d = st["dyadic"]
    assert [S[s] for s in d["status"][0][:6]] == ["NO_ENTRY", "MATCHED", "AMBIGUOUS", "AMBIGUOUS", "AMBIGUOUS", "MATCHED"]
    assert d["dist2"][0][2] == np.float32(2.0 ** -8) and st["dyadic_plain"]["entry"][0][2] == 2      # the tie goes to the lower of 2 and 3
    assert [S[s] for s in d["status"][1][2:6]] == ["NO_ENTRY"] * 4 and [S[s] for s in d["status"][1][6:10]] == ["MATCHED"] * 4      # the lattice
    u = st["dyadic_unique"]
    assert [S[s] for s in u["status"][0][6:11]] == ["DISPLACED", "DISPLACED", "MATCHED", "MATCHED", "DISPLACED"]
    assert u["entry"][0][8] == u["entry"][1][0] == 10 and u["entry"][0][9] == u["entry"][1][1] == 11      # the same entries in two frames
    s = st["special"]
    assert s["stats"]["n_nan"] == 2 and S[s["status"][0][3]] == S[s["status"][0][4]] == S[s["status"][0][8]] == "NO_ENTRY"
    assert s["entry"][0][5] == 6 and S[s["status"][0][6]] == "DISPLACED"      # +0 row and -0 row on the entry of mixed zeros
    assert np.signbit(s["app"][0][5][[1, 4]]).all() and not np.signbit(Nc.case("special")["frames"][0][5]).any()      # ... whose bytes it takes


@pytest.mark.parametrize("fault", N.FAULTS)
def test_every_planted_fault_is_seen_by_the_gpu_tests_comparison(fault):
    seen = [n for n in Nc.CASES if N.compare(Nc.reference(n), Nc.reference(n, fault=fault))]
    print(fault, "seen on", seen)
    assert seen and set(seen) & set(Nc.DYADIC)
