"""CPU checks behind voe_map_keyframes*: the ABI of declarations that live in vo_hip.h itself -- by the voe_ rule -- on a machine
without a device, struct sizes, offsets and verdict names (header = Python = C++ = kernels), the refusals that need no device, the
conditions on the cases of the GPU test (each is what tests/map_keyframes_cases.py says, each planted fault changes some case), the
monotonicity the header claims, a replay that verifies every drop from the outputs alone, the experiment on the example data
(the restatement's counts, the two invariants at 1000 per mille, the refinement from the kept frames), and the host check of the
inline rules the kernels compile (tests/hostcheck/keyframes_check.cpp, built with sanitizers and run as a program)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import map_covis_cases as Cc
import map_covis_restatement as V
import map_keyframes_cases as Kc
import map_keyframes_restatement as K
import map_refine_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("voe_map_keyframes_dev", "voe_map_keyframes")
ALL_RUNS = [(n, k) for n in Kc.CASES for k in Kc.runs(n)]


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---- ABI ----
def test_the_voe_rule_holds_with_the_keyframes_calls_in_vo_hip_h(vo):
    lib = vo.load_library()
    hip = _read("include", "vo_hip.h")
    includes = re.findall(r'^#include "([a-z0-9_]+\.h)"', hip, flags=re.M)
    assert len(includes) == 8                                 # the extension headers stay eight
    declared = {}
    for h in ["vo_hip.h"] + includes:
        for n in re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _read("include", h), flags=re.S)):
            declared[n] = h
    assert all(declared[n] == "vo_hip.h" for n in NAMES)
    # behind the FUSE block, in front of the closing extern "C" and the extension headers
    assert (hip.index("int voe_map_fuse(") < hip.index("/* KEYFRAMES.") < hip.index("int voe_map_keyframes_dev(") < hip.index("int voe_map_keyframes(")
            < hip.rindex("#ifdef __cplusplus\n}") < hip.index('#include "vo_map_adjust.h"'))
    for n in declared:
        assert hasattr(lib, n), f"{n} is declared in include/{declared[n]} but not exported"
    assert lib.vo_abi_version() == 1
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M)) == set(declared)      # unversioned, and nothing else
        assert not re.search(r"map_keyframes_layout|map_keyframes_check|launch_map_keyframes", out)      # the helpers stay hidden
    assert "voe_" not in _read("visual-odometry_amd", "csrc", "vo_map_adjust.map")
    mk = _read("visual-odometry_amd", "csrc", "Makefile")
    assert "map_keyframes.hip" in mk and "keyframes_rules.h" in mk and "bin/keyframes_map" in _read("apps", "Makefile")
    # the covisibility's header and source are not touched: the call is declared and built next to them
    assert "keyframes" not in _read("include", "vo_map_covis.h") and "keyframes" not in _read("visual-odometry_amd", "csrc", "map_covis.hip")


def test_structs_verdicts_and_names_header_python_cpp(vo):
    P, S = vo.MapKeyframesParams, vo.MapKeyframesStats
    assert C.sizeof(P) == 32 and C.sizeof(S) == 32
    assert [(k, getattr(P, k).offset) for k, _ in P._fields_] == [("min_observers", 0), ("share_permille", 4), ("min_seen", 8), ("max_gap", 12),
                                                                  ("max_dropped", 16), ("reserved", 20)]
    assert [(k, getattr(S, k).offset) for k, _ in S._fields_] == [(k, 4 * i) for i, k in enumerate(K.STATS)]
    hdr = _read("include", "vo_hip.h")
    fields = re.search(r"typedef struct voe_map_keyframes_stats\s*\{(.*?)\} voe_map_keyframes_stats;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\b(n_[a-z_]+)\s*[,;]", fields)) == K.STATS
    fields = re.search(r"typedef struct voe_map_keyframes_params\s*\{(.*?)\} voe_map_keyframes_params;", hdr, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?:\[3\])?\s*[,;]", fields)) == tuple(k for k, _ in P._fields_)
    assert vo.MAP_KEYFRAMES_VERDICT == K.VERDICT and vo.MAP_KEYFRAMES_FLAG == ("FREE", "PROTECTED", "GONE")
    for names in (vo.MAP_KEYFRAMES_VERDICT, vo.MAP_KEYFRAMES_FLAG):      # a PROTECTED or GONE frame's verdict is its flag
        for k, name in enumerate(names):
            assert re.search(r"#define VOE_MAP_KEYFRAMES_%s\s+%d\b" % (name, k), hdr), name
    assert re.search(r"#define VOE_MAP_KEYFRAMES_MAX_STEPS\s+%d\b" % vo.MAP_KEYFRAMES_MAX_STEPS, hdr) and vo.MAP_KEYFRAMES_MAX_STEPS == K.MAX_STEPS
    assert "static_assert(sizeof(voe_map_keyframes_params) == 32 && sizeof(voe_map_keyframes_stats) == 32" in _read("visual-odometry_amd", "csrc", "capi_map.hip")
    loc = _read("include", "vo", "localise.hpp")
    names = re.search(r"keyframes_verdict_name\(int verdict\) \{\s*static const char\* names\[\] = \{([^}]*)\}", loc).group(1)
    assert tuple(re.findall(r'"([A-Z_]+)"', names)) == vo.MAP_KEYFRAMES_VERDICT
    assert " keyframes(" in loc and "struct MapKeyframes" in loc
    assert hasattr(vo.Map, "keyframes") and hasattr(vo.Map, "keyframes_dev")
    # the kernels: the header's numbers, integers alone, nothing that waits for another workgroup, one kind of atomic
    src = _read("visual-odometry_amd", "csrc", "map_keyframes.hip")
    rules = _read("visual-odometry_amd", "csrc", "keyframes_rules.h")
    enum = re.search(r"enum \{ (KV_LEFT.*?) \};", src).group(1)
    assert [(a[3:], int(b)) for a, b in re.findall(r"(KV_[A-Z_]+) = (\d)", enum)] == list(zip(K.VERDICT, range(7)))
    for text in (src, rules):
        assert not re.search(r"\b(float|double|half|__fp16)\b", re.sub(r"//.*", "", text))
        assert "cooperative" not in text.lower() and "grid.sync" not in text and "atomicCAS" not in text
    code = re.sub(r"//.*", "", src)
    assert code.count("atomicAdd(") == 1 and len(re.findall(r"\batomic\w+\(", code)) == 1 and "while" not in code
    assert "MONOTONE" in hdr and Kc.CHUNK == 256


def test_refusals_that_need_no_device(vo):
    """the argument checks come before the map is looked at: with a null map every one of them is reported as itself"""
    lib = vo.load_library()
    z, i = None, C.c_int
    buf = (C.c_int32 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd, off2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    err = lambda: lib.vo_last_error()

    def call(fn=lib.voe_map_keyframes_dev, F=3, W=1, bits=p, n_max=4, flags=z, prm=(3, 900, 1, 0, 8), reserved=(0, 0, 0), verdict=p, rows=p, keep=p,
             step=p, order=z, seen=p, red=p, stats=p):
        q = vo.MapKeyframesParams(*prm, (C.c_int32 * 3)(*reserved)) if prm is not None else None
        return fn(z, i(F), i(W), bits, z, i(n_max), flags, C.byref(q) if q is not None else None, verdict, rows, keep, step, order, seen, red, stats)
    rows = ((dict(F=0), b"n_frames"), (dict(F=4097), b"n_frames"), (dict(W=0), b"n_words"), (dict(W=(1 << 26) + 1), b"n_words"), (dict(bits=z), b"null"),
            (dict(stats=z), b"null"), (dict(stats=odd), b"8-byte"), (dict(verdict=z), b"null"), (dict(rows=z), b"null"), (dict(keep=z), b"null"),
            (dict(step=z), b"null"), (dict(seen=z), b"null"), (dict(red=z), b"null"), (dict(prm=None), b"null"), (dict(n_max=-1), b"negative"),
            (dict(prm=(0, 900, 1, 0, 8)), b"min_observers"), (dict(prm=(3, -1, 1, 0, 8)), b"share_permille"), (dict(prm=(3, 1001, 1, 0, 8)), b"share_permille"),
            (dict(prm=(3, 900, 0, 0, 8)), b"min_seen"), (dict(prm=(3, 900, 1, -1, 8)), b"max_gap"), (dict(prm=(3, 900, 1, 0, -1)), b"max_dropped"),
            (dict(prm=(3, 900, 1, 0, K.MAX_STEPS + 1)), b"max_dropped"), (dict(reserved=(0, 0, 1)), b"reserved"), (dict(reserved=(1, 0, 0)), b"reserved"),
            (dict(order=off2), b"4-byte"), (dict(seen=off2), b"4-byte"))
    for bad, word in rows:
        assert call(**bad) == -1 and word in err() and b"voe_map_keyframes_dev" in err(), bad
        if word not in (b"8-byte", b"4-byte"):               # (the host form takes its arrays at any address)
            assert call(fn=lib.voe_map_keyframes, **bad) == -1 and word in err() and b"voe_map_keyframes:" in err(), bad
    flags = (C.c_uint8 * 3)(0, 2, 3)
    assert call(fn=lib.voe_map_keyframes, flags=flags) == -1 and b"flag 3 of frame 2" in err()
    assert call(flags=flags) == -1 and b"null map" in err()   # (the device form cannot look: PROTECTED there)
    assert call() == -1 and b"null map" in err()
    assert call(prm=(1, 0, 1, 0, 0)) == -1 and b"null map" in err() and call(prm=(2 ** 31 - 1, 1000, 2 ** 31 - 1, 2 ** 31 - 1, K.MAX_STEPS), F=4096) == -1 and b"null map" in err()
    assert call(fn=lib.voe_map_keyframes, flags=(C.c_uint8 * 3)(0, 1, 2), order=p) == -1 and b"null map" in err()


# ---- conditions on the cases ----
def test_the_cases_are_what_they_say():
    ref = lambda n, k=0: Kc.reference(n, k)
    V_ = lambda r: [K.VERDICT[v] for v in r["verdict"]]
    assert Kc.WORD_COUNTS == (1, 255, 256, 257, 513) and Kc.FRAME_COUNTS == (1, 2, 63, 64, 65, 129)
    for W in Kc.WORD_COUNTS:
        c = Kc.case(f"words_{W}")
        B = V.unpack_bits(c["bits"])
        assert c["bits"].shape == (6, W) and B[:, 0].all() and B[:, -1].all() and (c["bits"] != 0).all()      # every word takes part
        assert ref(f"words_{W}")["stats"]["n_dropped"] >= 2 and ref(f"words_{W}", 1)["stats"]["n_dropped"] >= 1
        assert ref(f"words_{W}", 2)["stats"]["n_dropped"] == 0 and ref(f"words_{W}", 2)["stats"]["n_blocked"] >= 2
    c = Kc.case("padded_words")
    assert c["bits"].shape == (6, Kc.CHUNK + 5) and (c["bits"][:, 40:] == 0).all() and (c["bits"][:, :40] != 0).all() and ref("padded_words")["stats"]["n_dropped"] >= 2
    assert Kc.case("wide")["bits"].shape == (3, 2049) and ref("wide")["stats"]["n_dropped"] >= 1
    for F in Kc.FRAME_COUNTS:
        c = Kc.case(f"frames_{F}")
        assert len(c["bits"]) == F
        if F > 2:
            assert ref(f"frames_{F}")["stats"]["n_dropped"] > F // 2 and ref(f"frames_{F}", 1)["stats"]["n_blocked"] > 0 and ref(f"frames_{F}", 2)["stats"]["n_dropped"] == 3
            assert (ref(f"frames_{F}", 1)["verdict"] == K.GAP).any()
    # the carries: every count at every bit position; thresholds 2, 4, 8, 9 cross a power of two; the drops take counts through one
    c = Kc.case("carries")
    cnt = V.unpack_bits(c["bits"]).sum(0)
    assert len(c["bits"]) == 129 and [int(cnt[32 * i + b]) for i in range(10) for b in Kc.CARRY_BITS] == [n for n in Kc.CARRY_COUNTS for _ in Kc.CARRY_BITS]
    assert int((cnt > 0).sum()) == 30 and [r["min_observers"] for r in c["runs"]] == [1, 3, 7, 8, 3]
    for k in Kc.runs("carries"):
        r = ref("carries", k)
        assert r["stats"]["n_dropped"] >= 12
        left = V.unpack_bits(c["bits"])[r["keep"] == 1].sum(0)
        assert left[32 * 8 + 13] < 128 <= cnt[32 * 8 + 13] and left[32 * 7] < 127      # a borrow through seven planes, and on
    # all frames identical: frames 0 .. F - k - 1 go in index order, exactly k are left; the budget
    r = ref("identical")
    assert r["order"][:6].tolist() == [0, 1, 2, 3, 4, 5] and (r["order"][6:] == -1).all() and V_(r)[6:] == ["NEEDED"] * 3 and r["stats"]["n_kept"] == 3
    assert r["red"][:6].tolist() == [40] * 6 and r["red"][6:].tolist() == [0] * 3 and (r["seen"] == 40).all()
    r0, r1, r6 = ref("identical", 1), ref("identical", 2), ref("identical", 3)
    assert V_(r0) == ["LEFT"] * 9 and r0["stats"]["n_blocked"] == 9 and (r0["step"] == -1).all() and (r0["red"] == 40).all()
    assert V_(r1) == ["DROPPED"] + ["LEFT"] * 8 and K.compare(r6, r) == []      # a budget of exactly the possible drops
    # equal shares in other terms go to the lower frame; 9/10 passes 900 per mille and 899/1000 does not
    r = ref("share")
    assert (r["seen"][:3].tolist(), r["red"][:3].tolist()) == ([20, 10, 1000], [18, 9, 899]) and r["order"][:3].tolist() == [0, 1, -1]
    assert V_(r) == ["DROPPED", "DROPPED", "NEEDED", "PROTECTED"] and ref("share", 1)["order"][:2].tolist() == [0, -1] and V_(ref("share", 2))[2] == "DROPPED"
    r = ref("close_shares")
    assert np.float32(11999) / np.float32(12000) == np.float32(12000) / np.float32(12001) and r["order"][0] == 1 and r["red"][1] == 12000
    # the greedy step matters
    r = ref("greedy")
    assert V_(ref("greedy", 1)) == ["LEFT", "LEFT", "NEEDED"] and V_(r) == ["DROPPED", "NEEDED", "NEEDED"] and r["red"].tolist() == [12, 0, 0]
    # the gap rule: runs that touch frame 0 and the last frame, a GONE frame inside a run
    r1, r2 = ref("gap_chain", 0), ref("gap_chain", 1)
    assert V_(r1) == ["DROPPED", "GAP"] * 5 and r1["order"][:5].tolist() == [0, 2, 4, 6, 8]
    assert V_(r2) == ["DROPPED", "DROPPED", "GAP", "DROPPED", "DROPPED", "GAP", "DROPPED", "DROPPED", "GAP", "DROPPED"]      # the last run touches the end
    g1, g2 = ref("gap_gone", 0), ref("gap_gone", 1)
    assert V_(g1) == ["DROPPED", "GAP", "DROPPED", "GAP", "GONE", "GAP", "DROPPED", "GAP", "DROPPED", "PROTECTED", "GAP", "GONE"]
    assert V_(g2)[3:6] == ["DROPPED", "GONE", "GAP"] and V_(g2)[10] == "DROPPED"      # 4 is missing already: 3 goes, then 5 may not; 10 and the GONE 11 are a run of 2 at the end
    assert ref("gap_gone", 2)["stats"]["n_dropped"] == 3 and (ref("gap_gone", 2)["verdict"] == K.LEFT).any() and (ref("gap_gone", 2)["verdict"] == K.GAP).any()
    # flags
    r = ref("protected")
    assert V_(r)[:3] == ["PROTECTED", "DROPPED", "PROTECTED"] and r["order"][:6].tolist() == [1, 3, 4, 5, 6, 7] and V_(r)[8] == "NEEDED"
    r = ref("gone")
    assert V_(r) == ["NEEDED", "GONE", "NEEDED", "GONE", "NEEDED"] and ref("gone_none")["stats"]["n_dropped"] == 2      # their rows would have counted
    assert r["seen"].tolist() == [40, 0, 40, 0, 40] and r["n_rows"].tolist() == [3, 0, 5, 0, 7] and r["keep"].tolist() == [1, 0, 1, 0, 1]
    assert all(Kc.case(n)["flags"] is None for n in ("identical", "greedy", "carries"))
    c = Kc.case("no_row_counts")
    assert c["n_rows"] is None and c["n_max"] == 17 and ref("no_row_counts")["n_rows"].tolist() == [0] * 6 + [17] * 3
    # EMPTY
    assert V_(ref("empty"))[1] == "EMPTY" and V_(ref("empty"))[3] == "DROPPED" and V_(ref("empty", 1))[3] == "EMPTY" and ref("empty")["seen"][[1, 3]].tolist() == [0, 2]
    assert Kc.case("example")["bits"].shape == (121, 32) and Kc.case("example")["flags"][[0, 120]].tolist() == [1, 1]
    assert {len(Kc.case(n)["runs"]) for n in Kc.CASES} >= {1, 2, 3} and any(r["max_dropped"] == 0 for n in Kc.CASES for r in Kc.case(n)["runs"])


@pytest.mark.parametrize("fault", K.FAULTS)
def test_every_planted_fault_changes_some_case(fault):
    seen = [(n, k) for n, k in ALL_RUNS if K.compare(Kc.reference(n, k), Kc.reference(n, k, fault=fault))]
    print(fault, "seen on", seen)
    assert seen
    assert {"tie_to_highest": ("identical", 0), "float_share": ("close_shares", 0), "counts_not_updated": ("greedy", 0)}[fault] in seen


@pytest.mark.parametrize("name", list(Kc.CASES))
def test_monotone_and_every_drop_obeys_the_rules(name):
    """rule 6 on the restatement's own history -- the set of candidates only shrinks --, and the replay checker, which knows the
    outputs alone, accepts the reference and rejects every planted fault that changed it"""
    c = Kc.case(name)
    for k in Kc.runs(name):
        r, p = Kc.reference(name, k), c["runs"][k]
        assert K.monotone(r), (name, k)
        assert len(r["candidates"]) == min(r["stats"]["n_dropped"] + 1, p["max_dropped"])      # one list per step that looked
        assert K.replay(c["bits"], r, c["flags"], **p) == [], (name, k)
        assert K.compare(r, r) == [] and sum(r["stats"][s] for s in ("n_kept", "n_dropped", "n_gone")) == len(c["bits"])
        assert r["stats"]["n_kept"] == sum(r["stats"][s] for s in ("n_protected", "n_needed", "n_blocked", "n_empty"))
        for fault in K.FAULTS:
            bad = Kc.reference(name, k, fault=fault)
            if K.compare(bad, r):
                assert K.replay(c["bits"], bad, c["flags"], **p) != [], (name, k, fault)


# ---- the experiment on the example data ----
def test_example_data_counts_and_invariants_at_1000_per_mille():
    c, ex = Kc.case("example"), Cc.case("example")
    B = V.unpack_bits(c["bits"])
    assert np.array_equal(B[:, :1000], Cc.reference("example")["sees"])
    r = Kc.reference("example", 0)
    kept = r["keep"] == 1
    print("min_observers 3, 1000 per mille, frames 0 and 120 protected:", r["stats"], "observations", int(B.sum()), "->", int(B[kept].sum()))
    assert (r["stats"]["n_dropped"], r["stats"]["n_kept"], int(B.sum()), int(B[kept].sum())) == (74, 47, 10012, 4489)
    assert [Kc.reference("example", k)["stats"]["n_kept"] for k in (1, 2, 3)] == [27, 43, 57]
    assert kept[0] and kept[120] and r["stats"]["n_protected"] == 2 and r["stats"]["n_blocked"] == 0
    # every entry seen by more than k frames before is seen by at least k kept frames after
    before, after = B.sum(0), B[kept].sum(0)
    assert (after[before > 3] >= 3).all() and (after[before <= 3] == before[before <= 3]).all()
    # refine's set of OK landmarks with min_obs 3 is the one it has over all frames, and the kept frames serve them as well
    pushed = R.perturbed(ex["map_pts"], 1, 0.1)
    a = R.refine(ex["K"], pushed, ex["map_app"], ex["frames"], ex["poses"], n_rounds=5, min_obs=3)
    b = R.refine(ex["K"], pushed, ex["map_app"], ex["frames"], ex["poses"], n_rounds=5, min_obs=3, n_rows=r["n_rows"])
    ok = a["status"] == R.OK
    assert int(ok.sum()) == 462 and np.array_equal(b["status"] == R.OK, ok) and b["stats"]["n_obs"] == 4489 and a["stats"]["n_obs"] == 10012
    world = np.asarray(ex["map_pts"], np.float64)
    ea = np.linalg.norm(a["points"][ok] - world[ok], axis=1)
    eb = np.linalg.norm(b["points"][ok] - world[ok], axis=1)
    print(f"error to world.dat: median {np.median(ea):.3g} (all frames) {np.median(eb):.3g} (kept); max {ea.max():.3g} / {eb.max():.3g}")
    assert np.median(eb) < 2 * np.median(ea)                  # (a landmark left with 3 of its ~20 observations is legitimately noisier)


# ---- the rules the kernels compile ----
def test_host_check_of_the_inline_rules(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/hostcheck/keyframes_check.cpp"
    exe = str(tmp_path / "keyframes_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "visual-odometry_amd", "csrc"), os.path.join(ROOT, "tests", "hostcheck", "keyframes_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "keyframes_check: ok" in r.stdout
