"""CPU checks behind voe_map_prune*: the ABI of declarations that live in vo_hip.h itself -- by the voe_ rule -- on a machine
without a device, struct sizes and status names (header = Python = C++ = kernels), the refusals that need no device, the
conditions on the cases of the GPU test (no marginal decision but the planted exact ties; each is what tests/map_prune_cases.py
says; the contract of rule 11 through the NumPy lookup; idempotence with the guards off; every planted fault changes some case),
the outcome on the example data at the committed seeds, and the host check of the inline rules the kernels compile
(tests/hostcheck/prune_rules_check.cpp, built with sanitizers and run as a program).

WHAT FAILS WITHOUT THE FEATURE.  The ABI, struct, refusal and host-check tests (and every test of tests/test_gpu_map_prune.py) need
the library's new symbols, headers and prune_rules.h and fail on a tree without them.  The tests on the cases -- no marginal
decision, the contract, idempotence, the planted faults, the example outcome -- exercise the NumPy restatement and the cases
alone: they hold the REFERENCE to its own properties, which is what lets the GPU test compare exactly, and they pass wherever
these two modules exist.

THE EXAMPLE DATA (tests/map_prune_cases.py: example_case; 121 frames, 10 012 clean observations whose largest error is 0.024 px):
20 of the 422 landmarks with >= 5 observations pushed by +-0.2 .. 0.4 (seed 2; each at least 1 in front of its cameras), frames 30,
60 and 90 pushed by 0.05 in t, 100 rows of such landmarks outside those frames re-pointed to another such landmark that is not
pushed (seed 1); max_err_px 1, rel_factor 5 over a floor of 0.5 px from 5 observations on, unique, guards at 500 and 300 per
mille.  ONE call: 100 rows pruned -- 39 BEHIND, 31 DUPLICATE, 30 HIGH_ERROR --, exactly the planted ones; 20 landmarks named,
exactly the pushed ones, their 435 soft rows kept; 3 frames named, exactly the pushed ones, their 222 soft rows kept.  A
voe_map_cull at max_err_px = 1 on the same window would drop 232 landmarks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import map_cull_restatement as Cu
import map_prune_cases as Pc
import map_prune_restatement as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("voe_map_prune_batch_dev", "voe_map_prune_dev", "voe_map_prune")
FAULT_CASES = [n for n in Pc.SMALL]


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---- ABI ----
def test_the_voe_rule_holds_with_the_prune_calls_in_vo_hip_h(vo):
    lib = vo.load_library()
    hip = _read("include", "vo_hip.h")
    includes = re.findall(r'^#include "([a-z0-9_]+\.h)"', hip, flags=re.M)
    assert len(includes) == 8                                 # the extension headers stay eight
    declared = {}
    for h in ["vo_hip.h"] + includes:
        for n in re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _read("include", h), flags=re.S)):
            declared[n] = h
    assert all(declared[n] == "vo_hip.h" for n in NAMES)
    # behind the KEYFRAMES block, in front of the closing extern "C" and the extension headers
    assert (hip.index("int voe_map_keyframes(") < hip.index("/* PRUNE.") < hip.index("int voe_map_prune_batch_dev(") < hip.index("int voe_map_prune_dev(")
            < hip.index("int voe_map_prune(") < hip.rindex("#ifdef __cplusplus\n}") < hip.index('#include "vo_map_adjust.h"'))
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is declared in include/vo_hip.h but not exported"
    assert lib.vo_abi_version() == 1
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(NAMES) <= set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M))      # unversioned
        assert not re.search(r"map_prune_layout|map_prune_blocks|map_prune_check|launch_map_prune", out)      # the helpers stay hidden
    mk = _read("visual-odometry_amd", "csrc", "Makefile")
    assert "map_prune.hip" in mk and "prune_rules.h" in mk and "bin/prune_map" in _read("apps", "Makefile")
    # the cull's header and sources are not touched: the call shares its device function through map_score.h
    assert "prune" not in _read("include", "vo_map_cull.h") and "prune" not in _read("visual-odometry_amd", "csrc", "map_cull.hip")
    assert "prune" not in _read("visual-odometry_amd", "csrc", "map_score.h") and "score_obs(" in _read("visual-odometry_amd", "csrc", "map_prune.hip")


def test_structs_statuses_and_names_header_python_cpp(vo):
    P, S = vo.MapPruneParams, vo.MapPruneStats
    assert C.sizeof(P) == 32 and C.sizeof(S) == 64
    assert [(k, getattr(P, k).offset) for k, _ in P._fields_] == [("max_err_px", 0), ("rel_factor", 4), ("rel_floor_px", 8), ("rel_min_obs", 12),
                                                                  ("unique", 16), ("max_share_landmark", 20), ("max_share_frame", 24), ("reserved", 28)]
    assert [(k, getattr(S, k).offset) for k, _ in S._fields_] == [("n_frames", 0), ("n_entries", 4), ("by_status", 8), ("n_landmarks_at_fault", 48),
                                                                  ("n_frames_at_fault", 52), ("n_obs", 56), ("n_pruned", 60)]
    assert vo.MAP_PRUNE_LANDMARK_DTYPE.names == ("n_obs", "n_el", "n_soft", "n_pruned", "at_fault", "reserved", "med_sq")
    assert vo.MAP_PRUNE_LANDMARK_DTYPE.fields["med_sq"][1] == 24 and vo.MAP_PRUNE_FRAME_DTYPE.names == ("n_obs", "n_el", "n_soft", "at_fault")
    hdr = _read("include", "vo_hip.h")
    for name, fields in (("params", [k for k, _ in P._fields_]), ("landmark", vo.MAP_PRUNE_LANDMARK_DTYPE.names), ("frame", vo.MAP_PRUNE_FRAME_DTYPE.names),
                         ("stats", [k for k, _ in S._fields_])):
        text = re.search(r"typedef struct voe_map_prune_%s\s*\{(.*?)\} voe_map_prune_%s;" % (name, name), hdr, flags=re.S).group(1)
        assert re.findall(r"\b([a-z_]+)(?:\[10\])?\s*[,;]", text) == list(fields), name
    assert vo.MAP_PRUNE_STATUS == Q.STATUS
    for k, name in enumerate(Q.STATUS):
        assert re.search(r"#define VOE_MAP_PRUNE_%s\s+%d\b" % (name, k), hdr), name
    assert "sizeof(voe_map_prune_params) == 32 && sizeof(voe_map_prune_landmark) == 32 && sizeof(voe_map_prune_frame) == 16" in _read("visual-odometry_amd", "csrc", "capi_map.hip")
    rules = _read("visual-odometry_amd", "csrc", "prune_rules.h")
    enum = re.search(r"enum \{\s*(PS_KEPT.*?)\};", rules, flags=re.S).group(1)
    assert [(a[3:], int(b)) for a, b in re.findall(r"(PS_[A-Z_]+) = (\d+)", enum)][:10] == list(zip(Q.STATUS, range(10)))
    loc = _read("include", "vo", "localise.hpp")
    names = re.search(r"prune_status_name\(int status\) \{\s*static const char\* names\[\] = \{([^}]*)\}", loc).group(1)
    assert tuple(re.findall(r'"([A-Z_]+)"', names)) == vo.MAP_PRUNE_STATUS
    assert " prune(" in loc and "struct PruneOptions" in loc
    assert hasattr(vo.Map, "prune") and hasattr(vo.Map, "prune_batch_dev") and hasattr(vo.Map, "prune_dev")
    # the kernels: no float atomic, nothing that waits for another workgroup, and the map is only read
    code = re.sub(r"//.*", "", _read("visual-odometry_amd", "csrc", "map_prune.hip"))
    assert "cooperative" not in code.lower() and "grid.sync" not in code and "atomicCAS" not in code and "while" not in code
    assert not re.search(r"a\.v\.pts\[[^\]]*\]\s*=[^=]", code) and not re.search(r"a\.v\.hdr\[[^\]]*\]\s*=[^=]", code)
    for call in re.findall(r"\batomic\w+\(([^;]*);", code):
        assert re.match(r"\s*(&s_f|&s_t|&s_fault|a\.stats|&static_cast<PruneLandmark\*>)", call), call      # LDS tallies, the statistics, n_pruned: integers


def test_refusals_that_need_no_device(vo):
    """the argument checks of the device form come before the map is looked at: with a null map every one of them is reported as
    itself, and what is NOT refused reaches the map"""
    lib = vo.load_library()
    z, i = None, C.c_int
    buf = (C.c_double * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd, off2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    inside = C.c_void_p(p.value + 80)
    K = (C.c_float * 9)(500, 0, 0, 0, 500, 0, 320, 240, 1)
    K0 = (C.c_float * 9)()
    err = lambda: lib.vo_last_error()
    good = (1.0, 0.0, 0.0, 3, 1, 1000, 1000, 0)

    def call(F=2, K=K, uv=p, uvs=8, app=p, apps=8, n_max=4, T=p, prm=good, entry=p, status=z, sq=z, app_out=z, lm=z, fr=z, stats=p):
        q = vo.MapPruneParams(*prm) if prm is not None else None
        return lib.voe_map_prune_batch_dev(z, i(F), K, uv, C.c_size_t(uvs), app, C.c_size_t(apps), i(n_max), z, T, C.byref(q) if q is not None else None,
                                           entry, status, sq, app_out, lm, fr, stats)
    prm = lambda **kw: tuple(kw.get(k, v) for k, v in zip(("max_err_px", "rel_factor", "rel_floor_px", "rel_min_obs", "unique", "max_share_landmark",
                                                           "max_share_frame", "reserved"), good))
    rows = ((dict(F=0), b"n_frames"), (dict(F=65536), b"n_frames"), (dict(n_max=-1), b"negative"), (dict(uv=z), b"null"), (dict(app=z), b"null"),
            (dict(uv=odd), b"8-byte"), (dict(app=odd), b"8-byte"), (dict(stats=odd), b"8-byte"), (dict(uvs=3), b"stride"), (dict(apps=3), b"stride"),
            (dict(K=K0), b"singular"), (dict(K=z), b"null"), (dict(T=z), b"null"), (dict(stats=z), b"null"),
            (dict(prm=None), b"null params"), (dict(entry=z), b"null params or d_entry_out"),
            (dict(prm=prm(max_err_px=-1.0)), b"max_err_px"), (dict(prm=prm(max_err_px=float("inf"))), b"max_err_px"), (dict(prm=prm(max_err_px=float("nan"))), b"max_err_px"),
            (dict(prm=prm(rel_factor=-0.5)), b"rel_factor"), (dict(prm=prm(rel_factor=float("nan"))), b"rel_factor"),
            (dict(prm=prm(rel_floor_px=-1.0)), b"rel_floor_px"), (dict(prm=prm(rel_floor_px=float("inf"))), b"rel_floor_px"),
            (dict(prm=prm(rel_min_obs=2)), b"rel_min_obs"), (dict(prm=prm(max_share_landmark=-1)), b"max_share_landmark"),
            (dict(prm=prm(max_share_landmark=1001)), b"max_share_landmark"), (dict(prm=prm(max_share_frame=-1)), b"max_share_frame"),
            (dict(prm=prm(max_share_frame=1001)), b"max_share_frame"), (dict(prm=prm(unique=2)), b"unique"), (dict(prm=prm(unique=-1)), b"unique"),
            (dict(prm=prm(reserved=1)), b"reserved"), (dict(entry=off2), b"4-byte"), (dict(status=off2), b"4-byte"), (dict(sq=odd), b"8-byte"),
            (dict(app_out=odd), b"8-byte"), (dict(lm=odd), b"8-byte"), (dict(fr=odd), b"8-byte"), (dict(app_out=inside), b"overlaps"))
    for bad, word in rows:
        assert call(**bad) == -1 and word in err() and b"voe_map_prune_batch_dev" in err(), (bad, err())
    # not refused: everything off, the rows in place, a guard at 0
    assert call() == -1 and b"null map" in err()
    assert call(prm=prm(max_err_px=0.0, unique=0)) == -1 and b"null map" in err()
    assert call(app_out=p) == -1 and b"null map" in err()
    assert call(prm=prm(max_share_landmark=0, max_share_frame=0, rel_factor=2.0, rel_min_obs=2 ** 31 - 1)) == -1 and b"null map" in err()
    # the host form names itself
    q = vo.MapPruneParams(*good)
    assert lib.voe_map_prune(z, i(1), K, p, p, z, i(4), p, z, p, z, z, z, z, z, z) == -1 and b"voe_map_prune:" in err()
    assert lib.voe_map_prune(z, i(1), K, p, p, z, i(4), p, C.byref(q), z, z, z, z, z, z, z) == -1 and b"voe_map_prune:" in err()
    assert lib.voe_map_prune(z, i(1), K, p, p, z, i(4), p, C.byref(q), p, z, z, z, z, z, z) == -1 and b"null map" in err()


# ---- conditions on the cases ----
@pytest.mark.parametrize("name", list(Pc.CASES))
def test_no_case_takes_a_marginal_decision_and_the_contract_holds(name):
    c, r = Pc.case(name), Pc.reference(name)
    assert r["marginal"] == [], r["marginal"][:5]
    ties = {"duplicates": 1, "duplicates_relative": 1}
    assert len(r["ties"]) == ties.get(name, 0)
    # rule 11: the lookup on the rows that go out returns the entries that go out
    assert Q.lookup_contract(c["map_app"], r, c["n_rows"])
    st = r["status"]
    assert ((r["entry"] >= 0) == ((st == Q.KEPT) | (st == Q.LANDMARK_AT_FAULT) | (st == Q.FRAME_AT_FAULT))).all()
    assert (np.isinf(r["sq"]) == ((st == Q.NOT_LIVE) | (st == Q.MISS)))[st != Q.NOT_FINITE].all()
    s = r["stats"]
    assert sum(s["by_status"]) == st.size and s["n_pruned"] == int(Q.pruned(st).sum()) == int(r["landmarks"]["n_pruned"].sum())
    assert s["n_obs"] == int(r["landmarks"]["n_obs"].sum()) == int(r["frames"]["n_obs"].sum())
    assert int(r["landmarks"]["n_el"].sum()) == int(r["frames"]["n_el"].sum()) == int(Q.eligible(st).sum())


@pytest.mark.parametrize("name", ["lists", "lists_all_off", "duplicates", "duplicates_not_unique", "guards_off", "corners", "layout", "example"])
def test_a_second_call_with_the_guards_off_prunes_nothing(name):
    c = Pc.case(name)
    kw = dict(rel_factor=0.0, max_share_landmark=1000, max_share_frame=1000)
    a = Pc.run(c, **kw)
    again = dict(c, frames=[(uv, out) for (uv, _), out in zip(c["frames"], a["app_out"])])
    b = Pc.run(again, **kw)
    assert b["stats"]["n_pruned"] == 0 and np.array_equal(b["entry"], a["entry"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a["app_out"], b["app_out"]))
    if name != "lists_all_off" and name != "duplicates_not_unique":
        assert a["stats"]["n_pruned"] > 0


def test_the_cases_are_what_they_say():
    S = lambda name: Pc.reference(name)["status"]
    L = lambda name: Pc.reference(name)["landmarks"]
    # list lengths: every length, even and odd medians, rel_min_obs at n_el and one above
    r = Pc.reference("lists")
    assert list(r["landmarks"]["n_obs"]) == Pc.LISTS and list(r["landmarks"]["n_el"]) == Pc.LISTS
    assert list(r["landmarks"]["n_soft"]) == [0, 0, 0, 1] + [2] * 7 and (r["landmarks"]["med_sq"][3:] > 0).all() and (r["landmarks"]["med_sq"][:3] == 0).all()
    assert r["stats"]["by_status"][Q.HIGH_ERROR] == 8 and r["stats"]["by_status"][Q.RELATIVE] == 7      # (3 observations: the median IS the 0.8 px row)
    m = L("lists_rel_min_17")["med_sq"]
    assert list(m > 0) == [n >= 17 for n in Pc.LISTS] and 16 in Pc.LISTS and 17 in Pc.LISTS
    g = Pc.reference("lists_guarded")
    assert list(np.nonzero(g["landmarks"]["at_fault"])[0]) == [3] and g["stats"]["by_status"][Q.LANDMARK_AT_FAULT] == 1      # 1 of 3 > 300, 2 of 15 is not
    assert Pc.reference("lists_all_off")["stats"]["n_pruned"] == 0
    # duplicate runs
    c, r = Pc.case("duplicates"), Pc.reference("duplicates")
    st, n_max = r["status"], c["n_max"]
    lists = Q.R.observation_lists(c["map_app"], c["frames"], None, n_max)[0]
    run = [k for k in lists[0] if k // n_max == 14]
    assert [lists[0].index(k) for k in run] == [14, 15, 16]                                   # across the 16th lane
    assert [int(st[14, k % n_max]) for k in run] == [Q.DUPLICATE, Q.KEPT, Q.DUPLICATE]        # 0.3 px stays
    assert [int(x) for x in st[21, :2]] == [Q.KEPT, Q.DUPLICATE] and r["ties"] == [("duplicate", 1, 21 * n_max + 1)]
    assert [int(x) for x in st[31, :2]] == [Q.DUPLICATE, Q.KEPT] and len(lists[2]) == 5
    assert [int(x) for x in st[40, :3]] == [Q.NOT_FINITE, Q.DUPLICATE, Q.KEPT]                # the best is hard-failed: the next one stays
    assert [int(x) for x in st[63, :2]] == [Q.BEHIND, Q.BEHIND]
    assert Pc.reference("duplicates_not_unique")["stats"]["by_status"][Q.DUPLICATE] == 0
    # the guards at equality
    r = Pc.reference("guards")
    assert list(np.nonzero(r["landmarks"]["at_fault"])[0]) == [2, 3, 16] and list(np.nonzero(r["frames"]["at_fault"])[0]) == [8]
    assert [(int(a), int(b)) for a, b in zip(r["landmarks"]["n_soft"][:4], r["landmarks"]["n_el"][:4])] == [(1, 2), (2, 4), (3, 4), (2, 2)]
    assert [(int(a), int(b)) for a, b in zip(r["frames"]["n_soft"][5:9], r["frames"]["n_el"][5:9])] == [(1, 4), (1, 2), (2, 4), (3, 4)]
    assert r["stats"]["by_status"][Q.HIGH_ERROR] == 7 and r["stats"]["by_status"][Q.LANDMARK_AT_FAULT] == 7 and r["stats"]["by_status"][Q.FRAME_AT_FAULT] == 3
    assert Pc.reference("guards_share_0")["stats"]["by_status"][Q.LANDMARK_AT_FAULT] == 17 and Pc.reference("guards_share_0")["stats"]["n_frames_at_fault"] == 0
    assert Pc.reference("guards_frame_0")["stats"]["by_status"][Q.FRAME_AT_FAULT] == 17
    assert Pc.reference("guards_off")["stats"]["by_status"][Q.HIGH_ERROR] == 17
    # corner rows
    c, r = Pc.case("corners"), Pc.reference("corners")
    st = r["status"]
    assert st[2, 0] == Q.NOT_FINITE and (st[:6, 1] == Q.NOT_FINITE).all() and st[7, 0] == Q.NOT_FINITE and st[8, 0] == Q.BEHIND
    z = Cu.observation_terms(np.asarray(c["K"], np.float64), c["poses"][7][None, :3, :3], c["poses"][7][None, :3, 3], c["frames"][7][0][:1], c["map_pts"][2].astype(np.float64))[1]
    assert z[0] == 0.0
    assert st[3, 4] == Q.MISS and st[4, 5] == Q.MISS and r["stats"]["by_status"][Q.NOT_FINITE] == 8
    # the frames' layout
    r = Pc.reference("layout")
    assert (r["status"][6] == Q.NOT_LIVE).all() and r["frames"]["n_obs"][6] == 0 and (r["status"][12, len(Pc.case("layout")["frames"][12][1]):] == Q.MISS).all()
    a, b = Pc.reference("layout"), Pc.reference("layout_no_row_counts")
    assert np.array_equal(a["entry"], b["entry"]) and np.array_equal(a["status"] == Q.NOT_LIVE, (b["status"] == Q.MISS) & (a["status"] == Q.NOT_LIVE))
    # the launch's stride
    c, r = Pc.case("stride"), Pc.reference("stride")
    assert np.array_equal(np.nonzero(Q.pruned(r["status"][0]))[0], c["planted"]) and len(c["planted"]) == 207 and c["n_max"] == 20000 > 4 * 256 * 16


@pytest.mark.parametrize("fault", Q.FAULTS)
def test_every_planted_fault_changes_some_output_of_some_case(fault):
    changed = []
    for name in FAULT_CASES:
        a, b = Pc.reference(name), Pc.run(Pc.case(name), fault=fault)
        if not (np.array_equal(a["status"], b["status"]) and np.array_equal(a["landmarks"]["med_sq"], b["landmarks"]["med_sq"])
                and np.array_equal(a["landmarks"]["at_fault"], b["landmarks"]["at_fault"]) and np.array_equal(a["frames"]["at_fault"], b["frames"]["at_fault"])):
            changed.append(name)
    print(fault, changed)
    assert changed
    where = dict(upper_median="lists", guard_ge="guards", dup_by_key="duplicates", frame_guard_first="guards")
    assert where[fault] in changed


def test_the_example_data_outcome_at_the_committed_seeds():
    """the numbers of this module's docstring"""
    c, r = Pc.case("example"), Pc.reference("example")
    st, lm, fr = r["status"], r["landmarks"], r["frames"]
    named_l, named_f = set(np.nonzero(lm["at_fault"])[0]), set(np.nonzero(fr["at_fault"])[0])
    assert named_l == set(int(e) for e in c["pushed"]) and len(named_l) == 20
    assert named_f == set(c["pushed_frames"]) == {30, 60, 90}
    planted = set(c["planted"])
    assert len(planted) == 100
    # where a planted row landed: the entry its new appearance finds
    tab = Q.M.table(c["map_app"])
    on_named = set()
    for f, i in planted:
        e = int(Q.M.lookup(c["map_app"], c["frames"][f][1][i: i + 1], tab=tab)[0][0])
        assert e >= 0
        if e in named_l or f in named_f:
            on_named.add((f, i))
    assert Pc.pruned_rows(r) == planted - on_named
    by = r["stats"]["by_status"]
    print("pruned", r["stats"]["n_pruned"], {Q.STATUS[k]: by[k] for k in range(3, 10)}, "planted on named", len(on_named))
    assert (r["stats"]["n_pruned"], by[Q.BEHIND], by[Q.DUPLICATE], by[Q.HIGH_ERROR], by[Q.RELATIVE], by[Q.NOT_FINITE]) == (100, 39, 31, 30, 0, 0)
    assert by[Q.LANDMARK_AT_FAULT] == 435 and by[Q.FRAME_AT_FAULT] == 222 and len(on_named) == 0      # (the draw keeps them apart: map_prune_cases.py)
    # the only remover the library had: a cull at 1 px on the same window
    cull = Cu.cull(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], min_obs=1, min_frames=1, max_rms_px=0.0, max_err_px=1.0, dry_run=True)
    dropped = int((~cull["keep"]).sum())
    print("a cull at 1 px would drop", dropped, "landmarks")
    assert dropped == 232 and dropped > len(planted) // 2


# ---- the rules the kernels compile ----
def test_host_check_of_the_inline_rules(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/hostcheck/prune_rules_check.cpp"
    exe = str(tmp_path / "prune_rules_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "visual-odometry_amd", "csrc"), os.path.join(ROOT, "tests", "hostcheck", "prune_rules_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "prune_rules_check: ok" in r.stdout
