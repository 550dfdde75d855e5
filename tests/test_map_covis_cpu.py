"""CPU checks behind voe_map_covis* and voe_map_window*: the ABI (the voe_ rule with the fifth extension header, the struct
sizes, the refusals that need no device), the conditions on the cases of the GPU test (every tie, every edge and the example
data are what tests/map_covis_cases.py says they are), the window of the example data handed to the bundle restatement, and
the host check of the inline rules the kernels compile (tests/hostcheck/covis_check.cpp, built with sanitizers and run as a
program)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import map_bundle_restatement as B
import map_covis_cases as Cc
import map_covis_restatement as V
import map_refine_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"voe_map_covis_batch_dev", "voe_map_covis", "voe_map_window_dev", "voe_map_window"}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- ABI ----
def test_the_voe_rule_holds_with_the_fifth_header(vo):
    lib = vo.load_library()
    hip = _read("include", "vo_hip.h")
    assert hip.count('#include "vo_map_covis.h"') == 1 and hip.index('#include "vo_map_align.h"') < hip.index('#include "vo_map_covis.h"')
    header = re.sub(r"/\*.*?\*/", "", _read("include", "vo_map_covis.h"), flags=re.S)
    assert set(re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", header)) == NAMES
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is declared in include/vo_map_covis.h but not exported"
    assert lib.vo_abi_version() == 1
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert NAMES <= set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M))               # exported, unversioned
        assert not re.findall(r" [A-Za-z] (voe_[a-z0-9_]+)@", out, flags=re.M)
    assert "voe_" not in _read("visual-odometry_amd", "csrc", "vo_map_adjust.map")
    mk = _read("visual-odometry_amd", "csrc", "Makefile")
    assert "map_covis.hip" in mk and "vo_map_covis.h" in mk and "covis_rules.h" in mk
    apps = _read("apps", "Makefile")
    assert "vo_map_covis.h" in apps and "bin/window_map" in apps


def test_structs_names_and_source(vo):
    assert C.sizeof(vo.MapCovisStats) == 32 and C.sizeof(vo.MapWindowParams) == 16 and C.sizeof(vo.MapWindowStats) == 32
    assert vo.MapCovisStats.n_entries_seen.offset == 16 and vo.MapWindowStats.query_seen.offset == 24 and vo.MapWindowParams.min_shared.offset == 12
    hdr = _read("include", "vo_map_covis.h")
    assert vo.MAP_WINDOW_ROLE == ("OUTSIDE", "FREE", "FIXED") and vo.MAP_WINDOW_STATUS == ("OK", "NO_FIXED", "QUERY_UNSEEN")
    for k, name in enumerate(vo.MAP_WINDOW_ROLE):
        assert re.search(r"#define VOE_MAP_WINDOW_%s\s+%d\b" % (name, k), hdr), name
    for k, name in enumerate(vo.MAP_WINDOW_STATUS):
        assert re.search(r"#define VOE_MAP_WINDOW_%s\s+%d\b" % (name, k), hdr), name
    assert re.search(r"#define VOE_MAP_COVIS_MAX_FRAMES\s+%d\b" % vo.MAP_COVIS_MAX_FRAMES, hdr) and vo.MAP_COVIS_MAX_FRAMES == 4096
    assert (V.OUTSIDE, V.FREE, V.FIXED) == (0, 1, 2) and (V.OK, V.NO_FIXED, V.QUERY_UNSEEN) == (0, 1, 2)
    for n in ("covisibility", "covis_batch_dev", "window", "window_dev"):
        assert hasattr(vo.Map, n)
    hpp = _read("include", "vo", "localise.hpp")
    assert " covisibility(" in hpp and " window(" in hpp and "struct Covisibility" in hpp and "struct MapWindow" in hpp
    # the kernels: integers alone, nothing that waits for another workgroup, the tile and the chunk the cases are built around
    src = _read("visual-odometry_amd", "csrc", "map_covis.hip")
    rules = _read("visual-odometry_amd", "csrc", "covis_rules.h")
    for text in (src, rules):
        assert not re.search(r"\b(float|double|half|__fp16)\b", text)
        assert "cooperative" not in text.lower() and "grid.sync" not in text and "atomicAdd" not in text and "atomicCAS" not in text
    assert src.count("atomicOr(") == 1 and "while" not in re.sub(r"//.*", "", src)
    assert int(re.search(r"constexpr int COVIS_TILE = (\d+);", rules).group(1)) == Cc.TILE
    assert int(re.search(r"constexpr int COVIS_CHUNK = (\d+);", rules).group(1)) == Cc.CHUNK


def test_refusals_that_need_no_device(vo):
    """the argument checks come before the map is looked at: with a null map every one of them is reported as itself"""
    lib = vo.load_library()
    z, i, s = None, C.c_int, C.c_size_t
    buf = (C.c_int32 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    st, ws = vo.MapCovisStats(), vo.MapWindowStats()
    err = lambda: lib.vo_last_error()
    covis = lambda F=2, W=1, bits=p, stats=p: lib.voe_map_covis_batch_dev(z, i(F), z, s(1), i(1), z, i(W), bits, z, stats)
    for bad, word in ((dict(F=0), b"n_frames"), (dict(F=4097), b"n_frames"), (dict(W=0), b"n_words"), (dict(bits=z), b"null argument"),
                      (dict(stats=z), b"null argument"), (dict(stats=odd), b"8-byte")):
        assert covis(**bad) == -1 and word in err() and b"voe_map_covis_batch_dev" in err(), bad
    assert covis() == -1 and b"null map" in err()
    assert lib.voe_map_covis(z, i(0), z, z, i(1), i(1), p, z, C.byref(st)) == -1 and b"n_frames" in err()
    assert lib.voe_map_covis(z, i(1), z, z, i(1), i(1), p, z, C.byref(st)) == -1 and b"null map" in err()

    def window(F=3, W=1, bits=p, n_max=4, prm=(0, 1, 0, 1), role=p, rows=p, fixed=p, stats=p, fn=lib.voe_map_window_dev):
        q = vo.MapWindowParams(*prm) if prm is not None else None
        return fn(z, i(F), i(W), bits, z, i(n_max), C.byref(q) if q is not None else None, role, rows, fixed, z, z, stats)
    for bad, word in ((dict(F=0), b"n_frames"), (dict(F=4097), b"n_frames"), (dict(W=0), b"n_words"), (dict(bits=z), b"null"), (dict(stats=z), b"null"),
                      (dict(stats=odd), b"8-byte"), (dict(role=z), b"null"), (dict(rows=z), b"null"), (dict(fixed=z), b"null"), (dict(prm=None), b"null"),
                      (dict(n_max=-1), b"negative"), (dict(prm=(-1, 1, 0, 1)), b"query"), (dict(prm=(3, 1, 0, 1)), b"query"),
                      (dict(prm=(0, 0, 0, 1)), b"k_free"), (dict(prm=(0, 4, 0, 1)), b"k_free"), (dict(prm=(0, 1, -1, 1)), b"k_fixed"),
                      (dict(prm=(0, 1, 4, 1)), b"k_fixed"), (dict(prm=(0, 1, 0, 0)), b"min_shared")):
        assert window(**bad) == -1 and word in err() and b"voe_map_window_dev" in err(), bad
        if word != b"8-byte":                                # (the host form takes its statistics at any address)
            assert window(fn=lib.voe_map_window, **bad) == -1 and word in err(), bad
    assert window() == -1 and b"null map" in err()
    assert window(prm=(2, 3, 3, 1)) == -1 and b"null map" in err()      # (the largest values allowed)
    assert window(fn=lib.voe_map_window, stats=C.cast(C.pointer(ws), C.c_void_p)) == -1 and b"null map" in err()


# ---- conditions on the cases ----
def test_the_example_data_gives_a_non_trivial_window():
    c, r = Cc.case("example"), Cc.reference("example")
    assert r["bits"].shape == (121, 32) and r["stats"]["n_entries"] == 1000 and r["counts"].shape == (121, 121)
    assert r["stats"]["n_hits"] == r["stats"]["n_seen"]       # no frame of the example data hits an entry twice
    assert np.array_equal(r["counts"], r["counts"].T) and np.array_equal(np.diag(r["counts"]), r["sees"].sum(1))
    far = [(f, g) for f in range(121) for g in range(f + 31, 121) if r["counts"][f, g] >= 15]
    top = V.ranked(r["counts"][0], np.ones(121, bool))[:8]
    print(f"frame 0 shares most with {top}; {len(far)} pairs more than 30 frames apart share at least 15 landmarks")
    assert max(top) > 100 and len(far) > 1000                 # the trajectory comes back: picking neighbours by index misses these
    for k, prm in enumerate(c["windows"]):
        w = Cc.window_reference("example", k)
        st = w["stats"]
        print(prm, "free", w["order"][:st["n_free"]].tolist(), "fixed", w["order"][st["n_free"]:st["n_free"] + st["n_fixed"]].tolist(), st)
        assert st["status"] == V.OK and st["n_free"] == 8 and st["n_fixed"] == 8 and st["n_candidates"] > 8 and st["n_fixed_candidates"] > 8
        assert w["order"][0] == prm["query"] and (w["order"][16:] == -1).all() and len(set(w["order"][:16])) == 16
        assert st["n_points"] > st["query_seen"] > 15
        assert np.array_equal(w["c"], r["counts"][prm["query"]])      # the row the window counts itself is the matrix's


@pytest.mark.parametrize("size", Cc.MAP_SIZES)
def test_map_size_cases_have_their_sizes_after_the_lookup(size):
    c, r = Cc.case(f"map_{size}"), Cc.reference(f"map_{size}")
    assert r["stats"]["n_entries"] == size == len(c["map_app"]) and r["bits"].shape[1] == (size + 31) // 32
    assert r["sees"][:, 0].any() and r["sees"][:, size - 1].any()      # the first and the last entry are seen
    assert all(r["sees"][:, e].any() for e in (31, 32, 33, 63, 64, 1023, 1024, 2047, 2048) if e < size)
    assert not V.unpack_bits(r["bits"])[:, size:].any()


def test_word_edge_cases_are_what_they_say():
    p, b = Cc.case("padded_words"), Cc.reference("padded_words")
    assert b["bits"].shape[1] == 7 > V.words_for(len(p["map_app"])) == 3 and not b["bits"][:, 3:].any() and b["bits"][:, 2].any()
    c, r = Cc.case("bound_above_size"), Cc.reference("bound_above_size")
    assert c["dup_rows"] == 10 and r["stats"]["n_entries"] == 60 and r["bits"].shape[1] == 3 == V.words_for(70) > V.words_for(60)
    assert not r["bits"][:, 2].any()
    words = {Cc.reference(f"map_{n}")["bits"].shape[1] for n in Cc.MAP_SIZES}
    assert {Cc.CHUNK - 1, Cc.CHUNK, Cc.CHUNK + 1, 2 * Cc.CHUNK + 1} <= words      # the kernel's own chunk edges, in words
    big = Cc.reference("large_map")
    assert big["stats"]["n_entries"] == 65537 and big["bits"].shape == (3, 2049) and big["bits"].shape[1] > 32 * Cc.CHUNK      # 33 chunks
    assert big["sees"][:, 0].all() and big["sees"][:, 65536].all() and big["bits"][:, 2048].tolist() == [1, 1, 1]
    assert (np.diag(big["counts"]) > big["counts"][0, 1]).all() and big["counts"][0, 1] >= 22


@pytest.mark.parametrize("F", Cc.FRAME_COUNTS)
def test_frame_count_cases_have_their_sizes_after_the_lookup(F):
    c, r = Cc.case(f"frames_{F}"), Cc.reference(f"frames_{F}")
    assert r["stats"]["n_frames"] == F == len(c["frames"]) and (np.diag(r["counts"]) == 40).all() and r["stats"]["n_hits"] == 40 * F
    assert r["bits"].shape[1] == 10                           # an odd row stride in 64-bit words would be 5: rows 40 bytes apart
    if F > 2:
        off = r["counts"][~np.eye(F, dtype=bool)]
        assert off.max() > 5 and (F < 8 or off.min() == 0)    # near frames share, far ones do not
    assert {Cc.TILE - 1, Cc.TILE, Cc.TILE + 1, 2 * Cc.TILE + 1} <= set(Cc.FRAME_COUNTS)      # the kernel's own tile edges are among them


def test_content_case_is_what_it_says():
    c, r = Cc.case("content"), Cc.reference("content")
    S, C_ = r["sees"], r["counts"]
    n_rows = c["n_rows"]
    assert n_rows[c["empty"]] == 0 and not S[c["empty"]].any() and C_[c["empty"]].sum() == 0
    assert any(len(a) > n for (_, a), n in zip(c["frames"], n_rows))                      # garbage behind the live rows ...
    _, _, ents = R.observation_lists(c["map_app"], c["frames"], n_rows=n_rows)
    full = R.observation_lists(c["map_app"], c["frames"])[2]
    assert any((e_full[n:] >= 0).any() for e_full, n in zip(full, n_rows))                # ... which would hit, were it live
    assert r["stats"]["n_hits"] == r["stats"]["n_seen"] + 1                               # two rows of one frame on one entry: seen once
    twice = [f for f, e in enumerate(ents) if len(e[e >= 0]) != len(set(e[e >= 0]))]
    assert twice == [1]
    live = [a[:n] for (_, a), n in zip(c["frames"], n_rows)]
    assert any(np.isnan(a).any() for a in live)                                           # a NaN appearance row
    assert any(np.signbit(a[a == 0]).any() for a in live) and not np.signbit(c["map_app"][c["map_app"] == 0]).any()      # -0 against +0 ...
    assert S[:, 0].any()                                                                  # ... and the entry with the +0 is seen
    assert any(((e[:n] < 0) & ~np.isnan(a[:n]).any(1)).any() for e, (_, a), n in zip(ents, c["frames"], n_rows))        # rows of no map
    f, g = c["identical"]
    assert np.array_equal(S[f], S[g]) and C_[f, g] == C_[f, f] == C_[g, g] > 0
    f, g = c["disjoint"]
    assert C_[f, g] == 0 and C_[f, f] == 10 == C_[g, g]
    assert Cc.window_reference("content", 1)["stats"]["status"] == V.QUERY_UNSEEN


def test_window_tie_cases_have_equal_keys_at_the_boundary_they_name():
    c = Cc.case("window_ties")
    W = {name: Cc.window_reference("window_ties", k) for k, name in enumerate(c["window_names"])}
    P = dict(zip(c["window_names"], c["windows"]))

    def ranks(w, prm, which):
        if which == "free":
            cnt, elig = w["c"], (w["c"] >= prm["min_shared"]) & (np.arange(len(w["c"])) != prm["query"])
        else:
            cnt, elig = w["s"], (w["role"] != V.FREE) & (w["s"] >= prm["min_shared"])
        order = V.ranked(cnt, elig)
        return order, [int(cnt[g]) for g in order]
    w, prm = W["tie_across_k_free"], P["tie_across_k_free"]
    order, cnt = ranks(w, prm, "free")
    k = prm["k_free"] - 1                                     # candidates taken
    assert cnt[k - 1] == cnt[k] and order[k - 1] < order[k] and w["role"][order[k - 1]] == V.FREE and w["role"][order[k]] != V.FREE
    w, prm = W["ties_inside"], P["ties_inside"]
    order, cnt = ranks(w, prm, "free")
    k = prm["k_free"] - 1
    assert len(set(cnt[:k])) < k and cnt[k - 1] > cnt[k]      # equal keys among the taken, none across the boundary
    assert w["order"][: k + 1].tolist() == [prm["query"]] + order[:k]
    w, prm = W["tie_across_k_fixed"], P["tie_across_k_fixed"]
    order, cnt = ranks(w, prm, "fixed")
    k = prm["k_fixed"]
    assert cnt[k - 1] == cnt[k] and order[k - 1] < order[k] and w["role"][order[k - 1]] == V.FIXED and w["role"][order[k]] == V.OUTSIDE
    forder, fcnt = ranks(W["ties_inside"], P["ties_inside"], "fixed")
    assert len(set(fcnt[: P["ties_inside"]["k_fixed"]])) < P["ties_inside"]["k_fixed"]      # ties inside the second ranking too
    st = {n: W[n]["stats"] for n in W}
    assert st["k_free_1"]["n_free"] == 1 and st["k_free_1"]["n_points"] == st["k_free_1"]["query_seen"] and st["k_free_1"]["status"] == V.OK
    assert st["k_fixed_0"]["status"] == V.NO_FIXED and st["k_fixed_0"]["n_fixed"] == 0 and st["k_fixed_0"]["n_fixed_candidates"] > 0
    assert (W["k_fixed_0"]["role"] == V.FREE).sum() == 3 and (W["k_fixed_0"]["fixed"] == (W["k_fixed_0"]["role"] != V.FREE)).all()
    a, pa = st["above_candidates"], P["above_candidates"]
    assert a["n_free"] == 1 + a["n_candidates"] < pa["k_free"] and a["n_fixed"] == a["n_fixed_candidates"] < pa["k_fixed"] and a["n_fixed"] > 0
    assert st["no_candidate"] == dict(status=V.NO_FIXED, n_free=1, n_fixed=0, n_candidates=0, n_fixed_candidates=0, n_points=24, query_seen=24)
    u = W["query_unseen"]
    assert u["stats"] == dict(status=V.QUERY_UNSEEN, n_free=0, n_fixed=0, n_candidates=0, n_fixed_candidates=0, n_points=0, query_seen=0)
    assert not u["role"].any() and not u["n_rows"].any() and u["fixed"].all() and (u["order"] == -1).all() and not u["union"].any()
    last = W["query_last"]
    assert P["query_last"]["query"] == len(last["role"]) - 1 and last["order"][0] == P["query_last"]["query"] and last["stats"]["status"] == V.OK
    # the outputs that plug into the bundle: the live rows inside the window, 0 outside; the mask
    w = W["tie_across_k_free"]
    assert np.array_equal(w["n_rows"], np.where(w["role"] != V.OUTSIDE, c["n_rows"], 0)) and (w["n_rows"][w["role"] != V.OUTSIDE] > 0).all()
    n = Cc.window_reference("window_no_row_counts", 0)
    assert set(n["n_rows"]) == {0, 17} and np.array_equal(n["role"], w["role"])


# ---- composition on the CPU: the window handed to the bundle restatement ----
def test_the_window_handed_to_the_bundle_restatement():
    c, r = Cc.case("example"), Cc.reference("example")
    live = np.array([len(a) for _, a in c["frames"]], np.int32)
    w = V.window(r["bits"], n_rows=live, **c["windows"][1])
    role = w["role"]
    res = B.bundle(c["K"], R.perturbed(c["map_pts"], 1, 0.02), c["map_app"], c["frames"], c["poses"], fixed=w["fixed"].astype(bool), n_rows=w["n_rows"])
    st = res["stats"]
    inside = role != V.OUTSIDE
    hits = int(np.diag(r["counts"])[inside].sum())
    seen = r["sees"][inside].any(0)
    print(f"window of frame 60: {int(inside.sum())} frames, {hits} hits, {int(seen.sum())} entries; bundle: {st}")
    assert st["status"] == B.OK and st["n_free_frames"] == 8 and int(inside.sum()) == 16
    assert st["n_obs"] == hits
    assert np.array_equal(res["point_status"] != B.POINT_UNSEEN, seen)
    assert np.array_equal(res["pose_status"] == B.POSE_OK, role == V.FREE)
    assert st["cost_after"] < st["cost_before"]
    # a FIXED frame brings in all of its own hits: landmarks outside U are points of the problem
    assert int(seen.sum()) > w["stats"]["n_points"]


# ---- the inline rules the kernels compile, on the host, under sanitizers ----
def test_host_check_of_the_inline_rules(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/hostcheck/covis_check.cpp"
    exe = str(tmp_path / "covis_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "visual-odometry_amd", "csrc"), os.path.join(ROOT, "tests", "hostcheck", "covis_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0 and "covis_check: ok" in r.stdout
