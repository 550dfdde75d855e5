"""voe_map_covis* and voe_map_window* on the GPU: every case of tests/map_covis_cases.py against the restatement
(tests/map_covis_restatement.py).  Every output is an integer, so every comparison is of bytes: the bits, the counts, the
statistics, the roles, the row counts, the mask, the order, the union.  Equal bytes as well between three calls, with and without
the optional outputs, the host forms, capture and replay; the map keeps every byte; and the window handed to vox_map_bundle over
all frames of the example data adjusts exactly what the window names."""
import ctypes as C
import os

import numpy as np
import pytest

import map_bundle_restatement as B
import map_covis_cases as Cc
import map_covis_restatement as V
import map_refine_restatement as R
from map_covis_dev import CovisDev, same
from map_refine_dev import CAM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("role", "n_rows", "fixed", "order", "union")


def _live_frames(c):
    if c["n_rows"] is None:
        return c["frames"]
    return [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], c["n_rows"])]


def _check_window(d, name, k, got):
    ref = Cc.window_reference(name, k)
    st = d.wstats(got["stats"])
    assert st == ref["stats"], (name, k, st, ref["stats"])
    for key in KEYS:
        assert got[key].tobytes() == ref[key].tobytes(), (name, k, key, got[key].tolist(), ref[key].tolist())


def _windows_every_form(d, name):
    c = Cc.case(name)
    n_rows, n_max = Cc.live_rows(c)
    for k, prm in enumerate(c["windows"]):
        runs = []
        for _ in range(3):                                    # three calls: the same bytes
            d.clear_window_out()
            assert d.window(prm) == 0, d.lib.vo_last_error()
            runs.append(d.window_results())
        assert all(same(list(r.values()), list(runs[0].values())) for r in runs[1:])
        _check_window(d, name, k, runs[0])
        d.clear_window_out()                                  # without the optional outputs: the same required ones
        assert d.window(prm, optional=False) == 0
        bare = d.window_results()
        assert all(bare[key].tobytes() == runs[0][key].tobytes() for key in ("role", "n_rows", "fixed", "stats"))
        assert (bare["order"] == -7).all() and (bare["union"].view(np.int32) == -7).all()
        bits = d.read(d.d_bits, (d.F, d.W), np.uint32)        # the host form on the same bits
        h = d.m.window(bits, n_rows=n_rows, n_max=n_max, **prm)
        assert all(h[key].tobytes() == runs[0][key].tobytes() for key in KEYS) and h["stats"] == d.wstats(runs[0]["stats"])


@pytest.mark.parametrize("name", list(Cc.CASES))
def test_covisibility_and_window_against_the_restatement(vo, ctx, name):
    c, ref = Cc.case(name), Cc.reference(name)
    d = CovisDev(vo, ctx, c)
    try:
        if c["dup_rows"]:                                     # the host's bound lies above the size the device holds
            assert d.m.size_bound() == d.M + c["dup_rows"] and 32 * d.W >= d.m.size_bound() > d.M
        start = d.map_state()
        runs = []
        for _ in range(3):                                    # three calls: the same bytes
            d.clear_covis_out()
            assert d.covis() == 0, ctx.lib.vo_last_error()
            runs.append(d.covis_results())
        assert all(same(r, runs[0]) for r in runs[1:])
        bits, counts, raw, guard = runs[0]
        st = d.cstats(raw)
        print(f"{name}: {st}, bits {bits.shape}")
        assert st == ref["stats"], (name, st, ref["stats"])
        assert bits.tobytes() == ref["bits"].tobytes() and (guard == 0xA5A5A5A5).all()
        assert counts.tobytes() == ref["counts"].tobytes()
        # without the counts: the same bits and statistics, the matrix untouched
        d.clear_covis_out()
        assert d.covis(counts=False) == 0
        b2, c2, raw2, _ = d.covis_results()
        assert b2.tobytes() == bits.tobytes() and raw2.tobytes() == raw.tobytes() and (c2 == -7).all()
        # the window, every form, on the bits the device holds
        _windows_every_form(d, name)
        assert same(d.map_state(), start)                     # the map, its table and its header keep every byte
        # the host form (it reads the size first: the bound becomes the size)
        for want in (True, False):
            h = d.m.covisibility(_live_frames(c), want_counts=want, n_words=d.W)
            assert h["bits"].tobytes() == bits.tobytes() and h["stats"] == st
            assert (h["counts"].tobytes() == counts.tobytes()) if want else h["counts"] is None
        assert same(d.map_state(), start) and len(d.m) == d.M
    finally:
        d.close()


@pytest.mark.parametrize("name", list(Cc.WINDOW_CASES))
def test_window_ties_and_statuses(vo, ctx, name):
    d = CovisDev(vo, ctx, Cc.case(name))
    try:
        _windows_every_form(d, name)
    finally:
        d.close()


def test_counts_row_is_what_the_window_counts(vo, ctx):
    """ranks recomputed from counts[query] give the free set the window chose"""
    c = Cc.case("example")
    d = CovisDev(vo, ctx, c)
    try:
        assert d.covis() == 0
        _, counts, _, _ = d.covis_results()
        for prm in c["windows"]:
            assert d.window(prm) == 0
            got = d.window_results()
            q = prm["query"]
            eligible = (counts[q] >= prm["min_shared"]) & (np.arange(d.F) != q)
            free = [q] + V.ranked(counts[q], eligible)[: prm["k_free"] - 1]
            assert got["order"][: len(free)].tolist() == free and set(np.nonzero(got["role"] == V.FREE)[0]) == set(free)
            assert d.wstats(got["stats"])["query_seen"] == counts[q, q]
    finally:
        d.close()


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c = Cc.case("content")
    prm = c["windows"][0]
    d, fresh = CovisDev(vo, ctx, c), CovisDev(vo, ctx, c)
    try:
        g = C.c_void_p()
        start = d.map_state()
        d.clear_covis_out(); d.clear_window_out()
        assert d.covis() == 0 and d.window(prm) == 0
        eager = list(d.covis_results()) + list(d.window_results().values())
        d.clear_covis_out(); d.clear_window_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        # a map on which no call has sized the workspaces: refused before anything is enqueued, and the capture stays valid --
        # the calls on the sized map are captured behind the refusals and replay below
        rf1 = fresh.covis()
        err1 = lib.vo_last_error()
        rf2 = fresh.window(prm)
        err2 = lib.vo_last_error()
        rc1, rc2 = d.covis(), d.window(prm)
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc1 == 0 and rc2 == 0, lib.vo_last_error()
        assert rf1 == -6 and b"capture" in err1 and rf2 == -6 and b"capture" in err2
        for _ in range(2):
            d.clear_covis_out(); d.clear_window_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            assert same(list(d.covis_results()) + list(d.window_results().values()), eager)
        assert lib.vo_graph_destroy(g) == 0
        assert same(d.map_state(), start)
    finally:
        fresh.close()
        d.close()


def test_refusals(vo, ctx):
    c = Cc.case("content")
    d = CovisDev(vo, ctx, c)
    try:
        start = d.map_state()
        for bad in (dict(F=0), dict(F=vo.MAP_COVIS_MAX_FRAMES + 1), dict(n_words=0), dict(n_words=1), dict(d_bits=None), dict(d_stats=None),
                    dict(d_stats=d.d_stats + 4), dict(n_max=-1), dict(app_stride=1), dict(d_app=None), dict(d_app=d.d_app + 4)):
            assert d.covis(**bad) == -1, bad
            assert b"voe_map_covis_batch_dev" in ctx.lib.vo_last_error() or b"vo_map_lookup" in ctx.lib.vo_last_error(), bad
        assert d.covis(m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        prm = c["windows"][0]
        for bad in (dict(F=0), dict(F=vo.MAP_COVIS_MAX_FRAMES + 1), dict(n_words=0), dict(d_bits=None), dict(d_stats=None), dict(d_stats=d.d_wstats + 4),
                    dict(d_role=None), dict(d_rows=None), dict(d_fixed=None), dict(prm=None), dict(n_max=-1)):
            assert d.window(prm, **bad) == -1, bad
            assert b"voe_map_window_dev" in ctx.lib.vo_last_error(), bad
        for bad in (dict(query=-1), dict(query=d.F), dict(k_free=0), dict(k_free=d.F + 1), dict(k_fixed=-1), dict(k_fixed=d.F + 1), dict(min_shared=0)):
            assert d.window(dict(prm, **bad)) == -1, bad
        assert d.window(prm, m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        assert same(d.map_state(), start)
    finally:
        d.close()


def test_the_window_handed_to_the_bundle_on_the_example_data(vo, ctx):
    """vox_map_bundle over ALL 121 frames with the window's n_rows and fixed: exactly the FREE frames move, exactly the entries the
    window's frames see are points of the problem"""
    c = Cc.case("example")
    pushed = R.perturbed(c["map_pts"], 1, 0.02)
    m = vo.Map(ctx)
    try:
        m.update(pushed, c["map_app"])
        cam = vo.Camera(*CAM, c["K"])
        cov = m.covisibility(c["frames"])
        assert cov["bits"].tobytes() == Cc.reference("example")["bits"].tobytes()
        live = np.array([len(a) for _, a in c["frames"]], np.int32)
        w = m.window(cov["bits"], n_rows=live, **c["windows"][1])
        role = w["role"]
        assert w["stats"]["status"] == V.OK and int((role == V.FREE).sum()) == 8 and int((role == V.FIXED).sum()) == 8
        frames = [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], w["n_rows"])]      # the window's row counts over the same frames
        poses, pose_status, point_status, _, st = m.bundle(cam, frames, c["poses"], w["fixed"])
        print(f"window of frame 60: {w['order'][:16].tolist()}; bundle {st}")
        assert st["status"] == B.OK and st["cost_after"] <= st["cost_before"] and st["n_free_frames"] == 8
        assert np.array_equal(pose_status == B.POSE_OK, role == V.FREE)
        T_in = np.stack([np.asarray(X, np.float32) for X in c["poses"]])
        assert poses[role != V.FREE].tobytes() == T_in[role != V.FREE].tobytes()
        seen = V.unpack_bits(cov["bits"])[role != V.OUTSIDE].any(0)[: len(pushed)]
        assert np.array_equal(point_status != B.POINT_UNSEEN, seen)
        assert cov["stats"]["n_hits"] == cov["stats"]["n_seen"]      # no frame hits an entry twice: hits are the diagonal
        assert st["n_obs"] == int(np.diag(cov["counts"])[role != V.OUTSIDE].sum())
        after = m.read()[0]
        assert after[~seen].tobytes() == pushed[~seen].tobytes()
    finally:
        m.close()


def test_window_map_app_on_the_example_data(vo, ctx):
    """apps/bin/window_map prints the window the Python call gives and, with --bundle, checks itself"""
    import subprocess
    exe = os.path.join(ROOT, "apps", "bin", "window_map")
    assert os.path.exists(exe), "apps/bin/window_map is missing: build() makes it"
    data = os.path.join(ROOT, "tests", "golden", "example_data", "data")
    c = Cc.case("example")
    m = vo.Map(ctx)
    try:
        m.update(c["map_pts"], c["map_app"])
        w = m.window(m.covisibility(c["frames"], want_counts=False)["bits"], **c["windows"][1])
    finally:
        m.close()
    n = w["stats"]["n_free"] + w["stats"]["n_fixed"]
    assert n == 16
    for extra in ([], ["--bundle"]):
        r = subprocess.run([exe, data, "--query=60"] + extra, capture_output=True, text=True, timeout=120)
        print(r.stdout[-2000:])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        assert "order: " + " ".join(str(f) for f in w["order"][:n]) + "\n" in r.stdout
        assert f"free {w['stats']['n_free']} fixed {w['stats']['n_fixed']} candidates {w['stats']['n_candidates']}" in r.stdout
    assert "window and bundle agree" in r.stdout
