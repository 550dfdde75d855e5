"""voe_map_keyframes* on the GPU: every run of every case of tests/map_keyframes_cases.py against the restatement
(tests/map_keyframes_restatement.py).  Every output is an integer, so every comparison is of bytes: the verdicts, the row counts,
the keep bytes, the steps, the order, seen and red, the statistics.  Equal bytes as well between three calls, with and without the
optional order, the host form, capture and replay; the input bits keep every byte; and on the example data the kept frames handed
to vo_map_refine give the landmarks all frames give, and the window and the bundle run on what is left."""
import ctypes as C
import os

import numpy as np
import pytest

import map_bundle_restatement as B
import map_covis_cases as Cc
import map_covis_restatement as V
import map_keyframes_cases as Kc
import map_keyframes_restatement as K
import map_refine_restatement as R
from map_keyframes_dev import KeyframesDev, same
from map_refine_dev import CAM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(d, name, k, got):
    ref = Kc.reference(name, k)
    st = d.stats(got["stats_raw"])
    assert st == ref["stats"], (name, k, st, ref["stats"])
    for key in K.KEYS:
        assert got[key].tobytes() == ref[key].tobytes(), (name, k, key, got[key].tolist(), ref[key].tolist())
    assert (got["guard"] == -7).all(), (name, k)


@pytest.mark.parametrize("name", list(Kc.CASES))
def test_keyframes_against_the_restatement(vo, ctx, name):
    c = Kc.case(name)
    d = KeyframesDev(vo, ctx, c)
    try:
        for k, prm in enumerate(c["runs"]):
            runs = []
            for _ in range(3):                                # three calls: the same bytes
                d.clear_out()
                assert d.call(prm) == 0, ctx.lib.vo_last_error()
                runs.append(d.results())
            assert all(same(r, runs[0]) for r in runs[1:])
            print(f"{name} run {k}: {d.stats(runs[0]['stats_raw'])}")
            _check(d, name, k, runs[0])
            d.clear_out()                                     # without the order: the same other outputs, the array untouched
            assert d.call(prm, with_order=False) == 0
            bare = d.results()
            assert all(bare[key].tobytes() == runs[0][key].tobytes() for key in bare if key != "order") and (bare["order"] == -7).all()
            h = d.m.keyframes(c["bits"], flags=c["flags"], n_rows=c["n_rows"], n_max=c["n_max"], **prm)      # the host form
            assert all(h[key].tobytes() == runs[0][key].tobytes() for key in K.KEYS) and h["stats"] == d.stats(runs[0]["stats_raw"])
        assert d.bits().tobytes() == c["bits"].tobytes()      # the input bits are untouched
    finally:
        d.close()


def test_analysis_only_call_reports_every_verdict(vo, ctx):
    """max_dropped == 0 on the example data, every setting: nothing is dropped, the verdicts and red are the restatement's"""
    c = Kc.case("example")
    d = KeyframesDev(vo, ctx, c)
    try:
        for prm in c["runs"]:
            prm = dict(prm, max_dropped=0)
            ref = K.run(c["bits"], c["flags"], n_rows=c["n_rows"], n_max=c["n_max"], **prm)
            d.clear_out()
            assert d.call(prm) == 0, ctx.lib.vo_last_error()
            got = d.results()
            assert d.stats(got["stats_raw"]) == ref["stats"] and ref["stats"]["n_dropped"] == 0 and ref["stats"]["n_blocked"] > 0
            assert all(got[key].tobytes() == ref[key].tobytes() for key in K.KEYS)
            assert (got["step"] == -1).all() and (got["order"] == -1).all() and (got["keep"] == 1).all()
            assert got["n_rows"].tobytes() == c["n_rows"].tobytes()
    finally:
        d.close()


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c = Kc.case("frames_65")
    prm = c["runs"][1]
    d, fresh = KeyframesDev(vo, ctx, c), KeyframesDev(vo, ctx, c)
    try:
        g = C.c_void_p()
        d.clear_out()
        assert d.call(prm) == 0
        eager = d.results()
        _check(d, "frames_65", 1, eager)
        d.clear_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        # a map on which no call has sized the workspace: refused before anything is enqueued, and the capture stays valid
        rf = fresh.call(prm)
        err = lib.vo_last_error()
        rc = d.call(prm)
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        assert rf == -6 and b"capture" in err and b"voe_map_keyframes_dev" in err
        for _ in range(2):
            d.clear_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            assert same(d.results(), eager)
        assert lib.vo_graph_destroy(g) == 0
        assert d.bits().tobytes() == c["bits"].tobytes()
    finally:
        fresh.close()
        d.close()


def test_refusals(vo, ctx):
    c = Kc.case("identical")
    d = KeyframesDev(vo, ctx, c)
    try:
        prm = c["runs"][0]
        d.clear_out()
        for bad in (dict(F=0), dict(F=vo.MAP_COVIS_MAX_FRAMES + 1), dict(n_words=0), dict(d_bits=None), dict(d_stats=None), dict(d_stats=d.d_stats + 4),
                    dict(verdict=None), dict(n_rows=None), dict(keep=None), dict(step=None), dict(seen=None), dict(red=None), dict(prm=None),
                    dict(n_max=-1), dict(reserved=(0, 1, 0)), dict(order=d.d["order"] + 2)):
            assert d.call(prm, **bad) == -1, bad
            assert b"voe_map_keyframes_dev" in ctx.lib.vo_last_error(), bad
        for bad in (dict(min_observers=0), dict(share_permille=-1), dict(share_permille=1001), dict(min_seen=0), dict(max_gap=-1), dict(max_dropped=-1),
                    dict(max_dropped=vo.MAP_KEYFRAMES_MAX_STEPS + 1)):
            assert d.call(dict(prm, **bad)) == -1, bad
        assert d.call(prm, m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        with pytest.raises(vo.VoError):
            d.m.keyframes(c["bits"], flags=[0, 3] + [0] * 7)
        got = d.results()                                     # nothing was enqueued
        assert all((got[k] == -7).all() for k in K.KEYS if k != "keep") and (got["keep"] == 0xEE).all() and (got["stats_raw"] == -7).all()
        # a flag byte above 2 on the device: PROTECTED
        flags = d.dev(np.array([0, 7, 0, 0, 0, 0, 0, 0, 0], np.uint8))
        assert d.call(prm, d_flags=flags) == 0
        got = d.results()
        ref = K.run(c["bits"], [0, 1, 0, 0, 0, 0, 0, 0, 0], n_rows=c["n_rows"], n_max=c["n_max"], **prm)
        assert all(got[key].tobytes() == ref[key].tobytes() for key in K.KEYS) and got["verdict"][1] == K.PROTECTED
    finally:
        d.close()


def test_kept_frames_refine_window_and_bundle_on_the_example_data(vo, ctx):
    """Map.covisibility -> Map.keyframes (frames 0 and 120 protected) -> Map.refine with the call's n_rows: the statuses are those
    of a refine over all frames wherever that one is OK, and the observations are the kept rows' bits.  Then Map.window on the
    bits with the dropped rows zeroed, and Map.bundle on that window."""
    c, k = Cc.case("example"), Kc.case("example")
    pushed = R.perturbed(c["map_pts"], 1, 0.1)
    cam = vo.Camera(*CAM, c["K"])
    live = np.array([len(a) for _, a in c["frames"]], np.int32)
    m, m_all = vo.Map(ctx), vo.Map(ctx)
    try:
        m.update(pushed, c["map_app"])
        m_all.update(pushed, c["map_app"])
        cov = m.covisibility(c["frames"])
        assert cov["bits"].tobytes() == k["bits"].tobytes()
        kf = m.keyframes(cov["bits"], flags=k["flags"], n_rows=live, **k["runs"][0])
        ref = Kc.reference("example", 0)
        assert all(kf[key].tobytes() == ref[key].tobytes() for key in K.KEYS) and kf["stats"] == ref["stats"]
        print("keyframes:", kf["stats"], "dropped in order", kf["order"][: kf["stats"]["n_dropped"]].tolist())
        assert kf["stats"]["n_dropped"] == 74 and kf["stats"]["n_kept"] == 47
        kept_frames = [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], kf["n_rows"])]
        status_all, st_all = m_all.refine(cam, c["frames"], c["poses"], n_rounds=5, min_obs=3)
        status, st = m.refine(cam, kept_frames, c["poses"], n_rounds=5, min_obs=3)
        ok = status_all == R.OK
        print(f"refine over all frames: {st_all}; over the kept: {st}")
        assert ok.sum() == 462 and np.array_equal(status[ok], status_all[ok])
        kept_bits = V.unpack_bits(cov["bits"])[kf["keep"] == 1]
        assert st["n_obs"] == int(kept_bits.sum()) == 4489 and st_all["n_obs"] == 10012
        # the window of a kept frame on what is left, and the bundle on it (a map pushed as the window's own test pushes it)
        m.clear()
        m.update(R.perturbed(c["map_pts"], 1, 0.02), c["map_app"])
        bits = cov["bits"] * kf["keep"][:, None].astype(np.uint32)
        query = int(np.nonzero(kf["keep"])[0][np.argmin(np.abs(np.nonzero(kf["keep"])[0] - 60))])
        w = m.window(bits, query, k_free=8, k_fixed=8, min_shared=15, n_rows=kf["n_rows"])
        wr = V.window(bits, query, 8, 8, 15, n_rows=kf["n_rows"])      # (of the 47 kept frames, 4 share 15 entries with the query)
        assert all(w[key].tobytes() == wr[key].tobytes() for key in ("role", "n_rows", "fixed", "order")) and w["stats"] == wr["stats"]
        assert w["stats"]["status"] == V.OK and (kf["keep"][w["role"] != V.OUTSIDE] == 1).all() and w["stats"]["n_free"] >= 2
        frames = [(uv[:n], a[:n]) for (uv, a), n in zip(c["frames"], w["n_rows"])]
        _, pose_status, _, _, bst = m.bundle(cam, frames, c["poses"], w["fixed"])
        print(f"window of frame {query}: {w['order'][:16].tolist()}; bundle {bst}")
        assert bst["status"] == B.OK and bst["cost_after"] <= bst["cost_before"] and np.array_equal(pose_status == B.POSE_OK, w["role"] == V.FREE)
    finally:
        m_all.close()
        m.close()


def test_keyframes_map_app_on_the_example_data(vo, ctx):
    """apps/bin/keyframes_map prints the counts the Python call gives and checks itself"""
    import subprocess
    exe = os.path.join(ROOT, "apps", "bin", "keyframes_map")
    assert os.path.exists(exe), "apps/bin/keyframes_map is missing: build() makes it"
    data = os.path.join(ROOT, "tests", "golden", "example_data", "data")
    ref = Kc.reference("example", 0)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert f"dropped {ref['stats']['n_dropped']} kept {ref['stats']['n_kept']}" in r.stdout
    assert "order: " + " ".join(str(f) for f in ref["order"][: ref["stats"]["n_dropped"]]) + "\n" in r.stdout
    assert "the kept frames refine the same landmarks" in r.stdout
