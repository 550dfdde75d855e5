"""voe_map_prune[_batch_dev] on the GPU: every case of tests/map_prune_cases.py against the float64 restatement
(tests/map_prune_restatement.py), the contract of rule 11 on the device, the map's bytes, the bits of voe_map_cull, equal bytes
(three calls, batched against single, the host form, optional outputs, capture and replay), the refusals, the workspace under
poison in fresh child processes and under a host bound above the size, and the joint adjustment downstream.

Against float64: statuses, entries, the integers of the landmark and frame records and the statistics are equal exactly
(tests/test_map_prune_cpu.py shows that no case takes a marginal decision but the planted exact ties, which go to the lowest
key).  d_sq_out and med_sq lie within TWICE the restatement's a-priori rounding bound of the term, derived from eps = 2^-53 and
the magnitudes (the docstring of tests/map_cull_restatement.py); NOT_FINITE rows are skipped.  d_app_out is compared by bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import map_prune_cases as Pc
import map_prune_restatement as Q
import map_states
from map_prune_dev import FILL, PruneDev, flat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = dict(rel_factor=0.0, max_share_landmark=1000, max_share_frame=1000)
POISON_CASES = ["lists", "duplicates", "guards", "corners", "layout"]


def _live_frames(c):
    if c["n_rows"] is None:
        return c["frames"]
    return [(uv[: max(0, n)], a[: max(0, n)]) for (uv, a), n in zip(c["frames"], c["n_rows"])]


def _compare(name, d, got, ref, in_place=False):
    """the device's outputs against the restatement's"""
    c = d.case
    assert got["tails_kept"]
    st = d.pstats(got["stats"])
    assert st == ref["stats"], (name, st, ref["stats"])
    assert np.array_equal(got["status"], ref["status"]), (name, np.argwhere(got["status"] != ref["status"])[:5].tolist())
    assert np.array_equal(got["entry"], ref["entry"])
    lm, fr = got["lm"], got["fr"]
    for k in ("n_obs", "n_el", "n_soft", "n_pruned", "at_fault"):
        assert np.array_equal(lm[k], ref["landmarks"][k]), (name, k)
    for k in ("n_obs", "n_el", "n_soft", "at_fault"):
        assert np.array_equal(fr[k], ref["frames"][k]), (name, k)
    assert not lm["reserved"].any()
    # |e|^2: +inf exactly where there is no observation, within twice the bound elsewhere (NOT_FINITE rows skipped)
    obs = (ref["status"] != Q.NOT_LIVE) & (ref["status"] != Q.MISS)
    assert np.isposinf(got["sq"][~obs]).all()
    ok = obs & (ref["status"] != Q.NOT_FINITE)
    dist = np.abs(got["sq"][ok] - ref["sq"][ok])
    ceil = 2 * ref["b_sq"][ok]
    worst = float(np.max(np.where(dist == 0, 0.0, dist / np.maximum(ceil, 1e-300)), initial=0.0))
    assert (dist <= ceil).all(), (name, worst)
    zero = ref["landmarks"]["med_sq"] == 0
    assert (lm["med_sq"][zero] == 0).all()
    dm = np.abs(lm["med_sq"] - ref["landmarks"]["med_sq"])
    assert (dm <= 2 * ref["landmarks"]["b_med"]).all(), (name, float(dm.max()))
    # the rows that go out, by bytes: a frame's own rows as the restatement writes them, NaN padding rows as they were, and
    # nothing behind the live rows or between the frames
    want = d.app0.copy() if in_place else np.full((d.F, d.stride, 10), FILL, np.int32).view(np.float32)
    for f, a in enumerate(ref["app_out"]):
        n = min(len(a), d.n_max)
        live = d.live[f]
        want[f, : d.n_max][live] = d.app0[f, : d.n_max][live]
        rows = live[:n]
        want[f, :n][rows] = a[:n][rows]
    assert got["app"].tobytes() == want.tobytes(), name
    print(f"{name}: {st['n_obs']} observations, pruned {st['n_pruned']}, by status {st['by_status']}, named {st['n_landmarks_at_fault']} landmarks and "
          f"{st['n_frames_at_fault']} frames; |e|^2 at {worst:.3g} of its ceiling")


@pytest.mark.parametrize("name", list(Pc.CASES))
def test_against_float64_and_every_form(vo, ctx, name):
    c, ref = Pc.case(name), Pc.reference(name)
    d = PruneDev(vo, ctx, c)
    try:
        before = d.map_state()
        runs = []
        for _ in range(3):                                    # three calls: the same bytes
            d.clear_prune_out()
            assert d.prune() == 0, ctx.lib.vo_last_error()
            runs.append(d.prune_results())
        assert flat(runs[1]) == flat(runs[0]) and flat(runs[2]) == flat(runs[0])
        _compare(name, d, runs[0], ref)
        # rule 11 on the device, out of place: the lookup on d_app_out returns d_entry_out at every position
        assert np.array_equal(d.lookups(d.d_app_out), runs[0]["entry"])
        # the map, its header and its table (probed by every row of the case) are as before
        assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), before))
        ent0 = d.lookups()
        # without the optional outputs: the same entries and statistics, the other arrays untouched
        d.clear_prune_out()
        assert d.prune(outputs=False) == 0
        bare = d.prune_results()
        assert bare["entry"].tobytes() == runs[0]["entry"].tobytes() and bare["stats"].tobytes() == runs[0]["stats"].tobytes() and bare["tails_kept"]
        for k in ("status", "sq", "app", "lm", "fr"):
            assert (np.ascontiguousarray(bare[k]).view(np.int32) == FILL).all(), k
        # in place: the same bytes in the live rows, and the contract again
        d.clear_prune_out()
        assert d.prune(in_place=True) == 0
        inp = d.prune_results(in_place=True)
        for k in ("entry", "status", "sq", "lm", "fr", "stats"):
            assert np.ascontiguousarray(inp[k]).tobytes() == np.ascontiguousarray(runs[0][k]).tobytes(), k
        _compare(name, d, inp, ref, in_place=True)
        assert np.array_equal(d.lookups(), runs[0]["entry"])
        d.restore_rows()
        assert np.array_equal(d.lookups(), ent0) and all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), before))
        # the host form (its n_max is the longest frame; rows it does not know are NOT_LIVE there and MISS here)
        h = d.m.prune(d.cam, _live_frames(c), c["poses"], **c["params"])
        cap = h["entry"].shape[1]
        for f, (_, a) in enumerate(_live_frames(c)):
            n = len(a)
            assert h["entry"][f, :n].tobytes() == runs[0]["entry"][f, :n].tobytes() and h["status"][f, :n].tobytes() == runs[0]["status"][f, :n].tobytes()
            assert h["sq"][f, :n].tobytes() == runs[0]["sq"][f, :n].tobytes() and h["frames"][f][1].tobytes() == runs[0]["app"][f, :n].tobytes()
            assert (h["status"][f, n:cap] == Q.NOT_LIVE).all()
        assert h["landmarks"].tobytes() == runs[0]["lm"].tobytes() and h["frame_records"].tobytes() == runs[0]["fr"].tobytes()
        hs, ds = h["stats"], d.pstats(runs[0]["stats"])
        assert {k: v for k, v in hs.items() if k != "by_status"} == {k: v for k, v in ds.items() if k != "by_status"}
        assert hs["by_status"][0] == ds["by_status"][0] and hs["by_status"][3:] == ds["by_status"][3:]
    finally:
        d.close()


@pytest.mark.parametrize("name", ["lists", "duplicates", "duplicates_not_unique", "corners", "guards", "layout", "example"])
def test_guards_off_idempotent_batched_is_single_and_the_bits_of_the_cull(vo, ctx, name):
    c = Pc.case(name)
    ref = Pc.reference(name, **OFF)
    d = PruneDev(vo, ctx, c)
    try:
        d.clear_prune_out()
        assert d.prune(**OFF) == 0, ctx.lib.vo_last_error()
        a = d.prune_results()
        _compare(name, d, a, ref)
        max_err = c["params"]["max_err_px"]
        # ---- the same bits as the cull: a dry run on the rows that went out ----
        ent, cst = d.cull_dry(d.d_app_out, max_err)
        kept = a["entry"] >= 0
        seen = np.nonzero(ent["n_obs"] > 0)[0]
        assert set(seen) == set(np.unique(a["entry"][kept])) and cst["n_obs"] == int(kept.sum())
        mx = np.zeros(d.M)
        np.maximum.at(mx, a["entry"][kept], a["sq"][kept])
        assert mx[seen].tobytes() == ent["max_sq_px"][seen].tobytes()               # bit for bit
        assert np.array_equal(ent["n_obs"], np.bincount(a["entry"][kept], minlength=d.M))
        # the call has no z output: the cull's min_z of the rows that went out is held to the restatement's z of the kept rows, within
        # twice the a-priori bound dz of the largest of them (a minimum of values that each lie within their own bound)
        zmin, zb = np.full(d.M, np.inf), np.zeros(d.M)
        np.minimum.at(zmin, a["entry"][kept], ref["z"][kept])
        np.maximum.at(zb, a["entry"][kept], ref["b_z"][kept])
        assert (np.abs(ent["min_z"][seen] - zmin[seen]) <= 2 * zb[seen]).all() and (ent["min_z"][seen] > 0).all()
        assert not np.isin(ent["verdict"][seen], (4, 5, 6)).any()                   # NOT_FINITE, BEHIND, HIGH_ERROR
        # ---- a second call on the rows that went out prunes nothing ----
        d.ctx.h2d(d.d_app, a["app"])
        d.clear_prune_out()
        assert d.prune(**OFF) == 0
        b = d.prune_results()
        assert d.pstats(b["stats"])["n_pruned"] == 0 and np.array_equal(b["entry"], a["entry"])
        live = d.live
        assert b["app"][:, : d.n_max][live].tobytes() == a["app"][:, : d.n_max][live].tobytes()
        d.restore_rows()
        # ---- frame f of the batched call is the single call, bit for bit ----
        frames = [f for f in range(d.F) if (a["status"][f] > Q.MISS).any()][:6] + [0]
        d.clear_prune_out()
        for f in frames:
            assert d.prune_one(f, **OFF) == 0, ctx.lib.vo_last_error()
        s = d.prune_results()
        for f in frames:
            for k in ("entry", "status", "sq"):
                assert s[k][f].tobytes() == a[k][f].tobytes(), (name, f, k)
            assert s["app"][f, : d.n_max][live[f]].tobytes() == a["app"][f, : d.n_max][live[f]].tobytes()
    finally:
        d.close()


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c = Pc.case("lists_guarded")
    d = PruneDev(vo, ctx, c)
    try:
        before = d.map_state()
        d.clear_prune_out()
        assert d.prune() == 0
        eager = flat(d.prune_results())
        g = C.c_void_p()
        d.clear_prune_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.prune()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        for _ in range(2):
            d.clear_prune_out()
            assert lib.vo_graph_launch(g) == 0
            ctx.synchronize()
            r = d.prune_results()
            assert flat(r) == eager and r["tails_kept"]
        assert lib.vo_graph_destroy(g) == 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), before))
        # frames wider than any call has sized: refused inside a capture before anything is enqueued
        big = PruneDev(vo, ctx, c, n_max=4096, m=d.m)
        try:
            big.clear_prune_out()
            assert lib.vo_ctx_begin_capture(ctx.h) == 0
            assert big.prune() == -6 and b"capture" in lib.vo_last_error()
            assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
            if g.value:
                assert lib.vo_graph_destroy(g) == 0
            r = big.prune_results()
            assert all((np.ascontiguousarray(r[k]).view(np.int32) == FILL).all() for k in ("entry", "status", "sq", "app", "lm", "fr", "stats"))
        finally:
            big.close()
    finally:
        d.close()


def test_refusals(vo, ctx):
    d = PruneDev(vo, ctx, Pc.case("guards"))
    try:
        start = d.map_state()
        nan, inf = float("nan"), float("inf")
        d.clear_prune_out()
        for bad in (dict(F=0), dict(F=65536), dict(n_max=-1), dict(uv_stride=1), dict(app_stride=1), dict(K=None), dict(K=np.zeros(9, np.float32)),
                    dict(d_T=None), dict(d_stats=None), dict(d_stats=d.d_pstats + 4), dict(d_uv=None), dict(d_app=None), dict(d_uv=d.d_uv + 4),
                    dict(d_app=d.d_app + 4), dict(prm=None), dict(d_entry=None), dict(max_err_px=-1.0), dict(max_err_px=nan), dict(max_err_px=inf),
                    dict(rel_factor=-1.0), dict(rel_factor=nan), dict(rel_factor=inf), dict(rel_floor_px=-0.5), dict(rel_floor_px=nan),
                    dict(rel_floor_px=inf), dict(rel_min_obs=2), dict(rel_min_obs=-1), dict(max_share_landmark=-1), dict(max_share_landmark=1001),
                    dict(max_share_frame=-1), dict(max_share_frame=1001), dict(unique=2), dict(unique=-1), dict(reserved=1), dict(d_entry=d.d_entry + 2),
                    dict(d_status=d.d_pstatus + 2), dict(d_sq=d.d_sq + 4), dict(d_app_out=d.d_app_out + 4), dict(d_lm=d.d_lm + 4), dict(d_fr=d.d_fr + 4),
                    dict(d_app_out=d.d_app + 40), dict(d_app_out=d.d_app + 40 * d.stride)):
            assert d.prune(**bad) == -1, bad
            assert b"voe_map_prune_batch_dev" in ctx.lib.vo_last_error(), bad
        assert d.prune(m=None) == -1 and b"null map" in ctx.lib.vo_last_error()
        r = d.prune_results()                                 # nothing was written
        assert all((np.ascontiguousarray(r[k]).view(np.int32) == FILL).all() for k in ("entry", "status", "sq", "app", "lm", "fr", "stats"))
        assert d.read(d.d_app, (d.F, d.stride, 10), np.float32).tobytes() == d.app0.tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(d.map_state(), start)) and len(d.m) == d.M
        assert d.prune(max_err_px=0.0, rel_factor=0.0, unique=0) == 0            # all tests off: rule 3 still runs (allowed)
    finally:
        d.close()


@pytest.mark.parametrize("byte", [0xFF, 0xA5])
def test_workspace_poison_in_a_fresh_process(vo, ctx, tmp_path, byte):
    """DESIGN.md 4.20.1's method: every workspace byte is `byte` before the call writes it, in a child that is started fresh (the
    variable is in its environment before the library is loaded; no process that has opened the GPU is replaced); its outputs,
    out of place and in place, are the bytes of this process's unpoisoned calls -- which the tests above hold to the restatement"""
    out = str(tmp_path / "poisoned.npz")
    env = dict(os.environ, VO_WS_POISON="0x%02X" % byte)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "map_prune_dev.py"), out] + POISON_CASES, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert z["poison"][1] == 1
    assert "VO_WS_POISON" not in os.environ
    for name in POISON_CASES:
        d = PruneDev(vo, ctx, Pc.case(name))
        try:
            for mode in (False, True):
                d.clear_prune_out()
                assert d.prune(in_place=mode) == 0
                mine = flat(d.prune_results(in_place=mode))
                d.restore_rows()
                for k, b in mine.items():
                    assert z[f"{name}/{int(mode)}/{k}"].tobytes() == b, (name, mode, k)
        finally:
            d.close()


def test_a_host_bound_above_the_size(vo, ctx):
    """the host's bound of the map's size is 3 above the size (three known rows sent again); launches and layouts
    are sized by it, the kernels read the size itself -- the same bytes as on the twin whose bound is exact"""
    c = Pc.case("guards")
    twin = PruneDev(vo, ctx, c)
    st = map_states.build_slack(vo, ctx, c["map_pts"], c["map_app"], 3)
    d = PruneDev(vo, ctx, c, m=st.m)
    try:
        for x in (twin, d):
            x.clear_prune_out()
            assert x.prune() == 0, ctx.lib.vo_last_error()
        a, b = twin.prune_results(), d.prune_results()
        assert flat(a) == flat(b) and b["tails_kept"]
        _compare("guards", d, b, Pc.reference("guards"))
        st.check_bound()
        p, ap, h = st.content()
        assert p.tobytes() == np.asarray(c["map_pts"], np.float32).tobytes() and ap.tobytes() == np.asarray(c["map_app"], np.float32).tobytes() and h[0] == d.M
    finally:
        d.close(); twin.close(); st.close()


def test_bundle_after_the_prune_on_the_example_data(vo, ctx):
    """the planted faults of 'example' spoil a joint adjustment: with a row behind its camera vox_map_bundle refuses, and its cost
    stays at the start's.  After ONE prune, the refinement of the map (the named landmarks among it) and two bundle rounds, the
    cost per observation is below that of the same steps on the unpruned rows.  Both are device runs; both costs are printed."""
    c = Pc.case("example")
    fixed = [True] + [False] * (len(c["frames"]) - 2) + [True]
    d = PruneDev(vo, ctx, c)
    try:
        h = d.m.prune(d.cam, c["frames"], c["poses"], **c["params"])
        assert h["stats"]["n_pruned"] == 100 and h["stats"]["n_landmarks_at_fault"] == 20 and h["stats"]["n_frames_at_fault"] == 3
        cost = []
        for rows in (h["frames"], c["frames"]):
            d.reset()
            d.m.refine(d.cam, rows, c["poses"], n_rounds=5, min_obs=3)
            _, _, _, _, s = d.m.bundle(d.cam, rows, c["poses"], fixed, n_rounds=2)
            cost.append((s["status"], s["cost_before"] / max(s["n_obs"], 1), s["cost_after"] / max(s["n_obs"], 1), s["n_obs"]))
        print("vox_map_bundle, 2 rounds after vo_map_refine: on the pruned rows status %d, %.6g -> %.6g px^2 per observation over %d; on the unpruned rows "
              "status %d, %.6g -> %.6g over %d" % (cost[0] + cost[1]))
        assert cost[0][0] == 0 and cost[0][2] < cost[1][2]
    finally:
        d.close()


def test_prune_map_app_on_the_example_data():
    """apps/bin/prune_map checks itself: exit 0 iff the pruned rows are exactly the planted ones (that sit on no named landmark or
    frame), the named landmarks exactly the pushed ones and the named frames exactly the pushed ones"""
    exe = os.path.join(ROOT, "apps", "bin", "prune_map")
    assert os.path.exists(exe), "apps/bin/prune_map is missing: build() makes it"
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "example_data", "data")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert "the pruned rows are exactly those" in r.stdout and "named 20 landmarks and 3 frames" in r.stdout
