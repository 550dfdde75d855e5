"""voe_map_apply_correction* on the device against NumPy in float64: the reference frame of every entry is the frame of the
smallest key f * n_max + i over the lookup's hits (exactly), a moved point is S_new[f]^-1 S_old[f] p, and everything that must
keep its bytes keeps them -- new == old, dry_run, unseen entries, the hash table.

A moved point is asserted to lie within ONE float32 ulp per coordinate of the float64 value rounded, not to equal it: the device
forms S_new^-1 (S_old p) by the adjugate and sums of three products, NumPy by LAPACK's inverse and its own order, so the two
doubles differ in their last bits and round to different float32 neighbours wherever the value lies that close to a midpoint.
How many coordinates are equal is printed."""
import ctypes as C

import numpy as np
import pytest

import map_covis_cases as Vc
import pose_graph_cases as Cc

pytestmark = pytest.mark.gpu


def _scene(name):
    if name == "example":
        c = Vc.example()
        S_old = np.array(c["poses"], np.float32)
    else:
        c = Vc.frame_count(17) if name == "frames17" else Vc.map_size(2049)
        rng = np.random.default_rng(7)
        S_old = np.array([Cc._sim(np.exp(0.1 * rng.standard_normal()), 0.5 * rng.standard_normal(3), rng.standard_normal(3)) for _ in c["frames"]],
                         np.float32)
    rng = np.random.default_rng(11)
    S_new = np.array([Cc._sim(1.0 + 0.002 * f, 0.01 * rng.standard_normal(3), 0.02 * rng.standard_normal(3)) @ S_old[f].astype(np.float64)
                      for f in range(len(S_old))], np.float32)
    S_new[1::4] = S_old[1::4]                                 # every fourth frame is not corrected: its entries keep their bytes
    return c, S_old, S_new


def _fresh(vo, ctx, c):
    m = vo.Map(ctx)
    m.update(c["map_pts"], c["map_app"])
    return m


def _min_keys(m, c):
    """the NumPy side of the reference frame: the lookup per frame, the minimum key per entry"""
    n_max = max(len(a) for _, a in c["frames"])
    key = np.full(len(m), np.iinfo(np.int64).max, np.int64)
    looks = []
    for f, (_, app) in enumerate(c["frames"]):
        pairs, ent = m.lookup(app)[:2]
        looks.append((pairs.copy(), ent.copy()))
        for i, e in enumerate(ent[: len(app)]):
            if e >= 0:
                key[e] = min(key[e], f * n_max + i)
    ref = np.where(key == np.iinfo(np.int64).max, -1, key // n_max).astype(np.int32)
    return ref, looks


def _moved64(p, So, Sn):
    So, Sn = So.astype(np.float64), Sn.astype(np.float64)
    q = So[:3, :3] @ p.astype(np.float64) + So[:3, 3]
    return np.linalg.solve(Sn[:3, :3], q - Sn[:3, 3])


@pytest.mark.parametrize("name", ["frames17", "map2049", "example"])
def test_apply_against_float64(vo, ctx, name):
    c, S_old, S_new = _scene(name)
    m = _fresh(vo, ctx, c)
    try:
        pts0, app0 = (a.copy() for a in m.read())
        ref_np, looks = _min_keys(m, c)
        # dry_run first: outputs as they would be, the map bit for bit
        ref_dry, st_dry = m.apply_correction(c["frames"], S_old, S_new, dry_run=True)
        assert m.read()[0].tobytes() == pts0.tobytes()
        # new == old: nothing moves, the map bit for bit
        ref_same, st_same = m.apply_correction(c["frames"], S_old, S_old)
        assert m.read()[0].tobytes() == pts0.tobytes() and st_same["n_moved"] == 0 and np.array_equal(ref_same, ref_np)
        # the call
        ref, st = m.apply_correction(c["frames"], S_old, S_new)
        pts1, app1 = m.read()
        assert np.array_equal(ref, ref_np) and np.array_equal(ref_dry, ref_np)      # the NumPy minimum key, exactly
        changed = np.array([f >= 0 and S_old[f].tobytes() != S_new[f].tobytes() for f in ref_np])
        assert st == st_dry == dict(n_entries=len(pts0), n_seen=int((ref_np >= 0).sum()), n_moved=int(changed.sum()))
        assert (ref_np < 0).any() or name == "example"          # the hand-made scenes have unseen entries
        assert pts1[~changed].tobytes() == pts0[~changed].tobytes() and app1.tobytes() == app0.tobytes()
        want = np.array([_moved64(pts0[e], S_old[ref_np[e]], S_new[ref_np[e]]) for e in np.nonzero(changed)[0]])
        want32 = want.astype(np.float32)
        ulps = np.abs(pts1[changed].astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
        print(f"{name}: {int(changed.sum())} of {len(pts0)} entries moved, {int((ref_np < 0).sum())} unseen; "
              f"{float((pts1[changed] == want32).mean()):.6f} of the coordinates equal the float64 value rounded, the rest within {ulps.max():.0f} ulp")
        assert ulps.max() <= 1.0
        assert changed.any() and (np.abs(pts1[changed] - pts0[changed]).max() > 1e-4)
        # the hash table still finds every entry: the lookup before and after is byte-equal
        for (pairs, ent), (_, app) in zip(looks, c["frames"]):
            p2, e2 = m.lookup(app)[:2]
            assert p2.tobytes() == pairs.tobytes() and e2.tobytes() == ent.tobytes()
        assert len(m) == len(pts0)
        # three calls from the same start give the same bytes; the device form gives the host form's
        for _ in range(2):
            m.clear()
            m.update(c["map_pts"], c["map_app"])
            r2, s2 = m.apply_correction(c["frames"], S_old, S_new)
            assert m.read()[0].tobytes() == pts1.tobytes() and r2.tobytes() == ref.tobytes() and s2 == st
        m.clear()
        m.update(c["map_pts"], c["map_app"])
        F, n_max = len(c["frames"]), max(len(a) for _, a in c["frames"])
        app = np.zeros((F, n_max, 10), np.float32)
        n = np.zeros(F, np.int32)
        for f, (_, a) in enumerate(c["frames"]):
            app[f, : len(a)], n[f] = a, len(a)
        cm = lambda S: np.ascontiguousarray(S.reshape(-1, 4, 4).transpose(0, 2, 1))
        d = [ctx.to_device(x) for x in (app, n, cm(S_old), cm(S_new))]
        d_ref, d_st = ctx.alloc(4 * len(pts0) + 16), ctx.alloc(16)
        m.apply_correction_batch_dev(F, d[0], n_max, n_max, d[1], d[2], d[3], False, d_ref, d_st)
        ctx.synchronize()
        ref_dev, st_dev = np.zeros(len(pts0), np.int32), np.zeros(4, np.int32)
        ctx.d2h(ref_dev, d_ref)
        ctx.d2h(st_dev, d_st)
        assert m.read()[0].tobytes() == pts1.tobytes() and ref_dev.tobytes() == ref.tobytes()
        assert st_dev.tolist() == [st["n_entries"], st["n_seen"], st["n_moved"], 0]
        for p in d + [d_ref, d_st]:
            ctx.free(p)
    finally:
        m.close() if hasattr(m, "close") else None


def test_projections_in_the_reference_frame_stay_on_the_example_data(vo, ctx):
    """every seen entry's projection in its reference frame, under rigid_pose(S_new), moves by at most what half an ulp of each
    stored coordinate of the moved point can move it: with d the length of the half-ulp vector (a rotation keeps it) and
    (X, Y, Z) the camera point, |du| <= fx d (1 + |X / Z|) / Z and |dv| <= fy d (1 + |Y / Z|) / Z; 1e-9 px on top for the
    float64 arithmetic of the check itself"""
    c, S_old, S_new = _scene("example")
    K = np.asarray(c["K"], np.float64).reshape(3, 3)
    m = _fresh(vo, ctx, c)
    try:
        pts0 = m.read()[0].copy()
        ref, st = m.apply_correction(c["frames"], S_old, S_new)
        pts1 = m.read()[0]
        worst = 0.0
        for e in np.nonzero(ref >= 0)[0]:
            f = ref[e]
            T0, T1 = vo.rigid_pose(S_old[f]), vo.rigid_pose(S_new[f])
            q0 = T0[:3, :3] @ pts0[e].astype(np.float64) + T0[:3, 3]
            q1 = T1[:3, :3] @ pts1[e].astype(np.float64) + T1[:3, 3]
            uv0, uv1 = (K @ q0)[:2] / q0[2], (K @ q1)[:2] / q1[2]
            d = np.linalg.norm(np.spacing(np.abs(pts1[e])).astype(np.float64) / 2)
            bound = np.array([K[0, 0] * d * (1 + abs(q1[0] / q1[2])), K[1, 1] * d * (1 + abs(q1[1] / q1[2]))]) / abs(q1[2]) + 1e-9
            worst = max(worst, float((np.abs(uv1 - uv0) / bound).max()))
            assert np.all(np.abs(uv1 - uv0) <= bound), (int(e), int(f), uv0, uv1, bound)
        print(f"example: {st['n_seen']} seen entries, the worst projection moved by {worst:.3f} of its half-ulp bound")
        assert st["n_seen"] > 400
    finally:
        m.close() if hasattr(m, "close") else None


def test_refusals(vo, ctx):
    c, S_old, S_new = _scene("frames17")
    m = _fresh(vo, ctx, c)
    try:
        d_st = ctx.alloc(16)
        d_S = ctx.to_device(np.zeros((17, 16), np.float32))
        d_app = ctx.to_device(np.zeros((17, 4, 10), np.float32))
        call = lambda **k: m.lib.voe_map_apply_correction_batch_dev(
            m.h, C.c_int(k.get("F", 17)), None, C.c_size_t(4), C.c_void_p(k.get("app", d_app)), C.c_size_t(k.get("stride", 4)), C.c_int(k.get("n_max", 4)),
            None, C.c_void_p(k.get("So", d_S)), C.c_void_p(d_S), C.c_int(0), None, C.c_void_p(k.get("st", d_st)))
        assert call() == 0
        for kw in (dict(F=0), dict(F=65536), dict(n_max=-1), dict(app=None), dict(So=None), dict(st=None), dict(st=d_st + 4), dict(So=d_S + 2),
                   dict(stride=3)):
            assert call(**kw) == -1, kw
        ctx.synchronize()
        for p in (d_st, d_S, d_app):
            ctx.free(p)
    finally:
        m.close() if hasattr(m, "close") else None


def test_close_loop_app_on_the_example_data():
    """apps/bin/close_loop: the drifted example chain, loop edges from the covisibility measured by vo_map_localise, one
    voe_pose_graph call, one voe_map_apply_correction call; exit 0 iff the median camera-centre error falls below a fifth"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "apps", "bin", "close_loop")
    assert os.path.exists(exe), "apps/bin/close_loop is not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([exe, os.path.join(root, "tests", "golden", "example_data", "data")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "the loop is closed" in r.stdout and "status OK" in r.stdout
