"""vo_estimate_pose_ransac[_dev] on the GPU: scoring against the float64 restatement (tests/pose_ransac_restatement.py), the
solve that follows it against the same solve on host-compacted pairs, recovery from mismatched pairs, the fallbacks, the
_dev form's semantics (determinism, live count, graph capture), refusals, and the opt-in paths of vo_complete,
DeviceSequence and SequencePipeline."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_ransac_restatement as P
from ransac_dev import CAM, Dev, _K, _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
DATA = os.path.join(ROOT, "tests", "golden", "example_data", "data")
TOL_ROT, TOL_T = 1e-3, 5e-3            # as tests/test_pose_ransac_cpu.py
THR_PX = 2.0


def _problem(vo, n, frac, seed=2001, big=True):
    kw = dict(max_angle=0.3, max_t=0.5) if big else {}
    return P.tracking_problem(vo, n, seed=seed, noise_px=0.5, frac=frac, **kw)


def test_scoring_matches_restatement(vo, ctx):
    fp, world, meas, pairs, bad, clean = _problem(vo, 2000, 0.4)
    d = Dev(vo, ctx, fp["K"], world, meas, pairs)
    try:
        assert d.call() == 0, ctx.lib.vo_last_error()
        T, inl, nin, mask, counts, st = d.results()
        ref, win, ref_mask, T_ref = P.ransac(fp["K"], world, meas, pairs, THR_PX, 2048, 0, *CAM)
        assert st == 0
        assert np.array_equal(counts < 0, ref < 0)                           # invalid hypotheses agree
        ok = np.abs(counts.astype(np.int64) - ref) <= 2
        assert ok.mean() >= 0.99, (ok.mean(), np.abs(counts - ref).max())
        assert nin == counts.max() == int(mask.sum()) and abs(int(counts.max()) - int(ref.max())) <= 2
        assert np.array_equal(inl, pairs[mask.astype(bool)])                 # compacted in their original order
        # n = 4: every hypothesis draws the same four pairs (in its own order) -- the invalid ones agree there too
        d4 = Dev(vo, ctx, fp["K"], world, meas, clean[:4])
        assert d4.call() == 0
        counts4 = d4.results()[4]
        d4.close()
        assert np.array_equal(counts4 < 0, P.ransac(fp["K"], world, meas, clean[:4], THR_PX, 2048, 0, *CAM)[0] < 0)
    finally:
        d.close()


def test_solve_after_it_equals_solve_on_host_compacted_pairs(vo, ctx):
    fp, world, meas, pairs, bad, clean = _problem(vo, 2000, 0.4, seed=7)
    d = Dev(vo, ctx, fp["K"], world, meas, pairs, n_max=2300)
    try:
        assert d.call() == 0
        T_win, inl, nin, mask, counts, st = d.results()
        assert st == 0 and nin >= 6
        a = d.solve(d.d_T, d.d_inl, d.d_nin)
        b = d.solve_host_pairs(T_win, pairs[mask[: len(pairs)].astype(bool)])
        assert a.tobytes() == b.tobytes()
    finally:
        d.close()


@pytest.mark.parametrize("n,frac", [(2000, 0.4), (50000, 0.3)])
def test_outlier_recovery(vo, ctx, n, frac):
    fp, world, meas, pairs, bad, clean = _problem(vo, n, frac)
    d = Dev(vo, ctx, fp["K"], world, meas, pairs)
    try:
        T_clean = d.solve_host_pairs(np.eye(4), clean).reshape(4, 4).T
        assert P.pose_errors(T_clean, fp["X_gt"])[0] < 1e-3
        assert d.call() == 0
        T_win, inl, nin, mask, counts, st = d.results()
        m = mask[: len(pairs)].astype(bool)
        assert st == 0 and (~bad[m]).mean() >= 0.99 and nin == m.sum()
        T = d.solve(d.d_T, d.d_inl, d.d_nin).reshape(4, 4).T
        e = P.pose_errors(T, T_clean)
        assert e[0] < TOL_ROT and e[1] < TOL_T, e
        T_plain = d.solve(d.d_I, d.d_pairs, d.d_n).reshape(4, 4).T          # vo_picp_solve from the identity on every pair
        e_plain = P.pose_errors(T_plain, T_clean)
        assert e_plain[0] > TOL_ROT or e_plain[1] > TOL_T, e_plain
    finally:
        d.close()


def test_fallbacks_are_the_plain_frame(vo, ctx):
    fp, world, meas, pairs, bad, clean = _problem(vo, 500, 0.2, seed=3, big=False)
    d = Dev(vo, ctx, fp["K"], world, meas, pairs)
    try:
        plain = d.solve(d.d_I, d.d_pairs, d.d_n)
        # (1) fewer than 4 live pairs
        d.set_live(3)
        assert d.call() == 0
        T, inl, nin, mask, counts, st = d.results()
        assert st == 1 and nin == 3 and np.array_equal(inl, pairs[:3]) and np.array_equal(T, np.eye(4)) and (counts == -1).all()
        assert mask[:3].all() and not mask[3:].any()
        assert d.solve(d.d_T, d.d_inl, d.d_nin).tobytes() == d.solve(d.d_I, d.d_pairs, d.d_n).tobytes()
        d.set_live(d.n)
        # (3) a winner with fewer than 6 inliers: a threshold nothing passes
        assert d.call(thr=1e-6) == 0
        T, inl, nin, mask, counts, st = d.results()
        assert st == 3 and nin == d.n and np.array_equal(inl, pairs) and np.array_equal(T, np.eye(4))
        assert d.solve(d.d_T, d.d_inl, d.d_nin).tobytes() == plain.tobytes()
    finally:
        d.close()
    # (4) a bad index: the code, and the plain frame (whose solver drops that pair itself)
    wild = pairs.copy()
    wild[17, 1] = len(world) + 5
    d = Dev(vo, ctx, fp["K"], world, meas, wild)
    try:
        plain = d.solve(d.d_I, d.d_pairs, d.d_n, bad_index=True)
        assert d.call() == 0
        T, inl, nin, mask, counts, st = d.results()
        assert st == 4 and nin == d.n and np.array_equal(inl, wild) and np.array_equal(T, np.eye(4))
        assert d.solve(d.d_T, d.d_inl, d.d_nin, bad_index=True).tobytes() == plain.tobytes()
    finally:
        d.close()
    # (2) no valid hypothesis: every world point the same (a degenerate triangle in every sample)
    same = np.tile(world[:1], (len(world), 1))
    d = Dev(vo, ctx, fp["K"], same, meas, pairs)
    try:
        plain = d.solve(d.d_I, d.d_pairs, d.d_n)
        assert d.call(n_hyp=256) == 0
        T, inl, nin, mask, counts, st = d.results(256)
        assert st == 2 and (counts == -1).all() and nin == d.n and np.array_equal(T, np.eye(4))
        assert d.solve(d.d_T, d.d_inl, d.d_nin).tobytes() == plain.tobytes()
    finally:
        d.close()


def test_determinism_live_count_and_capture(vo, ctx):
    fp, world, meas, pairs, bad, clean = _problem(vo, 2000, 0.3, seed=11)
    d = Dev(vo, ctx, fp["K"], world, meas, pairs, n_max=2048)
    try:
        assert d.call(seed=99) == 0
        a = d.results()
        assert d.call(seed=99) == 0
        b = d.results()
        assert a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[1:5], b[1:5])) and a[5] == b[5] == 0
        assert d.call(seed=100) == 0
        assert not np.array_equal(a[4], d.results()[4])                     # another seed, other samples
        # *d_n = 1500: the pairs beyond are never sampled and get mask 0 -- the call on the first 1500 pairs alone
        d.set_live(1500)
        assert d.call(seed=5) == 0
        live = d.results()
        head = Dev(vo, ctx, fp["K"], world, meas, pairs[:1500])
        assert head.call(seed=5) == 0
        h = head.results()
        head.close()
        assert live[5] == h[5] == 0 and not live[3][1500:].any()
        assert live[0].tobytes() == h[0].tobytes() and np.array_equal(live[1], h[1]) and np.array_equal(live[4], h[4])
        # graph capture of call + solve (the eager run above sized every workspace), replayed
        d.set_live(d.n)
        assert d.call() == 0
        eager = d.solve(d.d_T, d.d_inl, d.d_nin)
        eager_res = d.results()
        ctx.h2d(d.d_T, np.zeros(16, np.float32)); ctx.h2d(d.d_nin, np.zeros(1, np.int32))
        g = C.c_void_p()
        lib = ctx.lib
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.call()
        assert lib.vo_picp_set_pose_dev(d.solver, C.c_void_p(d.d_T)) == 0
        rc2 = lib.vo_picp_solve_dev(d.solver, C.c_void_p(d.d_inl), C.c_int(d.n_max), C.c_void_p(d.d_nin), C.c_int(0), C.c_int(100))
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0 and rc2 == 0, lib.vo_last_error()
        assert lib.vo_graph_launch(g) == 0
        T = np.zeros(16, np.float32)
        assert lib.vo_picp_get_pose(d.solver, _p(T)) == 0
        assert T.tobytes() == eager.tobytes()
        replay = d.results()
        assert replay[0].tobytes() == eager_res[0].tobytes() and replay[2] == eager_res[2]
        assert lib.vo_graph_destroy(g) == 0
        # a capture that would need a bigger workspace is refused, and the capture stays usable
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        assert d.call(n_hyp=65536) == -6 and b"capture" in lib.vo_last_error()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
        if g.value:
            assert lib.vo_graph_destroy(g) == 0
    finally:
        d.close()


def test_refusals(vo):
    c = vo.Context(0)
    lib, h, I = c.lib, c.h, C.c_int
    fp, world, meas, pairs, bad, clean = _problem(vo, 500, 0.2, seed=3, big=False)
    w = np.ascontiguousarray(world, np.float32); m = np.ascontiguousarray(meas, np.float32); K = _K(fp["K"])
    T = np.zeros(16, np.float32); mask = np.zeros(len(pairs), np.uint8); n_in = C.c_int()

    def call(prs=pairs, n=None, prm=(2048, THR_PX, 0), k=K, To=T):
        prs = np.ascontiguousarray(prs, np.int32)
        p = C.byref(vo.RansacParams(*prm)) if prm is not None else None
        return lib.vo_estimate_pose_ransac(h, *map(I, CAM), _p(k) if k is not None else None, _p(w), I(len(w)), _p(m), I(len(m)),
                                           _p(prs), I(len(prs) if n is None else n), p, _p(To) if To is not None else None,
                                           _p(mask), C.byref(n_in))

    assert call() == 0 and n_in.value == mask.sum() >= 6
    T_api, mask_api, n_api = vo.estimate_pose_ransac(fp["K"], *CAM, world, meas, pairs, THR_PX, ctx=c)
    assert n_api == n_in.value and np.array_equal(mask_api, mask.astype(bool)) and T_api.T.ravel().tobytes() == T.tobytes()
    assert call(prm=None) == -1 and call(To=None) == -1 and call(k=None) == -1
    assert call(n=3) == -1 and b"4" in lib.vo_last_error()
    wild = pairs.copy(); wild[17, 1] = len(w) + 3
    assert call(prs=wild) == -5
    wild = pairs.copy(); wild[9, 0] = -1
    assert call(prs=wild) == -5
    for prm in ((0, 1.0, 0), (65537, 1.0, 0), (64, 0.0, 0), (64, -1.0, 0), (64, float("inf"), 0), (64, float("nan"), 0)):
        assert call(prm=prm) == -1, prm
    assert call(prm=(64, 1e-6, 0)) == -1 and b"fewer than 6" in lib.vo_last_error()
    same = np.ascontiguousarray(np.tile(w[:1], (len(w), 1)))
    assert lib.vo_estimate_pose_ransac(h, *map(I, CAM), _p(K), _p(same), I(len(w)), _p(m), I(len(m)), _p(pairs), I(len(pairs)),
                                       C.byref(vo.RansacParams(64, THR_PX, 0)), _p(T), None, None) == -1
    assert b"no valid hypothesis" in lib.vo_last_error()
    g = C.c_void_p()
    assert lib.vo_ctx_begin_capture(h) == 0
    assert call() == -6
    assert lib.vo_ctx_end_capture(h, C.byref(g)) in (0, -3)
    if g.value:
        assert lib.vo_graph_destroy(g) == 0
    assert call() == 0
    c.close()


def _run_vo_complete(out_dir, *flags):
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run([os.path.join(BIN, "vo_complete"), DATA, str(out_dir), *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def _example_sequence():
    from oracle import vo_pipeline as vp
    import re
    files = sorted(f for f in os.listdir(DATA) if re.search(r"^meas-\d.*\.dat$", f))
    K, H, ints = vp.read_camera(os.path.join(DATA, "camera.dat"))
    frames = []
    for f in files:
        pts, app = vp.read_meas(os.path.join(DATA, f))[:2]
        frames.append(dict(pts=np.asarray(pts, np.float32).reshape(-1, 2), app=np.asarray(app, np.float32).reshape(-1, 10)))
    return dict(K=K, rows=ints["height"], cols=ints["width"], z_near=ints["z_near"], z_far=ints["z_far"], frames=frames)


def test_vo_complete_track_ransac_and_pipeline(vo, ctx, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s"])
    a = _run_vo_complete(tmp_path / "fbf", "--track-ransac")
    b = _run_vo_complete(tmp_path / "res", "--track-ransac", "--resident")
    assert len(a) >= 6 and a == b                                            # frame by frame == DeviceSequence, every file
    plain = _run_vo_complete(tmp_path / "plain")
    assert set(plain) == set(a)
    c = _run_vo_complete(tmp_path / "combo", "--track-ransac=1.5", "--ransac", "--exact")
    d = _run_vo_complete(tmp_path / "combo_res", "--track-ransac=1.5", "--ransac", "--exact", "--resident")
    assert c == d
    # SequencePipeline(track_ransac=...) on the same frames: the trajectory of poses_raw.txt
    seq = _example_sequence()
    sp = vo.SequencePipeline(ctx, seq, n_iters=100, track_ransac={})       # the defaults of --track-ransac
    sp.run()
    traj = sp.trajectory()
    st, npairs = sp.track_stats()
    sp.close()
    raw = np.loadtxt(os.path.join(tmp_path / "fbf", "poses_raw.txt"), dtype=np.float64).astype(np.float32).reshape(-1, 4, 4)
    assert raw.shape == traj.shape and raw.tobytes() == traj.tobytes()
    assert st[0] == st[1] == 0 and (st[2:] >= 0).all() and (st[2:] <= 4).all() and (st[2:] == 0).sum() > len(st) // 2
    assert (npairs[2:][st[2:] == 0] >= 6).all()


def test_track_ransac_beats_plain_on_mismatched_matches(vo, ctx):
    """a synthetic sequence in which ~20 % of every frame's appearance rows are swapped with other rows of the same frame, so that
    the matcher pairs those measurements with the wrong landmarks: tracked through the RANSAC, the relative poses follow the
    ground truth more closely than the plain chain's"""
    seq = vo.synth.sequence(seed=3000, n_frames=16, n_visible=600)
    rng = np.random.default_rng(5)
    for f in seq["frames"][1:]:
        k = len(f["app"])
        sel = rng.choice(k, int(0.2 * k) // 2 * 2, replace=False)
        a, b = sel[: len(sel) // 2], sel[len(sel) // 2:]
        app = f["app"].copy()
        app[a], app[b] = f["app"][b], f["app"][a]
        f["app"] = app
    Xgt = vo.synth.sequence_gt_relative(seq)

    def err(traj):
        e = []
        for t in range(2, len(traj)):
            R, Rg = traj[t][:3, :3].astype(np.float64), Xgt[t - 1][:3, :3]
            e.append(np.arccos(np.clip((np.trace(R.T @ Rg) - 1) / 2, -1, 1)))
        return float(np.mean(e))

    out = {}
    for name, opt in (("plain", None), ("track", dict(threshold_px=2.0))):
        sp = vo.SequencePipeline(ctx, seq, n_iters=100, track_ransac=opt)
        sp.run()
        out[name] = sp.trajectory()
        if opt:
            st, npairs = sp.track_stats()
            assert (st[2:] == 0).mean() > 0.9, st
        sp.close()
    assert err(out["track"]) < err(out["plain"]), (err(out["track"]), err(out["plain"]))
