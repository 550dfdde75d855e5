"""vo_map_localise[_dev|_batch_dev] on the GPU: the known answer of the example data (every frame localised from scratch in
the map of world.dat lands on trajectory.dat), the contract (the call equals the explicit sequence of public calls byte for
byte), the fallbacks, capture and replay, refusals, and the application.

Measured on an MI355X (largest absolute entry difference of inv(T) inv(C) to trajectory.dat over the 121 frames, bound 1e-4;
the float64 restatement reaches 4.72e-5): see DESIGN.md section 4.12."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_localise_restatement as M
from map_dev import Localise, same_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
SYNTH_CAM = (480, 640, 0, 10)


@pytest.fixture(scope="module")
def data():
    return M.example_data()


@pytest.fixture(scope="module")
def world_map(vo, ctx, data):
    m = vo.Map(ctx)
    m.update(data["world_pts"], data["world_app"])
    assert len(m) == 1000
    yield m
    m.close()


def _err(T, data, f):
    return float(np.abs(M.robot_pose(T, data["C"]) - data["gt"][f]).max())


def test_known_answer_single_and_batched(vo, ctx, data, world_map):
    cam = vo.Camera(*data["cam"], data["K"])
    frames = [(uv, app) for uv, app, _ in data["frames"]]
    single = []
    for f, (uv, app, ids) in enumerate(data["frames"]):
        pairs, ent = world_map.lookup(app)
        assert np.array_equal(ent, ids) and np.array_equal(pairs, np.stack([np.arange(len(ids)), ids], 1))
        single.append(world_map.localise(cam, uv, app, threshold_px=2.0, n_hypotheses=64, seed=0, kernel_threshold=10000.0, n_iters=50))
    batched = world_map.localise_batch(cam, frames, threshold_px=2.0, n_hypotheses=64, seed=0, kernel_threshold=10000.0, n_iters=50)
    worst_s = worst_b = worst_sb = 0.0
    for f, ((Ts, ss), (Tb, sb)) in enumerate(zip(single, batched)):
        n = len(data["frames"][f][2])
        assert ss["status"] == 0 and sb["status"] == 0, (f, ss, sb)
        assert ss["n_rows"] == sb["n_rows"] == ss["n_hits"] == sb["n_hits"] == n
        assert ss["ransac_status"] == sb["ransac_status"] == 0 and ss["ransac_inliers"] == sb["ransac_inliers"] >= 6
        worst_s, worst_b = max(worst_s, _err(Ts, data, f)), max(worst_b, _err(Tb, data, f))
        worst_sb = max(worst_sb, float(np.abs(Ts.astype(np.float64) - Tb).max()))
    print(f"largest pose difference to trajectory.dat: single {worst_s:.3g}, batched {worst_b:.3g}; single against batched {worst_sb:.3g}")
    assert worst_s < 1e-4 and worst_b < 1e-4
    assert worst_sb < 1e-4                                   # the bound stated between the single and the batched solver


def _three_frames(data):
    sizes = np.array([len(f[2]) for f in data["frames"]])
    pick = [int(np.argmin(sizes)), int(np.argmin(np.abs(sizes - 60))), int(np.argmax(sizes))]
    assert sizes[pick[0]] == 14 and sizes[pick[2]] == 127
    return pick


def _compose(vo, ctx, m, cam, K, frames, n_hyp):
    """single, batched and prior-only forms against the explicit sequences, byte for byte; returns the poses found"""
    d = Localise(vo, ctx, cam, K, frames)
    found = []
    try:
        d.clear_out()
        for f in range(d.F):
            assert d.single(m, f, n_hyp=n_hyp) == 0, ctx.lib.vo_last_error()
        T, raw = d.results()
        for f in range(d.F):
            Te, want = d.explicit_single(m, f, n_hyp=n_hyp)
            got = d.stats(raw[f])
            assert got["status"] == 0, got
            same_stats(got, want)
            assert T[f].tobytes() == Te.tobytes()
            found.append(T[f].reshape(4, 4).T.copy())
        d.clear_out()
        assert d.batch(m, n_hyp=n_hyp) == 0, ctx.lib.vo_last_error()
        Tb, rawb = d.results()
        Te, want = d.explicit_batch(m, n_hyp=n_hyp)
        for f in range(d.F):
            got = d.stats(rawb[f])
            assert got["status"] == 0, got
            same_stats(got, want[f])
            assert Tb[f].tobytes() == Te[f].tobytes()
            # against the single form: hits and RANSAC bit for bit, the pose within the solvers' 1e-4
            s = d.stats(raw[f])
            assert (got["n_hits"], got["ransac_status"], got["ransac_inliers"]) == (s["n_hits"], s["ransac_status"], s["ransac_inliers"])
            assert np.abs(Tb[f].astype(np.float64) - T[f]).max() < 1e-4
    finally:
        d.close()
    # n_hypotheses == 0: every hit, from the prior (here: the pose just found, moved a little)
    bump = np.eye(4, dtype=np.float32); bump[:3, 3] = (0.01, -0.02, 0.015)
    d = Localise(vo, ctx, cam, K, frames, T0=[bump @ T for T in found])
    try:
        d.clear_out()
        for f in range(d.F):
            assert d.single(m, f, n_hyp=0) == 0, ctx.lib.vo_last_error()
        T, raw = d.results()
        for f in range(d.F):
            Te, want = d.explicit_single(m, f, n_hyp=0)
            got = d.stats(raw[f])
            assert got["status"] == 0 and got["ransac_status"] == 0 and got["ransac_inliers"] == got["n_hits"], got
            same_stats(got, want)
            assert T[f].tobytes() == Te.tobytes()
        d.clear_out()
        assert d.batch(m, n_hyp=0) == 0, ctx.lib.vo_last_error()
        Tb, rawb = d.results()
        Te, want = d.explicit_batch(m, n_hyp=0)
        for f in range(d.F):
            same_stats(d.stats(rawb[f]), want[f])
            assert Tb[f].tobytes() == Te[f].tobytes()
    finally:
        d.close()
    return found


def test_composition_on_three_example_frames(vo, ctx, data, world_map):
    pick = _three_frames(data)
    frames = [data["frames"][f][:2] for f in pick]
    found = _compose(vo, ctx, world_map, data["cam"], data["K"], frames, 64)
    for f, T in zip(pick, found):
        assert _err(T, data, f) < 1e-4


def test_composition_on_a_synthetic_frame_with_swapped_rows(vo, ctx):
    """the model of synth.frame_pair(2000, noise_px=0.5) is the map; 30 % of the current image's appearance rows are swapped
    among themselves, so that 30 % of the hits name another landmark"""
    fp = vo.synth.frame_pair(2000, noise_px=0.5)
    assert np.array_equal(fp["model_pairs"][:, 0], fp["model_pairs"][:, 1])
    m = vo.Map(ctx)
    try:
        m.update(fp["model"], fp["ref_app"])
        app = fp["cur_app"].copy()
        rng = np.random.default_rng(9)
        idx = rng.permutation(len(app))[: int(0.3 * len(app))]
        app[idx] = app[np.roll(idx, 1)]
        found = _compose(vo, ctx, m, SYNTH_CAM, fp["K"], [(fp["cur_pts"], app), (fp["cur_pts"][:700], app[:700])], 256)
        X = fp["X_gt"].astype(np.float64)
        for T in found:
            assert np.abs(T[:3, :3] - X[:3, :3]).max() < 2e-3 and np.abs(T[:3, 3] - X[:3, 3]).max() < 2e-2
    finally:
        m.close()


def test_fallbacks(vo, ctx, data, world_map):
    cam = vo.Camera(*data["cam"], data["K"])
    rng = np.random.default_rng(2)
    uv, app, ids = data["frames"][60]
    assert len(ids) >= 40
    T0 = rng.uniform(-2, 2, (4, 4)).astype(np.float32)                       # any bits: they must come back as they are
    I4 = np.eye(4, dtype=np.float32)

    def lost(n_keep):
        a = rng.uniform(-1, 1, app.shape).astype(np.float32)
        a[:n_keep] = app[:n_keep]
        return a

    # no row of the frame is in the map; exactly 5 hits
    for keep in (0, 5):
        T, s = world_map.localise(cam, uv, lost(keep))
        assert s["status"] == 1 and s["n_hits"] == keep and s["n_rows"] == len(ids) and T.tobytes() == I4.tobytes(), s
        T, s = world_map.localise(cam, uv, lost(keep), T0=T0)
        assert s["status"] == 1 and T.tobytes() == T0.tobytes()
        T, s = world_map.localise(cam, uv, lost(keep), n_hypotheses=0, T0=T0)
        assert s["status"] == 1 and T.tobytes() == T0.tobytes()
    # 6 hits: no longer FEW_MATCHES (the six are exact, the RANSAC keeps them all)
    T, s = world_map.localise(cam, uv, lost(6))
    print("six hits:", s, _err(T, data, 60))
    assert s["n_hits"] == 6 and s["status"] != 1, s
    # min_inliers above what the frame has
    T, s = world_map.localise(cam, uv, app, min_inliers=len(ids) + 1, T0=T0)
    assert s["status"] == 3 and s["num_inliers"] <= len(ids) and T.tobytes() == T0.tobytes(), s
    # a map whose points were scrambled: the hits are there, the geometry is not
    bad = vo.Map(ctx)
    try:
        bad.update(data["world_pts"][rng.permutation(1000)], data["world_app"])
        T, s = bad.localise(cam, uv, app)
        assert s["n_hits"] == len(ids) and s["status"] in (2, 3) and T.tobytes() == I4.tobytes(), s
        T, s = bad.localise(cam, uv, app, T0=T0)
        assert s["status"] in (2, 3) and T.tobytes() == T0.tobytes(), s
    finally:
        bad.close()
    # batched: lost frames leave their neighbours' bytes alone
    A, B, Cc, D = (data["frames"][f][:2] for f in (10, 60, 90, 110))
    n = min(len(x[1]) for x in (A, B, Cc, D))
    cut = lambda fr: (fr[0][:n], fr[1][:n])
    good = world_map.localise_batch(cam, [cut(A), cut(Cc), cut(B), cut(D)])
    mixed = world_map.localise_batch(cam, [cut(A), (Cc[0][:n], rng.uniform(-1, 1, (n, 10))), cut(B), (D[0][:n], lost(5)[:n])],
                                     T0=[T0, T0, T0, T0])
    assert [s["status"] for _, s in good] == [0, 0, 0, 0]
    assert [s["status"] for _, s in mixed] == [0, 1, 0, 1] and [s["n_hits"] for _, s in mixed] == [n, 0, n, 5]
    for f in (0, 2):
        assert mixed[f][0].tobytes() == good[f][0].tobytes() and mixed[f][1] == good[f][1]
    for f in (1, 3):
        assert mixed[f][0].tobytes() == T0.tobytes()


def test_capture_and_replay_of_the_single_device_form(vo, ctx, data, world_map):
    lib = ctx.lib
    pick = _three_frames(data)
    fa, fb = data["frames"][pick[2]], data["frames"][pick[1]]
    d = Localise(vo, ctx, data["cam"], data["K"], [fa[:2]])
    try:
        d.clear_out()
        assert d.single(world_map, 0) == 0
        eager = d.results()
        assert d.stats(eager[1][0])["status"] == 0
        d.clear_out()
        g = C.c_void_p()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.single(world_map, 0)
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        assert lib.vo_graph_launch(g) == 0
        ctx.synchronize()
        replay = d.results()
        assert replay[0].tobytes() == eager[0].tobytes() and replay[1].tobytes() == eager[1].tobytes()
        # another frame in the same buffers, replayed: the answer of an eager call on it
        n = len(fb[2])
        uv = np.zeros((d.n_max, 2), np.float32); app = np.zeros((d.n_max, 10), np.float32)
        uv[:n], app[:n] = fb[0], fb[1]
        ctx.h2d(d.d_uv, uv); ctx.h2d(d.d_app, app); ctx.h2d(d.d_n, np.array([n], np.int32))
        assert lib.vo_graph_launch(g) == 0
        ctx.synchronize()
        replay = d.results()
        assert d.single(world_map, 0) == 0
        again = d.results()
        assert replay[0].tobytes() == again[0].tobytes() and replay[1].tobytes() == again[1].tobytes()
        assert d.stats(replay[1][0])["n_hits"] == n and _err(replay[0][0].reshape(4, 4).T, data, pick[1]) < 1e-4
        assert lib.vo_graph_destroy(g) == 0
        # a bigger frame than any call has sized: refused inside a capture, the context stays usable
        big = Localise(vo, ctx, data["cam"], data["K"], [fa[:2]], n_max=4096)
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        assert big.single(world_map, 0) == -6 and b"capture" in lib.vo_last_error()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
        if g.value:
            assert lib.vo_graph_destroy(g) == 0
        assert big.single(world_map, 0) == 0
        assert big.stats(big.results()[1][0])["status"] == 0 and _err(big.results()[0][0].reshape(4, 4).T, data, pick[2]) < 1e-4
        big.close()
    finally:
        d.close()


def test_refusals(vo, ctx, data, world_map):
    uv, app, ids = data["frames"][0]
    d = Localise(vo, ctx, data["cam"], data["K"], [(uv, app)])
    cam = vo.Camera(*data["cam"], data["K"])
    try:
        assert d.single(world_map, 0) == 0
        assert d.single(world_map, 0, n_iters=0) == -1
        assert d.single(world_map, 0, min_inliers=-1) == -1
        assert d.single(world_map, 0, n_hyp=0) == -1 and b"prior" in ctx.lib.vo_last_error()      # no T0
        assert d.single(world_map, 0, n_hyp=-1) == -1 and d.single(world_map, 0, n_hyp=65537) == -1
        assert d.single(world_map, 0, px=0.0) == -1 and d.single(world_map, 0, px=float("nan")) == -1
        keep = d.K
        d.K = np.zeros(9, np.float32)
        assert d.single(world_map, 0) == -1 and b"singular" in ctx.lib.vo_last_error()
        d.K = keep
        d.F = 0
        assert d.batch(world_map) == -1
        d.F = 65536
        assert d.batch(world_map) == -1
        d.F = 1
        d.stride = d.n_max - 1
        assert d.batch(world_map) == -1
        d.stride = d.n_max
        assert d.batch(world_map) == 0
        with pytest.raises(vo.VoError):
            world_map.localise(cam, uv, app, n_hypotheses=0)
        with pytest.raises(vo.VoError):
            world_map.localise(cam, uv[:0], app[:0])
    finally:
        d.close()


@pytest.mark.parametrize("flags", [(), ("--batch",)])
def test_localise_app_on_the_example_data(tmp_path, flags):
    exe = os.path.join(BIN, "localise")
    assert os.path.exists(exe), "apps/bin/localise is missing: build() makes it"
    r = subprocess.run([exe, M.DATA, str(tmp_path), *flags], capture_output=True, text=True, timeout=120)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "lookup equal to the ids" in r.stdout and "statuses all OK" in r.stdout
    est = np.loadtxt(tmp_path / "trajectory_est.txt")
    gt = np.loadtxt(tmp_path / "trajectory_gt.txt")
    assert est.shape == (121, 3) and np.abs(est[:, :2] - gt[:121, :2]).max() < 1e-4
