"""vo_refine_transform[_dev] on the GPU: parity with the float64 restatement (tests/epi_refine_restatement.py), bit identity
across tile edges, live counts, repeated calls and the mask, refusals and fallbacks, host form against device form, and the
opt-in paths of SequencePipeline and vo_complete."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import epi_refine_restatement as E
import ransac_restatement as R
from oracle import vo_pipeline as vp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
DATA = os.path.join(ROOT, "tests", "golden", "example_data", "data")
# what the project holds the linear initialisation to against its oracle (tests/test_gpu_known_answers.py,
# tests/test_gpu_fullsize.py): rotation angle, translation direction (rad)
TOL_ROT, TOL_DIR = 2e-5, 5e-5
# both sides sum in double: what is left is the rounding of the 16 floats written (entries <= 1: an ulp is 1.2e-7 at most)
TOL_ENTRY = 1e-6
# costs: sums of <= 2000 terms in double on both sides, each term exact to ~1e-12 relative (the cancellation in x1^T F x2)
TOL_COST = 1e-9
N_CAP = 2304


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _K(K):
    return np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()


def dev_call(vo, ctx, K, pairs, p1, p2, X, n_rounds=10, huber_px=0.0, n_max=None, n_live=None, mask=None, x_on_device=False):
    """vo_refine_transform_dev from device copies: (return code, the 64 bytes of d_X_out, the 40 bytes of d_stats).  n_max: the
    capacity (the pairs are padded with (0, 0)); n_live: *d_n_pairs; mask: one flag per position; x_on_device: the start
    pose through d_X_in.  The outputs start as 0xEE bytes: what no kernel wrote shows."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n_max = len(pairs) if n_max is None else n_max
    buf = np.zeros((max(n_max, 1), 2), np.int32)
    buf[: min(len(pairs), n_max)] = pairs[:n_max]
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    Xc = np.ascontiguousarray(np.asarray(X, np.float32).reshape(4, 4).T).ravel()
    m = None
    if mask is not None:
        m = np.zeros(max(n_max, 8), np.uint8)
        m[: len(mask)] = np.asarray(mask, np.uint8)[:n_max]
    ds = [ctx.to_device(buf), ctx.to_device(p1), ctx.to_device(p2), ctx.to_device(np.full(104, 0xEE, np.uint8)),
          ctx.to_device(np.array([n_live if n_live is not None else 0, 0], np.int32)), ctx.to_device(Xc)]
    if m is not None:
        ds.append(ctx.to_device(m))
    try:
        prm = vo.EpiRefineParams(n_rounds, huber_px)
        rc = ctx.lib.vo_refine_transform_dev(
            ctx.h, _p(_K(K)), C.c_void_p(ds[0]), C.c_int(n_max), C.c_void_p(ds[4]) if n_live is not None else None,
            C.c_void_p(ds[6]) if m is not None else None, C.c_void_p(ds[1]), C.c_int(len(p1)), C.c_void_p(ds[2]), C.c_int(len(p2)),
            None if x_on_device else _p(Xc), C.c_void_p(ds[5]) if x_on_device else None, C.byref(prm), C.c_void_p(ds[3]),
            C.c_void_p(ds[3] + 64))
        out = np.zeros(104, np.uint8)
        ctx.d2h(out, ds[3])
        return rc, out[:64].tobytes(), out[64:].tobytes()
    finally:
        for d in ds:
            ctx.free(d)


def _pose(b):
    return np.frombuffer(b, np.float32).reshape(4, 4).T.copy()


def _stats(vo, b):
    return vo.EpiRefineStats.from_buffer_copy(b).as_dict()


def _bits(X):
    return np.ascontiguousarray(np.asarray(X, np.float32).reshape(4, 4).T).tobytes()


@pytest.fixture(scope="module")
def noisy(vo, ctx):
    fp = vo.synth.frame_pair(2000, seed=2000, noise_px=0.5)
    X_lin = vo.estimate_transform(fp["K"], fp["gt_matches"], fp["ref_pts"], fp["cur_pts"], ctx=ctx)
    return fp, X_lin


@pytest.mark.parametrize("case", ["true pairs", "30% mismatched, huber 1 px"])
def test_parity_with_the_restatement(vo, ctx, noisy, case):
    """Both cases run the host form and the restatement from the same start pose.  The first starts from the linear fit of the
    true pairs.  The second -- 30 % of the second indices replaced, huber_px = 1 over ALL pairs -- does NOT start from the
    linear fit of its own pairs, which 30 % mismatches leave useless, but from the pose
    vo_estimate_transform_ransac gives for them: the start a caller would have.  Parity is what is checked here, not the
    gain: the Huber weight alone does not make gross mismatches harmless."""
    fp, X0 = noisy
    pairs, huber = fp["gt_matches"], 0.0
    if case != "true pairs":
        pairs, _ = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), 0.3)
        huber = 1.0
        X0 = vo.estimate_transform_ransac(fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], 1.0, 2048, 0, ctx=ctx)[0]
    X, st = vo.refine_transform(fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], X0, 10, huber, ctx=ctx)
    Xr, sr = E.refine_transform(fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], X0, 10, huber)
    for k in ("status", "rounds", "n_used", "n_skipped", "n_bad"):
        assert st[k] == sr[k], (k, st, sr)
    e_rot, e_dir = E.pose_errors(X, Xr)
    d = float(np.abs(X.astype(np.float64) - np.asarray(Xr, np.float64)).max())
    c0 = abs(st["cost_before"] - sr["cost_before"]) / sr["cost_before"]
    c1 = abs(st["cost_after"] - sr["cost_after"]) / sr["cost_after"]
    print("%s: status %s, cost %.6g -> %.6g; against the restatement: rotation %.3g rad, direction %.3g rad, max entry %.3g, "
          "cost rel. %.3g / %.3g" % (case, E.STATUS_NAMES[st["status"]], st["cost_before"], st["cost_after"], e_rot, e_dir, d, c0, c1))
    assert st["status"] == E.OK and st["cost_after"] < st["cost_before"]
    assert e_rot <= TOL_ROT and e_dir <= TOL_DIR and d <= TOL_ENTRY
    assert c0 <= TOL_COST and c1 <= TOL_COST
    tn = np.linalg.norm(X0[:3, 3].astype(np.float64))
    assert abs(np.linalg.norm(X[:3, 3].astype(np.float64)) - tn) <= 2e-7 * tn                 # |t| kept, to the output's rounding


@pytest.fixture(scope="module")
def tiles(vo, ctx):
    fp = vo.synth.frame_pair(N_CAP, seed=2001, noise_px=0.5)
    X_lin = vo.estimate_transform(fp["K"], fp["gt_matches"], fp["ref_pts"], fp["cur_pts"], ctx=ctx)
    return fp, X_lin


@pytest.mark.parametrize("live", [8, 9, 255, 256, 257, 1023, 1024, 1025, 2304])
def test_tile_edges_and_liveness(vo, ctx, tiles, live):
    fp, X0 = tiles
    pairs, p1, p2 = fp["gt_matches"], fp["ref_pts"], fp["cur_pts"]
    assert len(pairs) == N_CAP
    a = dev_call(vo, ctx, fp["K"], pairs, p1, p2, X0, n_max=N_CAP, n_live=live)
    assert a[0] == 0 and _stats(vo, a[2])["status"] == E.OK and _stats(vo, a[2])["n_used"] == live and a[1] != _bits(X0)
    # the capacity does not enter: the same pairs with n_max = the live count
    assert dev_call(vo, ctx, fp["K"], pairs[:live], p1, p2, X0) == a
    # the same call again
    assert dev_call(vo, ctx, fp["K"], pairs, p1, p2, X0, n_max=N_CAP, n_live=live) == a
    # a mask of every second pair == those pairs at their positions, the others skipped through a NaN pixel
    mask = (np.arange(N_CAP) % 2 == 0).astype(np.uint8)
    m = dev_call(vo, ctx, fp["K"], pairs, p1, p2, X0, n_max=N_CAP, n_live=live, mask=mask)
    p2n = np.concatenate([p2, np.full((1, 2), np.nan, np.float32)])
    holes = pairs.copy()
    holes[1::2, 1] = len(p2)
    h = dev_call(vo, ctx, fp["K"], holes, p1, p2n, X0, n_max=N_CAP, n_live=live)
    sm = _stats(vo, m[2])
    assert m == h and sm["n_used"] == (live + 1) // 2 and sm["n_skipped"] == live // 2 and sm["n_bad"] == 0
    assert sm["status"] == (E.OK if (live + 1) // 2 >= 8 else E.FEW_PAIRS)


def test_refusals_and_fallbacks(vo, ctx, noisy):
    fp, X0 = noisy
    pairs, p1, p2 = fp["gt_matches"], fp["ref_pts"], fp["cur_pts"]
    rc, X, st = dev_call(vo, ctx, fp["K"], pairs, p1, p2, X0, n_max=300, n_live=7)
    s = _stats(vo, st)
    assert rc == 0 and s["status"] == E.FEW_PAIRS and s["n_used"] == 7 and s["rounds"] == 0 and X == _bits(X0)
    wild = pairs[:600].copy()
    wild[[17, 300], 1] = [len(p2), len(p2) + 5]                     # caught by the index check, never loaded
    wild[555, 0] = -1
    rc, X, st = dev_call(vo, ctx, fp["K"], wild, p1, p2, X0)
    s = _stats(vo, st)
    assert rc == 0 and s["status"] == E.BAD_INDEX and s["n_bad"] == 3 and s["n_used"] == 597 and X == _bits(X0)
    Z = X0.copy()
    Z[:3, 3] = 0
    for on_dev in (False, True):
        rc, X, st = dev_call(vo, ctx, fp["K"], pairs, p1, p2, Z, x_on_device=on_dev)
        s = _stats(vo, st)
        assert rc == 0 and s["status"] == E.BAD_INPUT and s["n_used"] == 0 and s["n_skipped"] == len(pairs) and X == _bits(Z)
    # a pose half a radian off: a lower cost, or the input's bits
    B = X0.copy()
    B[:3, :3] = (vo.synth.rodrigues([1.0, -2.0, 0.5], 0.5) @ X0[:3, :3].astype(np.float64)).astype(np.float32)
    rc, X, st = dev_call(vo, ctx, fp["K"], pairs, p1, p2, B, n_rounds=3)
    s, sr = _stats(vo, st), E.refine_transform(fp["K"], pairs, p1, p2, B, 3)[1]
    assert rc == 0 and s["status"] == sr["status"] and s["rounds"] == sr["rounds"]
    assert s["cost_after"] <= s["cost_before"] and (s["status"] == E.OK or (s["status"] in (E.COST_ROSE, E.SINGULAR) and X == _bits(B)))
    # parameter errors: refused before anything is launched, the outputs untouched
    for kw in (dict(n_rounds=0), dict(n_rounds=101), dict(huber_px=-1.0), dict(huber_px=float("nan")), dict(huber_px=float("inf"))):
        rc, X, st = dev_call(vo, ctx, fp["K"], pairs, p1, p2, X0, **kw)
        assert rc == -1 and X == b"\xee" * 64 and st == b"\xee" * 40, kw
        assert ctx.lib.vo_last_error()
    # both, or neither, of X_in and d_X_in
    d = [ctx.to_device(np.ascontiguousarray(pairs, np.int32)), ctx.to_device(p1), ctx.to_device(p2), ctx.alloc(128)]
    try:
        prm, Xc = vo.EpiRefineParams(10, 0.0), _bits(X0)
        Xh = np.frombuffer(Xc, np.float32).copy()
        ctx.h2d(d[3], Xh)

        def call(x_host, x_dev):
            return ctx.lib.vo_refine_transform_dev(ctx.h, _p(_K(fp["K"])), C.c_void_p(d[0]), C.c_int(len(pairs)), None, None,
                                                   C.c_void_p(d[1]), C.c_int(len(p1)), C.c_void_p(d[2]), C.c_int(len(p2)), x_host, x_dev,
                                                   C.byref(prm), C.c_void_p(d[3]), C.c_void_p(d[3] + 64))
        assert call(_p(Xh), C.c_void_p(d[3])) == -1 and call(None, None) == -1
        assert call(None, C.c_void_p(d[3])) == 0                  # in place: d_X_out may be d_X_in
        out = np.zeros(16, np.float32)
        ctx.d2h(out, d[3])
        assert out.tobytes() == dev_call(vo, ctx, fp["K"], pairs, p1, p2, X0)[1]
    finally:
        for x in d:
            ctx.free(x)


def test_capture_after_a_sizing_call(vo, noisy):
    """a capture on a context whose workspace no call has sized is refused (the capture stays valid); after one plain call
    the same call is captured, and the replayed graph writes the plain call's bytes"""
    fp, X0 = noisy
    c = vo.Context(0)
    pairs, p1, p2 = np.ascontiguousarray(fp["gt_matches"], np.int32), fp["ref_pts"], fp["cur_pts"]
    d = [c.to_device(pairs), c.to_device(p1), c.to_device(p2), c.to_device(np.full(104, 0xEE, np.uint8))]
    prm = vo.EpiRefineParams(10, 0.0)
    Xh = np.frombuffer(_bits(X0), np.float32).copy()

    def call():
        return c.lib.vo_refine_transform_dev(c.h, _p(_K(fp["K"])), C.c_void_p(d[0]), C.c_int(len(pairs)), None, None, C.c_void_p(d[1]),
                                             C.c_int(len(p1)), C.c_void_p(d[2]), C.c_int(len(p2)), _p(Xh), None, C.byref(prm),
                                             C.c_void_p(d[3]), C.c_void_p(d[3] + 64))

    def captured():
        g = C.c_void_p()
        assert c.lib.vo_ctx_begin_capture(c.h) == 0
        rc = call()
        assert c.lib.vo_ctx_end_capture(c.h, C.byref(g)) in (0, -3)
        return rc, g

    try:
        rc, g = captured()
        assert rc == -6 and b"workspace" in c.lib.vo_last_error()
        if g.value:
            assert c.lib.vo_graph_destroy(g) == 0
        assert call() == 0
        plain = np.zeros(104, np.uint8)
        c.d2h(plain, d[3])
        rc, g = captured()
        assert rc == 0 and g.value
        c.h2d(d[3], np.full(104, 0xEE, np.uint8))
        assert c.lib.vo_graph_launch(g) == 0
        replay = np.zeros(104, np.uint8)
        c.d2h(replay, d[3])
        assert c.lib.vo_graph_destroy(g) == 0
        assert replay.tobytes() == plain.tobytes() and _stats(vo, plain[64:].tobytes())["status"] == E.OK
    finally:
        for x in d:
            c.free(x)
        c.close()


def test_host_form_equals_device_form(vo, ctx, noisy):
    fp, X0 = noisy
    pairs, p1, p2 = fp["gt_matches"], fp["ref_pts"], fp["cur_pts"]
    mask = np.random.default_rng(3).uniform(size=len(pairs)) < 0.7
    for m, huber in ((None, 0.0), (mask, 1.0)):
        X, st = vo.refine_transform(fp["K"], pairs, p1, p2, X0, 10, huber, mask=m, ctx=ctx)
        rc, Xd, sd = dev_call(vo, ctx, fp["K"], pairs, p1, p2, X0, huber_px=huber, mask=m)
        assert rc == 0 and _bits(X) == Xd and st == _stats(vo, sd) and st["status"] == E.OK
        rc, Xd2, sd2 = dev_call(vo, ctx, fp["K"], pairs, p1, p2, X0, huber_px=huber, mask=m, x_on_device=True)
        assert rc == 0 and (Xd2, sd2) == (Xd, sd)


def _example_sequence():
    files = sorted(f for f in os.listdir(DATA) if re.search(r"^meas-\d.*\.dat$", f))
    K, H, ints = vp.read_camera(os.path.join(DATA, "camera.dat"))
    frames = []
    for f in files:
        pts, app = vp.read_meas(os.path.join(DATA, f))[:2]
        frames.append(dict(pts=np.asarray(pts, np.float32).reshape(-1, 2), app=np.asarray(app, np.float32).reshape(-1, 10)))
    return dict(K=K, rows=ints["height"], cols=ints["width"], z_near=ints["z_near"], z_far=ints["z_far"], frames=frames), H


PLAIN_CHAIN_SHA256 = "35d76bcf028c987f254f74f5dec7468dd3b07de62e803c2b58d5585eb7613273"


def test_sequence_pipeline_init_refine(vo, ctx):
    """The example data through SequencePipeline with and without init_refine (and behind init_ransac).  Without it the
    chain is the parent commit's: sha256 over trajectory().tobytes() + counts().tobytes() of this very run, dumped once
    from a build of the parent commit on an MI355X, = PLAIN_CHAIN_SHA256 above."""
    seq, H = _example_sequence()
    runs = {}
    for name, kw in (("plain", {}), ("refine", dict(init_refine=dict(n_rounds=10, huber_px=1.0))),
                     ("ransac+refine", dict(init_ransac={}, init_refine={}))):
        sp = vo.SequencePipeline(ctx, seq, n_iters=100, **kw)
        sp.run()
        runs[name] = (sp.trajectory(), sp.counts(), sp.refine_stats() if kw else None)
        sp.close()
    T, c, _ = runs["plain"]
    for name in ("refine", "ransac+refine"):
        Tr, cr, st = runs[name]
        assert Tr.shape == T.shape == (121, 4, 4) and np.isfinite(Tr).all()
        d = float(np.abs(Tr[1].astype(np.float64) - T[1]).max())
        print(name, st, "first pose moved by", d)
        assert st["status"] == E.OK and st["n_used"] == c[1, 0] and st["cost_after"] <= st["cost_before"]
        assert d <= 1e-5                                            # noise-free data: the bound of the CPU test
        assert np.array_equal(cr[:, 0], c[:, 0])                     # the matches do not depend on the pose
        # the evaluation's scale inside the interval tests/test_gpu_vo_complete.py holds the plain run to.  gt_errors(...,
        # up_to_scale=True) restates evaluate.cpp:40-60: the median over all frames of |t_est| / |t_gt| of the relative robot
        # motions, inverted -- the "ratio used for map correction" the evaluate binary prints (which
        # test_vo_complete_refine_init_flag below runs on the files vo_complete --refine-init writes)
        scale = vp.gt_errors(DATA, list(Tr), H, up_to_scale=True)[1]
        assert abs(scale - 0.47337) < 0.015 * 0.47337, scale
    assert hashlib.sha256(T.tobytes() + c.tobytes()).hexdigest() == PLAIN_CHAIN_SHA256


def _run_vo_complete(out_dir, *flags):
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run([os.path.join(BIN, "vo_complete"), DATA, str(out_dir), *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "refine-init: status 0, 10 rounds" in r.stdout, r.stdout[:500]
    return {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def test_vo_complete_refine_init_flag(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s"])
    for flags in (["--refine-init"], ["--refine-init=0", "--ransac"]):
        a = _run_vo_complete(tmp_path / ("fbf" + "".join(flags)), *flags)
        b = _run_vo_complete(tmp_path / ("res" + "".join(flags)), *flags, "--resident")
        assert len(a) >= 6 and a["trajectory_est_data.txt"] == b["trajectory_est_data.txt"], flags
        assert a == b, flags
    # `evaluate` on the --refine-init run: the interval tests/test_gpu_vo_complete.py holds the plain run to
    e = subprocess.run([os.path.join(BIN, "evaluate"), DATA, str(tmp_path / "fbf--refine-init")], capture_output=True, text=True, timeout=60)
    assert e.returncode == 0, e.stdout + e.stderr
    val = {k: float(v) for k, v in re.findall(r"^(.*?):\s*([-0-9.e+]+)", e.stdout, flags=re.M)}
    print("evaluate:", val)
    assert abs(val["ratio used for map correction"] - 0.47337) < 0.015 * 0.47337
    r = subprocess.run([os.path.join(BIN, "vo_complete"), DATA, str(tmp_path), "--refine-init=-1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "huber_px" in r.stdout
