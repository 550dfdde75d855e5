"""vo_estimate_transform_ransac[_dev] on the GPU: scoring against the float64 restatement (tests/ransac_restatement.py),
the refit's bit identity with vo_estimate_transform, the all-inlier example data, recovery from mismatched pairs, the
_dev form's semantics, refusals, and the opt-in paths of vo_complete and SequencePipeline."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ransac_restatement as R
from ransac_dev import _p, dev_call as _dev_call
from oracle import vo_pipeline as vp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
DATA = os.path.join(ROOT, "tests", "golden", "example_data", "data")
# tolerances of tests/test_ransac_cpu.py (calibrated there): rotation angle, translation direction (rad)
TOL_ROT, TOL_DIR = 1e-2, 0.25
NOISE_PX, THR_PX = 0.25, 1.0


def _corrupted(vo, n, frac, seed=2000):
    fp = vo.synth.frame_pair(n, seed=seed, noise_px=NOISE_PX)
    pairs, bad = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), frac)
    return fp, pairs, bad


def test_scoring_matches_restatement(vo, ctx):
    fp, pairs, _ = _corrupted(vo, 2000, 0.4)
    rc, X, mask, counts, n_in = _dev_call(vo, ctx, fp["K"], pairs, fp["ref_pts"], fp["cur_pts"])
    assert rc == 0, ctx.lib.vo_last_error()
    ref, win, ref_mask, _ = R.ransac(pairs, fp["ref_pts"], fp["cur_pts"], THR_PX, 2048, 0)
    assert np.array_equal(counts < 0, ref < 0)                               # invalid hypotheses agree
    ok = np.abs(counts.astype(np.int64) - ref) <= 2
    assert ok.mean() >= 0.99, (ok.mean(), np.abs(counts - ref).max())
    assert n_in == counts.max() == int(mask.sum()) and abs(int(counts.max()) - int(ref.max())) <= 2
    # n = 8: some hypotheses cannot find 8 distinct draws in 64 -- the same ones on both sides
    rc, _, _, counts8, _ = _dev_call(vo, ctx, fp["K"], fp["gt_matches"][:8], fp["ref_pts"], fp["cur_pts"])
    idx, valid = R.samples(0, 2048, 8)
    assert rc == 0 and (~valid).sum() > 0 and np.array_equal(counts8 < 0, ~valid)


def test_refit_is_plain_estimate_on_inliers(vo, ctx):
    fp, pairs, _ = _corrupted(vo, 2000, 0.4, seed=7)
    X, mask, n_in = vo.estimate_transform_ransac(fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], THR_PX, 2048, 0, ctx=ctx)
    assert n_in == int(mask.sum()) >= 8
    X_plain = vo.estimate_transform(fp["K"], pairs[mask], fp["ref_pts"], fp["cur_pts"], ctx=ctx)
    assert X.tobytes() == X_plain.tobytes()
    rc, X_dev, mask_dev, _, n_dev = _dev_call(vo, ctx, fp["K"], pairs, fp["ref_pts"], fp["cur_pts"])
    assert rc == 0 and X_dev.tobytes() == X.tobytes() and np.array_equal(mask_dev.astype(bool), mask) and n_dev == n_in


def test_all_inliers_on_example_data(vo, ctx, o32):
    r = vp.run_real_init(DATA, o32)
    K, corr, p0, p1 = r["K"], r["corr"], r["p0"], r["p1"]
    F = vp.estimate_fundamental(corr, p0, p1)
    d = np.sqrt(R.sampson_sq((F / np.linalg.norm(F))[None], corr, p0, p1)[0])
    assert len(corr) == 115 and d.max() < 1e-3, d.max()                    # measured: 8.3e-4 px
    X, mask, n_in = vo.estimate_transform_ransac(K, corr, p0, p1, 1.0, 2048, 0, ctx=ctx)
    assert mask.all() and n_in == 115
    assert X.tobytes() == vo.estimate_transform(K, corr, p0, p1, ctx=ctx).tobytes()


@pytest.mark.parametrize("n,frac", [(2000, 0.4), (50000, 0.3)])
def test_outlier_recovery(vo, ctx, n, frac):
    fp, pairs, bad = _corrupted(vo, n, frac)
    X_clean = R.pose_8point(fp["K"], fp["gt_matches"], fp["ref_pts"], fp["cur_pts"])
    X, mask, n_in = vo.estimate_transform_ransac(fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], THR_PX, 2048, 0, ctx=ctx)
    e_rot, e_dir = R.pose_errors(X, X_clean)
    assert e_rot < TOL_ROT and e_dir < TOL_DIR, (e_rot, e_dir)
    assert (~bad[mask]).mean() >= 0.99 and n_in == mask.sum()
    X_plain = vo.estimate_transform(fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], ctx=ctx)
    p_rot, p_dir = R.pose_errors(X_plain, X_clean)
    assert p_rot > TOL_ROT or p_dir > TOL_DIR, (p_rot, p_dir)


def test_determinism_and_live_count(vo, ctx):
    fp, pairs, _ = _corrupted(vo, 2000, 0.4, seed=11)
    a = _dev_call(vo, ctx, fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], seed=12345)
    b = _dev_call(vo, ctx, fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], seed=12345)
    assert a[0] == b[0] == 0
    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]
    c = _dev_call(vo, ctx, fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], seed=12346)
    assert not np.array_equal(a[3], c[3])                                   # another seed, other samples
    # *d_n = 1500 of 2000: the pairs beyond are never sampled and never inliers
    live = _dev_call(vo, ctx, fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], seed=5, n_live=1500)
    head = _dev_call(vo, ctx, fp["K"], pairs[:1500], fp["ref_pts"], fp["cur_pts"], seed=5)
    assert live[0] == head[0] == 0 and not live[2][1500:].any()
    assert live[1].tobytes() == head[1].tobytes() and np.array_equal(live[2][:1500], head[2]) and np.array_equal(live[3], head[3])
    X, mask, n_in = vo.estimate_transform_ransac(fp["K"], pairs[:1500], fp["ref_pts"], fp["cur_pts"], THR_PX, 2048, 5, ctx=ctx)
    assert X.tobytes() == live[1].tobytes() and np.array_equal(mask, live[2][:1500].astype(bool)) and n_in == live[4]


def test_refusals(vo):
    c = vo.Context(0)
    lib, h, I = c.lib, c.h, C.c_int
    fp, pairs, _ = _corrupted(vo, 500, 0.2, seed=3)
    p1 = np.ascontiguousarray(fp["ref_pts"], np.float32); p2 = np.ascontiguousarray(fp["cur_pts"], np.float32)
    K = np.ascontiguousarray(fp["K"].T, np.float32).ravel()
    X = np.zeros(16, np.float32); mask = np.zeros(len(pairs), np.uint8); n_in = C.c_int()

    def call(prs=pairs, n=None, prm=(2048, 1.0, 0), a=p1, Xo=X, k=K):
        prs = np.ascontiguousarray(prs, np.int32)
        p = C.byref(vo.RansacParams(*prm)) if prm is not None else None
        return lib.vo_estimate_transform_ransac(h, _p(k) if k is not None else None, _p(prs), I(len(prs) if n is None else n),
                                                _p(a) if a is not None else None, I(len(p1)), _p(p2), I(len(p2)), p,
                                                _p(Xo) if Xo is not None else None, _p(mask), C.byref(n_in))

    assert call() == 0
    assert call(prm=None) == -1 and call(Xo=None) == -1 and call(a=None) == -1 and call(k=None) == -1
    assert lib.vo_estimate_transform_ransac(None, _p(K), _p(pairs), I(len(pairs)), _p(p1), I(len(p1)), _p(p2), I(len(p2)),
                                            C.byref(vo.RansacParams(2048, 1.0, 0)), _p(X), None, None) < 0
    assert call(n=7) == -1 and b"8" in lib.vo_last_error()
    wild = pairs.copy(); wild[17, 1] = len(p2) + 3
    assert call(prs=wild) == -5
    for prm in ((0, 1.0, 0), (65537, 1.0, 0), (-1, 1.0, 0), (64, 0.0, 0), (64, -1.0, 0), (64, float("inf"), 0), (64, float("nan"), 0)):
        assert call(prm=prm) == -1, prm
        assert lib.vo_last_error()
    assert call(prm=(64, 1e-6, 0)) == -1 and b"fewer than 8" in lib.vo_last_error()    # no hypothesis keeps 8 inliers
    # the _dev form: a bad index found on the device, fewer than 8 live pairs
    rc = _dev_call(vo, c, fp["K"], wild, p1, p2)[0]
    assert rc == -5
    assert _dev_call(vo, c, fp["K"], pairs, p1, p2, n_live=5)[0] == -1
    # inside a graph capture: refused before any HIP call
    g = C.c_void_p()
    assert lib.vo_ctx_begin_capture(h) == 0
    assert call() == -6
    assert lib.vo_ctx_end_capture(h, C.byref(g)) in (0, -3)
    if g.value:
        assert lib.vo_graph_destroy(g) == 0
    assert call() == 0                                                       # the context is still usable
    c.close()


def _run_vo_complete(out_dir, *flags):
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run([os.path.join(BIN, "vo_complete"), DATA, str(out_dir), *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return {f: open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))}


def test_vo_complete_ransac_flag(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s"])
    for form in ([], ["--resident"]):
        a = _run_vo_complete(tmp_path / ("plain" + "".join(form)), *form)
        b = _run_vo_complete(tmp_path / ("ransac" + "".join(form)), "--ransac", *form)
        assert len(a) >= 6 and a == b, form
    assert set(_run_vo_complete(tmp_path / "ransac_px", "--ransac=2.5")) == set(a)      # the threshold form runs


def test_sequence_pipeline_init_ransac(vo, ctx):
    """no mismatch in the first pair: every pair is an inlier and the refit is the plain call on the same pairs (frames of
    at most 256 points: the plain call's A^T A sums fall into one workgroup whether n_max is the capacity or the count)"""
    seq = vo.synth.sequence(seed=3000, n_frames=12, n_visible=200)
    runs = []
    for opt in (None, dict(threshold_px=1.0)):
        sp = vo.SequencePipeline(ctx, seq, n_iters=50, init_ransac=opt)
        sp.run()
        runs.append((sp.trajectory(), sp.counts()))
        sp.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
