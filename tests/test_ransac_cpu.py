"""CPU checks of the RANSAC restatement (tests/ransac_restatement.py) that the GPU tests compare
vo_estimate_transform_ransac against: the sampling rule, and the calibration of the noise / threshold pair and of the
pose tolerances that tests/test_gpu_ransac.py uses."""
import numpy as np

import ransac_restatement as R

# synth.frame_pair(2000) at 0.25 px noise, 40 % of the second indices replaced at random, 2048 hypotheses, 1 px, seed 0.
# Measured (seeds 2000 / 7 / 11), against the plain 8-point fit on the clean pairs:
#   RANSAC refit      rotation 1.7e-3 / 3e-4 / 9e-4 rad, translation direction 0.069 / 0.016 / 0.038 rad, >= 99.57 % true inliers
#   plain, corrupted  rotation 0.034 / 0.048 / 0.040 rad, translation direction 0.54 / 0.73 / 0.86 rad
# (50k pairs with 30 % corrupted, seed 2000: refit 7e-4 / 0.026, plain 0.019 / 0.54.)  The tolerances sit between, with a
# margin of at least 3.6x below them for the refit and 1.8x above them for the plain fit.
TOL_ROT, TOL_DIR = 1e-2, 0.25
NOISE_PX, THR_PX = 0.25, 1.0


def test_splitmix64_known_values():
    # splitmix64 of 0, 1 (the reference sequence of the generator seeded with 0 starts with 0xE220A8397B1DCDAF)
    out = R.splitmix64(np.array([0, 1, 0xFFFFFFFFFFFFFFFF], np.uint64))
    assert int(out[0]) == 0xE220A8397B1DCDAF
    assert out.dtype == np.uint64 and len(set(int(v) for v in out)) == 3


def test_samples_in_range_distinct_deterministic():
    for n in (8, 9, 50, 2000, 50000):
        idx, valid = R.samples(17, 512, n)
        assert idx.min() >= 0 and idx.max() < n
        for h in np.nonzero(valid)[0]:
            assert len(set(idx[h].tolist())) == 8
        idx2, valid2 = R.samples(17, 512, n)
        assert np.array_equal(idx, idx2) and np.array_equal(valid, valid2)
        if n >= 50:
            assert valid.all()
    d = R.draws(0, 4, 1000)
    assert not np.array_equal(d, R.draws(1, 4, 1000))                       # the seed matters
    # n = 8: a hypothesis is invalid when some value never shows up in 64 draws -- rare, but it happens
    _, v8 = R.samples(0, 2048, 8)
    assert 0 < (~v8).sum() < 20


def _data(seed):
    import __graft_entry__ as g
    vo = g.load_package()
    fp = vo.synth.frame_pair(2000, seed=seed, noise_px=NOISE_PX)
    pairs, bad = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), 0.4)
    return fp, pairs, bad


def test_restatement_recovers_from_mismatches():
    fp, pairs, bad = _data(2000)
    X_clean = R.pose_8point(fp["K"], fp["gt_matches"], fp["ref_pts"], fp["cur_pts"])
    counts, win, mask, F = R.ransac(pairs, fp["ref_pts"], fp["cur_pts"], THR_PX, 2048, 0)
    assert (counts >= 0).all() and counts[win] == counts.max() == mask.sum()
    assert (~bad[mask]).mean() >= 0.99
    X = R.pose_8point(fp["K"], pairs[mask], fp["ref_pts"], fp["cur_pts"])
    e_rot, e_dir = R.pose_errors(X, X_clean)
    assert e_rot < TOL_ROT / 3 and e_dir < TOL_DIR / 3, (e_rot, e_dir)        # measured 1.7e-3, 0.069
    # the same on the plain fit of the corrupted pairs: far off
    p_rot, p_dir = R.pose_errors(R.pose_8point(fp["K"], pairs, fp["ref_pts"], fp["cur_pts"]), X_clean)
    assert p_rot > 3 * TOL_ROT and p_dir > 2 * TOL_DIR, (p_rot, p_dir)      # measured 0.034, 0.54
    # the clean fit itself is close to the generating motion
    g_rot, _ = R.pose_errors(X_clean, fp["X_gt"])
    assert g_rot < 2e-3


def test_minimal_fit_fits_its_own_clean_sample():
    fp, pairs, bad = _data(7)
    idx, valid = R.samples(0, 2048, len(pairs))
    clean = np.nonzero(valid & ~bad[idx].any(1))[0]                          # samples of true matches only (0.6^8 of them)
    assert len(clean) >= 10
    F, ok = R.minimal_fits(pairs, fp["ref_pts"], fp["cur_pts"], idx[clean], valid[clean])
    d2 = R.sampson_sq(F, pairs, fp["ref_pts"], fp["cur_pts"])
    own = np.take_along_axis(d2, idx[clean], 1)
    assert ok.all() and np.median(np.sqrt(own)) < 0.25                       # the rank-2 projection moves its own sample little


def test_library_exports_the_ransac_entry_points(vo):
    """no device needed: the entry points exist, and the Python mirror of vo_ransac_params has the header's layout"""
    import ctypes as C
    import os
    lib = vo.load_library()
    assert hasattr(lib, "vo_estimate_transform_ransac") and hasattr(lib, "vo_estimate_transform_ransac_dev")
    assert C.sizeof(vo.RansacParams) == 16 and vo.RansacParams.seed.offset == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vo_hip.h")).read()
    assert "0x9E3779B97F4A7C15" in hdr and "typedef struct vo_ransac_params" in hdr


def test_float64_fit_helpers_restate_the_oracle(vo, o32):
    """fundamental() / estimate_transform() (thin SVD, maxima by image_maxima) are vp.estimate_fundamental /
    vp.estimate_transform on finite images, and image_maxima skips NaN and values <= 0"""
    from oracle import vo_pipeline as vp
    fp = vo.synth.frame_pair(1500, seed=4100)
    pairs, _ = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), 0.05, seed=2)
    p1, p2 = fp["ref_pts"], fp["cur_pts"]
    F, F_o = R.fundamental(pairs, p1, p2), vp.estimate_fundamental(pairs, p1, p2)
    F, F_o = F / np.linalg.norm(F), F_o / np.linalg.norm(F_o)
    assert min(np.abs(F - F_o).max(), np.abs(F + F_o).max()) < 1e-12
    X = R.estimate_transform(o32, fp["K"], pairs, p1, p2)
    assert np.abs(X - vp.estimate_transform(o32, fp["K"], pairs, p1, p2)).max() < 1e-6
    assert np.abs(R.pose_8point(fp["K"], pairs, p1, p2, F=R.fundamental(pairs, p1, p2)) - X).max() < 1e-6
    p = np.array([[np.nan, 3], [-5, np.nan], [2, -1], [1, 1]], np.float32)
    assert R.image_maxima(p) == (2, 3) and R.image_maxima(-np.abs(p)) == (0, 0)


def test_sampson_bands_bracket_the_exact_count(vo):
    fp = vo.synth.frame_pair(1500, seed=4200, noise_px=NOISE_PX)
    pairs, _ = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), 0.3, seed=4)
    p1, p2 = fp["ref_pts"], fp["cur_pts"]
    counts, win, mask, F = R.ransac(pairs, p1, p2, THR_PX, 300, 5)
    idx, valid = R.samples(5, 300, len(pairs))
    F2, valid2, cond = R.minimal_fits(pairs, p1, p2, idx, valid, with_conditioning=True)
    assert np.array_equal(F, F2) and np.array_equal(valid2, counts >= 0) and (cond[valid2] > 0).all()
    exact, lo, hi = R.sampson_bands(F2, valid2, pairs, p1, p2, THR_PX, 1e-2, chunk=7)
    assert np.array_equal(exact, counts) and (lo <= exact).all() and (exact <= hi).all() and (hi > lo).any()
    # the band grows with delta, and holds only pairs near the threshold
    d2, band0 = R.sampson_band(F2[win:win + 1], pairs, p1, p2, THR_PX, 0.0)
    _, band1 = R.sampson_band(F2[win:win + 1], pairs, p1, p2, THR_PX, 1e-2)
    assert d2.shape == band0.shape == (1, len(pairs)) and not (band0 & ~band1).any() and band1.sum() < 0.05 * len(pairs)
    assert (np.abs(d2[band1] / THR_PX ** 2 - 1) < 0.5).all()
