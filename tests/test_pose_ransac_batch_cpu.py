"""CPU side of the batched P3P RANSAC (vo_estimate_pose_ransac_batch_dev, vo_frames_batch_track_dev): the exports, and the
calibration on the float64 restatement (tests/pose_ransac_restatement.py) of the inputs whose recovery the GPU tests claim --
128 hypotheses, 2 px, seed 0, 50 Gauss-Newton rounds, 40 % mismatched pairs."""
import os

import numpy as np

import pose_ransac_batch_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_batched_entry_points(vo):
    lib = vo.load_library()
    assert hasattr(lib, "vo_estimate_pose_ransac_batch_dev") and hasattr(lib, "vo_frames_batch_track_dev")
    assert callable(vo.estimate_pose_ransac_batch) and callable(vo.estimate_pose_ransac_batch_dev)
    hdr = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    for s in ("vo_estimate_pose_ransac_batch_dev", "vo_frames_batch_track_dev", "vo_frame_track", "BIT FOR BIT"):
        assert s in hdr, s
    assert lib.vo_abi_version() == 1


def _check(e_robust, e_plain, share):
    print("robust %.2e rad %.2e | plain %.2e rad %.2e | true inliers %.4f" % (*e_robust, *e_plain, share))
    assert e_robust[0] < B.TOL_ROT / B.MARGIN and e_robust[1] < B.TOL_T / B.MARGIN, e_robust
    assert e_plain[0] > B.TOL_ROT and e_plain[1] > B.TOL_T, e_plain
    assert share >= 0.99, share


def test_recovery_inputs_are_calibrated(vo):
    """tracking_problem(1000, seed 2001..2008, 40 % mismatches, motion 0.3 / 0.5).  Measured, (rad, |t|) against GN on the true
    pairs: RANSAC + GN on the inliers at most 2.6e-4 / 1.6e-3 (seed 2003), plain GN on every pair at least 1.8e-3 (2001) and
    1.2e-2 (2002); every returned inlier true except on seed 2004 (99.8 %)."""
    for s in B.RECOVERY_SEEDS:
        fp, world, meas, pairs, bad, clean = B.recovery_problem(vo, s)
        assert 0.35 < bad.mean() < 0.45
        _check(*B.restatement_routes(fp["K"], world, meas, pairs, clean))


def test_frames_call_inputs_are_calibrated(vo, o32):
    """frame_pair(1000, motion 0.3 / 0.5) with 40 % of the model pairs' model indices replaced, through the oracle's matcher and
    join -- the pairs the many-frames call hands its RANSAC.  Measured per seed, robust (rad, |t|) | plain (rad, |t|):
      2001  2.3e-4 1.0e-3 | 6.5e-3 4.4e-2      2002  1.1e-4 7.8e-4 | 1.9e-3 1.2e-2      2003  0      5.6e-4 | 3.6e-3 2.8e-2
      2004  2.9e-4 2.6e-3 | 3.9e-3 1.3e-2  (left out: |t| misses TOL_T / 3 = 1.67e-3)
      2005  3.3e-4 7.6e-4 | 3.4e-3 1.4e-2      2006  2.4e-5 2.9e-4 | 3.7e-3 2.0e-2
    every returned inlier a true pair."""
    assert B.FRAME_SEEDS == (2001, 2002, 2003, 2005, 2006)
    for s in B.FRAME_SEEDS:
        bad, clean = B.track_frame(vo, s)
        j, jc = B.joined_pairs(o32, bad), B.joined_pairs(o32, clean)
        assert len(j) == len(jc) == 1000 and 0.35 < (j[:, 1] != jc[:, 1]).mean() < 0.45
        _check(*B.restatement_routes(bad["K"], bad["model"], bad["cur_pts"], j, jc))
    # the seed left out does miss the margin (and only the margin)
    bad, clean = B.track_frame(vo, 2004)
    e = B.restatement_routes(bad["K"], bad["model"], bad["cur_pts"], B.joined_pairs(o32, bad), B.joined_pairs(o32, clean))[0]
    assert e[1] > B.TOL_T / B.MARGIN and e[1] < B.TOL_T
