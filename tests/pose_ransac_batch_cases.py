"""Inputs shared by tests/test_pose_ransac_batch_cpu.py (which calibrates them on the float64 restatement) and the GPU tests of
the batched P3P RANSAC (tests/test_gpu_pose_ransac_batch.py, tests/test_gpu_frames_track.py)."""
import numpy as np

import pose_ransac_restatement as P

TOL_ROT, TOL_T = 1e-3, 5e-3            # as tests/test_pose_ransac_cpu.py
MARGIN = 3.0                           # the robust route is held to the tolerances with this factor of margin on the CPU
THR_PX, N_HYP, SEED, ROUNDS = 2.0, 128, 0, 50

# the recovery problems: tracking_problem(1000, 40 % mismatches, large motion)
RECOVERY_SEEDS = tuple(range(2001, 2009))

# the frames the many-frames call recovers: frame_pair(1000, large motion) with 40 % of the model pairs' model indices
# replaced at random; the seeds from 2001 upward for which the restatement meets TOL / MARGIN on the pairs the oracle's
# matcher and join produce (measured values in test_pose_ransac_batch_cpu.py)
FRAME_SEEDS = (2001, 2002, 2003, 2005, 2006)            # 2004 misses: |t - t_clean| = 2.6e-3 > TOL_T / 3


def recovery_problem(vo, seed):
    return P.tracking_problem(vo, 1000, seed=seed, noise_px=0.5, frac=0.4, max_angle=0.3, max_t=0.5)


def track_frame(vo, seed, n=1000, frac=0.4):
    """(frame with mismatched model pairs, the same frame with the true ones)"""
    clean = vo.synth.frame_pair(n, seed=seed, noise_px=0.5, max_angle=0.3, max_t=0.5)
    rng = np.random.default_rng(seed + 7)
    mp = clean["model_pairs"].copy()
    hit = rng.uniform(size=len(mp)) < frac
    mp[hit, 1] = rng.integers(0, len(clean["model"]), int(hit.sum()))
    return dict(clean, model_pairs=mp), clean


def joined_pairs(o, fp):
    """(cur_idx, model_idx) as the frames call joins them: the oracle's matcher, then its join"""
    return np.asarray(o.join(o.match(fp["ref_app"], fp["cur_app"]), fp["model_pairs"]), np.int32).reshape(-1, 2)


def restatement_routes(K, world, meas, pairs, clean):
    """(errors of RANSAC + GN on its inliers, errors of plain GN on every pair, share of true pairs among the inliers),
    both errors against GN on the true pairs; float64 throughout"""
    T_clean = P.picp(K, np.eye(4), world, meas, clean, n_iters=ROUNDS)
    counts, win, mask, T_win = P.ransac(K, world, meas, pairs, THR_PX, N_HYP, SEED)
    assert win >= 0 and mask.sum() >= 6
    e_robust = P.pose_errors(P.picp(K, T_win, world, meas, pairs[mask], n_iters=ROUNDS), T_clean)
    e_plain = P.pose_errors(P.picp(K, np.eye(4), world, meas, pairs, n_iters=ROUNDS), T_clean)
    true = set(map(tuple, np.asarray(clean).tolist()))
    share = np.mean([tuple(p) in true for p in pairs[mask].tolist()])
    return e_robust, e_plain, float(share)
