"""CPU checks of the P3P RANSAC restatement (tests/pose_ransac_restatement.py) that tests/test_gpu_pose_ransac.py compares
vo_estimate_pose_ransac against: the 4-of-64 sample rule, the minimal solve, and the case for the feature -- Gauss-Newton PICP
(PICPSolver::oneRound restated, keep_outliers = false, 50 rounds) on 2D-3D pairs of which a fraction has its world index
replaced at random, with and without the RANSAC in front."""
import numpy as np

import pose_ransac_restatement as P

# tolerances against the solve on the true pairs alone: rotation angle (rad), |t - t_clean|
TOL_ROT, TOL_T = 1e-3, 5e-3
THR_PX = 2.0


def test_samples4_in_range_distinct_deterministic():
    for n in (4, 5, 50, 1000, 50000):
        idx, valid = P.samples4(23, 512, n)
        assert idx.min() >= 0 and idx.max() < n
        for h in np.nonzero(valid)[0]:
            assert len(set(idx[h].tolist())) == 4
        idx2, valid2 = P.samples4(23, 512, n)
        assert np.array_equal(idx, idx2) and np.array_equal(valid, valid2)
        if n >= 5:
            assert valid.all()
    assert not np.array_equal(P.samples4(0, 64, 1000)[0], P.samples4(1, 64, 1000)[0])     # the seed matters
    # the sample is a prefix of the epipolar rule's draws: the first 4 distinct values in draw order
    d = P.RR.draws(5, 8, 1000)
    idx, _ = P.samples4(5, 8, 1000)
    for h in range(8):
        seen = []
        for v in d[h]:
            if v not in seen:
                seen.append(v)
        assert seen[:4] == idx[h].tolist()


def test_p3p_recovers_the_true_pose_and_the_4th_point_selects_it(vo):
    rng = np.random.default_rng(4)
    K = vo.synth.K_REF
    found = 0
    for trial in range(40):
        T = vo.synth.random_isometry(rng, 0.5, 0.5).astype(np.float64)
        world = np.stack([rng.uniform(-2, 2, 4), rng.uniform(-1.5, 1.5, 4), rng.uniform(3, 8, 4)], 1)
        pc = world @ T[:3, :3].T + T[:3, 3]
        if (pc[:, 2] <= 0.5).any():
            continue
        ph = pc @ K.astype(np.float64).T
        uv = ph[:, :2] / ph[:, 2:3]
        sols = P.p3p(K, world[:3], uv[:3])
        assert 1 <= len(sols) <= 4
        # T is float32, orthonormal to ~1e-7: compare entries (the arccos of the angle metric would amplify that to 1e-4)
        dist = lambda R, t: max(np.abs(R - T[:3, :3]).max(), np.abs(t - T[:3, 3]).max())
        errs = [dist(R, t) for _, R, t in sols]
        assert min(errs) < 1e-5, errs
        R, t = P.hypothesis(K, world, uv)
        assert dist(R, t) == min(errs)
        found += 1
    assert found >= 30
    # degenerate: collinear world points leave the hypothesis invalid
    line = np.array([[0, 0, 5.0], [1, 0, 5.0], [2, 0, 5.0], [0, 1, 5.0]])
    assert P.hypothesis(K, line, np.array([[320, 240], [356, 240], [392, 240], [320, 276.0]])) is None


def test_mismatched_pairs_table():
    """The case for the feature, on synth.frame_pair(1000, seed=2001, noise_px=0.5), 50 GN rounds:
      0 % mismatched, small motion   plain GN (thr 10000) is the clean solve
      40 %, small motion (0.05/0.1)  plain GN off by > TOL (measured 1.5e-3 rad / 1.8e-2)
      40 %, large motion (0.3/0.5)   plain GN off by 1.8e-3 rad / 5.0e-2; a tight kernel (thr 4 px^2) from the identity
                                     does not get there either; RANSAC (2048, 2 px) + GN on its inliers lands within
                                     1.1e-4 rad / 4.6e-4 of the clean solve, every returned inlier a true match."""
    import __graft_entry__ as g
    vo = g.load_package()
    fp, world, meas, pairs, bad, clean = P.tracking_problem(vo, 1000, frac=0.0)
    assert not bad.any()
    T_clean = P.picp(fp["K"], np.eye(4), world, meas, clean)
    assert P.pose_errors(T_clean, fp["X_gt"])[0] < 1e-3

    fp, world, meas, pairs, bad, clean = P.tracking_problem(vo, 1000, frac=0.4)
    assert 0.35 < bad.mean() < 0.45
    T_clean = P.picp(fp["K"], np.eye(4), world, meas, clean)
    e = P.pose_errors(P.picp(fp["K"], np.eye(4), world, meas, pairs), T_clean)
    assert e[0] > TOL_ROT or e[1] > TOL_T, e

    fp, world, meas, pairs, bad, clean = P.tracking_problem(vo, 1000, frac=0.4, max_angle=0.3, max_t=0.5)
    T_clean = P.picp(fp["K"], np.eye(4), world, meas, clean)
    assert P.pose_errors(T_clean, fp["X_gt"])[0] < 1e-3
    e_plain = P.pose_errors(P.picp(fp["K"], np.eye(4), world, meas, pairs), T_clean)
    assert e_plain[0] > TOL_ROT or e_plain[1] > TOL_T, e_plain
    e_tight = P.pose_errors(P.picp(fp["K"], np.eye(4), world, meas, pairs, thr=4.0), T_clean)
    assert e_tight[0] > TOL_ROT or e_tight[1] > TOL_T, e_tight
    counts, win, mask, T_win = P.ransac(fp["K"], world, meas, pairs, THR_PX, 2048, 0)
    assert win >= 0 and counts[win] == counts.max() == mask.sum()
    assert (~bad[mask]).mean() >= 0.99 and mask.sum() >= 0.9 * (~bad).sum()
    e = P.pose_errors(P.picp(fp["K"], T_win, world, meas, pairs[mask]), T_clean)
    assert e[0] < TOL_ROT and e[1] < TOL_T, e


def test_library_exports_the_pose_ransac_entry_points(vo):
    """no device needed: both entry points exist and the header documents the rule and the status codes"""
    import os
    lib = vo.load_library()
    assert hasattr(lib, "vo_estimate_pose_ransac") and hasattr(lib, "vo_estimate_pose_ransac_dev")
    assert callable(vo.estimate_pose_ransac)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vo_hip.h")).read()
    for s in ("VO_POSE_RANSAC_OK", "VO_POSE_RANSAC_FEW_PAIRS", "VO_POSE_RANSAC_NO_HYPOTHESIS", "VO_POSE_RANSAC_FEW_INLIERS",
              "VO_POSE_RANSAC_BAD_INDEX", "Grunert", "first 4"):
        assert s in hdr, s


def test_subset_restatement_and_error_bands(vo):
    """hypotheses_at() restates the hypotheses it is given exactly as hypotheses() does all of them; error_bands bracket
    the exact count, which is inliers()'s"""
    fp, world, meas, pairs, bad, clean = P.tracking_problem(vo, 400, seed=4300, noise_px=0.5, frac=0.3, max_angle=0.3, max_t=0.5)
    K = fp["K"]
    T, valid, idx = P.hypotheses(K, world, meas, pairs, 200, 9)
    hs = np.array([0, 63, 64, 127, 128, 199, 17, 101])
    Ts, vs, ids, nsol = P.hypotheses_at(K, world, meas, pairs, hs, 200, 9)
    assert np.array_equal(Ts, T[hs]) and np.array_equal(vs, valid[hs]) and np.array_equal(ids, idx[hs])
    assert (nsol[vs] >= 1).all() and (nsol[~vs] == 0).all()
    for h in np.nonzero(valid)[0][:40]:
        exact, lo, hi = P.error_bands(K, T[h], world, meas, pairs, THR_PX, 1e-2, 480, 640, 0, 10)
        assert exact == int(P.inliers(K, T[h], world, meas, pairs, THR_PX, 480, 640, 0, 10).sum()) and lo <= exact <= hi
    e2 = P.sq_errors(K, T[0], world, meas, pairs, 480, 640, 0, 10)
    assert e2.shape == (len(pairs),) and (e2 >= 0).all()


def test_constructed_samples_have_their_properties():
    def ratio(W):
        W = np.asarray(W, np.float64)
        e12, e13 = W[1] - W[0], W[2] - W[0]
        return np.linalg.norm(np.cross(e12, e13)) / (np.linalg.norm(e12) * np.linalg.norm(e13))

    for name, f in (("collinear_above", 1 + 1e-3), ("collinear_below", 1 - 1e-3)):
        K, W, uv = P.constructed(name)
        assert abs(ratio(W) / 1e-9 - f) < 1e-6 and P.degenerate(W[:3]) == (f < 1)
    # on the danger cylinder three roots meet (split by the float32 pixels); 1e-4 of the radius outside, two lie close
    for name in ("danger_cylinder", "near_cylinder"):
        qt = P.quartic_terms(*P.constructed(name))
        r = qt["re"] + 1j * qt["im"]
        close = sorted(abs(r[i] - r[j]) for i in range(4) for j in range(i + 1, 4))
        assert close[1] < 2e-3 and close[-1] > 0.05, close
    # wide-angle K, j3 orthogonal to j1 and j2: A3 and A1 vanish to rounding, so q = 0 (the biquadratic branch)
    qt = P.quartic_terms(*P.constructed("biquadratic"))
    assert abs(qt["q"]) < 1e-12 * qt["scale"] and abs(qt["A"][1]) < 1e-12 and abs(qt["A"][3]) < 1e-12
    # the 4th point behind the camera under every solution: all errors +inf, the smaller v chosen
    K, W, uv = P.constructed("tie_behind")
    sols = P.p3p(K, W[:3], uv[:3])
    assert len(sols) >= 2 and all((R_ @ W[3] + t_)[2] <= 0 for _, R_, t_ in sols)
    v_min = min(sols, key=lambda s: s[0])
    R_, t_ = P.hypothesis(K, W, uv)
    assert np.array_equal(R_, v_min[1]) and np.array_equal(t_, v_min[2])
    # behind one solution, in front of another: the one in front wins although the other reprojects it exactly
    K, W, uv = P.constructed("behind_one")
    sols = P.p3p(K, W[:3], uv[:3])
    z = [(R_ @ W[3] + t_)[2] for _, R_, t_ in sols]
    assert min(z) < 0 < max(z)
    R_, t_ = P.hypothesis(K, W, uv)
    assert (R_ @ W[3] + t_)[2] > 0
    # embedded: hypothesis 0 of seed 77 draws the sample in its order
    world, meas, pairs = P.embedded(K, W, uv, seed=77)
    idx = P.samples4(77, 1, len(pairs))[0][0]
    assert np.array_equal(world[idx], W) and np.array_equal(meas[idx], uv)


def test_tie_cases_are_ties(vo):
    """the hard-coded tie cases of tests/test_gpu_ransac_sizes.py, checked from the float64 side alone"""
    import test_gpu_ransac_sizes as S
    import ransac_restatement as R
    fp = vo.synth.frame_pair(300000, seed=4200, noise_px=0.25)
    pairs, _ = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), 0.3, seed=4)
    t = S.EPI_TIE
    pr, p1, p2 = pairs[:t["n"]], fp["ref_pts"], fp["cur_pts"]
    idx, valid = R.samples(t["seed"], t["n_hyp"], t["n"])
    F, valid = R.minimal_fits(pr, p1, p2, idx, valid)
    exact, lo, hi = R.sampson_bands(F, valid, pr, p1, p2, S.EPI_THR, S.DELTA)
    tied = np.nonzero(exact == exact.max())[0]
    d2, band = R.sampson_band(F[tied], pr, p1, p2, S.EPI_THR, S.DELTA)
    assert tied.tolist() == t["tied"] and not band.any() and not np.array_equal(d2[0] < 1, d2[-1] < 1)
