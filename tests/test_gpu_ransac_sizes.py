"""Both RANSAC front ends (vo_estimate_transform_ransac_dev, vo_estimate_pose_ransac_dev) across their hypothesis and pair
tiling, every hypothesis against the float64 restatements (tests/ransac_restatement.py, tests/pose_ransac_restatement.py):
64-hypothesis scoring blocks and 64-thread hypothesis workgroups (a partial last block, 1 hypothesis, the 65536 maximum),
256-pair gather / mask / scatter workgroups and 1024-pair scoring workgroups, the 1024-workgroup cap of the gather loops
(262 144 pairs a pass) and live counts below n_max.  Then single-hypothesis probes (n_hypotheses = 1 makes h = 0 the winner,
so the outputs expose that one hypothesis) and non-finite rows.

Per hypothesis the GPU count must lie in [#pairs with d^2 < thr^2 (1 - DELTA), #pairs with d^2 < thr^2 (1 + DELTA)], d^2 the
restatement's float64 distance.  Both DELTA and the conditioning rules below are decided from the float64 side alone."""
import numpy as np
import pytest

import pose_ransac_restatement as P
import ransac_restatement as R
from ransac_dev import CAM, Dev, dev_call

pytestmark = pytest.mark.gpu

# The GPU scores in float with F / the pose rounded to float: a relative error of d^2 of ~1e-4 on these images for most pairs
# (~1e3 cancellation in e = x1^T F x2 times float rounding; ~1e-4 px of projection error against a 2 px threshold).  The
# epipolar band also widens per pair by a first-order bound on the float error of d^2 (R.sampson_band), u = 2^-24: e is two
# nested 3-term float sums over F rounded to float, |de| <= 7u S_e; each denominator term a_k is a 3-term sum, |da_k| <= 4u S_k,
# so |dden| <= 4u S_den; then |d(d^2)| <= u (14 |e| S_e + 4 d^2 S_den) / den + 3u d^2.  c_float = 16 covers each term with
# a margin of at least 2 -- it matters next to an epipole, where e and den both cancel.
DELTA = 1e-2
# Epipolar: a minimal 8 x 9 system with s7 / s0 below COND_8PT leaves F sensitive beyond float rounding; such a hypothesis
# falls back to the old rule |count - exact| <= 2.
COND_8PT = 1e-6
# P3P: a hypothesis is ill-posed when the restatement's own float32 pose moves by more than P3P_MOVE under a 1-ulp change of
# every pixel coordinate (near-double roots, near-degenerate triangles); it falls back to |count - exact| <= 2 and is never
# compared pose for pose.
P3P_MOVE = 1e-4
ULPS = 4                               # T_out against the restatement's float32 pose: ulps of max(|entry|, 2^-10)
EPI_THR, POSE_THR = 1.0, 2.0


def _close_ulps(a, b, ulps=ULPS):
    b = np.asarray(b, np.float32)
    return bool((np.abs(np.asarray(a, np.float64) - b) <= ulps * np.spacing(np.maximum(np.abs(b), np.float32(2 ** -10)))).all())


def _wild_tail(pairs, n_max, n1, n2, seed):
    """pairs followed by wild (in-range) rows up to n_max"""
    rng = np.random.default_rng(seed)
    k = n_max - len(pairs)
    return np.concatenate([pairs, np.stack([rng.integers(0, n1, k), rng.integers(0, n2, k)], 1)]).astype(np.int32)


def _block_edges(n_hyp, n_random, seed):
    """hypotheses at the edges of every 64-block, the last 65, and a random sample"""
    b = np.arange(0, n_hyp, 64)
    hs = np.concatenate([b, np.minimum(b + 63, n_hyp - 1), np.arange(max(0, n_hyp - 65), n_hyp),
                         np.random.default_rng(seed).integers(0, n_hyp, n_random)])
    return np.unique(hs)


# ---- epipolar -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def epi_data(vo):
    """300 000 noisy pairs (0.25 px), 30 % of the second indices replaced at random"""
    fp = vo.synth.frame_pair(300000, seed=4200, noise_px=0.25)
    pairs, bad = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), 0.3, seed=4)
    return fp, pairs


def _epi_check(vo, ctx, fp, pairs, n_hyp, n, n_max, seed):
    """one call with n live pairs of an n_max buffer, every hypothesis against the restatement"""
    p1, p2, K = fp["ref_pts"], fp["cur_pts"], fp["K"]
    pr = np.ascontiguousarray(pairs[:n], np.int32)
    buf = _wild_tail(pr, n_max, len(p1), len(p2), seed + 1) if n_max > n else pr
    rc, X, mask, counts, n_in = dev_call(vo, ctx, K, buf, p1, p2, n_hyp, EPI_THR, seed, n_live=n if n_max > n else None,
                                         always_read=True)
    counts = counts.astype(np.int64)
    idx, valid = R.samples(seed, n_hyp, n)
    F, valid, cond = R.minimal_fits(pr, p1, p2, idx, valid, with_conditioning=True)
    exact, lo, hi = R.sampson_bands(F, valid, pr, p1, p2, EPI_THR, DELTA, chunk=max(1, (1 << 22) // n))
    assert np.array_equal(counts < 0, ~valid) and (counts >= -1).all()
    well = valid & (cond >= COND_8PT)
    bad = np.nonzero(well & ((counts < lo) | (counts > hi)))[0]
    assert len(bad) == 0, (bad[:10], counts[bad[:10]], lo[bad[:10]], hi[bad[:10]])
    assert (np.abs(counts - exact)[valid & ~well] <= 2).all()
    # the winner: the GPU's rule on its own counts, a hypothesis whose bounds reach the top; the restatement's winner where
    # its count beats every other upper bound
    w = int(np.argmax(counts))
    top = counts[w]
    assert lo[w] <= top <= hi[w] and hi[w] >= exact.max()
    others = np.delete(hi, int(np.argmax(exact)))
    if len(others) == 0 or exact.max() > others.max():
        assert w == int(np.argmax(exact))
    assert not mask[n:n_max].any() and int(mask[:n].sum()) == max(top, 0)
    if top >= 0:
        d2, band = R.sampson_band(F[w:w + 1], pr, p1, p2, EPI_THR, DELTA)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(mask[:n].astype(bool)[~band[0]], (d2[0] < EPI_THR ** 2)[~band[0]])
    if top >= 8:
        assert rc == 0 and n_in == top
        X_plain = vo.estimate_transform(K, pr[mask[:n].astype(bool)], p1, p2, ctx=ctx)    # inliers in their original order
        assert X.tobytes() == X_plain.tobytes()
    else:
        assert rc == -1
    return counts, valid, exact, mask


# every edge of both axes at least once: n_hyp 1, 2, 63, 64, 65, 127, 1023, 1024, 1025, 4097, 65535, 65536; pairs 8, 9, 255,
# 256, 257, 1023, 1024, 1025, 4097, 300 000; live counts 255 / 1025 / 4097 / 257 below a larger n_max
EPI_CASES = [  # (n_hyp, live pairs, n_max)
    (1, 9, 9), (2, 8, 8), (63, 255, 255), (64, 256, 256), (65, 257, 257), (127, 1023, 1023), (1023, 1024, 1024),
    (1024, 1025, 1025), (1025, 4097, 4097), (65, 300000, 300000), (65535, 255, 255), (65536, 257, 257),
    (1024, 255, 1025), (64, 1025, 4097), (127, 4097, 300000), (4097, 257, 511)]


@pytest.mark.parametrize("n_hyp,n,n_max", EPI_CASES)
def test_epipolar_tiling(vo, ctx, epi_data, n_hyp, n, n_max):
    fp, pairs = epi_data
    _epi_check(vo, ctx, fp, pairs, n_hyp, n, n_max, seed=n_hyp + n)


def test_epipolar_single_hypothesis_probes(vo, ctx, epi_data):
    """n_hypotheses = 1: the mask is hypothesis 0's Sampson predicate, and the call is refused where it keeps fewer than 8"""
    fp, pairs = epi_data
    refused = 0
    for seed in range(60):
        counts, valid, exact, mask = _epi_check(vo, ctx, fp, pairs, 1, 300, 300, seed=1000 + seed)
        refused += int(exact[0] < 8)
    assert 0 < refused < 60                                                  # both branches were taken


# ---- P3P --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pose_data(vo):
    """300 000 noisy 2D-3D pairs (0.5 px), 30 % of the world indices replaced at random"""
    fp, world, meas, pairs, bad, clean = P.tracking_problem(vo, 300000, seed=4300, noise_px=0.5, frac=0.3, max_angle=0.3, max_t=0.5)
    return fp, np.asarray(world, np.float32), np.asarray(meas, np.float32), pairs


def _nudged(meas):
    return np.nextafter(np.asarray(meas, np.float32), np.float32(np.inf))


def _pose_check(vo, ctx, K, world, meas, pairs, n_hyp, n, n_max, seed, hs=None, d=None):
    """one call with n live pairs of an n_max buffer; the hypotheses hs (all by default, plus the GPU winner) against the
    restatement.  Returns (status, T_out, restated valid, number of solutions, ill-posed) of hs."""
    pr = np.ascontiguousarray(pairs[:n], np.int32)
    buf = _wild_tail(pr, n_max, len(meas), len(world), seed + 1) if n_max > n else pr
    own = d is None
    if own:
        d = Dev(vo, ctx, K, world, meas, buf)
    try:
        d.set_live(n)
        assert d.call(n_hyp=n_hyp, thr=POSE_THR, seed=seed) == 0
        T_out, inl, nin, mask, counts, st = d.results(n_hyp)
    finally:
        if own:
            d.close()
    counts = counts.astype(np.int64)
    w = int(np.argmax(counts))
    hs = np.arange(n_hyp) if hs is None else np.unique(np.append(hs, w))
    T, valid, idx, nsol = P.hypotheses_at(K, world, meas, pr, hs, n_hyp, seed)
    T2, valid2, _, _ = P.hypotheses_at(K, world, _nudged(meas), pr, hs, n_hyp, seed)
    ill = (np.abs(T - T2).max((1, 2)) > P3P_MOVE) | (valid != valid2)
    # validity where the restatement's own validity survives the 1-ulp change
    assert np.array_equal((counts[hs] < 0)[valid == valid2], ~valid[valid == valid2]) and (counts >= -1).all()
    exact, lo, hi = np.full((3, len(hs)), -1, np.int64)
    exact2 = np.full(len(hs), -1, np.int64)
    for k in np.nonzero(valid)[0]:
        exact[k], lo[k], hi[k] = P.error_bands(K, T[k], world, meas, pr, POSE_THR, DELTA, *CAM)
        if valid2[k]:
            exact2[k] = P.error_bands(K, T2[k], world, meas, pr, POSE_THR, DELTA, *CAM)[0]
    c = counts[hs]
    well = valid & ~ill
    bad = np.nonzero(well & ((c < lo) | (c > hi)))[0]
    assert len(bad) == 0, (hs[bad[:10]], c[bad[:10]], lo[bad[:10]], hi[bad[:10]])
    # ill-posed: +-2, unless the restatement's own count moves by more than 2 under the 1-ulp change
    loose = valid & valid2 & ~well & (np.abs(exact - exact2) <= 2) & (c >= 0)
    assert (np.abs(c - exact)[loose] <= 2).all()
    if st == 0:
        kw = int(np.searchsorted(hs, w))
        top = counts[w]
        assert nin == top == int(mask[:n].sum()) and not mask[n:].any() and top >= 6
        assert lo[kw] <= top <= hi[kw] and hi[kw] >= exact.max()
        if len(hs) == n_hyp:
            others = np.delete(hi, int(np.argmax(exact)))
            if len(others) == 0 or exact.max() > others.max():
                assert w == int(np.argmax(exact))
        assert np.array_equal(inl, pr[mask[:n].astype(bool)])                  # compacted in their original order
        if not ill[kw]:
            assert _close_ulps(T_out, T[kw]), np.abs(T_out - T[kw]).max()
            e2 = P.sq_errors(K, T[kw], world, meas, pr, *CAM)
            thr2 = POSE_THR ** 2
            with np.errstate(invalid="ignore"):
                out_band = ~((e2 >= thr2 * (1 - DELTA)) & (e2 < thr2 * (1 + DELTA)))
            assert np.array_equal(mask[:n].astype(bool)[out_band], (e2 < thr2)[out_band])
    else:
        assert nin == n and np.array_equal(T_out, np.eye(4))
    return st, T_out, valid, nsol, ill, counts, exact, T, mask


POSE_CASES = [  # (n_hyp, live pairs, n_max)
    (1, 4, 4), (2, 9, 9), (63, 255, 255), (64, 256, 256), (65, 257, 257), (127, 1023, 1023), (1023, 1024, 1024),
    (1024, 1025, 1025), (1025, 4097, 4097), (65, 300000, 300000), (65535, 255, 255), (65536, 257, 257),
    (1024, 255, 1025), (64, 1025, 4097), (127, 4097, 300000), (4097, 257, 511)]


@pytest.mark.parametrize("n_hyp,n,n_max", POSE_CASES)
def test_pose_tiling(vo, ctx, pose_data, n_hyp, n, n_max):
    fp, world, meas, pairs = pose_data
    hs = _block_edges(n_hyp, 300, n_hyp) if n_hyp > 1100 else None
    _pose_check(vo, ctx, fp["K"], world, meas, pairs, n_hyp, n, n_max, seed=n_hyp + n, hs=hs)


def test_pose_single_hypothesis_probes(vo, ctx, pose_data):
    """n_hypotheses = 1 over 300 seeds: T_out is the restatement's hypothesis 0 (draw rule, P3P solve, root choice), the
    status its class (invalid -> 2, fewer than 6 inliers -> 3)"""
    fp, world, meas, pairs = pose_data
    n = 60
    d = Dev(vo, ctx, fp["K"], world, meas, pairs[:n])
    multi = compared = 0
    try:
        for seed in range(300):
            st, T_out, valid, nsol, ill, counts, exact, T, mask = _pose_check(vo, ctx, fp["K"], world, meas, pairs, 1, n, n, seed, d=d)
            if not valid[0]:
                assert st == 2
            elif exact[0] < 6 and not ill[0]:
                assert st == 3
            else:
                assert st == 0
            compared += int(st == 0 and not ill[0])
            multi += int(nsol[0] >= 2)
    finally:
        d.close()
    assert compared >= 30 and multi >= 60, (compared, multi)                  # the 4th point chose among 2+ solutions often


# ---- non-finite rows --------------------------------------------------------------------------------------------------------
def test_non_finite_rows(vo, ctx, epi_data, pose_data):
    """NaN and +-inf in pixel and world rows (no +inf in the images vo_estimate_transform normalises by): validity and counts
    as the restatement's, such pairs never inliers, the refit and the pose finite"""
    fp, pairs = epi_data
    p1, p2 = fp["ref_pts"].copy(), fp["cur_pts"].copy()
    pr = np.ascontiguousarray(pairs[:2000], np.int32)
    rng = np.random.default_rng(9)
    hit = rng.choice(2000, 40, replace=False)
    p1[pr[hit[:15], 0], 0] = np.nan; p2[pr[hit[15:30], 1], 1] = -np.inf; p1[pr[hit[30:], 0], 1] = -np.inf
    fpp = dict(fp, ref_pts=p1, cur_pts=p2)
    counts, valid, exact, mask = _epi_check(vo, ctx, fpp, pr, 1024, 2000, 2000, seed=3)     # the refit is X_plain's there
    assert (~valid).sum() > 0 and exact.max() >= 8 and not mask[hit].any()   # some samples hold a non-finite row
    fp, world, meas, pairs = pose_data
    world, meas = world.copy(), meas.copy()
    pr = np.ascontiguousarray(pairs[:2000], np.int32)
    world[pr[hit[:10], 1], 0] = np.nan; world[pr[hit[10:20], 1], 2] = np.inf; world[pr[hit[20:25], 1], 1] = -np.inf
    meas[pr[hit[25:35], 0], 0] = np.nan; meas[pr[hit[35:], 0], 1] = np.inf
    st, T_out, valid, nsol, ill, counts, exact, T, mask = _pose_check(vo, ctx, fp["K"], world, meas, pr, 1024, 2000, 2000, seed=3)
    assert st == 0 and (~valid).sum() > 0 and not mask[hit].any() and np.isfinite(T_out).all()


# ---- ties ---------------------------------------------------------------------------------------------------------------------
# Found by a search over seeds on the float64 side: several hypotheses share the top count, every other hypothesis's upper
# bound lies below it, no pair of a tied hypothesis lies in the band, and the tied hypotheses' masks (poses) differ.
EPI_TIE = dict(n=20, n_hyp=64, seed=9, tied=[8, 11, 12, 63])
POSE_TIE = dict(n=20, n_hyp=64, seed=28, tied=[19, 32, 49, 55, 57])


def test_ties_go_to_the_lowest_hypothesis(vo, ctx, epi_data, pose_data):
    fp, pairs = epi_data
    p1, p2, t = fp["ref_pts"], fp["cur_pts"], EPI_TIE
    pr = pairs[:t["n"]]
    idx, valid = R.samples(t["seed"], t["n_hyp"], t["n"])
    F, valid = R.minimal_fits(pr, p1, p2, idx, valid)
    exact, lo, hi = R.sampson_bands(F, valid, pr, p1, p2, EPI_THR, DELTA)
    tied = np.nonzero(exact == exact.max())[0]
    d2, band = R.sampson_band(F[tied], pr, p1, p2, EPI_THR, DELTA)
    masks = d2 < EPI_THR ** 2
    assert tied.tolist() == t["tied"] and (hi[exact < exact.max()] < exact.max()).all() and not band.any()
    assert not np.array_equal(masks[0], masks[-1])                          # the highest h would show
    counts, valid, exact, mask = _epi_check(vo, ctx, fp, pairs, t["n_hyp"], t["n"], t["n"], t["seed"])
    assert np.array_equal(mask.astype(bool), masks[0])
    fp, world, meas, pairs = pose_data
    t = POSE_TIE
    pr = pairs[:t["n"]]
    T, valid, _, _ = P.hypotheses_at(fp["K"], world, meas, pr, np.arange(t["n_hyp"]), t["n_hyp"], t["seed"])
    b = np.array([P.error_bands(fp["K"], T[h], world, meas, pr, POSE_THR, DELTA, *CAM) if valid[h] else (-1, -1, -1)
                  for h in range(t["n_hyp"])]).T
    tied = np.nonzero(b[0] == b[0].max())[0]
    assert tied.tolist() == t["tied"] and (b[2][b[0] < b[0].max()] < b[0].max()).all() and (b[1][tied] == b[2][tied]).all()
    st, T_out, *_ = _pose_check(vo, ctx, fp["K"], world, meas, pairs, t["n_hyp"], t["n"], t["n"], t["seed"])
    assert st == 0 and _close_ulps(T_out, T[tied[0]]) and np.abs(T_out - T[tied[-1]]).max() > 1e-3


# ---- constructed P3P samples (tests/pose_ransac_restatement.constructed; their properties: tests/test_pose_ransac_cpu.py) ------
@pytest.mark.parametrize("name", ["collinear_above", "collinear_below", "danger_cylinder", "near_cylinder", "biquadratic",
                                  "tie_behind", "behind_one"])
def test_constructed_p3p_samples(vo, ctx, name):
    """each sample as hypothesis 0 of one: T_out, status and count against the restatement"""
    K, W, uv = P.constructed(name)
    world, meas, pairs = P.embedded(K, W, uv, seed=77)
    st, T_out, valid, nsol, ill, counts, exact, T, mask = _pose_check(vo, ctx, K, world, meas, pairs, 1, len(pairs), len(pairs), 77)
    if name == "collinear_below":
        assert not valid[0] and st == 2
    else:
        # ill-posed by the float64 rule (a 1-ulp pixel change moves the restatement's own pose by > P3P_MOVE): validity and
        # the count within +-2 only; the others are compared pose for pose
        assert valid[0] and bool(ill[0]) == (name in ("collinear_above", "danger_cylinder", "near_cylinder"))
        assert ill[0] or (st == 0 and exact[0] >= 11)
