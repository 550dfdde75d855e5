"""vo_estimate_transform[_dev] across the tile edges and grid caps of epi.hip against the float64 fit: 256-row workgroups
(epi_ata_kernel, epi_vote_kernel), 64-row waves, the 512-workgroup cap of epi_max_kernel and epi_ata_kernel (131 072 rows a
pass) and the 1024-workgroup cap of epi_vote_kernel (262 144).  Every case also shows that its tolerance would see the faults
those edges invite: the float64 fit without the rows of the last partial tile, without the grid-stride passes after the
first, or normalised by the maxima of the first 131 072 points only, differs from the full fit by at least 4x the tolerance."""
import ctypes as C

import numpy as np
import pytest

import ransac_restatement as R
from ransac_dev import _p

pytestmark = pytest.mark.gpu

# |X - X_ref| (every entry of R and t): both fit the same 9 x 9 problem in double and round once to float32; the GPU forms the
# normalised rows in float (the float64 fit in double), which moves X by ~3e-8 here (tests/test_gpu_sequence.py uses 2e-5)
TOL = 2e-5
CAP = 512 * 256                        # rows of one grid-stride pass of epi_max_kernel / epi_ata_kernel
SIZES = (8, 9, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025, 4097, 300000)


def tail_rows(n):
    """the rows a skipped last partial tile would lose: the partial workgroup past the last full one; where there is none
    (n <= 256 or a multiple of 256) the partial wave, else the last row -- at least one row is always lost"""
    k = n % 256
    if k == 0 or k == n:
        k = n % 64 or 64
        if k >= n:
            k = 1
    return k


@pytest.fixture(scope="module")
def images(vo):
    """300 000 noisy pairs of synth.frame_pair; each image gets four unpaired points at indices past the first pass of
    epi_max_kernel: a NaN, a negative one, and the image's largest x and largest y (which the maxima must see)"""
    fp = vo.synth.frame_pair(300000, seed=4100)
    p1 = np.concatenate([fp["ref_pts"], [[np.nan, np.nan], [-5, -7], [1280, 3], [2, 960]]]).astype(np.float32)
    p2 = np.concatenate([fp["cur_pts"], [[np.nan, 4], [-9, np.nan], [1280.5, 1], [3, 961]]]).astype(np.float32)
    for p in (p1, p2):
        assert np.nanmax(p[:CAP], 0).max() < 640 and R.image_maxima(p)[0] > 1280 - 1 and R.image_maxima(p)[1] > 960 - 1
    return fp, p1, p2


def _pairs(fp, n):
    """the first n true pairs with far mismatches: ~1 % at random, the rows of tail_rows(n), and 20 past the first pass"""
    rng = np.random.default_rng(n)
    pr = np.ascontiguousarray(fp["gt_matches"][:n], np.int32).copy()
    bad = rng.uniform(size=n) < 0.01
    bad[n - tail_rows(n):] = True
    if n > CAP:
        bad[CAP + rng.integers(0, n - CAP, 20)] = True
    pr[bad, 1] = rng.integers(0, len(fp["cur_pts"]), int(bad.sum()))
    return pr


def _transform_dev(ctx, K, buf, n_live, p1, p2):
    """vo_estimate_transform_dev on device copies of the pair buffer (n_max = len(buf)) and the images: (rc, X)"""
    buf = np.ascontiguousarray(buf, np.int32)
    d_pairs, d_p1, d_p2, d_n = ctx.alloc(buf.nbytes), ctx.alloc(p1.nbytes), ctx.alloc(p2.nbytes), ctx.alloc(8)
    try:
        ctx.h2d(d_pairs, buf); ctx.h2d(d_p1, p1); ctx.h2d(d_p2, p2)
        ctx.h2d(d_n, np.array([n_live], np.int32))
        X = np.zeros(16, np.float32)
        rc = ctx.lib.vo_estimate_transform_dev(ctx.h, _p(np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()),
                                               C.c_void_p(d_pairs), C.c_int(len(buf)), C.c_void_p(d_n), C.c_void_p(d_p1),
                                               C.c_int(len(p1)), C.c_void_p(d_p2), C.c_int(len(p2)), _p(X))
        return rc, X.reshape(4, 4).T.copy()
    finally:
        for d in (d_pairs, d_p1, d_p2, d_n):
            ctx.free(d)


@pytest.mark.parametrize("n", SIZES)
def test_estimate_transform_at_tile_edges(vo, ctx, o32, images, n):
    fp, p1, p2 = images
    K = fp["K"]
    pr = _pairs(fp, n)
    X_ref = R.estimate_transform(o32, K, pr, p1, p2)
    # the tolerance tells the faults apart
    faults = {"last partial tile": R.estimate_transform(o32, K, pr[: n - tail_rows(n)], p1, p2),
              "maxima of the first pass": R.estimate_transform(o32, K, pr, p1, p2, [R.image_maxima(p[:CAP]) for p in (p1, p2)])}
    if n > CAP:
        faults["first grid-stride pass only"] = R.estimate_transform(o32, K, pr[:CAP], p1, p2)
    for name, Xf in faults.items():
        assert np.abs(Xf - X_ref).max() >= 4 * TOL, (name, np.abs(Xf - X_ref).max())
    # the chosen candidate is the one the float64 cheirality count picks
    assert np.abs(R.pose_8point(K, pr, p1, p2, F=R.fundamental(pr, p1, p2)) - X_ref).max() < TOL
    X = vo.estimate_transform(K, pr, p1, p2, ctx=ctx)
    assert np.abs(X - X_ref).max() < TOL, np.abs(X - X_ref).max()
    rc, X_dev = _transform_dev(ctx, K, pr, n, p1, p2)
    assert rc == 0 and X_dev.tobytes() == X.tobytes()                        # host form == _dev at n_max = n, bit for bit
    # n live pairs below a larger n_max: the rows beyond hold wild (in-range) pairs that must not count; the A^T A grid
    # follows n_max, so only the tolerance holds
    n_max = 2 * n + 77
    rng = np.random.default_rng(7 + n)
    buf = np.concatenate([pr, np.stack([rng.integers(0, len(p1), n_max - n), rng.integers(0, len(p2), n_max - n)], 1)])
    rc, X_live = _transform_dev(ctx, K, buf, n, p1, p2)
    assert rc == 0 and np.abs(X_live - X_ref).max() < TOL, np.abs(X_live - X_ref).max()
