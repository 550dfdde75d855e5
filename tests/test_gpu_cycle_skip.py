"""A launch-per-round solve skips the rounds whose pose has already occurred in it (picp.hip, picp_cycle_detect): once the
pose after round k equals, bit for bit, the pose after an earlier round j, the launches that follow return at once and the
last round launch takes its pose from the history.  The results must be the bytes of the full solve.

Every expectation comes from the solver with the detection OFF (VO_PICP_CYCLE=0, read per call), never from the code under
test: a case is solved with n_iters = 1 .. K from the identity, the first repeat (k, j) of the pose -- pose 0 = identity, the
most recent j -- is found on the host, and with the detection on and N rounds the solver must report

    detected_at = k + 1,  period = k - j,  skipped = max(0, N - 3 - k)        (nothing, where k > N - 2)

and leave the pose, T16, H, b, both chi sums, the inlier count and the bad-index state of the detection-off solve of N rounds.

Real trajectories: frame_pair(8193, seed) for seeds 2, 4, 6 and frame_pair(20000, seed) for seeds 1, 5, 6, K = N = 48 (33 and
79 workgroups).  At least two of the six must repeat with a period >= 2 by round 44 in the detection-off trajectory, or the
test fails as not exercising the path."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_ROUNDS = 48
REAL = [(8193, 2), (8193, 4), (8193, 6), (20000, 1), (20000, 5), (20000, 6)]
# PicpState behind T16 (vo_internal.h): the control block (5 ints), then the history of PICP_HIST poses of 12 floats
CTL_BYTES, HIST_FLOATS = 20, 64 * 12


@contextlib.contextmanager
def cycle(on):
    old = os.environ.get("VO_PICP_CYCLE")
    os.environ["VO_PICP_CYCLE"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["VO_PICP_CYCLE"]
        else:
            os.environ["VO_PICP_CYCLE"] = old


class Case:
    """one problem: points, pairs, camera, outlier handling; its detection-off trajectory is computed once and kept"""

    def __init__(self, vo, ctx, fp, keep=False, general=False):
        self.vo, self.ctx, self.fp, self.keep = vo, ctx, fp, keep
        gm = fp["gt_matches"]
        self.corr = np.stack([gm[:, 1], fp["model_pairs"][gm[:, 0], 1]], 1).astype(np.int32)
        K = fp["K"].copy()
        if general:                      # not a pinhole matrix (the general instantiation of the round kernels)
            K[0, 1] = 0.7
            K[2, 2] = 1.0009765625
        self.cam = vo.Camera(fp["rows"], fp["cols"], fp["z_near"], fp["z_far"], K, np.eye(4), ctx=ctx)
        self.thr = 40.0 if keep else 10000.0
        self._off = {}

    def start(self, s):
        s.setKernelThreshold(self.thr)
        s.init(self.cam, self.fp["model"], self.fp["cur_pts"])          # pose back to the identity, pairs to be gathered anew

    def solve(self, n, on, s=None):
        """(state bytes, cycleInfo) of a solve of n rounds from the identity, on a fresh handle unless one is given"""
        own = s is None
        if own:
            s = self.vo.PICPSolver(self.ctx)
        with cycle(on):
            self.start(s)
            s.solve(self.corr, self.keep, n)
        out = state(self.vo, self.ctx, s), s.cycleInfo()
        if own:
            s.close()
        return out

    def off(self, n):
        if n not in self._off:
            self._off[n] = self.solve(n, False)
        return self._off[n]

    def first_repeat(self, upto=K_ROUNDS):
        """(k, j) of the detection-off trajectory's first repeat within rounds 0 .. upto, or None"""
        poses = [np.eye(4, dtype=np.float32).tobytes()] + [self.off(n)[0][0] for n in range(1, upto + 1)]
        for k in range(1, upto + 1):
            for j in range(k - 1, -1, -1):
                if poses[j] == poses[k]:
                    return k, j
        return None


def state(vo, ctx, s):
    try:
        T = s.camera().worldInCameraPose()
    except vo.api.VoError as e:
        return ("error", e.code, str(e))
    p = C.c_void_p()
    vo.api._chk(ctx.lib.vo_picp_pose_dev_ptr(s.h, C.byref(p)))
    T16 = np.zeros(16, np.float32)
    ctx.d2h(T16, p.value)
    H, b = s.system()
    return (np.ascontiguousarray(T, np.float32).tobytes(), T16.tobytes(), H.tobytes(), b.tobytes(),
            float(s.chiInliers()).hex(), float(s.chiOutliers()).hex(), s.numInliers())


def expected_info(rep, n):
    if rep is None or rep[0] > n - 2:
        return (0, 0, 0)
    k, j = rep
    return (k + 1, k - j, max(0, n - 3 - k))


def check(case, n, rep, s=None):
    got, info = case.solve(n, True, s)
    want, info_off = case.off(n)
    print(f"N = {n}: first repeat {rep}, cycleInfo {info} (expected {expected_info(rep, n)})")
    assert info_off == (0, 0, 0)
    assert want[0] != "error"
    assert info == expected_info(rep, n)
    assert got == want
    return info


@pytest.fixture(scope="module")
def real(vo, ctx):
    return {key: Case(vo, ctx, vo.synth.frame_pair(key[0], seed=key[1])) for key in REAL}


@pytest.fixture(scope="module")
def repeating(real):
    """the first real case whose detection-off trajectory repeats with a period >= 2 by round 44"""
    for key in REAL:
        rep = real[key].first_repeat()
        if rep is not None and rep[0] <= 44 and rep[0] - rep[1] >= 2:
            return real[key], rep
    pytest.fail("no real trajectory repeats with a period >= 2 by round 44")


def test_all_gated_pair(vo, ctx):
    fp = vo.synth.frame_pair(600, seed=11)
    fp["model"] = fp["model"].copy()
    fp["model"][:, 2] = -np.abs(fp["model"][:, 2]) - 1.0            # every world point behind the camera: H = damping I, b = 0
    case = Case(vo, ctx, fp)
    rep = case.first_repeat(8)
    assert rep is not None and rep[0] - rep[1] == 1 and rep[0] <= 3, rep
    assert check(case, 6, rep)[2] == 3 - rep[0]
    assert check(case, 20, rep)[2] == 17 - rep[0] > 0


@pytest.mark.parametrize("key", REAL, ids=[f"{n}-pairs-seed-{s}" for n, s in REAL])
def test_real_trajectory(real, key):
    case = real[key]
    check(case, K_ROUNDS, case.first_repeat())


def test_real_trajectories_exercise_the_path(real):
    reps = {key: real[key].first_repeat() for key in REAL}
    print(reps)
    good = [key for key, r in reps.items() if r is not None and r[0] <= 44 and r[0] - r[1] >= 2]
    assert len(good) >= 2, reps


def test_edges(repeating):
    """N = k + 2: the repeat is found in the last round launch, N = k + 3: in the one before it -- too late to skip anything;
    N = k + 4: exactly one skipped launch; on to N = k + 3 + period: the target lands on every residue of the period.  One
    round fewer than k + 2 and the repeat is not seen at all."""
    case, (k, j) = repeating
    skipped = {n: check(case, n, (k, j))[2] for n in range(k + 2, k + 4 + (k - j))}
    assert skipped[k + 2] == 0 and skipped[k + 3] == 0 and skipped[k + 4] == 1
    assert check(case, k + 1, (k, j)) == (0, 0, 0)


def test_reset_between_solves(vo, ctx, real, repeating):
    """nothing of a solve that skipped is left for the next: another pair behind a pose reset, then the same pairs again
    (cached: round 0 does not gather), each the bytes of a fresh handle that never detected anything"""
    case, rep = repeating
    other = real[REAL[0]] if case is not real[REAL[0]] else real[REAL[1]]
    n = 30
    fresh = vo.PICPSolver(ctx)
    with cycle(False):
        other.start(fresh)
        fresh.solve(other.corr, other.keep, n)
        want1 = state(vo, ctx, fresh)
        fresh.solve(other.corr, other.keep, n)                        # from the pose the first solve left
        want2 = state(vo, ctx, fresh)
    fresh.close()
    s = vo.PICPSolver(ctx)
    assert check(case, K_ROUNDS, rep, s)[2] > 0
    with cycle(True):
        other.start(s)
        s.solve(other.corr, other.keep, n)
        got1, info1 = state(vo, ctx, s), s.cycleInfo()
        s.solve(other.corr, other.keep, n)
        got2, info2 = state(vo, ctx, s), s.cycleInfo()
    s.close()
    print(info1, info2)
    assert info1 == expected_info(other.first_repeat(), n)
    assert got1 == want1 and got2 == want2


@pytest.mark.parametrize("form", ["keep_outliers", "general_camera"])
def test_other_instantiations(vo, ctx, form):
    """one repeating case each with the outliers kept (threshold 40) and with a camera matrix that is not a pinhole's"""
    tried = {}
    for n, seed in REAL:
        case = Case(vo, ctx, vo.synth.frame_pair(n, seed=seed), keep=form == "keep_outliers", general=form == "general_camera")
        rep = case.first_repeat()
        tried[(n, seed)] = rep
        if rep is not None and rep[0] <= 44:
            assert check(case, K_ROUNDS, rep)[2] > 0
            return
    pytest.fail(f"no trajectory repeats by round 44: {tried}")


def test_switched_off(vo, ctx, repeating):
    """VO_PICP_CYCLE=0: nothing detected, nothing skipped, and no detector workgroup in any launch -- the history, which only
    that workgroup writes, keeps what was put there before the solve; with the detection on it holds the solve's poses"""
    case, rep = repeating
    s = vo.PICPSolver(ctx)
    p = C.c_void_p()
    vo.api._chk(ctx.lib.vo_picp_pose_dev_ptr(s.h, C.byref(p)))
    d_hist = p.value + 16 * 4 + CTL_BYTES
    mark = np.full(HIST_FLOATS, -77.0, np.float32)
    hist = np.zeros(HIST_FLOATS, np.float32)
    ctx.h2d(d_hist, mark)
    got, info = case.solve(K_ROUNDS, False, s)
    ctx.d2h(hist, d_hist)
    assert info == (0, 0, 0) and got == case.off(K_ROUNDS)[0]
    assert np.array_equal(hist, mark)
    got, info = case.solve(K_ROUNDS, True, s)
    ctx.d2h(hist, d_hist)
    assert info == expected_info(rep, K_ROUNDS) and got == case.off(K_ROUNDS)[0]
    k = rep[0]
    rows = hist.reshape(64, 12)
    assert not (rows[:k + 1] == -77.0).any() and (rows[k + 1:] == -77.0).all()      # rounds 0 .. k, and nothing behind them
    assert rows[0].tobytes() == np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32).tobytes()
    s.close()
