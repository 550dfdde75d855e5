"""The rounds behind round M of a launch-per-round solve share ONE launch (picp.hip, picp_tail_kernel; M = PICP_TAIL_FROM = 16,
VO_PICP_TAIL_FROM per call).  After a detected repeat that launch does the last round's work from the pose history (skip path);
where nothing has repeated yet it runs the rounds in a loop with a grid barrier between two rounds (loop path).  Either way
the results must be the bytes of the launch-per-round solve.

Every expectation comes from the same solver with VO_PICP_TAIL=0 (read per call), never from the tail form: "equal" means the
full state -- pose, T16, H, b, both chi sums, inlier count -- and cycleInfo(), bit for bit.  Where a first repeat (k, j) is
needed it comes from the solver with the detection off (VO_PICP_CYCLE=0), as in test_gpu_cycle_skip.py, and is ASSERTED against
the value the case was chosen by, so that a changed generator fails loudly instead of hollowing a case out.

Sizes: 257 pairs (2 workgroups + the detector: the smallest grid with an exchange) and 8193 pairs (33 workgroups: a second
row group, workgroups on all eight XCDs).  First repeats of the pairs used (detection off):
    frame_pair(257, seed 7)   k, j = 19, 17      frame_pair(8193, seed 3)  10, 8      frame_pair(8193, seed 4)  34, 33
    frame_pair(8193, seed 5)  14, 9              frame_pair(8193, seed 10), outliers kept at threshold 60:  11, 6
No real 257-pair trajectory of seeds 1 .. 119 repeats below round 16 (the pairs are too few for the step to reach rounding
level that early), so the 257-pair case of the skip path at the default M is the all-gated pair of test_gpu_cycle_skip.py --
every world point behind the camera, H = damping I, b = 0: a repeat by round 3.

Which eligible solves take the form is the host's choice from what earlier tail launches of the handle reported (capi.hip,
picp_tail_policy): a fresh handle's first solve does, as a probe.  An explicit VO_PICP_TAIL=1 or VO_PICP_TAIL_FROM takes the
form for every eligible solve, and that is what the cases below set; test_the_host_learns_which_form_pays runs without either.

The real rounds a solve runs inside the tail launch follow from the reference's cycleInfo (d = detected_at, the launch that
found the repeat): with launches skipped the rounds M + 1 .. d, i.e. max(0, d - M); without, all of M + 1 .. N - 1."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M_DEFAULT = 16
# PicpState behind the pose of vo_picp_pose_dev_ptr (vo_internal.h): T16, the control block (5 ints), the history
# (64 poses of 12 floats), then PicpTail: used, rounds, aborted, bar
TAIL_AT = 16 * 4 + 5 * 4 + 64 * 12 * 4
ABORTED_AT = TAIL_AT + 2 * 4


@contextlib.contextmanager
def env(**kv):
    """VO_PICP_<KEY> = value for the duration (None: unset)"""
    names = {"VO_PICP_" + k.upper(): v for k, v in kv.items()}
    old = {n: os.environ.get(n) for n in names}
    try:
        for n, v in names.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = str(v)
        yield
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def state(vo, ctx, s):
    T = s.camera().worldInCameraPose()
    p = C.c_void_p()
    vo.api._chk(ctx.lib.vo_picp_pose_dev_ptr(s.h, C.byref(p)))
    T16 = np.zeros(16, np.float32)
    ctx.d2h(T16, p.value)
    H, b = s.system()
    return (np.ascontiguousarray(T, np.float32).tobytes(), T16.tobytes(), H.tobytes(), b.tobytes(),
            float(s.chiInliers()).hex(), float(s.chiOutliers()).hex(), s.numInliers())


class Case:
    """one problem; its reference solves (VO_PICP_TAIL=0) and detection-off poses are computed once and kept unchanged"""

    def __init__(self, vo, ctx, fp, keep=False, thr=None):
        self.vo, self.ctx, self.fp, self.keep = vo, ctx, fp, keep
        gm = fp["gt_matches"]
        self.corr = np.stack([gm[:, 1], fp["model_pairs"][gm[:, 0], 1]], 1).astype(np.int32)
        self.cam = vo.Camera(fp["rows"], fp["cols"], fp["z_near"], fp["z_far"], fp["K"].copy(), np.eye(4), ctx=ctx)
        self.thr = thr if thr is not None else (40.0 if keep else 10000.0)
        self._ref, self._off = {}, {}

    def start(self, s):
        s.setKernelThreshold(self.thr)
        s.init(self.cam, self.fp["model"], self.fp["cur_pts"])          # pose back to the identity, pairs to be gathered anew

    def solve(self, n, s=None, **kv):
        """(state, cycleInfo, tailInfo) of a solve of n rounds from the identity under VO_PICP_<kv>, on a fresh handle unless
        one is given"""
        own = s is None
        if own:
            s = self.vo.PICPSolver(self.ctx)
        with env(**kv):
            self.start(s)
            s.solve(self.corr, self.keep, n)
        out = state(self.vo, self.ctx, s), s.cycleInfo(), s.tailInfo()
        if own:
            s.close()
        return out

    def ref(self, n):
        """the launch-per-round solve"""
        if n not in self._ref:
            st, info, tail = self.solve(n, tail=0)
            assert tail == (False, 0, False)
            self._ref[n] = (st, info)
        return self._ref[n]

    def first_repeat(self, upto):
        """(k, j) of the detection-off trajectory's first repeat within rounds 0 .. upto, or None"""
        poses = [np.eye(4, dtype=np.float32).tobytes()]
        for k in range(1, upto + 1):
            if k not in self._off:
                self._off[k] = self.solve(k, cycle=0)[0][0]
            poses.append(self._off[k])
            for j in range(k - 1, -1, -1):
                if poses[j] == poses[k]:
                    return k, j
        return None


def real_in_launch(info, n, m):
    """real rounds inside the tail launch of a solve of n rounds with M = m, from the reference's cycleInfo"""
    d, _, skipped = info
    return max(0, d - m) if skipped > 0 else n - 1 - m


def check(case, n, m=None, s=None):
    """a solve of n rounds in the tail form with M = m (None: the default) against the launch-per-round solve"""
    st, info, tail = case.solve(n, s, tail_from=m, tail=1 if m is None else None)      # (either asks for the form explicitly)
    want_st, want_info = case.ref(n)
    mm = M_DEFAULT if m is None else m
    used = n - 1 > mm + 1
    want_tail = (True, real_in_launch(want_info, n, mm), False) if used else (False, 0, False)
    print(f"N = {n}, M = {mm}: cycleInfo {info} (reference {want_info}), tailInfo {tail} (expected {want_tail})")
    assert info == want_info
    assert st == want_st
    assert tail == want_tail
    return info, tail


def gated_pair(vo, n):
    fp = vo.synth.frame_pair(n, seed=11)
    fp["model"] = fp["model"].copy()
    fp["model"][:, 2] = -np.abs(fp["model"][:, 2]) - 1.0            # every world point behind the camera
    return fp


@pytest.fixture(scope="module")
def cases(vo, ctx):
    c = {
        "gated257": Case(vo, ctx, gated_pair(vo, 257)),
        "p257": Case(vo, ctx, vo.synth.frame_pair(257, seed=7)),
        "p8193_early": Case(vo, ctx, vo.synth.frame_pair(8193, seed=3)),
        "p8193_late": Case(vo, ctx, vo.synth.frame_pair(8193, seed=4)),
        "p8193": Case(vo, ctx, vo.synth.frame_pair(8193, seed=5)),
        "p8193_keep": Case(vo, ctx, vo.synth.frame_pair(8193, seed=10), keep=True, thr=60.0),
    }
    for name, case in c.items():
        assert len(case.corr) == (257 if "257" in name else 8193), name      # 2 and 33 workgroups
    return c


@pytest.mark.parametrize("name", ["gated257", "p8193_early"])
def test_skip_path_at_the_default_m(cases, name):
    """the repeat lies below M: the tail launch does launch N - 1's work from the history, no round runs inside it; a solve of
    M + 2 rounds is too short for the form"""
    case = cases[name]
    rep = case.first_repeat(M_DEFAULT)
    assert rep is not None and rep[0] < M_DEFAULT - 1, rep
    if name == "p8193_early":
        assert rep == (10, 8)
    for n in (M_DEFAULT + 2, M_DEFAULT + 3, M_DEFAULT + 4, 50, 100):
        info, tail = check(case, n)
        assert info[0] == rep[0] + 1 and tail == (n > M_DEFAULT + 2, 0, False)


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("name,rep", [("p257", (19, 17)), ("p8193", (14, 9))])
def test_loop_path(cases, name, rep, m):
    """M = 1 and 2: the tally round alone, or one more round, has a launch of its own and real rounds run inside the tail
    launch.  N = k + 2 .. k + 3 + period (the edges of test_gpu_cycle_skip.py::test_edges): the repeat is found inside the loop
    in its last or last but one round (nothing to skip), with exactly one skipped round, and with the target on every residue of
    the period; N = 4 and 5: the shortest solves"""
    case = cases[name]
    assert case.first_repeat(rep[0]) == rep
    k, j = rep
    ran = {n: check(case, n, m) for n in [4, 5] + list(range(k + 2, k + 4 + (k - j)))}
    assert ran[k + 2][0][2] == 0 and ran[k + 3][0][2] == 0 and ran[k + 4][0][2] == 1
    assert ran[k + 4][1] == (True, k + 1 - m, False)                # rounds M + 1 .. k + 1 ran, round k + 2 was skipped
    assert ran[4][1][0] == (m == 1) and ran[5][1] == (True, 4 - m, False)


@pytest.mark.parametrize("name,rep", [("p257", (19, 17)), ("p8193_late", (34, 33))])
def test_loop_path_without_a_repeat(cases, name, rep):
    """N <= k: ten real rounds inside the launch, nothing detected, nothing skipped"""
    case = cases[name]
    assert case.first_repeat(rep[0]) == rep and rep[0] >= 7
    info, tail = check(case, 12, 1)
    assert info == (0, 0, 0) and tail == (True, 10, False)


def test_uneven_arrival(vo, ctx, cases):
    """outliers kept at threshold 60: the workgroups hold different numbers of inliers and reach the barrier at different
    times; and once the solve is enqueued directly behind a large unrelated kernel on the same stream (a matcher call)"""
    case, (k, j) = cases["p8193_keep"], (11, 6)
    assert case.first_repeat(k) == (k, j)
    for n in [8] + list(range(k + 2, k + 4 + (k - j))):
        check(case, n, 1)
    big = vo.synth.frame_pair(20000, seed=1)
    d_ref, d_cur = ctx.to_device(big["ref_app"]), ctx.to_device(big["cur_app"])
    nq = min(len(big["ref_app"]), len(big["cur_app"]))
    d_m, d_cnt, d_ident = ctx.alloc(nq * 8), ctx.alloc(64), ctx.to_device(np.eye(4, dtype=np.float32))
    n = k + 4

    def match():
        vo.api._chk(ctx.lib.vo_match_appearances_dev(ctx.h, C.c_void_p(d_ref), C.c_int(len(big["ref_app"])), C.c_void_p(d_cur),
                                                     C.c_int(len(big["cur_app"])), C.c_float(0.1), C.c_void_p(d_m), C.c_void_p(d_cnt)))

    def behind_matcher(s, **kv):
        """warm the handle and the matcher (pairs uploaded, graph captured, workspaces made), then pose reset + matcher +
        solve without a host wait between"""
        with env(**kv):
            case.start(s)
            s.solve(case.corr, case.keep, n)
            match()
            ctx.synchronize()
            vo.api._chk(ctx.lib.vo_picp_set_pose_dev(s.h, C.c_void_p(d_ident)))
            match()
            s.solve(case.corr, case.keep, n)
        return state(vo, ctx, s), s.cycleInfo(), s.tailInfo()

    a, b = vo.PICPSolver(ctx), vo.PICPSolver(ctx)
    want = behind_matcher(a, tail=0)
    got = behind_matcher(b, tail_from=1)
    a.close()
    b.close()
    for p in (d_ref, d_cur, d_m, d_cnt, d_ident):
        ctx.free(p)
    assert want[2] == (False, 0, False) and want[:2] == case.ref(n)
    assert got[:2] == want[:2]
    assert got[2] == (True, real_in_launch(want[1], n, 1), False) and got[2][1] >= 5


def test_host_choice(vo, ctx):
    """the tail launch needs a CU per workgroup, the detector's included: 256 n_CU + 1 pairs (n_CU + 1 workgroups) keep a
    launch per round, 256 (n_CU - 1) pairs are the largest problem in the form"""
    n_cu = ctx.device_info()[1]
    assert n_cu >= 8
    over = Case(vo, ctx, vo.synth.frame_pair(256 * n_cu + 1, seed=3))
    assert len(over.corr) == 256 * n_cu + 1
    st, info, tail = over.solve(18, tail_from=14)
    assert tail == (False, 0, False) and (st, info) == over.ref(18)
    full = Case(vo, ctx, vo.synth.frame_pair(256 * (n_cu - 1), seed=3))
    assert len(full.corr) == 256 * (n_cu - 1)
    info, tail = check(full, 18, 14)
    assert tail[0]
    # (a pair of this size repeats within ten rounds, so at M = 14 the launch takes the skip path: the rounds that cross the
    # barrier with a workgroup on every CU are those of a short solve at M = 1)
    info, tail = check(full, 8, 1)
    assert tail[0] and tail[1] >= 4


def test_nothing_left_behind(vo, ctx, cases):
    """a solve that went through the loop path, another pair behind a pose reset, the first pair again: each the bytes of the
    launch-per-round solve on a fresh handle; and a chain of oneRound calls behind a tail solve gives the bytes of the same
    chain on a handle that never ran the form"""
    a, b = cases["p8193"], cases["p8193_keep"]
    s = vo.PICPSolver(ctx)
    assert check(a, 12, 1, s)[1] == (True, 10, False)
    assert check(b, 30, None, s)[1][0]
    assert check(a, 12, 1, s)[1] == (True, 10, False)
    assert check(a, 30, None, s)[1] == (True, 0, False)

    def chain(h, **kv):
        with env(**kv):
            a.start(h)
            for _ in range(6):
                h.oneRound(a.corr, a.keep)
        return state(vo, ctx, h)

    fresh = vo.PICPSolver(ctx)
    want = chain(fresh, tail=0)
    got = chain(s)
    fresh.close()
    s.close()
    assert got == want


def test_abort_is_reported_by_the_getters(vo, ctx, cases):
    """host side only: `aborted` written behind a finished solve makes the next getter fail with the reason; cleared, the
    getters answer again, and the next solve starts clean whatever the word held"""
    case = cases["p8193_early"]
    s = vo.PICPSolver(ctx)
    st, info, tail = case.solve(30, s)
    assert tail == (True, 0, False) and (st, info) == case.ref(30)
    p = C.c_void_p()
    vo.api._chk(ctx.lib.vo_picp_pose_dev_ptr(s.h, C.byref(p)))
    ctx.h2d(p.value + ABORTED_AT, np.array([1], np.int32))
    assert s.tailInfo() == (True, 0, True)
    with pytest.raises(vo.api.VoError, match="tail launch of the last solve gave up"):
        s.camera()
    with pytest.raises(vo.api.VoError, match="tail launch of the last solve gave up"):
        s.numInliers()
    ctx.h2d(p.value + ABORTED_AT, np.array([0], np.int32))
    assert state(vo, ctx, s) == st
    ctx.h2d(p.value + ABORTED_AT, np.array([1], np.int32))
    assert case.solve(30, s) == (st, info, (True, 0, False))
    s.close()


def test_the_host_learns_which_form_pays(vo, ctx, cases):
    """no VO_PICP_TAIL, no VO_PICP_TAIL_FROM: a fresh handle's first eligible solve takes the form, as a probe.  Where its tail
    launch had to run real rounds (the pair repeats at round 34, M = 16: 13 of them) the handle goes back to a launch per round;
    where it took the skip path the handle stays in the form -- until a tail launch runs real rounds.  Same bytes throughout.
    (Every solve here is followed by getters, so each report has arrived before the next solve is enqueued.)"""
    late, early = cases["p8193_late"], cases["p8193_early"]
    s = vo.PICPSolver(ctx)
    tails = []
    for _ in range(4):
        st, info, tail = late.solve(30, s)
        assert (st, info) == late.ref(30)
        tails.append(tail)
    assert tails == [(True, 13, False)] + 3 * [(False, 0, False)], tails
    s.close()
    s = vo.PICPSolver(ctx)
    tails = []
    for case in (early, early, early, late, late, early):
        st, info, tail = case.solve(30, s)
        assert (st, info) == case.ref(30)
        tails.append(tail)
    assert tails == 3 * [(True, 0, False)] + [(True, 13, False)] + 2 * [(False, 0, False)], tails
    s.close()
