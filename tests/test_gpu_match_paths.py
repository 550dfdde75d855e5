"""Every public matcher mode (vo_match_set_mode 0..5) through every entry point that shares the one host path of the matcher
(capi.hip: match_frames): vo_match_appearances_dev, vo_match_appearances_batch_dev with equal and with per-frame sizes, and
the matches / counts of vo_frames_batch_dev, vo_frames_batch_ragged_dev and vo_frames_batch_track_dev.  Every frame of every
call must give the oracle's pairs, entry for entry: the matcher is exact, whatever search the mode picks.

Sizes: the larger image of a frame has n = 700, 1793 (one row past a level-1 slice of the cell sort) or 3201 rows (one past the
fill at which the exact-duplicate pass changes its table size), the smaller one n - n // 8; calls of 1 and of 9 frames (one
past the grouping by eight).  Frames come from synth.frame_pair with rows dropped and distractors; every third row of the
current image is moved a little, so that it is no bitwise copy any more and the search BEHIND the exact-duplicate pass has
pairs to find too.  At n = 3201 and 9 frames mode 0 sorts and runs the pass by itself, steering included.

Per-frame sizes in modes 2 and 4: the bucket-pruned scan takes one size only, so such a call runs the full scan or -- where the
rule sorts -- the cell-hash search.  Pairs cannot tell those two apart, but they do tell them from a bucket-pruned scan that
ignored the sizes: the rows beyond a frame's size are zeros in BOTH images, which such a scan would pair with each other."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_frames_track import Call

pytestmark = pytest.mark.gpu

NS = (700, 1793, 3201)
MODES = (0, 1, 2, 3, 4, 5)
F = 9
V = C.c_void_p


def _cut(f, n_ref=None, n_cur=None):
    """frame f with its images cut to their first n_ref / n_cur rows (model pairs of the rows that went are dropped)"""
    g = dict(f)
    if n_ref is not None:
        g["ref_app"], g["ref_pts"] = f["ref_app"][:n_ref].copy(), f["ref_pts"][:n_ref].copy()
        g["model_pairs"] = f["model_pairs"][f["model_pairs"][:, 0] < n_ref].copy()
    if n_cur is not None:
        g["cur_app"], g["cur_pts"] = f["cur_app"][:n_cur].copy(), f["cur_pts"][:n_cur].copy()
    return g


class Case:
    """the frames of one n and what the oracle says about them, computed once"""

    def __init__(self, vo, o32, n):
        self.n, m = n, n - n // 8
        self.m = m
        rng = np.random.default_rng(n)
        self.frames = []
        for k in range(F):
            fp = vo.synth.frame_pair(n, seed=7100 + 16 * n + k, drop=0.1, distractors=n // 10, model_drop=0.1)
            assert len(fp["ref_app"]) >= m and len(fp["cur_app"]) >= n
            f = _cut(fp, m, n)
            f["cur_app"][::3] += rng.normal(0, 2e-3, f["cur_app"][::3].shape).astype(np.float32)
            self.frames.append(f)
        A = [f["ref_app"] for f in self.frames]
        B = [f["cur_app"] for f in self.frames]
        match = lambda a1, a2: o32.match(a1, a2) if len(a1) and len(a2) else np.zeros((0, 2), np.int32)
        self.exp = [match(a, b) for a, b in zip(A, B)]
        assert all(0.7 * m < len(e) < m for e in self.exp)               # most queries have a partner, some have none
        # per-frame sizes n, n - 1, 1, 0 with either image the larger
        self.r1 = [A[0], B[1], A[2], B[3][: n - 1], A[4][:1], B[5], A[6][:0], B[7][:1], A[8]]
        self.r2 = [B[0], A[1], B[2][: n - 1], A[3], B[4], A[5][:0], B[6][:0], A[7][:1], B[8]]
        self.exp_r = [self.exp[k] if k in (0, 8) else match(a1, a2) for k, (a1, a2) in enumerate(zip(self.r1, self.r2))]
        # whole frames of different sizes: the current image one row short, either image the larger, a short reference image
        cuts = {1: (None, m // 2), 2: (None, n - 1), 3: (m // 3, None), 5: (None, m // 2), 6: (m // 3, None)}
        self.frames_r = [_cut(f, *cuts[k]) if k in cuts else f for k, f in enumerate(self.frames)]
        self.exp_fr = [self.exp_r[2] if k == 2 else match(f["ref_app"], f["cur_app"]) if k in cuts else self.exp[k]
                       for k, f in enumerate(self.frames_r)]
        assert any(len(f["ref_app"]) > len(f["cur_app"]) for f in self.frames_r)
        self.calls = {}

    def call(self, vo, ctx, n_frames, ragged):
        """the resident many-frames call of these frames (kept for all modes)"""
        key = (n_frames, ragged)
        if key not in self.calls:
            self.calls[key] = Call(vo, ctx, (self.frames_r if ragged else self.frames)[:n_frames], n_iters=0, ragged=ragged)
        return self.calls[key]

    def close(self):
        for c in self.calls.values():
            c.close()


@pytest.fixture(scope="module")
def cases(vo, o32):
    made = {}

    def get(n):
        if n not in made:
            made[n] = Case(vo, o32, n)
        return made[n]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(params=MODES, ids=lambda m: f"mode{m}")
def mode(request, ctx):
    assert ctx.lib.vo_match_set_mode(ctx.h, request.param) == 0
    yield request.param
    assert ctx.lib.vo_match_set_mode(ctx.h, 0) == 0


def _batch(vo, ctx, a1, a2, ragged):
    """vo_match_appearances_batch_dev on the lists a1 / a2 of one array per frame; equal sizes: no size arrays"""
    if ragged:
        return vo.match_batch_ragged(ctx, a1, a2)
    n_f, n1, n2 = len(a1), len(a1[0]), len(a2[0])
    q = min(n1, n2)
    d = [ctx.to_device(np.ascontiguousarray(np.stack(a1))), ctx.to_device(np.ascontiguousarray(np.stack(a2))),
         ctx.alloc(n_f * q * 8), ctx.alloc(n_f * 4)]
    try:
        rc = ctx.lib.vo_match_appearances_batch_dev(ctx.h, C.c_int(n_f), V(d[0]), C.c_int(n1), None, V(d[1]), C.c_int(n2), None,
                                                    C.c_float(0.1), V(d[2]), V(d[3]))
        assert rc == 0, ctx.lib.vo_last_error()
        cnt = np.zeros(n_f, np.int32); ctx.d2h(cnt, d[3])
        out = np.zeros((n_f, q, 2), np.int32); ctx.d2h(out, d[2])
    finally:
        for x in d:
            ctx.free(x)
    return [out[f, : cnt[f]] for f in range(n_f)]


def _same(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        assert np.array_equal(g, e), (what, k, len(g), len(e))


@pytest.mark.parametrize("n", NS)
def test_single_frame_call(vo, ctx, cases, mode, n):
    """vo_match_appearances_dev, the reference image the smaller and the larger set"""
    c = cases(n)
    f = c.frames[0]
    assert np.array_equal(vo.compute_correspondences_images(f["ref_app"], f["cur_app"], ctx=ctx), c.exp[0])
    assert np.array_equal(vo.compute_correspondences_images(c.r1[1], c.r2[1], ctx=ctx), c.exp_r[1])


@pytest.mark.parametrize("n", NS)
def test_batched_call_of_equal_sizes(vo, ctx, cases, mode, n):
    """vo_match_appearances_batch_dev without size arrays: 9 frames, and 1 frame with the first image the larger"""
    c = cases(n)
    _same(_batch(vo, ctx, [f["ref_app"] for f in c.frames], [f["cur_app"] for f in c.frames], False), c.exp, "9 frames")
    _same(_batch(vo, ctx, c.r1[1:2], c.r2[1:2], False), c.exp_r[1:2], "1 frame")


@pytest.mark.parametrize("n", NS)
def test_batched_call_of_per_frame_sizes(vo, ctx, cases, mode, n):
    """the same call with size arrays: sizes n, n - 1, 1 and 0, either image the larger; 9 frames and 1 frame"""
    c = cases(n)
    _same(_batch(vo, ctx, c.r1, c.r2, True), c.exp_r, "9 frames")
    _same(_batch(vo, ctx, c.r1[3:4], c.r2[3:4], True), c.exp_r[3:4], "1 frame")


@pytest.mark.parametrize("n_frames", (1, F))
@pytest.mark.parametrize("n", NS)
def test_many_frames_calls(vo, ctx, cases, mode, n, n_frames):
    """matches / counts of vo_frames_batch_dev and vo_frames_batch_track_dev (equal sizes), vo_frames_batch_ragged_dev and
    vo_frames_batch_track_dev (per-frame sizes)"""
    c = cases(n)
    for ragged, exp in ((False, c.exp), (True, c.exp_fr)):
        call = c.call(vo, ctx, n_frames, ragged)
        for what, r in (("plain", call.plain()), ("track", call.track())):
            got = [np.frombuffer(b, np.int32).reshape(-1, 2) for b in r["matches"]]
            assert r["counts"][0].tolist() == [len(e) for e in exp[:n_frames]], (what, ragged)
            _same(got, exp[:n_frames], (what, ragged))
