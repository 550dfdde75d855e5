"""vo_estimate_pose_ransac_batch_dev on the GPU: every problem bit for bit the single call on it alone (sizes at the tile
edges, ragged and full), isolation of a bad index, scoring against the float64 restatement, the batched solve it feeds,
the fallback, determinism, graph capture and the refusals."""
import ctypes as C

import numpy as np
import pytest

import pose_ransac_batch_cases as B
import pose_ransac_restatement as P
from ransac_batch_dev import BatchDev, V, same, single_results
from ransac_dev import CAM

pytestmark = pytest.mark.gpu

STRIDE = 2304                                                    # 9 workgroups of 256, 2.25 scoring tiles of 1024
LIVE = (0, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 2304)
HYPS = (1, 63, 64, 65, 200)


def _sized(vo, n, seed, frac=0.3):
    """a tracking problem with exactly n pairs (the first n of a problem of at least 16)"""
    fp, world, meas, pairs, bad, clean = P.tracking_problem(vo, max(n, 16), seed=seed, noise_px=0.5, frac=frac, max_angle=0.3, max_t=0.5)
    return fp["K"], (world, meas, pairs[:n])


@pytest.fixture(scope="module")
def edge(vo, ctx):
    """the 12 problems of the edge sizes and their single calls at every hypothesis count, computed once"""
    probs = [_sized(vo, n, 3100 + i) for i, n in enumerate(LIVE)]
    K = probs[0][0]
    probs = [p for _, p in probs]
    singles = [single_results(vo, ctx, K, p, STRIDE, HYPS) for p in probs]
    return K, probs, singles


def test_bit_identity_at_the_edges(vo, ctx, edge):
    K, probs, singles = edge
    b = BatchDev(vo, ctx, K, probs, pairs_stride=STRIDE)
    try:
        for H in HYPS:
            assert b.call(n_hyp=H) == 0, ctx.lib.vo_last_error()
            r = b.results(H)
            for p in range(len(probs)):
                assert same(b.problem(r, p), singles[p][H]), (H, LIVE[p])
            assert r["st"][0] == 1 and r["st"][1] == 1 and r["nin"][0] == 0 and r["nin"][1] == 3
        # a permutation of the problems permutes the outputs
        perm = np.random.default_rng(0).permutation(len(probs))
        b2 = BatchDev(vo, ctx, K, [probs[i] for i in perm], pairs_stride=STRIDE)
        try:
            assert b2.call(n_hyp=65) == 0
            r2 = b2.results(65)
            for k, i in enumerate(perm):
                assert same(b2.problem(r2, k), singles[i][65]), (k, i)
        finally:
            b2.close()
    finally:
        b.close()


def test_full_problems_without_counts_one_problem_and_twins(vo, ctx):
    probs = [_sized(vo, STRIDE, 3200 + i) for i in range(3)]
    K = probs[0][0]
    probs = [p for _, p in probs]
    singles = [single_results(vo, ctx, K, p, STRIDE, HYPS, use_live=False) for p in probs]
    b = BatchDev(vo, ctx, K, probs)
    try:
        for H in HYPS:
            assert b.call(n_hyp=H, live=False) == 0, ctx.lib.vo_last_error()         # d_n_pairs = NULL
            r = b.results(H)
            for p in range(3):
                assert same(b.problem(r, p), singles[p][H]), (H, p)
    finally:
        b.close()
    one = BatchDev(vo, ctx, K, probs[1:2])
    try:
        assert one.call(n_hyp=200) == 0
        assert same(one.problem(one.results(200), 0), singles[1][200])
    finally:
        one.close()
    twins = BatchDev(vo, ctx, K, [probs[2], probs[0], probs[2]])
    try:
        assert twins.call(n_hyp=200) == 0
        r = twins.results(200)
        assert same(twins.problem(r, 0), twins.problem(r, 2)) and same(twins.problem(r, 0), singles[2][200])
    finally:
        twins.close()


def test_a_bad_index_stays_in_its_problem(vo, ctx):
    probs = [_sized(vo, 300 + 7 * i, 3300 + i) for i in range(7)]
    K = probs[0][0]
    probs = [p for _, p in probs]
    stride = max(len(p[2]) for p in probs)
    wild = probs[3][2].copy()
    wild[17, 1] = max(len(p[0]) for p in probs) + 5                  # outside every problem's points, and the stride
    probs[3] = (probs[3][0], probs[3][1], wild)
    b = BatchDev(vo, ctx, K, probs)
    try:
        assert b.call() == 0, ctx.lib.vo_last_error()
        r = b.results()
        T, inl, nin, mask, counts, st = b.problem(r, 3)
        assert st == 4 and nin == len(wild) and np.array_equal(inl, wild) and T == np.eye(4, dtype=np.float32).tobytes()
        assert mask[: len(wild)].all() and not mask[len(wild):].any()
        for p in range(7):
            s = single_results(vo, ctx, K, probs[p], stride, (128,))[128]
            assert same(b.problem(r, p), s), p
            assert (s[5] == 0) == (p != 3)
    finally:
        b.close()


def test_scoring_matches_restatement(vo, ctx):
    fp, world, meas, pairs, bad, clean = P.tracking_problem(vo, 2000, seed=2001, noise_px=0.5, frac=0.4, max_angle=0.3, max_t=0.5)
    others = [_sized(vo, n, 3400 + n)[1] for n in (700, 1999)]
    b = BatchDev(vo, ctx, fp["K"], [others[0], (world, meas, pairs), others[1]])
    try:
        assert b.call(n_hyp=2048) == 0, ctx.lib.vo_last_error()
        T, inl, nin, mask, counts, st = b.problem(b.results(2048), 1)
        ref, win, ref_mask, T_ref = P.ransac(fp["K"], world, meas, pairs, 2.0, 2048, 0, *CAM)
        assert st == 0
        assert np.array_equal(counts < 0, ref < 0)                           # invalid hypotheses agree
        ok = np.abs(counts.astype(np.int64) - ref) <= 2
        assert ok.mean() >= 0.99, (ok.mean(), np.abs(counts - ref).max())
        assert nin == counts.max() == int(mask.sum()) and abs(int(counts.max()) - int(ref.max())) <= 2
        assert np.array_equal(inl, pairs[mask[: len(pairs)].astype(bool)])   # compacted in their original order
    finally:
        b.close()


@pytest.fixture(scope="module")
def recovery(vo, ctx):
    probs = [B.recovery_problem(vo, s) for s in B.RECOVERY_SEEDS]
    K = probs[0][0]["K"]
    b = BatchDev(vo, ctx, K, [(w, m, q) for _, w, m, q, _, _ in probs])
    yield b, probs
    b.close()


def test_feeds_the_batched_solver(vo, ctx, recovery):
    b, probs = recovery
    T_clean = b.solve_host([c for *_, c in probs]).reshape(-1, 4, 4).transpose(0, 2, 1)
    assert b.call(n_hyp=B.N_HYP, thr=B.THR_PX, seed=B.SEED) == 0, ctx.lib.vo_last_error()
    r = b.results(B.N_HYP)
    assert (r["st"] == 0).all() and (r["nin"] >= 6).all()
    T = b.solve(b.d_inl, b.d_nin, b.d_T, B.ROUNDS)
    T_plain = b.solve(b.d_pairs, b.d_n, None, B.ROUNDS)
    for p in range(b.P):
        e = P.pose_errors(T[p].reshape(4, 4).T, T_clean[p])
        e_plain = P.pose_errors(T_plain[p].reshape(4, 4).T, T_clean[p])
        print(B.RECOVERY_SEEDS[p], "robust %.2e %.2e plain %.2e %.2e" % (*e, *e_plain))
        assert e[0] < B.TOL_ROT and e[1] < B.TOL_T, (p, e)
        assert e_plain[0] > B.TOL_ROT or e_plain[1] > B.TOL_T, (p, e_plain)
    # the same batched solve on host-compacted pairs from host-copied winners
    host = [probs[p][3][r["mask"][p, : len(probs[p][3])].astype(bool)] for p in range(b.P)]
    assert all(np.array_equal(host[p], r["inl"][p, : r["nin"][p]]) for p in range(b.P))
    assert b.solve_host(host, r["T"], B.ROUNDS).tobytes() == T.tobytes()


def test_fallback_is_the_plain_problem(vo, ctx, recovery):
    b, probs = recovery
    assert b.call(n_hyp=B.N_HYP, thr=1e-6) == 0
    r = b.results(B.N_HYP)
    assert (r["st"] == 3).all() and np.array_equal(r["nin"], b.n)
    assert r["T"].tobytes() == np.tile(np.eye(4, dtype=np.float32).ravel(), b.P).tobytes()
    assert b.solve(b.d_inl, b.d_nin, b.d_T, B.ROUNDS).tobytes() == b.solve(b.d_pairs, b.d_n, None, B.ROUNDS).tobytes()


def test_determinism_and_capture(vo, ctx, recovery):
    b, probs = recovery
    lib = ctx.lib
    assert b.call(seed=99) == 0
    r1 = b.results()
    assert b.call(seed=99) == 0
    r2 = b.results()
    assert all(r1[k].tobytes() == r2[k].tobytes() for k in ("T", "nin", "mask", "counts", "st"))
    assert all(np.array_equal(r1["inl"][p, : r1["nin"][p]], r2["inl"][p, : r2["nin"][p]]) for p in range(b.P))
    assert b.call(seed=100) == 0
    assert not np.array_equal(r1["counts"], b.results()["counts"])          # another seed, other samples
    # captured after the sizing calls above, replayed twice
    assert b.call(seed=99) == 0
    ctx.h2d(b.d_T, np.zeros(b.P * 16, np.float32)); ctx.h2d(b.d_nin, np.zeros(b.P, np.int32))
    g = C.c_void_p()
    assert lib.vo_ctx_begin_capture(ctx.h) == 0
    rc = b.call(seed=99, fill=False)
    assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
    for _ in range(2):
        ctx.h2d(b.d_T, np.zeros(b.P * 16, np.float32)); ctx.h2d(b.d_nin, np.zeros(b.P, np.int32))
        assert lib.vo_graph_launch(g) == 0
        rr = b.results()
        assert all(rr[k].tobytes() == r1[k].tobytes() for k in ("T", "nin", "mask", "counts", "st"))
    assert lib.vo_graph_destroy(g) == 0
    # a capture that would need a bigger workspace is refused, and the capture stays usable
    assert lib.vo_ctx_begin_capture(ctx.h) == 0
    assert b.call(n_hyp=65536, fill=False) == -6 and b"capture" in lib.vo_last_error()
    assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
    if g.value:
        assert lib.vo_graph_destroy(g) == 0


def test_refusals(vo, ctx):
    K, prob = _sized(vo, 300, 3500)
    b = BatchDev(vo, ctx, K, [prob, prob])
    lib = ctx.lib
    try:
        assert b.call() == 0
        assert b.call(n_problems=C.c_int(0)) == -1 and b.call(n_problems=C.c_int(-2)) == -1
        assert b.call(n_problems=C.c_int(65536)) == -1
        assert b.call(world_stride=C.c_size_t(b.ws - 1)) == -1 and b"stride" in lib.vo_last_error()
        assert b.call(meas_stride=C.c_size_t(b.ms - 1)) == -1 and b"stride" in lib.vo_last_error()
        assert b.call(pairs_stride=C.c_size_t(0)) == -1
        assert b.call(n_world=C.c_int(-1)) == -1
        for k in ("K", "world", "meas", "pairs", "params", "T", "inl", "nin", "st"):
            assert b.call(**{k: None}) == -1, k
        assert b.call(mask=None, counts=None) == 0                           # the optional outputs
        assert b.call(pairs=V(b.d_pairs + 4)) == -1                          # not on an 8-byte boundary
        for prm in ((0, 1.0), (65537, 1.0), (64, 0.0), (64, -1.0), (64, float("inf")), (64, float("nan"))):
            assert b.call(n_hyp=prm[0], thr=prm[1], fill=False) == -1, prm
        singular = np.zeros(9, np.float32)
        assert b.call(K=singular.ctypes.data_as(C.c_void_p)) == -1
        assert b.call() == 0 and (b.results()["st"] == 0).all()
    finally:
        b.close()
