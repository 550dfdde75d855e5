"""vo_map_lookup[_dev|_batch_dev] on the GPU against the dictionary restatement (tests/map_localise_restatement.py), exactly:
entries, pairs, counts and gathered points over the tile edges of the 256-row workgroups and the map sizes at which the table
is empty, full at its initial capacity, just grown and re-hashed; the batched form against the single one; capture and
replay; what a lookup must leave alone; refusals."""
import ctypes as C

import numpy as np
import pytest

import map_localise_restatement as M
from map_dev import Lookup, check_lookup, make_map_rows, make_queries

pytestmark = pytest.mark.gpu

QUERY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2304)


def _map(vo, ctx, n, seed=0):
    rng = np.random.default_rng(seed)
    pts, app = make_map_rows(rng, n)
    m = vo.Map(ctx)                                  # initial capacity: 1024 entries
    if n:
        m.update(pts[:1024], app[:1024])             # up to a full map ...
    if n > 1024:
        m.update(pts[1024:], app[1024:])             # ... that grows, and re-hashes the 1024 entries it holds
    return m, rng


@pytest.mark.parametrize("size", [0, 1, 1024, 1025, 5000])
def test_every_query_count_against_the_restatement(vo, ctx, size):
    m, rng = _map(vo, ctx, size, seed=size)
    try:
        m_pts, m_app = m.read()
        assert len(m_app) == size
        tab = M.table(m_app)
        for n in QUERY_COUNTS:
            q = make_queries(rng, m_app, n)
            ent, pairs, xyz = M.lookup(m_app, q, m_pts, tab=tab)
            if size >= 1024:
                assert 0 < len(pairs) < n or n == 1
            d = Lookup(ctx, q)
            assert d.call(m) == 0, ctx.lib.vo_last_error()
            check_lookup(d.results(), 0, ent, pairs, xyz)
            d.close()
            # *d_n below n_max: the rows behind it are not looked up, their positions read -1
            live = (2 * n) // 3
            ent, pairs, xyz = M.lookup(m_app, q, m_pts, n_live=live, tab=tab)
            d = Lookup(ctx, q, n_live=[live], entries=(n % 2 == 0))          # with and without the per-position output
            assert d.call(m) == 0, ctx.lib.vo_last_error()
            check_lookup(d.results(), 0, ent, pairs, xyz)
            d.close()
            # the host form
            hp, he, hx = m.lookup(q, want_points=True)
            ent, pairs, xyz = M.lookup(m_app, q, m_pts, tab=tab)
            assert np.array_equal(he, ent) and np.array_equal(hp, pairs) and hx.tobytes() == xyz.tobytes()
        assert len(m) == size                                                # a lookup never grows the map
    finally:
        m.close()


def test_duplicates_zero_signs_and_nans(vo, ctx):
    """the rules one by one, on a map whose entries are known"""
    rng = np.random.default_rng(3)
    app = rng.uniform(-1, 1, (40, 10)).astype(np.float32)
    app[4, 2] = 0.0
    app[9, 5] = np.nan
    pts = rng.uniform(-5, 5, (40, 3)).astype(np.float32)
    m = vo.Map(ctx)
    try:
        m.update(pts, app)
        q = np.stack([app[7], app[7], app[4], app[4], app[9], app[3], app[3] + 1])
        q[3, 2] = -0.0
        q[5, 0] = np.nan
        pairs, ent = m.lookup(q)
        assert ent.tolist() == [7, 7, 4, 4, -1, -1, -1]
        assert pairs.tolist() == [[0, 7], [1, 7], [2, 4], [3, 4]]
    finally:
        m.close()


def test_clear_transform_and_the_map_is_left_alone(vo, ctx):
    m, rng = _map(vo, ctx, 1025, seed=11)
    try:
        p0, a0 = m.read()
        q = make_queries(rng, a0, 700)
        d = Lookup(ctx, q)
        assert d.call(m) == 0
        before = d.results()
        p1, a1 = m.read()
        assert p0.tobytes() == p1.tobytes() and a0.tobytes() == a1.tobytes() and len(m) == 1025
        # a second update of the same rows finds every class where the first one left it: the table was not touched
        m.update(p0, a0)
        p2, a2 = m.read()
        nan_rows = int(np.isnan(a0).any(1).sum())
        assert len(a2) == 1025 + nan_rows and a2[:1025].tobytes() == a0.tobytes()
        m.clear(); m.update(p0, a0)
        # map = T * map: the same entries, the gathered points are the moved bits
        T = vo.synth.random_isometry(np.random.default_rng(5), 0.4, 2.0)
        m.transform(T)
        p3, a3 = m.read()
        assert a3.tobytes() == a0.tobytes() and p3.tobytes() != p0.tobytes()
        d.fill()
        assert d.call(m) == 0
        after = d.results()
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and np.array_equal(after[4], before[4])
        k = int(after[0][0])
        assert k > 100 and after[2][0, :k].tobytes() == p3[after[1][0, :k, 1]].tobytes()
        # after vo_map_clear nothing is found
        m.clear()
        d.fill()
        assert d.call(m) == 0
        cnt, _, _, _, ent = d.results()
        assert cnt[0] == 0 and (ent == -1).all()
        d.close()
    finally:
        m.close()


def test_large_map_built_by_50k_row_updates(vo, ctx):
    """300 001 entries, 50 000 queries, half of them present: exact.  (At this size rows of different classes share a 32-bit
    tag by chance, and probe chains run through foreign slots.)"""
    rng = np.random.default_rng(77)
    n = 300001
    app = rng.uniform(-1, 1, (n, 10)).astype(np.float32)
    pts = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    m = vo.Map(ctx)
    try:
        for lo in range(0, n, 50000):
            m.update(pts[lo: lo + 50000], app[lo: lo + 50000])
        assert len(m) == n
        q = rng.uniform(-1, 1, (50000, 10)).astype(np.float32)
        present = rng.permutation(50000)[:25000]
        src = rng.integers(0, n, 25000)
        q[present] = app[src]
        ent_ref = np.full(50000, -1, np.int32)
        ent_ref[present] = src                                               # the rows are distinct (checked below)
        assert len({r.tobytes() for r in app[src]}) == len(set(src.tolist()))
        hit = np.nonzero(ent_ref >= 0)[0]
        d = Lookup(ctx, q)
        assert d.call(m) == 0
        check_lookup(d.results(), 0, ent_ref, np.stack([hit, ent_ref[hit]], 1).astype(np.int32), pts[ent_ref[hit]])
        d.close()
    finally:
        m.close()


def test_batched_equals_single(vo, ctx):
    m, rng = _map(vo, ctx, 5000, seed=21)
    try:
        m_pts, m_app = m.read()
        sizes = [40, 1500, 255, 256, 257, 64, 1024, 1025, 63, 700, 1, 1499, 512, 90]
        assert len(sizes) == 14
        cap, stride = 1500, 1504
        q = np.zeros((14, stride, 10), np.float32)
        for f, n in enumerate(sizes):
            q[f, :n] = make_queries(rng, m_app, n)
            q[f, n:cap] = m_app[:cap - n]                                    # rows behind the live ones that WOULD be found
        b = Lookup(ctx, q, n_max=cap, n_live=sizes, n_frames=14, stride=stride)
        assert b.call(m) == 0, ctx.lib.vo_last_error()
        rb = b.results()
        tab = M.table(m_app)
        for f, n in enumerate(sizes):
            s = Lookup(ctx, q[f, :cap], n_max=cap, n_live=[n])
            assert s.call(m) == 0
            rs = s.results()
            s.close()
            assert rs[0][0] == rb[0][f]
            for x, y in zip(rs[1:], rb[1:]):
                assert x[0].tobytes() == y[f].tobytes()                      # whole arrays, what lies behind the count included
            ent, pairs, xyz = M.lookup(m_app, q[f, :cap], m_pts, n_live=n, tab=tab)
            check_lookup(rb, f, ent, pairs, xyz)
        b.close()
    finally:
        m.close()


def test_capture_replay_and_refused_growth(vo, ctx):
    m, rng = _map(vo, ctx, 1025, seed=31)
    lib = ctx.lib
    try:
        m_pts, m_app = m.read()
        q = make_queries(rng, m_app, 900)
        d = Lookup(ctx, q)
        assert d.call(m) == 0
        ctx.synchronize()
        eager = d.results()
        d.fill()
        g = C.c_void_p()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.call(m)
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        assert (d.results()[0] == -7).all()                                  # captured, not run
        assert lib.vo_graph_launch(g) == 0
        ctx.synchronize()
        for x, y in zip(eager, d.results()):
            assert x.tobytes() == y.tobytes()
        # other rows in the same buffer, replayed
        q2 = make_queries(rng, m_app, 900)
        ctx.h2d(d.d_q, q2)
        assert lib.vo_graph_launch(g) == 0
        ctx.synchronize()
        ent, pairs, xyz = M.lookup(m_app, q2, m_pts)
        r = d.results()
        assert r[0][0] == len(pairs) and np.array_equal(r[4][0], ent) and np.array_equal(r[1][0, :len(pairs)], pairs)
        assert lib.vo_graph_destroy(g) == 0
        # a capture that would have to grow the scratch is refused before anything is enqueued; the context stays usable
        big = Lookup(ctx, np.zeros((200000, 10), np.float32), entries=False)
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        assert big.call(m) == -6 and b"capture" in lib.vo_last_error()
        rc = d.call(m)
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0
        assert lib.vo_graph_destroy(g) == 0
        assert big.call(m) == 0 and int(big.results()[0][0]) == 0
        big.close()
        d.fill()
        assert d.call(m) == 0
        assert d.results()[0][0] == len(pairs)
        d.close()
    finally:
        m.close()


def test_bad_arguments(vo, ctx):
    m, rng = _map(vo, ctx, 100, seed=41)
    lib, I, S, V = ctx.lib, C.c_int, C.c_size_t, C.c_void_p
    try:
        d = Lookup(ctx, make_queries(rng, m.read()[1], 64))
        ok = (V(d.d_q), I(64), None, V(d.d_pairs), V(d.d_cnt), V(d.d_xyz), V(d.d_local), V(d.d_ent))
        assert lib.vo_map_lookup_dev(m.h, *ok) == 0
        assert lib.vo_map_lookup_dev(None, *ok) == -1 and b"null map" in lib.vo_last_error()
        assert lib.vo_map_lookup_dev(m.h, V(d.d_q + 4), *ok[1:]) == -1 and b"aligned" in lib.vo_last_error()
        assert lib.vo_map_lookup_dev(m.h, V(d.d_q), I(64), None, V(d.d_pairs + 4), *ok[4:]) == -1
        assert lib.vo_map_lookup_dev(m.h, V(d.d_q), I(-1), *ok[2:]) == -1
        assert lib.vo_map_lookup_dev(m.h, None, *ok[1:]) == -1
        assert lib.vo_map_lookup_dev(m.h, V(d.d_q), I(64), None, None, *ok[4:]) == -1
        assert lib.vo_map_lookup_dev(m.h, V(d.d_q), I(64), None, V(d.d_pairs), None, *ok[5:]) == -1
        for F in (0, -1, 65536):
            assert lib.vo_map_lookup_batch_dev(m.h, I(F), V(d.d_q), S(32), I(32), None, *ok[3:]) == -1, F
        assert lib.vo_map_lookup_batch_dev(m.h, I(2), V(d.d_q), S(31), I(32), None, *ok[3:]) == -1      # stride below n_max
        assert lib.vo_map_lookup_batch_dev(m.h, I(2), V(d.d_q), S(32), I(32), None, *ok[3:]) == 0
        # n_max = 0: nothing to look up, the count is written
        d.fill()
        assert lib.vo_map_lookup_dev(m.h, V(d.d_q), I(0), *ok[2:]) == 0
        assert d.results()[0][0] == 0
        # the host form: refused inside a capture, and on bad arrays
        n_out = C.c_int()
        assert lib.vo_map_lookup(m.h, None, I(3), None, C.byref(n_out), None, None) == -1
        g = V()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        q = np.zeros((4, 10), np.float32); pr = np.zeros((4, 2), np.int32)
        assert lib.vo_map_lookup(m.h, q.ctypes.data_as(V), I(4), pr.ctypes.data_as(V), C.byref(n_out), None, None) == -6
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
        if g.value:
            assert lib.vo_graph_destroy(g) == 0
        assert lib.vo_map_lookup(m.h, q.ctypes.data_as(V), I(4), pr.ctypes.data_as(V), C.byref(n_out), None, None) == 0
        d.close()
    finally:
        m.close()
