"""Device-memory calls of vo_map_lookup*_dev / vo_map_localise*_dev through the C ABI, shared by the GPU tests."""
import ctypes as C

import numpy as np

SENTINEL = -7


def _v(d):
    return C.c_void_p(d) if d else None


def make_map_rows(rng, M):
    """M distinct appearance rows: every seventh has a zero component, and (from 11 rows on) every fiftieth a NaN"""
    app = rng.uniform(-1, 1, (M, 10)).astype(np.float32)
    app[::7, 3] = 0.0
    if M > 10:
        app[5::50, 8] = np.nan
    pts = rng.uniform(-5, 5, (M, 3)).astype(np.float32)
    return pts, app


def make_queries(rng, m_app, n):
    """present rows, absent rows, duplicates of one row, rows differing from an entry in the sign of a zero, NaN queries and
    copies of NaN entries"""
    q = rng.uniform(-1, 1, (n, 10)).astype(np.float32)                       # absent
    M = len(m_app)
    if M:
        kind = rng.integers(0, 6, n)
        src = rng.integers(0, M, n)
        take = kind <= 3
        q[take] = m_app[src[take]]                                           # present (or a copy of a NaN entry)
        flip = np.nonzero(kind == 3)[0]
        if len(flip):
            src[flip] = (src[flip] // 7) * 7                                 # entries with a zero component
            rows = m_app[src[flip]].copy()
            rows[rows == 0] = -0.0
            q[flip] = rows
        q[kind == 4, 2] = np.nan
        if n > 2:
            q[n // 2] = q[0]                                                 # both find the same entry
    return q


class Lookup:
    """one (batched) lookup problem in device memory"""

    def __init__(self, ctx, q, n_max=None, n_live=None, n_frames=1, stride=None, entries=True):
        self.ctx = ctx
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 10)
        self.F = n_frames
        self.n_max = (len(q) // n_frames if n_max is None else n_max)
        self.stride = self.n_max if stride is None else stride
        a = ctx.alloc
        N = max(self.n_max * self.F, 1)
        self.d_q = ctx.to_device(q) if len(q) else a(16)
        self.d_n = ctx.to_device(np.asarray(n_live, np.int32).reshape(-1)) if n_live is not None else None
        self.d_pairs, self.d_local, self.d_xyz, self.d_cnt = a(8 * N), a(8 * N), a(12 * N), a(max(4 * self.F, 16))
        self.d_ent = a(4 * N) if entries else None
        self.N = N
        self.fill()

    def fill(self):
        c = self.ctx
        c.h2d(self.d_pairs, np.full(2 * self.N, SENTINEL, np.int32)); c.h2d(self.d_local, np.full(2 * self.N, SENTINEL, np.int32))
        c.h2d(self.d_xyz, np.full(3 * self.N, -1234.5, np.float32)); c.h2d(self.d_cnt, np.full(max(self.F, 4), SENTINEL, np.int32))
        if self.d_ent:
            c.h2d(self.d_ent, np.full(self.N, SENTINEL, np.int32))

    def call(self, m, single=None):
        lib = self.ctx.lib
        if (self.F == 1) if single is None else single:
            return lib.vo_map_lookup_dev(m.h, _v(self.d_q), C.c_int(self.n_max), _v(self.d_n), _v(self.d_pairs), _v(self.d_cnt),
                                         _v(self.d_xyz), _v(self.d_local), _v(self.d_ent))
        return lib.vo_map_lookup_batch_dev(m.h, C.c_int(self.F), _v(self.d_q), C.c_size_t(self.stride), C.c_int(self.n_max), _v(self.d_n),
                                           _v(self.d_pairs), _v(self.d_cnt), _v(self.d_xyz), _v(self.d_local), _v(self.d_ent))

    def results(self):
        """(counts (F,), pairs (F, n_max, 2), xyz (F, n_max, 3), local (F, n_max, 2), entries (F, n_max) or None) -- raw, whole"""
        c, F, n = self.ctx, self.F, self.n_max
        cnt = np.zeros(max(F, 4), np.int32); c.d2h(cnt, self.d_cnt)
        pairs = np.zeros((self.N, 2), np.int32); c.d2h(pairs, self.d_pairs)
        local = np.zeros((self.N, 2), np.int32); c.d2h(local, self.d_local)
        xyz = np.zeros((self.N, 3), np.float32); c.d2h(xyz, self.d_xyz)
        ent = None
        if self.d_ent:
            ent = np.zeros(self.N, np.int32); c.d2h(ent, self.d_ent)
            ent = ent[: F * n].reshape(F, n)
        return cnt[:F], pairs[: F * n].reshape(F, n, 2), xyz[: F * n].reshape(F, n, 3), local[: F * n].reshape(F, n, 2), ent

    def close(self):
        for d in (self.d_q, self.d_n, self.d_pairs, self.d_local, self.d_xyz, self.d_cnt, self.d_ent):
            if d:
                self.ctx.free(d)


def check_lookup(res, f, ent_ref, pairs_ref, xyz_ref):
    """frame f of Lookup.results() against the restatement's answer, exactly; what lies behind the count is untouched"""
    cnt, pairs, xyz, local, ent = res
    k = len(pairs_ref)
    assert cnt[f] == k, (cnt[f], k)
    if ent is not None:
        assert np.array_equal(ent[f], ent_ref)
    assert np.array_equal(pairs[f, :k], pairs_ref)
    assert xyz[f, :k].tobytes() == np.ascontiguousarray(xyz_ref, np.float32).tobytes()
    assert np.array_equal(local[f, :k], np.stack([pairs_ref[:, 0], np.arange(k)], 1).reshape(-1, 2))
    assert (pairs[f, k:] == SENTINEL).all() and (local[f, k:] == SENTINEL).all() and (xyz[f, k:] == np.float32(-1234.5)).all()


class Localise:
    """F frames (pixels, appearances) in device memory, vo_map_localise[_batch]_dev on them, and the EXPLICIT sequence of public
    calls the header's contract names, on buffers of its own"""

    def __init__(self, vo, ctx, cam, K, frames, T0=None, n_max=None, uv_stride=None):
        self.vo, self.ctx, self.lib, self.cam = vo, ctx, ctx.lib, cam
        self.K = np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()
        self.F = F = len(frames)
        self.n = np.array([len(a) for _, a in frames], np.int32)
        self.n_max = cap = int(n_max or max(int(self.n.max()), 1))
        self.stride = st = int(uv_stride or cap)
        uv = np.zeros((F, st, 2), np.float32); app = np.zeros((F, st, 10), np.float32)
        for f, (p, a) in enumerate(frames):
            uv[f, : self.n[f]] = p; app[f, : self.n[f]] = a
        a = ctx.alloc
        self.d_uv, self.d_app, self.d_n = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(self.n)
        self.d_T0 = None
        if T0 is not None:
            self.T0 = np.stack([np.ascontiguousarray(np.asarray(T, np.float32).T).ravel() for T in T0])
            self.d_T0 = ctx.to_device(self.T0)
        N = F * cap
        self.d_T, self.d_st = a(64 * F), a(32 * F)
        # the explicit sequence's own buffers
        self.e_pairs, self.e_local, self.e_inl, self.e_xyz = a(8 * N), a(8 * N), a(8 * N), a(12 * N)
        self.e_hits, self.e_ninl, self.e_rst = a(max(4 * F, 16)), a(max(4 * F, 16)), a(max(4 * F, 16))
        self.e_Tw, self.e_T, self.e_s4 = a(64 * F), a(64 * F), a(16 * F)
        self.solver = None
        self.bufs = [self.d_uv, self.d_app, self.d_n, self.d_T0, self.d_T, self.d_st, self.e_pairs, self.e_local, self.e_inl, self.e_xyz,
                     self.e_hits, self.e_ninl, self.e_rst, self.e_Tw, self.e_T, self.e_s4]

    def prm(self, n_hyp, px, seed):
        return self.vo.RansacParams(int(n_hyp), float(px), int(seed))

    def clear_out(self):
        self.ctx.h2d(self.d_T, np.full(16 * self.F, -3.0, np.float32)); self.ctx.h2d(self.d_st, np.full(8 * self.F, SENTINEL, np.int32))

    def single(self, m, f, n_hyp=64, px=2.0, seed=0, thr=10000.0, n_iters=50, min_inliers=6, live=True):
        """vo_map_localise_dev on frame f -> outputs slot f"""
        I = C.c_int
        return self.lib.vo_map_localise_dev(
            m.h, *map(I, self.cam), _p(self.K), _v(self.d_uv + 8 * f * self.stride), _v(self.d_app + 40 * f * self.stride), I(self.n_max),
            _v(self.d_n + 4 * f) if live else None, C.byref(self.prm(n_hyp, px, seed)), C.c_float(thr), I(n_iters), I(min_inliers),
            _v(self.d_T0 + 64 * f) if self.d_T0 else None, _v(self.d_T + 64 * f), _v(self.d_st + 32 * f))

    def batch(self, m, n_hyp=64, px=2.0, seed=0, thr=10000.0, n_iters=50, min_inliers=6):
        I, S = C.c_int, C.c_size_t
        return self.lib.vo_map_localise_batch_dev(
            m.h, I(self.F), *map(I, self.cam), _p(self.K), _v(self.d_uv), S(self.stride), _v(self.d_app), S(self.stride), I(self.n_max),
            _v(self.d_n), C.byref(self.prm(n_hyp, px, seed)), C.c_float(thr), I(n_iters), I(min_inliers), _v(self.d_T0), _v(self.d_T),
            _v(self.d_st))

    def results(self):
        """(T (F, 16) raw column-major, stats (F,) structured)"""
        T = np.zeros((self.F, 16), np.float32); self.ctx.d2h(T, self.d_T)
        raw = np.zeros((self.F, 8), np.int32); self.ctx.d2h(raw, self.d_st)
        return T, raw

    @staticmethod
    def stats(raw_row):
        keys = ("status", "n_rows", "n_hits", "ransac_status", "ransac_inliers", "num_inliers")
        d = {k: int(v) for k, v in zip(keys, raw_row[:6])}
        d["chi_inliers"], d["chi_outliers"] = (float(x) for x in raw_row[6:8].view(np.float32))
        return d

    def explicit_single(self, m, f, n_hyp=64, px=2.0, seed=0, thr=10000.0, n_iters=50):
        """the sequence of public calls on frame f: (T (16,) raw, dict of what the statistics must equal)"""
        lib, I, cap = self.lib, C.c_int, self.n_max
        d_uv, d_app, d_n = self.d_uv + 8 * f * self.stride, self.d_app + 40 * f * self.stride, self.d_n + 4 * f
        assert lib.vo_map_lookup_dev(m.h, _v(d_app), I(cap), _v(d_n), _v(self.e_pairs), _v(self.e_hits), _v(self.e_xyz), _v(self.e_local),
                                     None) == 0
        if n_hyp > 0:
            assert lib.vo_estimate_pose_ransac_dev(self.ctx.h, *map(I, self.cam), _p(self.K), _v(self.e_xyz), I(cap), _v(d_uv), I(cap),
                                                   _v(self.e_local), I(cap), _v(self.e_hits), C.byref(self.prm(n_hyp, px, seed)),
                                                   _v(self.e_Tw), _v(self.e_inl), _v(self.e_ninl), None, None, _v(self.e_rst)) == 0
            start, pairs, cnt = self.e_Tw, self.e_inl, self.e_ninl
        else:
            start, pairs, cnt = self.d_T0 + 64 * f, self.e_local, self.e_hits
        if self.solver is None:
            h = C.c_void_p()
            assert lib.vo_picp_create(self.ctx.h, C.byref(h)) == 0
            self.solver = h
        s = self.solver
        assert lib.vo_picp_set_camera(s, *map(I, self.cam), _p(self.K), _p(np.eye(4, dtype=np.float32))) == 0
        assert lib.vo_picp_set_kernel_threshold(s, C.c_float(thr)) == 0
        assert lib.vo_picp_set_points_dev(s, _v(self.e_xyz), I(cap), _v(d_uv), I(cap)) == 0
        assert lib.vo_picp_set_pose_dev(s, _v(start)) == 0
        assert lib.vo_picp_solve_dev(s, _v(pairs), I(cap), _v(cnt), I(0), I(n_iters)) == 0
        assert lib.vo_picp_get_pose_dev(s, _v(self.e_T)) == 0
        chi_in, chi_out, n_in = C.c_float(), C.c_float(), C.c_int()
        assert lib.vo_picp_get_stats(s, C.byref(chi_in), C.byref(chi_out), C.byref(n_in)) == 0
        T = np.zeros(16, np.float32); self.ctx.d2h(T, self.e_T)
        hits = np.zeros(4, np.int32); self.ctx.d2h(hits, self.e_hits)
        handed = np.zeros(4, np.int32); self.ctx.d2h(handed, cnt)
        rst = np.zeros(4, np.int32)
        if n_hyp > 0:
            self.ctx.d2h(rst, self.e_rst)
        return T, dict(n_rows=int(self.n[f]), n_hits=int(hits[0]), ransac_status=int(rst[0]), ransac_inliers=int(handed[0]),
                       num_inliers=n_in.value, chi_inliers=chi_in.value, chi_outliers=chi_out.value)

    def explicit_batch(self, m, n_hyp=64, px=2.0, seed=0, thr=10000.0, n_iters=50):
        """the batched sequence of public calls: (T (F, 16), list of dicts)"""
        lib, I, S, cap, F = self.lib, C.c_int, C.c_size_t, self.n_max, self.F
        assert lib.vo_map_lookup_batch_dev(m.h, I(F), _v(self.d_app), S(self.stride), I(cap), _v(self.d_n), _v(self.e_pairs), _v(self.e_hits),
                                           _v(self.e_xyz), _v(self.e_local), None) == 0
        if n_hyp > 0:
            assert lib.vo_estimate_pose_ransac_batch_dev(
                self.ctx.h, I(F), *map(I, self.cam), _p(self.K), _v(self.e_xyz), S(cap), I(cap), _v(self.d_uv), S(self.stride), I(cap),
                _v(self.e_local), S(cap), _v(self.e_hits), C.byref(self.prm(n_hyp, px, seed)), _v(self.e_Tw), _v(self.e_inl), _v(self.e_ninl),
                None, None, _v(self.e_rst)) == 0, lib.vo_last_error()
            start, pairs, cnt = self.e_Tw, self.e_inl, self.e_ninl
        else:
            start, pairs, cnt = self.d_T0, self.e_local, self.e_hits
        assert lib.vo_picp_solve_batch_dev(self.ctx.h, I(F), *map(I, self.cam), _p(self.K), C.c_float(thr), I(0), _v(self.e_xyz), S(cap),
                                           _v(self.d_uv), S(self.stride), _v(pairs), S(cap), _v(cnt), _v(start), I(n_iters), _v(self.e_T),
                                           _v(self.e_s4)) == 0, lib.vo_last_error()
        T = np.zeros((F, 16), np.float32); self.ctx.d2h(T, self.e_T)
        s4 = np.zeros((F, 4), np.float32); self.ctx.d2h(s4, self.e_s4)
        hits = np.zeros(max(F, 4), np.int32); self.ctx.d2h(hits, self.e_hits)
        handed = np.zeros(max(F, 4), np.int32); self.ctx.d2h(handed, cnt)
        rst = np.zeros(max(F, 4), np.int32)
        if n_hyp > 0:
            self.ctx.d2h(rst, self.e_rst)
        return T, [dict(n_rows=int(self.n[f]), n_hits=int(hits[f]), ransac_status=int(rst[f]), ransac_inliers=int(handed[f]),
                        num_inliers=int(s4[f, 2]), chi_inliers=float(s4[f, 0]), chi_outliers=float(s4[f, 1])) for f in range(F)]

    def close(self):
        if self.solver is not None:
            self.lib.vo_picp_destroy(self.solver)
        for d in self.bufs:
            if d:
                self.ctx.free(d)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def same_stats(got, want):
    """the statistics of the call against those of the explicit sequence: integers equal, the chi^2 sums bit for bit"""
    for k, v in want.items():
        if isinstance(v, float):
            assert np.float32(got[k]).tobytes() == np.float32(v).tobytes(), (k, got[k], v)
        else:
            assert got[k] == v, (k, got[k], v)
