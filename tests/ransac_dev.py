"""Device-memory calls of the two RANSAC front ends through the C ABI, shared by the GPU tests: dev_call for
vo_estimate_transform_ransac_dev and Dev (a 2D-3D problem in device memory) for vo_estimate_pose_ransac_dev."""
import ctypes as C

import numpy as np

CAM = (480, 640, 0, 10)                # synth.frame_pair's rows, cols, z_near, z_far
THR_PX = 1.0                           # the epipolar threshold of tests/test_gpu_ransac.py
POSE_THR_PX = 2.0                      # the tracking threshold of tests/test_gpu_pose_ransac.py


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def dev_call(vo, ctx, K, pairs, p1, p2, n_hyp=2048, thr=THR_PX, seed=0, n_live=None, always_read=False):
    """the _dev form from device copies: (status, X, mask, counts, n_inliers) -- mask and counts read back after a success,
    or after any return when always_read (counts start at -2 there, the mask at 2: what no kernel wrote shows)"""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
    n = len(pairs)
    d_pairs, d_p1, d_p2 = ctx.alloc(max(pairs.nbytes, 8)), ctx.alloc(p1.nbytes), ctx.alloc(p2.nbytes)
    d_mask, d_counts, d_n = ctx.alloc(max(n, 8)), ctx.alloc(4 * n_hyp), ctx.alloc(8)
    try:
        ctx.h2d(d_pairs, pairs); ctx.h2d(d_p1, p1); ctx.h2d(d_p2, p2)
        if n_live is not None:
            ctx.h2d(d_n, np.array([n_live], np.int32))
        if always_read:
            ctx.h2d(d_counts, np.full(n_hyp, -2, np.int32)); ctx.h2d(d_mask, np.full(max(n, 8), 2, np.uint8))
        X = np.zeros(16, np.float32)
        n_in = C.c_int(-7)
        prm = vo.RansacParams(n_hyp, thr, seed)
        rc = ctx.lib.vo_estimate_transform_ransac_dev(
            ctx.h, _p(np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()), C.c_void_p(d_pairs), C.c_int(n),
            C.c_void_p(d_n) if n_live is not None else None, C.c_void_p(d_p1), C.c_int(len(p1)), C.c_void_p(d_p2),
            C.c_int(len(p2)), C.byref(prm), _p(X), C.c_void_p(d_mask), C.c_void_p(d_counts), C.byref(n_in))
        mask = np.zeros(n, np.uint8); counts = np.zeros(n_hyp, np.int32)
        if rc == 0 or always_read:
            ctx.d2h(mask, d_mask); ctx.d2h(counts, d_counts)
        return rc, X.reshape(4, 4).T.copy(), mask, counts, n_in.value
    finally:
        for d in (d_pairs, d_p1, d_p2, d_mask, d_counts, d_n):
            ctx.free(d)


def _K(K):
    return np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()


class Dev:
    """one 2D-3D problem in device memory, the _dev call on it and a PICP handle to solve it"""

    def __init__(self, vo, ctx, K, world, meas, pairs, n_max=None, thr=10000.0):
        self.vo, self.ctx, self.lib = vo, ctx, ctx.lib
        self.K = _K(K)
        self.world = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
        self.meas = np.ascontiguousarray(meas, np.float32).reshape(-1, 2)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self.n = len(pairs)
        self.n_max = max(n_max or self.n, 1)
        buf = np.zeros((self.n_max, 2), np.int32)
        buf[: self.n] = pairs
        self.pairs = buf
        a = ctx.alloc
        self.d_world, self.d_meas, self.d_pairs = a(self.world.nbytes), a(self.meas.nbytes), a(buf.nbytes)
        self.d_T, self.d_inl, self.d_nin, self.d_mask = a(64), a(buf.nbytes), a(16), a(max(self.n_max, 8))
        self.d_counts, self.d_n, self.d_st, self.d_I, self.d_host = a(4 * 65536), a(16), a(16), a(64), a(buf.nbytes)
        ctx.h2d(self.d_world, self.world); ctx.h2d(self.d_meas, self.meas); ctx.h2d(self.d_pairs, buf)
        ctx.h2d(self.d_I, np.eye(4, dtype=np.float32))
        ctx.h2d(self.d_counts, np.full(65536, -2, np.int32)); ctx.h2d(self.d_mask, np.full(max(self.n_max, 8), 2, np.uint8))
        self.set_live(self.n)
        h = C.c_void_p()
        assert self.lib.vo_picp_create(ctx.h, C.byref(h)) == 0
        self.solver = h
        assert self.lib.vo_picp_set_camera(h, *map(C.c_int, CAM), _p(self.K), _p(np.eye(4, dtype=np.float32))) == 0
        assert self.lib.vo_picp_set_kernel_threshold(h, C.c_float(thr)) == 0
        assert self.lib.vo_picp_set_points_dev(h, C.c_void_p(self.d_world), C.c_int(len(self.world)), C.c_void_p(self.d_meas),
                                               C.c_int(len(self.meas))) == 0

    def set_live(self, n):
        self.ctx.h2d(self.d_n, np.array([n], np.int32))

    def call(self, n_hyp=2048, thr=POSE_THR_PX, seed=0, live=True, capture_safe=False):
        prm = self.vo.RansacParams(n_hyp, thr, seed)
        return self.lib.vo_estimate_pose_ransac_dev(
            self.ctx.h, *map(C.c_int, CAM), _p(self.K), C.c_void_p(self.d_world), C.c_int(len(self.world)), C.c_void_p(self.d_meas),
            C.c_int(len(self.meas)), C.c_void_p(self.d_pairs), C.c_int(self.n_max), C.c_void_p(self.d_n) if live else None,
            C.byref(prm), C.c_void_p(self.d_T), C.c_void_p(self.d_inl), C.c_void_p(self.d_nin), C.c_void_p(self.d_mask),
            C.c_void_p(self.d_counts), C.c_void_p(self.d_st))

    def results(self, n_hyp=2048):
        """(T (4x4), inlier pairs, n_inliers, mask, counts, status)"""
        T = np.zeros(16, np.float32); nin = np.zeros(1, np.int32); st = np.zeros(1, np.int32)
        inl = np.zeros((self.n_max, 2), np.int32); mask = np.zeros(self.n_max, np.uint8); counts = np.zeros(n_hyp, np.int32)
        c = self.ctx
        c.d2h(T, self.d_T); c.d2h(nin, self.d_nin); c.d2h(st, self.d_st); c.d2h(inl, self.d_inl); c.d2h(mask, self.d_mask)
        c.d2h(counts, self.d_counts)
        return T.reshape(4, 4).T.copy(), inl[: nin[0]], int(nin[0]), mask, counts, int(st[0])

    def solve(self, d_T, d_pairs, d_n, rounds=100, bad_index=False):
        """set_pose_dev + solve_dev at capacity n_max: the pose's bytes (bad_index: the solve drops a pair with a bad index and
        says so at the getter; the pose is then read where the solver keeps it)"""
        assert self.lib.vo_picp_set_pose_dev(self.solver, C.c_void_p(d_T)) == 0
        assert self.lib.vo_picp_solve_dev(self.solver, C.c_void_p(d_pairs), C.c_int(self.n_max), C.c_void_p(d_n), C.c_int(0),
                                          C.c_int(rounds)) == 0
        T = np.zeros(16, np.float32)
        rc = self.lib.vo_picp_get_pose(self.solver, _p(T))
        if bad_index:
            assert rc == -5
            p = C.c_void_p()
            assert self.lib.vo_picp_pose_dev_ptr(self.solver, C.byref(p)) == 0
            self.ctx.d2h(T, p.value)
        else:
            assert rc == 0
        return T

    def solve_host_pairs(self, T0, pairs, rounds=100):
        """the same solve on pairs compacted on the host, started from T0 (a 4x4), at the same capacity"""
        buf = np.zeros((self.n_max, 2), np.int32)
        buf[: len(pairs)] = pairs
        self.ctx.h2d(self.d_host, buf)
        d_T0, d_n0 = self.ctx.alloc(64), self.ctx.alloc(16)
        try:
            self.ctx.h2d(d_T0, np.ascontiguousarray(np.asarray(T0, np.float32).T))
            self.ctx.h2d(d_n0, np.array([len(pairs)], np.int32))
            return self.solve(d_T0, self.d_host, d_n0, rounds)
        finally:
            self.ctx.free(d_T0); self.ctx.free(d_n0)

    def close(self):
        self.lib.vo_picp_destroy(self.solver)
        for d in (self.d_world, self.d_meas, self.d_pairs, self.d_T, self.d_inl, self.d_nin, self.d_mask, self.d_counts, self.d_n,
                  self.d_st, self.d_I, self.d_host):
            self.ctx.free(d)
