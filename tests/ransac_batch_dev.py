"""vo_estimate_pose_ransac_batch_dev through the C ABI on device copies of a list of host problems, shared by the GPU tests of
the batched form: BatchDev holds the padded arrays, calls the entry point and vo_picp_solve_batch_dev, and reads back."""
import ctypes as C

import numpy as np

from ransac_dev import CAM, POSE_THR_PX, _K, _p

V = C.c_void_p


class BatchDev:
    def __init__(self, vo, ctx, K, problems, pairs_stride=None, live=None):
        """problems: [(world (n, 3), meas (m, 2), pairs (p, 2))]; live: per-problem live counts (default: len(pairs))"""
        self.vo, self.ctx, self.lib, self.K = vo, ctx, ctx.lib, _K(K)
        P = self.P = len(problems)
        W = [np.ascontiguousarray(w, np.float32).reshape(-1, 3) for w, _, _ in problems]
        M = [np.ascontiguousarray(m, np.float32).reshape(-1, 2) for _, m, _ in problems]
        Q = [np.ascontiguousarray(q, np.int32).reshape(-1, 2) for _, _, q in problems]
        self.ws, self.ms = max(max(map(len, W)), 1), max(max(map(len, M)), 1)
        self.ps = int(pairs_stride or max(max(map(len, Q)), 1))
        self.world = np.zeros((P, self.ws, 3), np.float32); self.meas = np.zeros((P, self.ms, 2), np.float32)
        self.pairs = np.zeros((P, self.ps, 2), np.int32)
        for i in range(P):
            self.world[i, : len(W[i])] = W[i]; self.meas[i, : len(M[i])] = M[i]; self.pairs[i, : len(Q[i])] = Q[i]
        self.n = np.array([len(q) for q in Q] if live is None else live, np.int32)
        a, t = ctx.alloc, ctx.to_device
        self.d_world, self.d_meas, self.d_pairs, self.d_n = t(self.world), t(self.meas), t(self.pairs), t(np.resize(self.n, max(P, 2)))
        self.d_T, self.d_inl, self.d_nin, self.d_st = a(P * 64), a(P * self.ps * 8), a(max(P * 4, 8)), a(max(P * 4, 8))
        self.d_mask, self.d_counts = a(max(P * self.ps, 8)), a(P * 65536 * 4 if P <= 3 else P * 2048 * 4)
        self.d_Ts, self.d_stats, self.d_host, self.d_T0, self.d_n0 = a(P * 64), a(P * 16), a(P * self.ps * 8), a(P * 64), a(max(P * 4, 8))
        self._all = [self.d_world, self.d_meas, self.d_pairs, self.d_n, self.d_T, self.d_inl, self.d_nin, self.d_st, self.d_mask,
                     self.d_counts, self.d_Ts, self.d_stats, self.d_host, self.d_T0, self.d_n0]

    def call(self, n_hyp=128, thr=POSE_THR_PX, seed=0, live=True, fill=True, **over):
        """the entry point; over: replacements of single arguments by name (the refusals); fill=False: no copies first (inside
        a capture)"""
        ctx = self.ctx
        if fill:
            ctx.h2d(self.d_mask, np.full(max(self.P * self.ps, 8), 2, np.uint8))          # what no kernel wrote shows
            ctx.h2d(self.d_counts, np.full(self.P * n_hyp, -2, np.int32))
        prm = self.vo.RansacParams(n_hyp, thr, seed)
        a = dict(n_problems=C.c_int(self.P), K=_p(self.K), world=V(self.d_world), world_stride=C.c_size_t(self.ws),
                 n_world=C.c_int(self.ws), meas=V(self.d_meas), meas_stride=C.c_size_t(self.ms), n_meas=C.c_int(self.ms),
                 pairs=V(self.d_pairs), pairs_stride=C.c_size_t(self.ps), n_pairs=V(self.d_n) if live else None, params=C.byref(prm),
                 T=V(self.d_T), inl=V(self.d_inl), nin=V(self.d_nin), mask=V(self.d_mask), counts=V(self.d_counts), st=V(self.d_st))
        a.update(over)
        return self.lib.vo_estimate_pose_ransac_batch_dev(
            ctx.h, a["n_problems"], *map(C.c_int, CAM), a["K"], a["world"], a["world_stride"], a["n_world"], a["meas"], a["meas_stride"],
            a["n_meas"], a["pairs"], a["pairs_stride"], a["n_pairs"], a["params"], a["T"], a["inl"], a["nin"], a["mask"], a["counts"],
            a["st"])

    def results(self, n_hyp=128):
        """dict of raw arrays: T (P, 16), inl (P, stride, 2), nin (P,), mask (P, stride), counts (P, n_hyp), st (P,)"""
        P, c = self.P, self.ctx
        r = dict(T=np.zeros((P, 16), np.float32), inl=np.zeros((P, self.ps, 2), np.int32), nin=np.zeros(P, np.int32),
                 mask=np.zeros((P, self.ps), np.uint8), counts=np.zeros((P, n_hyp), np.int32), st=np.zeros(P, np.int32))
        for k, d in (("T", self.d_T), ("inl", self.d_inl), ("nin", self.d_nin), ("mask", self.d_mask), ("counts", self.d_counts),
                     ("st", self.d_st)):
            c.d2h(r[k], d)
        return r

    def problem(self, r, p):
        """problem p of results() in the shape of ransac_dev.Dev.results(): (T bytes, inlier pairs, n, mask, counts, status)"""
        n = int(r["nin"][p])
        return r["T"][p].tobytes(), r["inl"][p, :n].copy(), n, r["mask"][p].copy(), r["counts"][p].copy(), int(r["st"][p])

    def solve(self, d_pairs, d_n, d_T0, rounds=50):
        """vo_picp_solve_batch_dev on this batch's points: the poses' bytes (P, 16)"""
        rc = self.lib.vo_picp_solve_batch_dev(
            self.ctx.h, C.c_int(self.P), *map(C.c_int, CAM), _p(self.K), C.c_float(10000.0), C.c_int(0), V(self.d_world),
            C.c_size_t(self.ws), V(self.d_meas), C.c_size_t(self.ms), V(d_pairs), C.c_size_t(self.ps), V(d_n),
            V(d_T0) if d_T0 else None, C.c_int(rounds), V(self.d_Ts), V(self.d_stats))
        assert rc == 0, self.lib.vo_last_error()
        T = np.zeros((self.P, 16), np.float32)
        self.ctx.d2h(T, self.d_Ts)
        return T

    def solve_host(self, pairs_list, T16=None, rounds=50):
        """the same solve on host pair lists (padded to the stride) from host poses T16 (P, 16) raw, or the identity"""
        buf = np.zeros((self.P, self.ps, 2), np.int32)
        for i, q in enumerate(pairs_list):
            buf[i, : len(q)] = q
        self.ctx.h2d(self.d_host, buf)
        self.ctx.h2d(self.d_n0, np.resize(np.array([len(q) for q in pairs_list], np.int32), max(self.P, 2)))
        if T16 is not None:
            self.ctx.h2d(self.d_T0, np.ascontiguousarray(T16, np.float32))
        return self.solve(self.d_host, self.d_n0, self.d_T0 if T16 is not None else None, rounds)

    def close(self):
        for d in self._all:
            self.ctx.free(d)


def single_results(vo, ctx, K, problem, n_max, n_hyps, thr=POSE_THR_PX, seed=0, live=None, use_live=True):
    """{n_hyp: (T bytes, inlier pairs, n, mask, counts, status)} of vo_estimate_pose_ransac_dev on the problem alone"""
    from ransac_dev import Dev
    world, meas, pairs = problem
    d = Dev(vo, ctx, K, world, meas, pairs, n_max=n_max)
    try:
        if live is not None:
            d.set_live(live)
        out = {}
        for H in n_hyps:
            assert d.call(n_hyp=H, thr=thr, seed=seed, live=use_live) == 0, ctx.lib.vo_last_error()
            T, inl, nin, mask, counts, st = d.results(H)
            out[H] = (np.ascontiguousarray(T.T).ravel().tobytes(), inl.copy(), nin, mask.copy(), counts.copy(), st)
        return out
    finally:
        d.close()


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and \
        np.array_equal(a[4], b[4]) and a[5] == b[5]
