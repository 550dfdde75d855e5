"""Device-side plumbing of tests/test_gpu_map_loops.py: a case of tests/map_loops_cases.py as a device map plus padded frame
arrays (strides above n_max), voe_map_loops_batch_dev on them with every argument switchable, and the read-back of its outputs
and of the problems it gathered in the shape map_loops_restatement.compare() takes."""
import ctypes as C

import numpy as np

GUARD = -7


class LoopsDev:
    def __init__(self, vo, ctx, case, stride_pad=3):
        self.vo, self.ctx, self.case, self.lib = vo, ctx, case, ctx.lib
        self.cam = vo.Camera(*case["cam"], case["K"], np.eye(4), ctx=ctx)
        self.m = vo.Map(ctx)
        self.bufs = []
        frames = case["frames"]
        self.F, self.n_max, self.M = len(frames), case["n_max"], len(case["map_app"])
        self.stride = self.n_max + stride_pad
        app = np.full((self.F, self.stride, 10), np.nan, np.float32)      # behind a frame's rows: NaN (they find nothing)
        uv = np.full((self.F, self.stride, 2), 1e9, np.float32)
        for f, (p, a) in enumerate(frames):
            app[f, : len(a)], uv[f, : len(a)] = np.asarray(a, np.float32).reshape(-1, 10), np.asarray(p, np.float32).reshape(-1, 2)
        n = case["n_rows"] if case["n_rows"] is not None else [len(a) for _, a in frames]
        self.d_uv, self.d_app, self.d_n = self.dev(uv), self.dev(app), self.dev(np.asarray(n, np.int32))
        self.d_S = self.dev(np.ascontiguousarray(np.asarray(case["S"], np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)))
        k = case["dup_rows"]                                  # rows entered twice: the host counts them, the device does not
        self.m.update(np.concatenate([case["map_pts"], case["map_pts"][:k]]), np.concatenate([case["map_app"], case["map_app"][:k]]))
        self.set_params(**case["params"])
        F, L, M = self.F, 64, self.M
        self.d_edges, self.d_Z, self.d_w, self.d_rec = self.alloc(8 * L), self.alloc(64 * L), self.alloc(12 * L), self.alloc(40 * L)
        self.d_hist, self.d_ref, self.d_stats = self.alloc(4 * F * F), self.alloc(4 * M), self.alloc(32)

    def set_params(self, **p):
        vo = self.vo
        self.p = p
        self.L = int(p["max_loops"])
        self.prm = vo.MapLoopsParams(p["gap"], p["ref_window"], p["min_shared"], p["separation"], p["max_loops"], 0,
                                     vo.RansacParams(p["n_hypotheses"], p["threshold_px"], p["seed"]), p["kernel_threshold"], p["n_iters"], p["min_inliers"],
                                     (C.c_float * 3)(*p["w_loop"]), 0)

    def alloc(self, n):
        p = self.ctx.alloc(n + 16)
        self.bufs.append(p)
        return p

    def dev(self, arr):
        p = self.ctx.to_device(arr)
        self.bufs.append(p)
        return p

    def read(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        self.ctx.d2h(out, d)
        return out

    def clear_out(self):
        F, L, M = self.F, self.L, self.M
        for d, n in ((self.d_edges, 2 * L), (self.d_Z, 16 * L), (self.d_w, 3 * L), (self.d_rec, 10 * L), (self.d_hist, F * F), (self.d_ref, M), (self.d_stats, 8)):
            self.ctx.h2d(d, np.full(n + 4, GUARD, np.int32))

    def call(self, m="own", optional=True, **kw):
        """the return code of voe_map_loops_batch_dev; kw overrides F, K (None: null), d_uv, uv_stride, d_app, app_stride, n_max, d_n,
        d_S, prm (None: null), d_edges, d_Z, d_w, d_rec, d_hist, d_ref, d_stats"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        cam = self.cam
        K = None if ("K" in kw and kw["K"] is None) else np.ascontiguousarray(np.asarray(g("K", cam._K), np.float32).reshape(3, 3).T).ctypes.data_as(C.c_void_p)
        return self.lib.voe_map_loops_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), C.c_int(cam._rows), C.c_int(cam._cols), C.c_int(cam._z_near), C.c_int(cam._z_far), K,
            v(g("d_uv", self.d_uv)), C.c_size_t(g("uv_stride", self.stride)), v(g("d_app", self.d_app)), C.c_size_t(g("app_stride", self.stride)),
            C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)), v(g("d_S", self.d_S)), None if ("prm" in kw and kw["prm"] is None) else C.byref(g("prm", self.prm)),
            v(g("d_edges", self.d_edges)), v(g("d_Z", self.d_Z)), v(g("d_w", self.d_w)), v(g("d_rec", self.d_rec)),
            v(g("d_hist", self.d_hist if optional else None)), v(g("d_ref", self.d_ref if optional else None)), v(g("d_stats", self.d_stats)))

    def outputs(self):
        """the bytes of every output array with its guard words, as the device holds them"""
        self.ctx.synchronize()
        F, L, M = self.F, self.L, self.M
        return [self.read(d, n + 4, np.int32) for d, n in ((self.d_edges, 2 * L), (self.d_Z, 16 * L), (self.d_w, 3 * L), (self.d_rec, 10 * L),
                                                           (self.d_hist, F * F), (self.d_ref, M), (self.d_stats, 8))]

    def problems(self):
        """what the call gathered and measured, from the map's workspace: dict of arrays"""
        self.ctx.synchronize()
        L, N, F = self.L, self.n_max, self.F
        p = self.m.loops_problems_dev()
        return dict(ptr=p, world=self.read(p["world"], (L, N, 3), np.float32), uv=self.read(p["uv"], (L, N, 2), np.float32),
                    pairs=self.read(p["pairs"], (L, N, 2), np.int32), n_pairs=self.read(p["n_pairs"], L, np.int32),
                    cand=self.read(p["candidates"], (F, 2), np.int32), inlier_pairs=self.read(p["inlier_pairs"], (L, N, 2), np.int32),
                    n_inliers=self.read(p["n_inliers"], L, np.int32), T16=self.read(p["T16"], (L, 16), np.float32),
                    solver_stats=self.read(p["solver_stats"], (L, 4), np.float32))

    def got(self):
        """the call's results in the shape map_loops_restatement.compare() takes, and the raw record array"""
        o = self.outputs()
        assert all((x[-4:] == GUARD).all() for x in o), "an output array was written behind its end"
        F, L, M = self.F, self.L, self.M
        pr = self.problems()
        rec = o[3][: 10 * L].reshape(L, 10).copy().view(self.vo.MAP_LOOP_RECORD_DTYPE).reshape(L)
        st = self.vo.MapLoopsStats()
        C.memmove(C.byref(st), o[6].ctypes.data, 32)
        assert list(st.reserved) == [0, 0]
        n = pr["n_pairs"]
        cand = pr["cand"].copy()
        cand[cand[:, 0] < 0, 1] = 0
        assert all((pr["pairs"][l, : n[l], 1] == np.arange(n[l])).all() for l in range(L))
        return dict(ref_frame=o[5][:M], hist=o[4][: F * F].reshape(F, F), cand=cand, edges=o[0][: 2 * L].reshape(L, 2),
                    Z=o[1][: 16 * L].view(np.float32).reshape(L, 4, 4).transpose(0, 2, 1), weights=o[2][: 3 * L].view(np.float32).reshape(L, 3),
                    stats=st.as_dict(), rows=[pr["pairs"][l, : n[l], 0] for l in range(L)], world=[pr["world"][l, : n[l]] for l in range(L)],
                    T=[pr["T16"][l].reshape(4, 4).T for l in range(L)], loops=[{k: rec[l][k] for k in rec.dtype.names} for l in range(L)]), rec, pr

    def map_state(self):
        """the bytes of the map: points, appearances and the header words as the device holds them, the history, and the entry
        the table finds for every row of the case's map (no call here refreshes the host's bound of the size)"""
        self.ctx.synchronize()
        px, pa, ph = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert self.lib.vo_map_dev_ptrs(self.m.h, C.byref(px), C.byref(pa), C.byref(ph)) == 0
        n = max(self.M, 1)
        return [self.read(px.value, 3 * n, np.float32), self.read(pa.value, 10 * n, np.float32), self.read(ph.value, 16, np.int32), self.m.history(),
                self.m.lookup(self.case["map_app"])[1]]

    def close(self):
        for d in self.bufs:
            self.ctx.free(d)
        self.m.close()


def same(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
