"""Device-side plumbing of tests/test_gpu_map_refine.py: a case of tests/map_refine_cases.py as a device map plus padded frame
arrays, and vo_map_refine_batch_dev on them with every optional argument switchable."""
import ctypes as C

import numpy as np

CAM = (480, 640, 0, 10)                                       # the refinement reads K alone


class RefineDev:
    def __init__(self, vo, ctx, case, n_max=None, stride_pad=3, m=None):
        self.vo, self.ctx, self.case, self.lib = vo, ctx, case, ctx.lib
        self.cam = vo.Camera(*CAM, case["K"])
        self.K = np.ascontiguousarray(np.asarray(case["K"], np.float32).reshape(3, 3).T).ravel()
        frames = case["frames"]
        self.F = len(frames)
        self.n_max = max([len(a) for _, a in frames] + [1]) if n_max is None else n_max
        self.stride = self.n_max + stride_pad
        # behind a frame's rows: NaN appearances (they find nothing) and wild pixels, so that a null d_n_rows sees the same observations
        uv = np.full((self.F, self.stride, 2), 1e9, np.float32)
        app = np.full((self.F, self.stride, 10), np.nan, np.float32)
        for f, (p, a) in enumerate(frames):
            uv[f, : len(a)] = np.asarray(p, np.float32).reshape(-1, 2)
            app[f, : len(a)] = np.asarray(a, np.float32).reshape(-1, 10)
        T = np.stack([np.ascontiguousarray(np.asarray(X, np.float32).reshape(4, 4).T).ravel() for X in case["poses"]])
        self.M = len(case["map_pts"])
        self.own_map = m is None
        self.m = vo.Map(ctx) if m is None else m
        if m is None:
            self.reset()
        self.d_uv, self.d_app, self.d_T = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(T)
        self.d_n = ctx.to_device(np.asarray(case["n_rows"], np.int32)) if case["n_rows"] is not None else None
        self.d_status, self.d_xyz, self.d_stats = ctx.alloc(4 * self.M + 16), ctx.alloc(12 * self.M + 16), ctx.alloc(64)
        self.params = dict(case["params"])

    def reset(self):
        """the map back at the case's start"""
        self.m.clear()
        self.m.update(self.case["map_pts"], self.case["map_app"])
        assert len(self.m) == self.M

    def clear_out(self):
        self.ctx.h2d(self.d_status, np.full(self.M + 4, -7, np.int32))
        self.ctx.h2d(self.d_xyz, np.full(3 * self.M + 4, -7.0, np.float32))
        self.ctx.h2d(self.d_stats, np.full(16, -7, np.int32))

    def call(self, status=True, xyz=False, m="own", **kw):
        """the return code of vo_map_refine_batch_dev; kw overrides: F, n_max, uv_stride, app_stride, K, d_uv, d_app, d_n, d_T,
        d_stats, prm (None: null), n_rounds, min_obs, huber_px, damping"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        p = dict(self.params)
        p.update({k: kw[k] for k in ("n_rounds", "min_obs", "huber_px", "damping") if k in kw})
        prm = self.vo.MapRefineParams(int(p["n_rounds"]), int(p["min_obs"]), float(p["huber_px"]), float(p["damping"]))
        K = g("K", self.K)
        return self.lib.vo_map_refine_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), K.ctypes.data_as(C.c_void_p) if K is not None else None,
            v(g("d_uv", self.d_uv)), C.c_size_t(g("uv_stride", self.stride)), v(g("d_app", self.d_app)),
            C.c_size_t(g("app_stride", self.stride)), C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)), v(g("d_T", self.d_T)),
            None if ("prm" in kw and kw["prm"] is None) else C.byref(prm), v(self.d_status if status else None),
            v(self.d_xyz if xyz else None), v(g("d_stats", self.d_stats)))

    def results(self):
        """(status (M,), xyz_out (M, 3), stats bytes (48,)) as the device holds them"""
        st = np.zeros(self.M, np.int32); self.ctx.d2h(st, self.d_status)
        xyz = np.zeros((self.M, 3), np.float32); self.ctx.d2h(xyz, self.d_xyz)
        raw = np.zeros(48, np.uint8); self.ctx.d2h(raw, self.d_stats)
        return st, xyz, raw

    def stats(self, raw):
        s = self.vo.MapRefineStats()
        C.memmove(C.byref(s), raw.ctypes.data, 48)
        return s.as_dict()

    def points(self):
        return self.m.read()[0]

    def close(self):
        for d in (self.d_uv, self.d_app, self.d_T, self.d_n, self.d_status, self.d_xyz, self.d_stats):
            if d:
                self.ctx.free(d)
        if self.own_map:
            self.m.close()
