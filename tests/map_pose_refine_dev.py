"""Device-side plumbing of tests/test_gpu_map_pose_refine.py and tests/test_gpu_map_adjust.py: a case of
tests/map_pose_refine_cases.py as a device map plus padded frame arrays, and vo_map_refine_poses_batch_dev,
vo_map_refine_batch_dev and vo_map_adjust_batch_dev on them with every optional argument switchable."""
import ctypes as C

import numpy as np

CAM = (480, 640, 0, 10)                                       # the refinement reads K alone


def colmajor16(poses):
    return np.ascontiguousarray(np.stack([np.ascontiguousarray(np.asarray(X, np.float32).reshape(4, 4).T).ravel() for X in poses]))


class PoseDev:
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
        self.T0 = colmajor16(case["poses"])
        self.M = len(case["map_pts"])
        self.own_map = m is None
        self.m = vo.Map(ctx) if m is None else m
        if m is None:
            self.reset_map()
        F = self.F
        self.d_uv, self.d_app, self.d_T = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(self.T0)
        self.d_n = ctx.to_device(np.asarray(case["n_rows"], np.int32)) if case["n_rows"] is not None else None
        self.d_fixed = ctx.to_device(np.asarray(case["fixed"]).astype(np.uint8)) if case.get("fixed") is not None else None
        self.d_Tout, self.d_status, self.d_H, self.d_stats = ctx.alloc(64 * F + 16), ctx.alloc(4 * F + 16), ctx.alloc(288 * F + 16), ctx.alloc(64)
        self.d_pstatus, self.d_rstats = ctx.alloc(4 * self.M + 16), ctx.alloc(64)
        self.params = dict(case.get("params") or {})

    def reset_map(self):
        self.m.clear()
        self.m.update(self.case["map_pts"], self.case["map_app"])
        assert len(self.m) == self.M

    def reset_poses(self):
        self.ctx.h2d(self.d_T, self.T0)

    def clear_out(self):
        F = self.F
        self.ctx.h2d(self.d_Tout, np.full(16 * F + 4, -7.0, np.float32))
        self.ctx.h2d(self.d_status, np.full(F + 4, -7, np.int32))
        self.ctx.h2d(self.d_H, np.full(36 * F + 2, -7.0, np.float64))
        self.ctx.h2d(self.d_stats, np.full(16, -7, np.int32))

    def call(self, status=True, H=True, in_place=False, m="own", **kw):
        """the return code of vo_map_refine_poses_batch_dev; kw overrides: F, n_max, uv_stride, app_stride, K, d_uv, d_app, d_n,
        d_T, d_Tout, d_fixed, d_H, d_stats, prm (None: null), n_rounds, min_obs, huber_px, damping"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        p = dict(self.params)
        p.update({k: kw[k] for k in ("n_rounds", "min_obs", "huber_px", "damping") if k in kw})
        prm = self.vo.MapPoseRefineParams(int(p["n_rounds"]), int(p["min_obs"]), float(p["huber_px"]), float(p["damping"]))
        K = g("K", self.K)
        return self.lib.vo_map_refine_poses_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), K.ctypes.data_as(C.c_void_p) if K is not None else None,
            v(g("d_uv", self.d_uv)), C.c_size_t(g("uv_stride", self.stride)), v(g("d_app", self.d_app)),
            C.c_size_t(g("app_stride", self.stride)), C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)), v(g("d_T", self.d_T)),
            v(g("d_fixed", self.d_fixed)), None if ("prm" in kw and kw["prm"] is None) else C.byref(prm),
            v(g("d_Tout", self.d_T if in_place else self.d_Tout)), v(self.d_status if status else None),
            v(g("d_H", self.d_H if H else None)), v(g("d_stats", self.d_stats)))

    def refine_points(self, n_rounds, min_obs, huber_px, damping, d_stats=None):
        """vo_map_refine_batch_dev in place on the map from the poses in d_T"""
        v = lambda d: C.c_void_p(d) if d else None
        prm = self.vo.MapRefineParams(int(n_rounds), int(min_obs), float(huber_px), float(damping))
        return self.lib.vo_map_refine_batch_dev(self.m.h, C.c_int(self.F), self.K.ctypes.data_as(C.c_void_p), v(self.d_uv), C.c_size_t(self.stride),
                                                v(self.d_app), C.c_size_t(self.stride), C.c_int(self.n_max), v(self.d_n), v(self.d_T), C.byref(prm),
                                                v(self.d_pstatus), None, v(d_stats or self.d_rstats))

    def adjust(self, d_stats, **p):
        """vo_map_adjust_batch_dev in place on d_T and the map; p: the fields of MapAdjustParams"""
        v = lambda d: C.c_void_p(d) if d else None
        prm = self.vo.MapAdjustParams(int(p["n_sweeps"]), int(p["pose_rounds"]), int(p["point_rounds"]), int(p["min_obs_pose"]),
                                      int(p["min_obs_point"]), float(p["huber_px"]), float(p["damping"]))
        return self.lib.vo_map_adjust_batch_dev(self.m.h, C.c_int(self.F), self.K.ctypes.data_as(C.c_void_p), v(self.d_uv), C.c_size_t(self.stride),
                                                v(self.d_app), C.c_size_t(self.stride), C.c_int(self.n_max), v(self.d_n), v(self.d_T),
                                                v(self.d_fixed), C.byref(prm), v(self.d_status), v(self.d_pstatus), v(d_stats))

    def read(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        self.ctx.d2h(out, d)
        return out

    def results(self, in_place=False):
        """(poses out (F, 16) float32 column-major, status (F,), H (F, 36) float64, stats bytes (48,)) as the device holds them"""
        F = self.F
        return (self.read(self.d_T if in_place else self.d_Tout, (F, 16), np.float32), self.read(self.d_status, F, np.int32),
                self.read(self.d_H, (F, 36), np.float64), self.read(self.d_stats, 48, np.uint8))

    def stats(self, raw):
        s = self.vo.MapPoseRefineStats()
        C.memmove(C.byref(s), raw.ctypes.data, 48)
        return s.as_dict()

    def points(self):
        return self.m.read()[0]

    def close(self):
        for d in (self.d_uv, self.d_app, self.d_T, self.d_n, self.d_fixed, self.d_Tout, self.d_status, self.d_H, self.d_stats, self.d_pstatus,
                  self.d_rstats):
            if d:
                self.ctx.free(d)
        if self.own_map:
            self.m.close()


def mats(T16):
    """(F, 16) column-major -> (F, 4, 4)"""
    return np.asarray(T16).reshape(-1, 4, 4).transpose(0, 2, 1)
