"""Device-side plumbing of tests/test_gpu_map_bundle.py: a case of tests/map_bundle_cases.py as a device map plus padded frame
arrays (PoseDev of tests/map_pose_refine_dev.py) and vox_map_bundle_batch_dev on them."""
import ctypes as C

import numpy as np

from map_pose_refine_dev import PoseDev


class BundleDev(PoseDev):
    def __init__(self, vo, ctx, case, **kw):
        super().__init__(vo, ctx, case, **kw)
        self.R = max(int(case["params"]["n_rounds"]), 1)
        self.d_rounds, self.d_bstats = ctx.alloc(40 * self.R + 16), ctx.alloc(64)

    def clear_bundle_out(self):
        self.ctx.h2d(self.d_status, np.full(self.F + 4, -7, np.int32))
        self.ctx.h2d(self.d_pstatus, np.full(self.M + 4, -7, np.int32))
        self.ctx.h2d(self.d_rounds, np.full(10 * self.R + 4, -7, np.int32))
        self.ctx.h2d(self.d_bstats, np.full(16, -7, np.int32))

    def bundle(self, m="own", outputs=True, **kw):
        """the return code of vox_map_bundle_batch_dev in place on d_T and the map; kw overrides fields of the params and
        d_T, d_stats, K, F, n_max, uv_stride, app_stride"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        p = dict(self.params)
        p.update({k: kw[k] for k in p if k in kw})
        prm = self.vo.MapBundleParams(int(p["n_rounds"]), int(p["n_cg"]), float(p["cg_tol"]), float(p["lambda0"]), int(p["min_obs_pose"]),
                                      int(p["min_obs_point"]), float(p["huber_px"]))
        K = g("K", self.K)
        return self.lib.vox_map_bundle_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), K.ctypes.data_as(C.c_void_p) if K is not None else None, v(self.d_uv),
            C.c_size_t(g("uv_stride", self.stride)), v(self.d_app), C.c_size_t(g("app_stride", self.stride)), C.c_int(g("n_max", self.n_max)),
            v(self.d_n), v(g("d_T", self.d_T)), v(self.d_fixed), None if ("prm" in kw and kw["prm"] is None) else C.byref(prm),
            v(self.d_status if outputs else None), v(self.d_pstatus if outputs else None), v(self.d_rounds if outputs else None),
            v(g("d_stats", self.d_bstats)))

    def bundle_results(self, n_rounds=None):
        """(poses (F, 16), points (M, 3), pose status, point status, round records as bytes, stats as bytes) as the device holds them"""
        n = self.params["n_rounds"] if n_rounds is None else n_rounds
        return (self.read(self.d_T, (self.F, 16), np.float32), self.points(), self.read(self.d_status, self.F, np.int32),
                self.read(self.d_pstatus, self.M, np.int32), self.read(self.d_rounds, 40 * n, np.uint8), self.read(self.d_bstats, 48, np.uint8))

    def rounds(self, raw):
        n = len(raw) // 40
        rec = (self.vo.MapBundleRound * max(n, 1))()
        C.memmove(rec, raw.ctypes.data, 40 * n)
        return [rec[k].as_dict() for k in range(n)]

    def bstats(self, raw):
        s = self.vo.MapBundleStats()
        C.memmove(C.byref(s), raw.ctypes.data, 48)
        return s.as_dict()

    def close(self):
        self.ctx.free(self.d_rounds); self.ctx.free(self.d_bstats)
        super().close()
