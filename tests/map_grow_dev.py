"""Device-side plumbing of tests/test_gpu_map_grow.py: a case of tests/map_grow_cases.py as a device map plus padded frame
arrays (CullDev of tests/map_cull_dev.py, which also brings the cull and the lookups) and voe_map_grow_batch_dev on them with
every optional argument switchable."""
import ctypes as C

import numpy as np

from map_cull_dev import CullDev

CULL_KEYS = ("min_obs", "min_frames", "max_rms_px", "max_err_px", "min_parallax_deg")


class GrowDev(CullDev):
    def __init__(self, vo, ctx, case, track_cap=None, **kw):
        grow_params = dict(case["params"])
        cull_view = dict(case, params=dict({k: grow_params[k] for k in CULL_KEYS}, drop_unseen=False, dry_run=True))
        super().__init__(vo, ctx, cull_view, **kw)
        self.case = case
        if case["n_rows"] is None and len({len(a) for _, a in case["frames"]}) > 1:
            # frames of several lengths without row counts: the counts ARE the lengths (the padding behind them is NaN rows, which a
            # null d_n_rows would count as live rows with a NaN); frames of one length keep the null pointer
            self.d_n = ctx.to_device(np.array([len(a) for _, a in case["frames"]], np.int32))
        self.grow_params = grow_params
        self.rows = max(self.F * self.n_max, 1)
        self.track_cap = self.rows if track_cap is None else track_cap
        self.d_rows, self.d_tracks, self.d_gstats = ctx.alloc(4 * self.rows + 16), ctx.alloc(80 * max(self.track_cap, 1) + 16), ctx.alloc(128)

    def clear_grow_out(self):
        self.ctx.h2d(self.d_rows, np.full(self.rows + 4, -7, np.int32))
        self.ctx.h2d(self.d_tracks, np.full(20 * max(self.track_cap, 1) + 4, -7, np.int32))
        self.ctx.h2d(self.d_gstats, np.full(32, -7, np.int32))

    def grow(self, m="own", outputs=True, **kw):
        """the return code of voe_map_grow_batch_dev; kw overrides fields of the params and F, n_max, uv_stride, app_stride, K,
        d_uv, d_app, d_n, d_T, d_stats, d_tracks, track_cap, prm (None: null)"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        p = dict(self.grow_params)
        p.update({k: kw[k] for k in p if k in kw})
        prm = self.vo.MapGrowParams(int(p["n_rounds"]), int(p["min_obs"]), int(p["min_frames"]), float(p["huber_px"]), float(p["damping"]),
                                    float(p["max_rms_px"]), float(p["max_err_px"]), float(p["min_parallax_deg"]), int(p["max_added"]),
                                    int(bool(p["dry_run"])))
        K = g("K", self.K)
        return self.lib.voe_map_grow_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), K.ctypes.data_as(C.c_void_p) if K is not None else None,
            v(g("d_uv", self.d_uv)), C.c_size_t(g("uv_stride", self.stride)), v(g("d_app", self.d_app)),
            C.c_size_t(g("app_stride", self.stride)), C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)), v(g("d_T", self.d_T)),
            None if ("prm" in kw and kw["prm"] is None) else C.byref(prm), v(self.d_rows if outputs else None),
            v(g("d_tracks", self.d_tracks if outputs else None)), C.c_int(g("track_cap", self.track_cap if outputs else 0)),
            v(g("d_stats", self.d_gstats)))

    def gstats(self, raw=None):
        raw = self.read(self.d_gstats, 96, np.uint8) if raw is None else raw
        s = self.vo.MapGrowStats()
        C.memmove(C.byref(s), raw.ctypes.data, 96)
        assert not any(s.reserved)
        return s.as_dict()

    def grow_results(self):
        """(rows (F, n_max) int32, tracks structured (min(n_tracks, track_cap),), stats bytes (96,)) as the device holds them"""
        self.ctx.synchronize()
        raw = self.read(self.d_gstats, 96, np.uint8)
        n = min(self.gstats(raw)["n_tracks"], self.track_cap)
        tr = self.read(self.d_tracks, 80 * max(self.track_cap, 1), np.uint8)[: 80 * n].view(self.vo.MAP_GROW_TRACK_DTYPE)
        return self.read(self.d_rows, self.rows, np.int32)[: self.F * self.n_max].reshape(self.F, self.n_max), tr, raw

    def close(self):
        for d in (self.d_rows, self.d_tracks, self.d_gstats):
            self.ctx.free(d)
        super().close()
