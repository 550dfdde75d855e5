"""Device-side plumbing of tests/test_gpu_map_guided.py: a case of tests/map_guided_cases.py as a device map plus padded frame
arrays (strides above n_max), voe_map_guided_batch_dev on them with every argument switchable, and the read-back of its outputs in
the shape map_guided_restatement.compare() takes."""
import ctypes as C

import numpy as np

from map_nearest_dev import GUARD, same      # noqa: F401  (re-exported)


def colmajor16(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(16)


class GuidedDev:
    def __init__(self, vo, ctx, case, stride_pad=3):
        self.vo, self.ctx, self.case, self.lib = vo, ctx, case, ctx.lib
        self.m = vo.Map(ctx, case["capacity"]) if case["capacity"] else vo.Map(ctx)
        self.bufs = []
        frames = case["frames"]
        self.F, self.n_max, self.M = len(frames), case["n_max"], len(case["map_app"])
        self.stride = self.n_max + stride_pad
        app = np.full((self.F, self.stride, 10), 0.25, np.float32)      # behind a frame's rows: rows nobody may read as live
        uv = np.full((self.F, self.stride, 2), 100.0, np.float32)
        for f, (p, a) in enumerate(frames):
            app[f, : len(a)] = a
            uv[f, : len(p)] = p
        self.app, self.uv = app, uv
        n = case["n_rows"] if case["n_rows"] is not None else [len(a) for _, a in frames]
        self.n = np.asarray(n, np.int32)
        self.T = np.stack([colmajor16(T) for T in case["poses"]])
        self.K = np.ascontiguousarray(np.asarray(case["K"], np.float32).T).reshape(9)      # column-major
        self.d_app, self.d_uv, self.d_n, self.d_T = self.dev(app), self.dev(uv), self.dev(self.n), self.dev(self.T)
        k = case["dup_rows"]                                  # rows entered twice: the host counts them, the device does not
        E, P = case["map_app"], case["map_pts"]
        if len(E):
            self.m.update(np.concatenate([P, P[:k]]), np.concatenate([E, E[:k]]))
        self.prm = vo.MapGuidedParams(case["radius_px"], case["radius"], case["ratio"], case["unique"], case["z_near"], case["z_far"])
        R = self.F * self.n_max
        self.d_entry, self.d_status, self.d_dist2, self.d_pix2 = self.alloc(4 * R), self.alloc(4 * R), self.alloc(4 * R), self.alloc(4 * R)
        self.d_out, self.d_stats = self.alloc(app.nbytes), self.alloc(48)

    def alloc(self, n):
        p = self.ctx.alloc(n + 16)
        self.bufs.append(p)
        return p

    def dev(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.to_device(arr if arr.size else np.zeros(4, arr.dtype))
        self.bufs.append(p)
        return p

    def read(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        self.ctx.d2h(out, d)
        return out

    def clear_out(self, d_out=None):
        R = self.F * self.n_max
        for d in (self.d_entry, self.d_status, self.d_dist2, self.d_pix2):
            self.ctx.h2d(d, np.full(R + 4, GUARD, np.int32))
        self.ctx.h2d(self.d_stats, np.full(16, GUARD, np.int32))
        guard = np.concatenate([self.app.ravel().view(np.int32), np.full(4, GUARD, np.int32)])      # the rows as they came in
        self.ctx.h2d(d_out if d_out else self.d_out, guard)

    def call(self, m="own", **kw):
        """the return code of voe_map_guided_batch_dev; kw overrides F, K (None: null), d_uv, uv_stride, d_app, app_stride, n_max,
        d_n, d_T, prm (None: null), d_entry, d_status, d_dist2, d_pix2, d_out, d_stats"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        K = g("K", self.K)
        return self.lib.voe_map_guided_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), None if K is None else K.ctypes.data_as(C.c_void_p), v(g("d_uv", self.d_uv)),
            C.c_size_t(g("uv_stride", self.stride)), v(g("d_app", self.d_app)), C.c_size_t(g("app_stride", self.stride)),
            C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)), v(g("d_T", self.d_T)),
            None if ("prm" in kw and kw["prm"] is None) else C.byref(g("prm", self.prm)), v(g("d_entry", self.d_entry)),
            v(g("d_status", self.d_status)), v(g("d_dist2", self.d_dist2)), v(g("d_pix2", self.d_pix2)), v(g("d_out", self.d_out)),
            v(g("d_stats", self.d_stats)))

    def outputs(self, d_out=None):
        """the bytes of every output array with its guard words, as the device holds them"""
        self.ctx.synchronize()
        R = self.F * self.n_max
        return [self.read(d, n + 4, np.int32) for d, n in ((self.d_entry, R), (self.d_status, R), (self.d_dist2, R), (self.d_pix2, R),
                                                           (d_out if d_out else self.d_out, self.app.size), (self.d_stats, 12))]

    def got(self, o=None):
        """the call's results in the shape map_guided_restatement.compare() takes"""
        o = self.outputs() if o is None else o
        assert all((x[-4:] == GUARD).all() for x in o), "an output array was written behind its end"
        F, N, R = self.F, self.n_max, self.F * self.n_max
        out = o[4][: self.app.size].view(np.float32).reshape(self.app.shape)
        keep = np.ones(self.app.shape[:2], bool)              # what the call must leave alone: the rows behind every frame's count
        for f in range(F):
            keep[f, : max(0, min(int(self.n[f]), N))] = False
        assert out[keep].tobytes() == self.app[keep].tobytes(), "a row behind the live count was written"
        st = self.vo.MapGuidedStats()
        C.memmove(C.byref(st), o[5].ctypes.data, 48)
        return dict(entry=o[0][:R].reshape(F, N), status=o[1][:R].reshape(F, N), dist2=o[2][:R].view(np.float32).reshape(F, N),
                    pix2=o[3][:R].view(np.float32).reshape(F, N), app=[out[f, : len(self.case["frames"][f][1])].copy() for f in range(F)],
                    stats=st.as_dict())

    def map_state(self):
        """the bytes of the map: points, appearances and the header words as the device holds them, and the entry the table finds
        for every row of the case's map (no call here refreshes the host's bound of the size)"""
        self.ctx.synchronize()
        px, pa, ph = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert self.lib.vo_map_dev_ptrs(self.m.h, C.byref(px), C.byref(pa), C.byref(ph)) == 0
        n = max(self.M, 1)
        E = self.case["map_app"]
        look = self.m.lookup(E[~np.isnan(E).any(axis=1)])[1] if self.M else np.zeros(0, np.int32)
        return [self.read(px.value, 3 * n, np.float32), self.read(pa.value, 10 * n, np.float32), self.read(ph.value, 16, np.int32), look]

    def lookup_entries(self, d_app):
        """vo_map_lookup_batch_dev on frames laid out as the case's: the entry per position, (F, n_max)"""
        R = self.F * self.n_max
        d_pairs, d_cnt, d_ent = self.alloc(8 * R), self.alloc(4 * self.F), self.alloc(4 * R)
        self.m.lookup_batch_dev(self.F, d_app, self.stride, self.n_max, self.d_n, d_pairs, d_cnt, d_entries=d_ent)
        self.ctx.synchronize()
        return self.read(d_ent, (self.F, self.n_max), np.int32)

    def close(self):
        for d in self.bufs:
            self.ctx.free(d)
        self.m.close()
