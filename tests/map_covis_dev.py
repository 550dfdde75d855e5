"""Device-side plumbing of tests/test_gpu_map_covis.py: a case of tests/map_covis_cases.py as a device map plus padded frame
arrays, and voe_map_covis_batch_dev / voe_map_window_dev on them with every optional argument switchable."""
import ctypes as C

import numpy as np

import map_covis_cases as Cc


class CovisDev:
    def __init__(self, vo, ctx, case, stride_pad=3):
        self.vo, self.ctx, self.case, self.lib = vo, ctx, case, ctx.lib
        self.m = vo.Map(ctx)
        self.bufs = []
        if "bits" in case:                                    # a window case: the bits are given
            self.F, self.W = case["bits"].shape
            self.n_max, self.stride, self.M = case["n_max"], case["n_max"], 0
            self.d_app = None
        else:
            frames = case["frames"]
            self.F, self.W, self.n_max, self.M = len(frames), Cc.n_words_of(case), Cc.n_max_of(case), len(case["map_app"])
            self.stride = self.n_max + stride_pad
            app = np.full((self.F, self.stride, 10), np.nan, np.float32)      # behind a frame's rows: NaN (they find nothing)
            for f, (_, a) in enumerate(frames):
                app[f, : len(a)] = np.asarray(a, np.float32).reshape(-1, 10)
            self.d_app = self.dev(app)
            k = case["dup_rows"]                              # rows entered twice: the host counts them, the device does not
            self.m.clear()
            self.m.update(np.concatenate([case["map_pts"], case["map_pts"][:k]]), np.concatenate([case["map_app"], case["map_app"][:k]]))
        self.d_n = self.dev(np.asarray(case["n_rows"], np.int32)) if case["n_rows"] is not None else None
        F, W = self.F, self.W
        self.d_bits = self.dev(case["bits"]) if "bits" in case else self.alloc(4 * F * W)
        self.d_counts, self.d_stats = self.alloc(4 * F * F), self.alloc(64)
        self.d_role, self.d_rows, self.d_fixed, self.d_order, self.d_union, self.d_wstats = (self.alloc(4 * F), self.alloc(4 * F), self.alloc(F),
                                                                                           self.alloc(4 * F), self.alloc(4 * W), self.alloc(64))

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

    # ---- covisibility ----
    def clear_covis_out(self):
        F, W = self.F, self.W
        self.ctx.h2d(self.d_bits, np.full(F * W + 4, 0xA5A5A5A5, np.uint32))
        self.ctx.h2d(self.d_counts, np.full(F * F + 4, -7, np.int32))
        self.ctx.h2d(self.d_stats, np.full(16, -7, np.int32))

    def covis(self, counts=True, m="own", **kw):
        """the return code of voe_map_covis_batch_dev; kw overrides F, d_app, app_stride, n_max, d_n, n_words, d_bits, d_stats"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        return self.lib.voe_map_covis_batch_dev(self.m.h if m == "own" else m, C.c_int(g("F", self.F)), v(g("d_app", self.d_app)),
                                                C.c_size_t(g("app_stride", self.stride)), C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)),
                                                C.c_int(g("n_words", self.W)), v(g("d_bits", self.d_bits)), v(self.d_counts if counts else None),
                                                v(g("d_stats", self.d_stats)))

    def covis_results(self):
        """(bits (F, W), counts (F, F), stats bytes (32,), the 4 words behind the bits) as the device holds them"""
        self.ctx.synchronize()
        F, W = self.F, self.W
        b = self.read(self.d_bits, F * W + 4, np.uint32)
        return b[: F * W].reshape(F, W), self.read(self.d_counts, (F, F), np.int32), self.read(self.d_stats, 32, np.uint8), b[F * W:]

    def cstats(self, raw):
        s = self.vo.MapCovisStats()
        C.memmove(C.byref(s), raw.ctypes.data, 32)
        assert list(s.reserved) == [0, 0, 0]
        return s.as_dict()

    # ---- the window ----
    def clear_window_out(self):
        F, W = self.F, self.W
        for d, n in ((self.d_role, F), (self.d_rows, F), (self.d_order, F), (self.d_union, W)):
            self.ctx.h2d(d, np.full(n + 4, -7, np.int32))
        self.ctx.h2d(self.d_fixed, np.full(F + 16, 0xEE, np.uint8))
        self.ctx.h2d(self.d_wstats, np.full(16, -7, np.int32))

    def window(self, params, optional=True, m="own", **kw):
        """the return code of voe_map_window_dev; kw overrides F, n_words, d_bits, d_n, n_max, prm (None: null), d_role, d_rows,
        d_fixed, d_stats"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        prm = self.vo.MapWindowParams(int(params["query"]), int(params["k_free"]), int(params["k_fixed"]), int(params["min_shared"]))
        return self.lib.voe_map_window_dev(self.m.h if m == "own" else m, C.c_int(g("F", self.F)), C.c_int(g("n_words", self.W)),
                                           v(g("d_bits", self.d_bits)), v(g("d_n", self.d_n)), C.c_int(g("n_max", self.n_max)),
                                           None if ("prm" in kw and kw["prm"] is None) else C.byref(prm), v(g("d_role", self.d_role)),
                                           v(g("d_rows", self.d_rows)), v(g("d_fixed", self.d_fixed)), v(self.d_order if optional else None),
                                           v(self.d_union if optional else None), v(g("d_stats", self.d_wstats)))

    def window_results(self):
        """dict(role, n_rows, fixed, order, union, stats bytes) as the device holds them"""
        self.ctx.synchronize()
        F, W = self.F, self.W
        return dict(role=self.read(self.d_role, F, np.int32), n_rows=self.read(self.d_rows, F, np.int32), fixed=self.read(self.d_fixed, F, np.uint8),
                    order=self.read(self.d_order, F, np.int32), union=self.read(self.d_union, W, np.uint32), stats=self.read(self.d_wstats, 32, np.uint8))

    def wstats(self, raw):
        s = self.vo.MapWindowStats()
        C.memmove(C.byref(s), raw.ctypes.data, 32)
        assert s.reserved == 0
        return s.as_dict()

    # ---- the map ----
    def map_state(self):
        """the bytes of the map: points, appearances and the header words as the device holds them, the history, and the entry
        the table finds for every class of the case (no call here refreshes the host's bound of the size)"""
        self.ctx.synchronize()
        px, pa, ph = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert self.lib.vo_map_dev_ptrs(self.m.h, C.byref(px), C.byref(pa), C.byref(ph)) == 0
        n = max(self.M, 1)
        out = [self.read(px.value, 3 * n, np.float32), self.read(pa.value, 10 * n, np.float32), self.read(ph.value, 16, np.int32), self.m.history()]
        if self.M:
            out.append(self.m.lookup(self.case["map_app"])[1])
        return out

    def close(self):
        for d in self.bufs:
            self.ctx.free(d)
        self.m.close()


def same(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
