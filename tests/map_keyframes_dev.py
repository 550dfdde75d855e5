"""Device-side plumbing of tests/test_gpu_map_keyframes.py: a case of tests/map_keyframes_cases.py as device buffers (the bit
rows, the row counts, the flags) and voe_map_keyframes_dev on them with every optional argument switchable."""
import ctypes as C

import numpy as np

INT_KEYS = ("verdict", "n_rows", "step", "order", "seen", "red")


class KeyframesDev:
    def __init__(self, vo, ctx, case):
        self.vo, self.ctx, self.case, self.lib = vo, ctx, case, ctx.lib
        self.m = vo.Map(ctx)
        self.bufs = []
        self.F, self.W = case["bits"].shape
        self.n_max = case["n_max"]
        self.d_bits = self.dev(case["bits"])
        self.d_n = self.dev(np.asarray(case["n_rows"], np.int32)) if case["n_rows"] is not None else None
        self.d_flags = self.dev(np.asarray(case["flags"], np.uint8)) if case["flags"] is not None else None
        self.d = {k: self.alloc(4 * self.F) for k in INT_KEYS}
        self.d_keep, self.d_stats = self.alloc(self.F), self.alloc(64)

    def alloc(self, n):
        p = self.ctx.alloc(n + 16)
        self.bufs.append(p)
        return p

    def dev(self, arr):
        p = self.ctx.to_device(np.ascontiguousarray(arr))
        self.bufs.append(p)
        return p

    def read(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        self.ctx.d2h(out, d)
        return out

    def clear_out(self):
        for k in INT_KEYS:
            self.ctx.h2d(self.d[k], np.full(self.F + 4, -7, np.int32))
        self.ctx.h2d(self.d_keep, np.full(self.F + 16, 0xEE, np.uint8))
        self.ctx.h2d(self.d_stats, np.full(16, -7, np.int32))

    def call(self, params, with_order=True, m="own", **kw):
        """the return code of voe_map_keyframes_dev; kw overrides F, n_words, d_bits, d_n, n_max, d_flags, prm (None: null),
        reserved, d_stats and the outputs by their names"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        prm = self.vo.MapKeyframesParams(int(params["min_observers"]), int(params["share_permille"]), int(params["min_seen"]), int(params["max_gap"]),
                                         int(params["max_dropped"]), (C.c_int32 * 3)(*kw.get("reserved", (0, 0, 0))))
        out = {k: g(k, self.d[k]) for k in INT_KEYS}
        return self.lib.voe_map_keyframes_dev(self.m.h if m == "own" else m, C.c_int(g("F", self.F)), C.c_int(g("n_words", self.W)),
                                              v(g("d_bits", self.d_bits)), v(g("d_n", self.d_n)), C.c_int(g("n_max", self.n_max)),
                                              v(g("d_flags", self.d_flags)), None if ("prm" in kw and kw["prm"] is None) else C.byref(prm),
                                              v(out["verdict"]), v(out["n_rows"]), v(g("keep", self.d_keep)), v(out["step"]),
                                              v(out["order"] if with_order else None), v(out["seen"]), v(out["red"]), v(g("d_stats", self.d_stats)))

    def results(self):
        """dict(verdict, n_rows, keep, step, order, seen, red, stats bytes, guard: the words behind every array) as the device
        holds them"""
        self.ctx.synchronize()
        F = self.F
        out, guard = {}, []
        for k in INT_KEYS:
            a = self.read(self.d[k], F + 4, np.int32)
            out[k] = a[:F]
            guard.append(a[F:])
        a = self.read(self.d_keep, F + 16, np.uint8)
        out["keep"] = a[:F]
        st = self.read(self.d_stats, 16, np.int32)
        out["stats_raw"] = st[:8].copy()
        out["guard"] = np.concatenate(guard + [a[F:].astype(np.int32) - 0xEE - 7, st[8:]])      # (every guard word is -7 when untouched)
        return out

    def stats(self, raw):
        s = self.vo.MapKeyframesStats()
        C.memmove(C.byref(s), raw.ctypes.data, 32)
        return s.as_dict()

    def bits(self):
        return self.read(self.d_bits, (self.F, self.W), np.uint32)

    def close(self):
        for d in self.bufs:
            self.ctx.free(d)
        self.m.close()


def same(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
