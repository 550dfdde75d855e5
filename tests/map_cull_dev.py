"""Device-side plumbing of tests/test_gpu_map_cull.py: a case of tests/map_cull_cases.py as a device map plus padded frame
arrays (RefineDev of tests/map_refine_dev.py) and voe_map_cull_batch_dev on them with every optional argument switchable."""
import ctypes as C

import numpy as np

from map_refine_dev import RefineDev


class CullDev(RefineDev):
    def __init__(self, vo, ctx, case, **kw):
        super().__init__(vo, ctx, case, **kw)
        M, rows = max(self.M, 1), max(self.F * self.stride, 1)
        self.d_verdict, self.d_remap, self.d_entry, self.d_cstats = ctx.alloc(4 * M + 16), ctx.alloc(4 * M + 16), ctx.alloc(48 * M + 16), ctx.alloc(64)
        self.d_pairs, self.d_cnt, self.d_ent = ctx.alloc(8 * rows), ctx.alloc(4 * self.F + 16), ctx.alloc(4 * rows)
        self.cull_params = dict(case["params"])

    def clear_cull_out(self):
        M = max(self.M, 1)
        self.ctx.h2d(self.d_verdict, np.full(M + 4, -7, np.int32))
        self.ctx.h2d(self.d_remap, np.full(M + 4, -7, np.int32))
        self.ctx.h2d(self.d_entry, np.full(12 * M + 4, -7, np.int32))
        self.ctx.h2d(self.d_cstats, np.full(16, -7, np.int32))

    def cull(self, m="own", outputs=True, **kw):
        """the return code of voe_map_cull_batch_dev; kw overrides fields of the params and F, n_max, uv_stride, app_stride, K,
        d_uv, d_app, d_n, d_T, d_stats, d_entry, prm (None: null)"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        p = dict(self.cull_params)
        p.update({k: kw[k] for k in p if k in kw})
        prm = self.vo.MapCullParams(int(p["min_obs"]), int(p["min_frames"]), float(p["max_rms_px"]), float(p["max_err_px"]),
                                    float(p["min_parallax_deg"]), int(bool(p["drop_unseen"])), int(bool(p["dry_run"])))
        K = g("K", self.K)
        return self.lib.voe_map_cull_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), K.ctypes.data_as(C.c_void_p) if K is not None else None,
            v(g("d_uv", self.d_uv)), C.c_size_t(g("uv_stride", self.stride)), v(g("d_app", self.d_app)),
            C.c_size_t(g("app_stride", self.stride)), C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)), v(g("d_T", self.d_T)),
            None if ("prm" in kw and kw["prm"] is None) else C.byref(prm), v(self.d_verdict if outputs else None),
            v(self.d_remap if outputs else None), v(g("d_entry", self.d_entry if outputs else None)), v(g("d_stats", self.d_cstats)))

    def read(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        self.ctx.d2h(out, d)
        return out

    def cull_results(self, n=None):
        """(verdict (n,), remap (n,), entries (n,) structured, stats bytes (48,)) as the device holds them; n: the old size"""
        n = self.M if n is None else n
        raw = self.read(self.d_entry, 48 * max(n, 1), np.uint8)[: 48 * n]
        return (self.read(self.d_verdict, max(n, 1), np.int32)[:n], self.read(self.d_remap, max(n, 1), np.int32)[:n],
                raw.view(self.vo.MAP_CULL_ENTRY_DTYPE), self.read(self.d_cstats, 48, np.uint8))

    def cstats(self, raw):
        s = self.vo.MapCullStats()
        C.memmove(C.byref(s), raw.ctypes.data, 48)
        return s.as_dict()

    def map_state(self):
        """(points, appearances, history) as the device holds them"""
        p, a = self.m.read()
        return p, a, self.m.history()

    def lookups(self):
        """vo_map_lookup_batch_dev of every frame of the case: the entry per position (F, n_max), -1 for none"""
        self.ctx.h2d(self.d_ent, np.full(max(self.F * self.stride, 1), -9, np.int32))
        self.m.lookup_batch_dev(self.F, self.d_app, self.stride, self.n_max, self.d_n, self.d_pairs, self.d_cnt, d_entries=self.d_ent)
        self.ctx.synchronize()
        return self.read(self.d_ent, max(self.F * self.n_max, 1), np.int32)[: self.F * self.n_max].reshape(self.F, self.n_max)

    def close(self):
        for d in (self.d_verdict, self.d_remap, self.d_entry, self.d_cstats, self.d_pairs, self.d_cnt, self.d_ent):
            self.ctx.free(d)
        super().close()


def remapped(entries, remap):
    """what a lookup returns after the cull: remap[the entry it returned before], -1 staying -1"""
    e = np.asarray(entries)
    return np.where(e >= 0, np.asarray(remap)[np.maximum(e, 0)], -1).astype(np.int32)
