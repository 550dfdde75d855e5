"""Device-side plumbing of tests/test_gpu_map_align.py: a case of tests/map_align_cases.py as two device maps, and
voe_map_align_dev / voe_map_merge_dev on them with every optional argument switchable."""
import ctypes as C

import numpy as np


class AlignDev:
    def __init__(self, vo, ctx, case, dst_capacity=0):
        self.vo, self.ctx, self.lib, self.case = vo, ctx, ctx.lib, case
        self.dst, self.src = vo.Map(ctx, dst_capacity), vo.Map(ctx)
        self.reset()
        self.n_max = self.src.size_bound()
        assert self.n_max == len(case["src_pts"])
        self.H = int(case["params"]["n_hypotheses"])
        n = max(self.n_max, 1)
        self.d_S, self.d_pairs, self.d_nm = ctx.alloc(64), ctx.alloc(8 * n + 16), ctx.alloc(16)
        self.d_mask, self.d_counts, self.d_stats = ctx.alloc(n + 16), ctx.alloc(4 * self.H + 16), ctx.alloc(64)
        self.d_remap, self.d_mstats, self.d_S_in = ctx.alloc(4 * n + 16), ctx.alloc(16), ctx.alloc(64)
        self.bufs = [self.d_S, self.d_pairs, self.d_nm, self.d_mask, self.d_counts, self.d_stats, self.d_remap, self.d_mstats, self.d_S_in]

    def reset(self):
        """both maps as the case has them"""
        c = self.case
        for m, p, a in ((self.dst, c["dst_pts"], c["dst_app"]), (self.src, c["src_pts"], c["src_app"])):
            m.clear()
            if len(p):
                m.update(p, a)
            assert len(m) == len(p)

    def params(self, **kw):
        p = dict(self.case["params"], **kw)
        return self.vo.MapAlignParams(int(p["seed"]) & 0xFFFFFFFFFFFFFFFF, int(p["n_hypotheses"]), int(p["with_scale"]), int(p["n_refits"]),
                                      int(p["min_inliers"]), float(p["threshold"]), 0)

    def clear_out(self):
        n = max(self.n_max, 1)
        self.ctx.h2d(self.d_S, np.full(16, -7, np.float32))
        self.ctx.h2d(self.d_pairs, np.full(2 * n + 4, -7, np.int32))
        self.ctx.h2d(self.d_nm, np.full(4, -7, np.int32))
        self.ctx.h2d(self.d_mask, np.full(n + 16, 7, np.uint8))
        self.ctx.h2d(self.d_counts, np.full(self.H + 4, -7, np.int32))
        self.ctx.h2d(self.d_stats, np.full(16, -7, np.int32))
        self.ctx.h2d(self.d_remap, np.full(n + 4, -7, np.int32))
        self.ctx.h2d(self.d_mstats, np.full(4, -7, np.int32))

    def align(self, optional=True, dst="own", src="own", prm="own", **kw):
        """the return code of voe_map_align_dev; kw overrides fields of the params and the pointers d_S, d_pairs, d_nm, d_stats"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw.pop(k) if k in kw else d
        d_S, d_pairs, d_nm, d_stats = g("d_S", self.d_S), g("d_pairs", self.d_pairs), g("d_nm", self.d_nm), g("d_stats", self.d_stats)
        p = self.params(**kw)
        return self.lib.voe_map_align_dev(self.dst.h if dst == "own" else dst, self.src.h if src == "own" else src,
                                          C.byref(p) if prm == "own" else prm, v(d_S), v(d_pairs), v(d_nm),
                                          v(self.d_mask if optional else None), v(self.d_counts if optional else None), v(d_stats))

    def read(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        self.ctx.d2h(out, d)
        return out

    def results(self):
        """dict of everything the call wrote, as the device holds it (after a synchronise)"""
        self.ctx.synchronize()
        n = max(self.n_max, 1)
        raw = self.read(self.d_stats, 48, np.uint8)
        st = self.vo.MapAlignStats()
        C.memmove(C.byref(st), raw.ctypes.data, 48)
        k = int(self.read(self.d_nm, 1, np.int32)[0])
        return dict(S=self.read(self.d_S, 16, np.float32).reshape(4, 4).T.copy(), n_matches=k,
                    pairs=self.read(self.d_pairs, (n, 2), np.int32)[: max(k, 0)], mask=self.read(self.d_mask, n, np.uint8)[: self.n_max],
                    counts=self.read(self.d_counts, self.H, np.int32), stats=st.as_dict(), raw_stats=raw)

    @staticmethod
    def same_bytes(x, y, optional=True):
        keys = ("S", "pairs", "raw_stats") + (("mask", "counts") if optional else ())
        return x["n_matches"] == y["n_matches"] and all(x[k].tobytes() == y[k].tobytes() for k in keys)

    def merge(self, S, policy, remap=True, dst="own", src="own", d_stats="own", upload=True):
        """the return code of voe_map_merge_dev; S: 4x4 or None (upload=False: the device holds it already, as inside a capture)"""
        v = lambda d: C.c_void_p(d) if d else None
        if S is not None and upload:
            self.ctx.h2d(self.d_S_in, np.ascontiguousarray(np.asarray(S, np.float32).T).ravel())
        return self.lib.voe_map_merge_dev(self.dst.h if dst == "own" else dst, self.src.h if src == "own" else src,
                                          v(self.d_S_in if S is not None else None), C.c_int(policy), v(self.d_remap if remap else None),
                                          v(self.d_mstats if d_stats == "own" else d_stats))

    def merge_results(self):
        self.ctx.synchronize()
        st = self.read(self.d_mstats, 4, np.int32)
        return dict(remap=self.read(self.d_remap, max(self.n_max, 1), np.int32)[: self.n_max],
                    stats=dict(n_src=int(st[0]), n_shared=int(st[1]), n_appended=int(st[2]), n_dst_after=int(st[3])))

    def state(self, m):
        """(points, appearances) of a map as the device holds them"""
        return m.read()

    def lookups(self, m, app):
        """the entry vo_map_lookup finds per row of app, -1 for none"""
        return m.lookup(app)[1] if len(app) else np.zeros(0, np.int32)

    def close(self):
        for d in self.bufs:
            self.ctx.free(d)
        self.dst.close(); self.src.close()
