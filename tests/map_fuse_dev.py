"""Device-side plumbing of tests/test_gpu_map_fuse.py: a case of tests/map_fuse_cases.py as a device map plus padded frame arrays
(a stride above n_max), voe_map_fuse_batch_dev on them with every argument switchable, the read-back of its outputs in the shape
map_fuse_restatement.compare() takes, and the map's bytes as the device holds them."""
import ctypes as C

import numpy as np

from map_nearest_dev import GUARD, same      # noqa: F401  (re-exported)

FILL = np.float32(0.5)                                        # what a separate d_app_out holds before the call


class FuseDev:
    def __init__(self, vo, ctx, case, stride_pad=3):
        self.vo, self.ctx, self.case, self.lib = vo, ctx, case, ctx.lib
        self.m = vo.Map(ctx, case["capacity"]) if case["capacity"] else vo.Map(ctx)
        self.bufs = []
        frames = case["frames"]
        self.has_frames = frames is not None
        self.F, self.n_max, self.M = (len(frames) if self.has_frames else 0), case["n_max"], len(case["map_app"])
        self.stride = self.n_max + stride_pad
        app = np.full((max(self.F, 1), self.stride, 10), 0.25, np.float32)      # behind a frame's rows: rows nobody may read as live
        n = []
        for f in range(self.F):
            app[f, : len(frames[f])] = frames[f]
            n.append(len(frames[f]) if case["n_rows"] is None else case["n_rows"][f])
        self.app, self.n = app, np.asarray(n, np.int32)
        self.live = np.zeros(app.shape[:2], bool)
        for f in range(self.F):
            self.live[f, : max(0, min(int(self.n[f]), self.n_max))] = True
        self.d_app = self.dev(app) if self.has_frames else 0
        # d_n_rows is NULL only where the case gives no counts and every frame holds n_max rows (NULL means n_max live rows each)
        counts = self.has_frames and (case["n_rows"] is not None or any(len(a) != self.n_max for a in frames))
        self.d_n = self.dev(self.n) if counts else 0
        self.d_count = self.dev(self.n) if self.has_frames else 0      # (the lookups of the tests always get the counts)
        self.prm = vo.MapFuseParams(case["radius_xyz"], case["radius"], case["position"], case["veto"], case["dry_run"])
        S = max(self.M + case["dup_rows"], 1)
        self.S = S
        self.d_per_entry = [self.alloc(4 * S) for _ in range(5)]      # partner, dist2, gap2, verdict, remap
        self.d_out, self.d_stats = self.alloc(app.nbytes), self.alloc(56)
        self.init_out = None
        self.reset()

    def reset(self):
        """the map back at the case's start (with dup_rows: rows entered twice, which the host counts and the device does not)"""
        k = self.case["dup_rows"]
        E, P = self.case["map_app"], self.case["map_pts"]
        self.m.clear()
        if len(E):
            self.m.update(np.concatenate([P, P[:k]]), np.concatenate([E, E[:k]]))

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

    def clear_out(self, d_out=None, in_place=False):
        for d in self.d_per_entry:
            self.ctx.h2d(d, np.full(self.S + 4, GUARD, np.int32))
        self.ctx.h2d(self.d_stats, np.full(18, GUARD, np.int32))
        self.init_out = self.app.copy() if in_place else np.full(self.app.shape, FILL, np.float32)
        self.ctx.h2d(d_out if d_out else self.d_out, np.concatenate([self.init_out.ravel().view(np.int32), np.full(4, GUARD, np.int32)]))

    def call(self, m="own", **kw):
        """the return code of voe_map_fuse_batch_dev; kw overrides F, d_app, app_stride, n_max, d_n, prm (None: null), d_partner,
        d_dist2, d_gap2, d_verdict, d_remap, d_out, d_stats"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        pe = [g(k, d) for k, d in zip(("d_partner", "d_dist2", "d_gap2", "d_verdict", "d_remap"), self.d_per_entry)]
        return self.lib.voe_map_fuse_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), v(g("d_app", self.d_app)), C.c_size_t(g("app_stride", self.stride if self.has_frames else 0)),
            C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)), None if ("prm" in kw and kw["prm"] is None) else C.byref(g("prm", self.prm)),
            v(pe[0]), v(pe[1]), v(pe[2]), v(pe[3]), v(pe[4]), v(g("d_out", self.d_out if self.has_frames else 0)), v(g("d_stats", self.d_stats)))

    def outputs(self, d_out=None):
        """the bytes of every output array with its guard words, as the device holds them"""
        self.ctx.synchronize()
        return [self.read(d, self.S + 4, np.int32) for d in self.d_per_entry] + [
            self.read(d_out if d_out else self.d_out, self.app.size + 4, np.int32), self.read(self.d_stats, 18, np.int32)]

    def got(self, o=None):
        """the call's per-entry results and statistics in the shape map_fuse_restatement.compare() takes (the rows: rows_as_expected)"""
        o = self.outputs() if o is None else o
        assert all((x[self.M:] == GUARD).all() for x in o[:5]), "a per-entry output was written behind the map's size"
        assert (o[5][-4:] == GUARD).all() and (o[6][14:] == GUARD).all(), "an output array was written behind its end"
        st = self.vo.MapFuseStats()
        C.memmove(C.byref(st), o[6].ctypes.data, 56)
        M = self.M
        return dict(partner=o[0][:M], dist2=o[1][:M].view(np.float32), gap2=o[2][:M].view(np.float32), verdict=o[3][:M], remap=o[4][:M],
                    stats=st.as_dict())

    def rows_as_expected(self, ref, o):
        """rule 7 on the bytes of d_app_out: the live rows are the reference's (unless dry_run), every other byte is what the array
        held before the call"""
        want = self.init_out.copy()
        if self.has_frames and not self.case["dry_run"]:
            for f in range(self.F):
                k = int(self.live[f].sum())
                want[f, :k] = ref["app"][f][:k]
        return o[5][: self.app.size].tobytes() == want.tobytes()

    def map_state(self):
        """the bytes of the map as the device holds them -- size, points, appearances, header -- and the entry the table finds for
        every row of the case's map (no call here refreshes the host's bound of the size)"""
        self.ctx.synchronize()
        px, pa, ph = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert self.lib.vo_map_dev_ptrs(self.m.h, C.byref(px), C.byref(pa), C.byref(ph)) == 0
        hdr = self.read(ph.value, 16, np.int32)
        n = max(int(hdr[0]), 1)
        E = self.case["map_app"]
        look = self.m.lookup(E[~np.isnan(E).any(axis=1)])[1] if self.M else np.zeros(0, np.int32)
        return [self.read(px.value, 3 * n, np.float32), self.read(pa.value, 10 * n, np.float32), hdr, look]

    def lookup_entries(self, d_app):
        """vo_map_lookup_batch_dev on frames laid out as the case's: the entry per position, (F, n_max)"""
        R = max(self.F * self.n_max, 1)
        d_pairs, d_cnt, d_ent = self.alloc(8 * R), self.alloc(4 * max(self.F, 1)), self.alloc(4 * R)
        self.ctx.h2d(d_ent, np.full(R, -1, np.int32))
        if self.F * self.n_max:
            self.m.lookup_batch_dev(self.F, d_app, self.stride, self.n_max, self.d_count, d_pairs, d_cnt, d_entries=d_ent)
        self.ctx.synchronize()
        return self.read(d_ent, R, np.int32)[: self.F * self.n_max].reshape(self.F, self.n_max)

    def close(self):
        for d in self.bufs:
            self.ctx.free(d)
        self.m.close()


def remapped(entries, remap):
    """rule 7's contract: remap[the entry the lookup returned before], -1 staying -1"""
    e = np.asarray(entries)
    return np.where(e >= 0, np.asarray(remap)[np.maximum(e, 0)], -1).astype(np.int32) if len(remap) else e.astype(np.int32)
