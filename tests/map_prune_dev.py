"""Device-side plumbing of tests/test_gpu_map_prune.py: a case of tests/map_prune_cases.py as a device map plus padded frame
arrays (RefineDev of tests/map_refine_dev.py: strides of n_max + 3, NaN appearance rows behind a frame's own) and
voe_map_prune_batch_dev on them with every optional argument switchable.  Run as a program it is the CHILD of the workspace
poison test: it runs the named cases under whatever VO_WS_POISON its environment holds and writes every output to an .npz."""
import ctypes as C
import os
import sys

import numpy as np

from map_refine_dev import RefineDev

FILL = -7
PARAMS = ("max_err_px", "rel_factor", "rel_floor_px", "rel_min_obs", "unique", "max_share_landmark", "max_share_frame")


class PruneDev(RefineDev):
    def __init__(self, vo, ctx, case, **kw):
        super().__init__(vo, ctx, case, n_max=kw.pop("n_max", case["n_max"]), **kw)
        self.rows, self.cells = max(self.F * self.n_max, 1), max(self.F * self.stride, 1)
        M = max(self.M, 1)
        a = ctx.alloc
        self.d_entry, self.d_pstatus, self.d_sq, self.d_app_out = a(4 * self.rows + 16), a(4 * self.rows + 16), a(8 * self.rows + 16), a(40 * self.cells + 16)
        self.d_lm, self.d_fr, self.d_pstats = a(32 * M + 16), a(16 * self.F + 16), a(64 + 16)
        self.d_pairs, self.d_cnt, self.d_ent = a(8 * self.cells), a(4 * self.F + 16), a(4 * self.cells)
        self.d_centry, self.d_cstats = a(48 * M + 16), a(64)
        self.app0 = self.read(self.d_app, (self.F, self.stride, 10), np.float32)
        self.prune_params = dict(case["params"])
        n = np.full(self.F, self.n_max, np.int64) if case["n_rows"] is None else np.clip(np.asarray(case["n_rows"], np.int64), 0, self.n_max)
        self.live = np.arange(self.n_max)[None, :] < n[:, None]

    def read(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        self.ctx.d2h(out, d)
        return out

    def clear_prune_out(self):
        M = max(self.M, 1)
        for d, words in ((self.d_entry, self.rows + 4), (self.d_pstatus, self.rows + 4), (self.d_sq, 2 * self.rows + 4), (self.d_app_out, 10 * self.cells + 4),
                         (self.d_lm, 8 * M + 4), (self.d_fr, 4 * self.F + 4), (self.d_pstats, 16 + 4)):
            self.ctx.h2d(d, np.full(words, FILL, np.int32))

    def restore_rows(self):
        """the frames' rows as the case gives them (after a call in place)"""
        self.ctx.h2d(self.d_app, self.app0)

    def prune(self, m="own", outputs=True, in_place=False, **kw):
        """the return code of voe_map_prune_batch_dev; kw overrides fields of the params, `reserved`, and F, n_max, uv_stride,
        app_stride, K, d_uv, d_app, d_n, d_T, d_entry, d_status, d_sq, d_app_out, d_lm, d_fr, d_stats, prm (None: null)"""
        v = lambda d: C.c_void_p(d) if d else None
        g = lambda k, d: kw[k] if k in kw else d
        p = dict(self.prune_params)
        p.update({k: kw[k] for k in PARAMS if k in kw})
        prm = self.vo.MapPruneParams(float(p["max_err_px"]), float(p["rel_factor"]), float(p["rel_floor_px"]), int(p["rel_min_obs"]), int(p["unique"]),
                                     int(p["max_share_landmark"]), int(p["max_share_frame"]), int(kw.get("reserved", 0)))
        K = g("K", self.K)
        opt = lambda d: d if outputs else None
        return self.lib.voe_map_prune_batch_dev(
            self.m.h if m == "own" else m, C.c_int(g("F", self.F)), K.ctypes.data_as(C.c_void_p) if K is not None else None,
            v(g("d_uv", self.d_uv)), C.c_size_t(g("uv_stride", self.stride)), v(g("d_app", self.d_app)),
            C.c_size_t(g("app_stride", self.stride)), C.c_int(g("n_max", self.n_max)), v(g("d_n", self.d_n)), v(g("d_T", self.d_T)),
            None if ("prm" in kw and kw["prm"] is None) else C.byref(prm), v(g("d_entry", self.d_entry)), v(g("d_status", opt(self.d_pstatus))),
            v(g("d_sq", opt(self.d_sq))), v(g("d_app_out", opt(self.d_app if in_place else self.d_app_out))), v(g("d_lm", opt(self.d_lm))),
            v(g("d_fr", opt(self.d_fr))), v(g("d_stats", self.d_pstats)))

    def prune_one(self, f, **kw):
        """voe_map_prune_dev on frame f of the arrays, its outputs at row f of the batched outputs' arrays"""
        v = lambda d: C.c_void_p(d) if d else None
        p = dict(self.prune_params)
        p.update({k: kw[k] for k in PARAMS if k in kw})
        prm = self.vo.MapPruneParams(float(p["max_err_px"]), float(p["rel_factor"]), float(p["rel_floor_px"]), int(p["rel_min_obs"]), int(p["unique"]),
                                     int(p["max_share_landmark"]), int(p["max_share_frame"]), 0)
        return self.lib.voe_map_prune_dev(self.m.h, self.K.ctypes.data_as(C.c_void_p), v(self.d_uv + 8 * f * self.stride), v(self.d_app + 40 * f * self.stride),
                                          C.c_int(self.n_max), v(self.d_n + 4 * f if self.d_n else None), v(self.d_T + 64 * f), C.byref(prm),
                                          v(self.d_entry + 4 * f * self.n_max), v(self.d_pstatus + 4 * f * self.n_max), v(self.d_sq + 8 * f * self.n_max),
                                          v(self.d_app_out + 40 * f * self.stride), None, None, v(self.d_pstats))

    def prune_results(self, in_place=False):
        """dict(entry, status (F, n_max) int32, sq (F, n_max) float64, app (F, stride, 10) float32: d_app_out or d_app, lm (M,),
        fr (F,) structured, stats (64,) uint8, tails: the words behind every array) as the device holds them"""
        self.ctx.synchronize()
        F, n, M = self.F, self.n_max, self.M
        r = dict(entry=self.read(self.d_entry, self.rows + 4, np.int32), status=self.read(self.d_pstatus, self.rows + 4, np.int32),
                 sq=self.read(self.d_sq, self.rows + 2, np.float64), app=self.read(self.d_app if in_place else self.d_app_out, (F, self.stride, 10), np.float32),
                 lm=self.read(self.d_lm, 32 * max(M, 1) + 16, np.uint8), fr=self.read(self.d_fr, 16 * F + 16, np.uint8), stats=self.read(self.d_pstats, 64 + 16, np.uint8))
        tails = [r["entry"][F * n:], r["status"][F * n:], r["sq"][F * n:].view(np.int32), r["lm"][32 * M:].view(np.int32), r["fr"][16 * F:].view(np.int32),
                 r["stats"][64:].view(np.int32)]
        r["tails_kept"] = all((t == FILL).all() for t in tails)
        r["entry"], r["status"], r["sq"] = r["entry"][: F * n].reshape(F, n), r["status"][: F * n].reshape(F, n), r["sq"][: F * n].reshape(F, n)
        r["lm"], r["fr"], r["stats"] = r["lm"][: 32 * M].view(self.vo.MAP_PRUNE_LANDMARK_DTYPE), r["fr"][: 16 * F].view(self.vo.MAP_PRUNE_FRAME_DTYPE), r["stats"][:64]
        return r

    def pstats(self, raw):
        s = self.vo.MapPruneStats()
        C.memmove(C.byref(s), np.ascontiguousarray(raw).ctypes.data, 64)
        return s.as_dict()

    def map_state(self):
        """(points, appearances, history, header) as the device holds them"""
        import map_states
        p, a = self.m.read()
        return p, a, self.m.history(), map_states.header(self.ctx, self.m)

    def lookups(self, d_app=None):
        """vo_map_lookup_batch_dev of every frame on the given rows (default: the case's): the entry per position (F, n_max)"""
        self.ctx.h2d(self.d_ent, np.full(self.cells, -9, np.int32))
        self.m.lookup_batch_dev(self.F, self.d_app if d_app is None else d_app, self.stride, self.n_max, self.d_n, self.d_pairs, self.d_cnt, d_entries=self.d_ent)
        self.ctx.synchronize()
        return self.read(self.d_ent, self.rows, np.int32)[: self.F * self.n_max].reshape(self.F, self.n_max)

    def cull_dry(self, d_app, max_err_px):
        """a dry-run voe_map_cull_batch_dev on the given rows: (entries (M,) structured, stats dict)"""
        v = lambda d: C.c_void_p(d) if d else None
        prm = self.vo.MapCullParams(1, 1, 0.0, float(max_err_px), 0.0, 0, 1)
        rc = self.lib.voe_map_cull_batch_dev(self.m.h, C.c_int(self.F), self.K.ctypes.data_as(C.c_void_p), v(self.d_uv), C.c_size_t(self.stride), v(d_app),
                                             C.c_size_t(self.stride), C.c_int(self.n_max), v(self.d_n), v(self.d_T), C.byref(prm), None, None, v(self.d_centry),
                                             v(self.d_cstats))
        assert rc == 0, self.lib.vo_last_error()
        self.ctx.synchronize()
        s = self.vo.MapCullStats()
        raw = self.read(self.d_cstats, 48, np.uint8)
        C.memmove(C.byref(s), raw.ctypes.data, 48)
        return self.read(self.d_centry, 48 * max(self.M, 1), np.uint8)[: 48 * self.M].view(self.vo.MAP_CULL_ENTRY_DTYPE), s.as_dict()

    def close(self):
        for d in (self.d_entry, self.d_pstatus, self.d_sq, self.d_app_out, self.d_lm, self.d_fr, self.d_pstats, self.d_pairs, self.d_cnt, self.d_ent,
                  self.d_centry, self.d_cstats):
            self.ctx.free(d)
        super().close()


def flat(r):
    """the outputs of a call as one dict of byte strings (what two runs are compared by)"""
    return {k: np.ascontiguousarray(r[k]).tobytes() for k in ("entry", "status", "sq", "app", "lm", "fr", "stats")}


def run_case(vo, ctx, case, in_place=False, **kw):
    d = PruneDev(vo, ctx, case)
    try:
        d.clear_prune_out()
        rc = d.prune(in_place=in_place, **kw)
        assert rc == 0, ctx.lib.vo_last_error()
        return d.prune_results(in_place=in_place)
    finally:
        d.close()


if __name__ == "__main__":                                    # the child of the poison test: python map_prune_dev.py out.npz case ...
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import __graft_entry__ as g
    import map_prune_cases as Pc
    vo_ = g.load_package()
    ctx_ = vo_.Context(0)
    out = {"poison": np.array([vo_.load_library().vo_abi_version(), 1 if os.environ.get("VO_WS_POISON") else 0])}
    for name in sys.argv[2:]:
        for mode in (False, True):
            r = run_case(vo_, ctx_, Pc.case(name), in_place=mode)
            assert r["tails_kept"]
            for k, b in flat(r).items():
                out[f"{name}/{int(mode)}/{k}"] = np.frombuffer(b, np.uint8)
    np.savez(sys.argv[1], **out)
    print("map_prune_dev: wrote", sys.argv[1])
