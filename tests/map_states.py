"""The states a device map can be in when a `_dev` call meets it, for tests/test_gpu_map_states.py: builders that leave a
vo.Map holding exactly the rows given -- in order, bit for bit -- while the HOST'S bound of the size (voe_map_size_bound; what
every call that must not wait sizes its launches and workspaces by) is not the size, and the device-side plumbing of every
`_dev` call on guarded output arrays.

    exact        capacity 4096, one eager update                                          bound M          (the twin)
    slack_1/300  as exact, then the first 1 / 300 rows again (same points: every byte stays)    bound M + 1 / M + 300
    replayed     capacity 1024; rows [0, 300) eager, the update of a 300-row buffer captured, two replays with rows
                 [300, 600) and [600, 900)                                                  bound 1024, size 900 (the host counted 600)
    overflowed   capacity 1024; 400 rows eager, captured, two replays of 400 rows: 1024 kept, 176 dropped (hdr[3] == 176)

No builder calls anything that refreshes the host's bound once the state is made (len(m), m.read(), any host form): the content
is verified through vo_map_dev_ptrs (_read_dev of tests/test_gpu_map_update.py), the state through m.size_bound().  A test
asserts the bound again AFTER the call under test (State.check_bound)."""
import ctypes as C

import numpy as np

from test_gpu_map_update import Captured, _read_dev

GUARD = 64                                                    # elements behind every output array, which must come back untouched
FILL = 0xA5
CAM = (480, 640, 0, 10)
V = lambda d: C.c_void_p(d) if d else None


def header(ctx, m):
    """the four header words as the device holds them (size, base and rows of the last update, rows dropped for lack of room)"""
    d_s = C.c_void_p()
    assert ctx.lib.vo_map_dev_ptrs(m.h, None, None, C.byref(d_s)) == 0
    h = np.zeros(4, np.int32)
    ctx.synchronize()
    ctx.d2h(h, d_s.value)
    return h


def content(ctx, m, cap):
    """(points (size, 3), appearances (size, 10), header (4,)) through vo_map_dev_ptrs: nothing here tells the host the size"""
    ctx.synchronize()
    p, a, size = _read_dev(ctx, m, cap)
    return p[:size].copy(), a[:size].copy(), header(ctx, m)


class State:
    def __init__(self, ctx, m, cap, bound, captured=None):
        self.ctx, self.m, self.cap, self.bound, self.captured = ctx, m, cap, bound, captured

    def check_bound(self, bound=None):
        assert self.m.size_bound() == (self.bound if bound is None else bound), (self.m.size_bound(), self.bound, bound)

    def content(self):
        return content(self.ctx, self.m, self.cap)

    def close(self):
        if self.captured is not None:
            self.captured.close()
        self.m.close()


def _verify(st, pts, app, dropped=0):
    p, a, h = st.content()
    assert h[0] == len(pts) and h[3] == dropped, (h, len(pts), dropped)
    assert p.tobytes() == np.ascontiguousarray(pts, np.float32).tobytes() and a.tobytes() == np.ascontiguousarray(app, np.float32).tobytes()
    st.check_bound()
    return st


def _rows_ok(app):
    app = np.asarray(app, np.float32)
    assert not np.isnan(app).any() and len({r.tobytes() for r in app}) == len(app), "the builders want unique, NaN-free appearances"


def build_exact(vo, ctx, pts, app, capacity=4096):
    """the twin: bound == size"""
    _rows_ok(app)
    m = vo.Map(ctx, capacity=capacity)
    m.update(pts, app)
    return _verify(State(ctx, m, capacity, len(pts)), pts, app)


def build_slack(vo, ctx, pts, app, k):
    _rows_ok(app)
    m = vo.Map(ctx, capacity=4096)
    m.update(pts, app)
    m.update(pts[:k], app[:k])                                # known classes, the same points: every byte stays, the host counts k more
    return _verify(State(ctx, m, 4096, len(pts) + k), pts, app)


def _by_replays(vo, ctx, pts, app, n, capacity=1024):
    """rows [0, n) eager, the update of an n-row buffer captured, then one replay per further n rows of `pts`"""
    _rows_ok(app)
    assert len(pts) % n == 0
    m = vo.Map(ctx, capacity=capacity)
    cap = Captured(vo, ctx, m, n, with_T=False)
    cap.write(pts[:n], app[:n], n)
    cap.eager()
    cap.capture()
    for k in range(1, len(pts) // n):
        cap.write(pts[k * n:(k + 1) * n], app[k * n:(k + 1) * n], n)
        cap.launch()
    return m, cap


def build_replayed(vo, ctx, pts, app):
    assert len(pts) == 900
    m, cap = _by_replays(vo, ctx, pts, app, 300)
    return _verify(State(ctx, m, 1024, 1024, cap), pts, app)


def build_overflowed(vo, ctx, pts, app):
    """pts, app: the 1200 rows sent; the map keeps the first 1024 and counts 176 dropped"""
    assert len(pts) == 1200
    m, cap = _by_replays(vo, ctx, pts, app, 400)
    return _verify(State(ctx, m, 1024, 1024, cap), pts[:1024], app[:1024], dropped=176)


def build(vo, ctx, state, pts, app):
    if state == "exact":
        return build_exact(vo, ctx, pts, app)
    if state.startswith("slack_"):
        return build_slack(vo, ctx, pts, app, int(state[6:]))
    return dict(replayed=build_replayed, overflowed=build_overflowed)[state](vo, ctx, pts, app)


# ---- output arrays with a guard ------------------------------------------------------------------------------------------------
class Outs:
    """device arrays of n elements + GUARD more, every byte FILL before the call; read() returns the n elements and asserts that
    the guard kept every byte"""

    def __init__(self, ctx):
        self.ctx, self.b, self.init = ctx, {}, {}

    def new(self, name, n, item, init=None):
        if name in self.b:                                    # a second call on the same arrays (a captured call: no allocation then)
            assert self.b[name][1:] == (max(int(n), 0), item)
            return self.b[name][0]
        n = max(int(n), 0)
        nbytes = (n + GUARD) * item
        d = self.ctx.alloc(nbytes + 16)
        raw = np.full(nbytes, FILL, np.uint8)
        if init is not None:
            init = np.ascontiguousarray(init).view(np.uint8).ravel()
            assert len(init) == n * item
            raw[: n * item] = init
        self.ctx.h2d(d, raw)
        self.b[name] = (d, n, item)
        self.init[name] = raw
        return d

    def __getitem__(self, name):
        return self.b[name][0]

    def refill(self):
        """every array as it was before the call (for a captured call, whose pointers are fixed)"""
        for name, (d, _, _) in self.b.items():
            self.ctx.h2d(d, self.init[name])

    def read(self):
        self.ctx.synchronize()
        out = {}
        for name, (d, n, item) in self.b.items():
            raw = np.zeros((n + GUARD) * item, np.uint8)
            self.ctx.d2h(raw, d)
            assert (raw[n * item:] == FILL).all(), f"{name}: written behind its {n} elements"
            out[name] = raw[: n * item].copy()
        return out

    def close(self):
        for d, _, _ in self.b.values():
            self.ctx.free(d)
        self.b = {}


def i32(raw):
    return np.asarray(raw, np.uint8).view(np.int32)


def untouched(raw):
    return (np.asarray(raw) == FILL).all()


# ---- a window of frames in device memory and every `_dev` call on it --------------------------------------------------------
class Win:
    def __init__(self, vo, ctx, case, stride_pad=3):
        self.vo, self.ctx, self.lib, self.case = vo, ctx, ctx.lib, case
        self.K = np.ascontiguousarray(np.asarray(case["K"], np.float32).reshape(3, 3).T).ravel()
        frames = case["frames"]
        self.F = len(frames)
        self.n_max = len(frames[0][1])
        assert all(len(a) == self.n_max for _, a in frames) and case["n_rows"] is None
        self.stride = self.n_max + stride_pad
        uv = np.full((self.F, self.stride, 2), 1e9, np.float32)
        app = np.full((self.F, self.stride, 10), np.nan, np.float32)
        for f, (p, a) in enumerate(frames):
            uv[f, : self.n_max] = p; app[f, : self.n_max] = a
        self.T0 = np.ascontiguousarray(np.stack([np.ascontiguousarray(np.asarray(X, np.float32).reshape(4, 4).T).ravel() for X in case["poses"]]))
        self.d_uv, self.d_app = ctx.to_device(uv), ctx.to_device(app)
        self.d_fixed = ctx.to_device(np.asarray(case["fixed"]).astype(np.uint8))
        self.rows = self.F * self.n_max

    def close(self):
        for d in (self.d_uv, self.d_app, self.d_fixed):
            self.ctx.free(d)

    def _frames(self, uv=True):
        I, S = C.c_int, C.c_size_t
        head = (I(self.F), self.K.ctypes.data_as(C.c_void_p), V(self.d_uv), S(self.stride)) if uv else (I(self.F),)
        return head + (V(self.d_app), S(self.stride), I(self.n_max), None)

    def _ok(self, rc):
        assert rc == 0, self.lib.vo_last_error()

    def poses(self, o, T=None):
        return o.new("T", self.F, 64, self.T0 if T is None else T)

    # every method: enqueues on map m with fresh guarded outputs in o (size: the entries the map holds); the caller reads o
    def lookup(self, m, o, size):
        R = self.rows
        self._ok(self.lib.vo_map_lookup_batch_dev(m.h, C.c_int(self.F), V(self.d_app), C.c_size_t(self.stride), C.c_int(self.n_max), None,
                                                  V(o.new("pairs", R, 8)), V(o.new("counts", self.F, 4)), V(o.new("xyz", R, 12)),
                                                  V(o.new("local", R, 8)), V(o.new("entries", R, 4))))

    def localise(self, m, o, size, n_hyp=64, px=2.0, seed=3, thr=10000.0, n_iters=10, min_inliers=6):
        I, S = C.c_int, C.c_size_t
        prm = self.vo.RansacParams(int(n_hyp), float(px), int(seed))
        self._ok(self.lib.vo_map_localise_batch_dev(m.h, I(self.F), *map(I, CAM), self.K.ctypes.data_as(C.c_void_p), V(self.d_uv), S(self.stride),
                                                    V(self.d_app), S(self.stride), I(self.n_max), None, C.byref(prm), C.c_float(thr), I(n_iters),
                                                    I(min_inliers), None, V(o.new("T_out", self.F, 64)), V(o.new("stats", self.F, 32))))

    def refine(self, m, o, size, p, xyz=False):
        """in place on the map; with xyz the map is NOT written and the array takes every entry's point"""
        prm = self.vo.MapRefineParams(int(p["n_rounds"]), int(p["min_obs"]), float(p["huber_px"]), float(p["damping"]))
        self._ok(self.lib.vo_map_refine_batch_dev(m.h, *self._frames(), V(self.poses(o)), C.byref(prm), V(o.new("status", size, 4)),
                                                  V(o.new("xyz", size, 12)) if xyz else None, V(o.new("stats", 1, 48))))

    def refine_poses(self, m, o, size, p):
        prm = self.vo.MapPoseRefineParams(int(p["n_rounds"]), int(p["min_obs"]), float(p["huber_px"]), float(p["damping"]))
        self._ok(self.lib.vo_map_refine_poses_batch_dev(m.h, *self._frames(), V(self.poses(o)), V(self.d_fixed), C.byref(prm),
                                                        V(o.new("T_out", self.F, 64)), V(o.new("status", self.F, 4)), V(o.new("H", self.F, 288)),
                                                        V(o.new("stats", 1, 48))))

    def adjust(self, m, o, size, p):
        prm = self.vo.MapAdjustParams(int(p["n_sweeps"]), int(p["pose_rounds"]), int(p["point_rounds"]), int(p["min_obs_pose"]),
                                      int(p["min_obs_point"]), float(p["huber_px"]), float(p["damping"]))
        self._ok(self.lib.vo_map_adjust_batch_dev(m.h, *self._frames(), V(self.poses(o)), V(self.d_fixed), C.byref(prm),
                                                  V(o.new("pose_status", self.F, 4)), V(o.new("point_status", size, 4)),
                                                  V(o.new("stats", p["n_sweeps"], 96))))

    def bundle(self, m, o, size, p):
        prm = self.vo.MapBundleParams(int(p["n_rounds"]), int(p["n_cg"]), float(p["cg_tol"]), float(p["lambda0"]), int(p["min_obs_pose"]),
                                      int(p["min_obs_point"]), float(p["huber_px"]))
        self._ok(self.lib.vox_map_bundle_batch_dev(m.h, *self._frames(), V(self.poses(o)), V(self.d_fixed), C.byref(prm),
                                                   V(o.new("pose_status", self.F, 4)), V(o.new("point_status", size, 4)),
                                                   V(o.new("rounds", p["n_rounds"], 40)), V(o.new("stats", 1, 48))))

    def cull(self, m, o, size, p, dry_run=False):
        prm = self.vo.MapCullParams(int(p["min_obs"]), int(p["min_frames"]), float(p["max_rms_px"]), float(p["max_err_px"]),
                                    float(p["min_parallax_deg"]), int(bool(p["drop_unseen"])), int(bool(dry_run)))
        self._ok(self.lib.voe_map_cull_batch_dev(m.h, *self._frames(), V(self.poses(o)), C.byref(prm), V(o.new("verdict", size, 4)),
                                                 V(o.new("remap", size, 4)), V(o.new("entry", size, 48)), V(o.new("stats", 1, 48))))

    def grow(self, m, o, size, p, dry_run=False):
        prm = self.vo.MapGrowParams(int(p["n_rounds"]), int(p["min_obs"]), int(p["min_frames"]), float(p["huber_px"]), float(p["damping"]),
                                    float(p["max_rms_px"]), float(p["max_err_px"]), float(p["min_parallax_deg"]), int(p["max_added"]),
                                    int(bool(dry_run)))
        return self.lib.voe_map_grow_batch_dev(m.h, *self._frames(), V(self.poses(o)), C.byref(prm), V(o.new("rows", self.rows, 4)),
                                               V(o.new("tracks", self.rows, 80, np.zeros(80 * self.rows, np.uint8))), C.c_int(self.rows),
                                               V(o.new("stats", 1, 96)))

    def covis(self, m, o, size, n_words):
        self._ok(self.lib.voe_map_covis_batch_dev(m.h, *self._frames(uv=False), C.c_int(n_words), V(o.new("bits", self.F * n_words, 4)),
                                                  V(o.new("counts", self.F * self.F, 4)), V(o.new("stats", 1, 32))))

    def window(self, m, o, n_words, p):
        prm = self.vo.MapWindowParams(int(p["query"]), int(p["k_free"]), int(p["k_fixed"]), int(p["min_shared"]))
        self._ok(self.lib.voe_map_window_dev(m.h, C.c_int(self.F), C.c_int(n_words), V(o["bits"]), None, C.c_int(self.n_max), C.byref(prm),
                                             V(o.new("role", self.F, 4)), V(o.new("n_rows", self.F, 4)), V(o.new("fixed", self.F, 1)),
                                             V(o.new("order", self.F, 4)), V(o.new("union", n_words, 4)), V(o.new("wstats", 1, 32))))


def align(vo, ctx, dst, src, o, n_max, p):
    """voe_map_align_dev; the header sizes pairs and mask by n_max = voe_map_size_bound(src), and ALL n_max mask bytes are written"""
    prm = vo.MapAlignParams(int(p["seed"]) & 0xFFFFFFFFFFFFFFFF, int(p["n_hypotheses"]), int(p["with_scale"]), int(p["n_refits"]),
                            int(p["min_inliers"]), float(p["threshold"]), 0)
    rc = ctx.lib.voe_map_align_dev(dst.h, src.h, C.byref(prm), V(o.new("S", 1, 64)), V(o.new("pairs", n_max, 8)), V(o.new("n_matches", 1, 4)),
                                   V(o.new("mask", n_max, 1)), V(o.new("counts", p["n_hypotheses"], 4)), V(o.new("stats", 1, 48)))
    assert rc == 0, ctx.lib.vo_last_error()


def merge(vo, ctx, dst, src, o, n_max, S, policy):
    """voe_map_merge_dev; d_remap_out is [n_max], -1 beyond src's size (the header)"""
    d_S = o.new("S_in", 1, 64, np.ascontiguousarray(np.asarray(S, np.float32).T).ravel())
    rc = ctx.lib.voe_map_merge_dev(dst.h, src.h, V(d_S), C.c_int(policy), V(o.new("remap", n_max, 4)), V(o.new("mstats", 1, 16)))
    assert rc == 0, ctx.lib.vo_last_error()
