"""ctypes binding of libvo_hip.so, shaped like the reference's interface for the
projective-ICP path: `Camera` (camera.h:12-63), `PICPSolver` (picp_solver.h:18-79),
`triangulate_points` (utils.h:131-160), `compute_correspondences_images` and
`extract_correspondences_world` (vo_complete.cpp:12-66).

The production host side of this repository is C++ (include/vo/*.hpp); this
module exists so that the parity tests and bench.py can drive the very same
C ABI from Python.  There is no Python/NumPy implementation of any operator
here: if the shared library or a gfx950 device is missing, everything raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VO_HIP_LIB selects another build of the same library (e.g. the stamped diagnostic build)
LIB_PATH = os.environ.get("VO_HIP_LIB") or os.path.join(_HERE, "libvo_hip.so")

VO_OK = 0


class VoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libvo_hip error {code}: {msg}")
        self.code = code


_lib = None


def load_library():
    """dlopen libvo_hip.so (built by __graft_entry__.build / make -C csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        _lib.vo_last_error.restype = C.c_char_p
        _lib.vo_ctx_stream.restype = C.c_void_p
    return _lib


def _chk(code):
    if code != VO_OK:
        raise VoError(code, load_library().vo_last_error().decode(errors="replace"))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(shape) if shape is not None else a


def _i32pairs(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1, 2))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _colmajor(M, n):
    return np.ascontiguousarray(np.asarray(M, dtype=np.float32).reshape(n, n).T).ravel()


class Context:
    """One (device, stream).  `stream` may be a raw hipStream_t (int), e.g.
    torch.cuda.current_stream().cuda_stream; None lets the library make one."""

    def __init__(self, device: int = 0, stream=None):
        self.lib = load_library()
        h = C.c_void_p()
        _chk(self.lib.vo_ctx_create(C.c_int(device), C.c_void_p(stream or 0), C.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.vo_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _chk(self.lib.vo_ctx_synchronize(self.h))

    @property
    def stream(self):
        return self.lib.vo_ctx_stream(self.h)

    def device_info(self):
        name = C.create_string_buffer(128)
        ncu = C.c_int()
        _chk(self.lib.vo_ctx_device_info(self.h, name, C.c_int(128), C.byref(ncu)))
        return name.value.decode(), ncu.value

    # raw device memory (for the *_dev entry points)
    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _chk(self.lib.vo_dev_alloc(self.h, C.c_size_t(nbytes), C.byref(p)))
        return p.value

    def free(self, dptr: int):
        _chk(self.lib.vo_dev_free(self.h, C.c_void_p(dptr)))

    def h2d(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        _chk(self.lib.vo_memcpy_h2d(self.h, C.c_void_p(dptr), _ptr(arr), C.c_size_t(arr.nbytes)))

    def d2h(self, arr: np.ndarray, dptr: int):
        assert arr.flags["C_CONTIGUOUS"]
        _chk(self.lib.vo_memcpy_d2h(self.h, _ptr(arr), C.c_void_p(dptr), C.c_size_t(arr.nbytes)))

    def to_device(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = self.alloc(max(arr.nbytes, 16))
        self.h2d(p, arr)
        return p

    def picp_batch_help_info(self, n_problems: int):
        """(own_chunks uint64, n_chunks int32, left_early int32) per problem of the last batched call, which ran with helper
        waves under VO_PICP_HELP_SCHEDULE (vo_picp_batch_help_info; test support)"""
        own = np.zeros(n_problems, np.uint64)
        n_chunks, left = np.zeros(n_problems, np.int32), np.zeros(n_problems, np.int32)
        _chk(self.lib.vo_picp_batch_help_info(self.h, C.c_int(n_problems), _ptr(own), _ptr(n_chunks), _ptr(left)))
        return own, n_chunks, left


class Event:
    """A point in one context's stream that another context can wait for (vo_event_*)."""

    def __init__(self, ctx: Context):
        self.lib = ctx.lib
        h = C.c_void_p()
        _chk(self.lib.vo_event_create(ctx.h, C.byref(h)))
        self.h = h

    def record(self, ctx: Context):
        _chk(self.lib.vo_event_record(self.h, ctx.h))

    def wait(self, ctx: Context):
        """make later work on `ctx` wait for the recorded point (the host does not block)"""
        _chk(self.lib.vo_ctx_wait_event(ctx.h, self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.vo_event_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class Camera:
    """Pinhole camera, camera.h:12-63.  K is 3x3, pose (world in camera) 4x4."""

    def __init__(self, rows=100, cols=100, z_near=0, z_far=10, camera_matrix=None,
                 world_in_camera_pose=None, ctx: Context | None = None):
        self._rows, self._cols = int(rows), int(cols)
        self._z_near, self._z_far = int(z_near), int(z_far)     # ints, camera.h:18-19
        self._K = np.eye(3, dtype=np.float32) if camera_matrix is None else _f32(camera_matrix, (3, 3)).copy()
        self._T = np.eye(4, dtype=np.float32) if world_in_camera_pose is None else _f32(world_in_camera_pose, (4, 4)).copy()
        self._ctx = ctx

    def rows(self): return self._rows
    def cols(self): return self._cols
    def cameraMatrix(self): return self._K
    def worldInCameraPose(self): return self._T
    def setWorldInCameraPose(self, T): self._T = _f32(T, (4, 4)).copy()

    def copy(self):
        return Camera(self._rows, self._cols, self._z_near, self._z_far, self._K, self._T, self._ctx)

    def projectPoints(self, world_points, keep_indices=False):
        """camera.cpp:16-37.  Returns (image_points, num_points_inside)."""
        ctx = self._ctx or default_context()
        w = _f32(world_points, (-1, 3))
        n = len(w)
        out = np.empty((max(n, 1), 2), dtype=np.float32)
        n_out, n_in = C.c_int(), C.c_int()
        _chk(ctx.lib.vo_project_points(ctx.h, C.c_int(self._rows), C.c_int(self._cols), C.c_int(self._z_near),
                                       C.c_int(self._z_far), _ptr(_colmajor(self._K, 3)), _ptr(_colmajor(self._T, 4)),
                                       _ptr(w), C.c_int(n), C.c_int(int(keep_indices)), _ptr(out),
                                       C.byref(n_out), C.byref(n_in)))
        return out[: n_out.value].copy(), n_in.value

    def projectPoint(self, world_point):
        """camera.h:25-37 through the batched kernel.  Returns (ok, uv)."""
        uv, n_in = self.projectPoints(np.asarray(world_point, dtype=np.float32).reshape(1, 3), keep_indices=True)
        return n_in == 1, uv[0]


class PICPSolver:
    """picp_solver.h:18-79 on the GPU.  oneRound() enqueues and returns; camera(),
    numInliers(), chiInliers(), chiOutliers() synchronise."""

    def __init__(self, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        h = C.c_void_p()
        _chk(self.lib.vo_picp_create(self.ctx.h, C.byref(h)))
        self.h = h
        self._cam = Camera(ctx=self.ctx)

    def close(self):
        if getattr(self, "h", None):
            self.lib.vo_picp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init(self, camera: Camera, world_points, image_points):
        """picp_solver.cpp:16-23"""
        self._cam = camera.copy()
        _chk(self.lib.vo_picp_set_camera(self.h, C.c_int(camera.rows()), C.c_int(camera.cols()),
                                         C.c_int(camera._z_near), C.c_int(camera._z_far),
                                         _ptr(_colmajor(camera.cameraMatrix(), 3)),
                                         _ptr(_colmajor(camera.worldInCameraPose(), 4))))
        w = _f32(world_points, (-1, 3))
        z = _f32(image_points, (-1, 2))
        _chk(self.lib.vo_picp_set_points(self.h, _ptr(w), C.c_int(len(w)), _ptr(z), C.c_int(len(z))))

    def kernelThreshold(self):
        t = C.c_float()
        _chk(self.lib.vo_picp_get_kernel_threshold(self.h, C.byref(t)))
        return t.value

    def setKernelThreshold(self, thr):
        _chk(self.lib.vo_picp_set_kernel_threshold(self.h, C.c_float(thr)))

    def _pairs(self, correspondences):
        # converted on every call (no copy for a C-contiguous int32 array): the library compares the whole array
        # with its GPU copy, so an in-place edit between two rounds is honoured (picp_solver.cpp:62)
        return _i32pairs(correspondences)

    def setExact(self, on=True):
        """reference-order arithmetic (vo_picp_set_exact): bit-identical to the reference's float32 loop"""
        _chk(self.lib.vo_picp_set_exact(self.h, C.c_int(int(bool(on)))))

    def graphInfo(self):
        """(use_graph, cached graphs, failed captures) of this handle: vo_picp_graph_info"""
        u, n, f = C.c_int(), C.c_int(), C.c_int()
        _chk(self.lib.vo_picp_graph_info(self.h, C.byref(u), C.byref(n), C.byref(f)))
        return u.value, n.value, f.value

    def submitInfo(self):
        """(multi-round solves of this handle replayed from a captured graph, ... submitted as plain launches):
        voe_picp_submit_info"""
        g, p = C.c_ulonglong(), C.c_ulonglong()
        _chk(self.lib.voe_picp_submit_info(self.h, C.byref(g), C.byref(p)))
        return g.value, p.value

    def chainInfo(self):
        """(rounds whose finishing launch is still to come, oneRound calls enqueued ahead of their comparison, how many
        of those were repeated): vo_picp_chain_info"""
        o, a, b = C.c_int(), C.c_ulonglong(), C.c_ulonglong()
        _chk(self.lib.vo_picp_chain_info(self.h, C.byref(o), C.byref(a), C.byref(b)))
        return o.value, a.value, b.value

    def cycleInfo(self):
        """(launch that found the pose of an earlier round again -- 0: none --, the repeat's period, launches of the last
        solve that returned at once): the five ints behind the pose of vo_picp_pose_dev_ptr (include/vo_hip.h); synchronises"""
        p = C.c_void_p()
        _chk(self.lib.vo_picp_pose_dev_ptr(self.h, C.byref(p)))
        blk = np.zeros(5, np.int32)
        self.ctx.d2h(blk, p.value + 16 * 4)
        return int(blk[2]), int(blk[3]), int(blk[4])

    def tailInfo(self):
        """(the last solve ran its rounds behind round M as one tail launch, real rounds that ran inside that launch, a
        workgroup of it gave up at the grid barrier): three of the four ints behind the 64 x 12 floats of pose history that
        follow the cycle report (csrc/vo_internal.h, PicpTail); synchronises.  Reads the words in place: an aborted solve
        makes the getters fail, not this accessor."""
        p = C.c_void_p()
        _chk(self.lib.vo_picp_pose_dev_ptr(self.h, C.byref(p)))
        blk = np.zeros(4, np.int32)
        self.ctx.d2h(blk, p.value + 16 * 4 + 5 * 4 + 64 * 12 * 4)
        return bool(blk[0]), int(blk[1]), bool(blk[2])

    TAIL_CLOSE = ("none", "ring", "recomputed", "looped", "early")

    def tailCloseInfo(self):
        """(how the last solve was closed, the M it ran with): "none" and 0 where the solve had no tail launch and a finishing
        launch closed it; "ring": the tail launch's workgroup 0 closed it from the partial rows an earlier launch had left in
        the ring; "recomputed": all workgroups linearised the last round again first; "looped": the launch ran the last round
        at the end of its loop; "early": the launch, in its early form (VO_PICP_TAIL_EARLY, or the handle's own choice),
        found the repeat in the round that computed the repeating pose and closed the solve there.  M: rounds 1 .. M had launches of their own.  The two words lie behind the tail words and the
        two tally counts (csrc/vo_internal.h, PicpTailClose); synchronises; reads in place like tailInfo()."""
        p = C.c_void_p()
        _chk(self.lib.vo_picp_pose_dev_ptr(self.h, C.byref(p)))
        blk = np.zeros(8, np.int32)
        self.ctx.d2h(blk, p.value + 16 * 4 + 5 * 4 + 64 * 12 * 4)
        if not blk[0]:
            return self.TAIL_CLOSE[0], 0
        return self.TAIL_CLOSE[int(blk[6])], int(blk[7])

    def setCorrespondences(self, correspondences):
        p = _i32pairs(correspondences)
        _chk(self.lib.vo_picp_set_correspondences(self.h, _ptr(p), C.c_int(len(p))))

    def rounds(self, keep_outliers=False, n_iters=1):
        _chk(self.lib.vo_picp_rounds(self.h, C.c_int(int(keep_outliers)), C.c_int(n_iters)))

    def oneRound(self, correspondences, keep_outliers=False) -> bool:
        """picp_solver.cpp:98-112; pairs are (measurement index, world index)."""
        p = self._pairs(correspondences)
        _chk(self.lib.vo_picp_one_round(self.h, _ptr(p), C.c_int(len(p)), C.c_int(int(keep_outliers))))
        return True   # min_num_inliers is 0 in the reference: oneRound cannot return false

    def solve(self, correspondences, keep_outliers=False, n_iters=1):
        p = self._pairs(correspondences)
        _chk(self.lib.vo_picp_solve(self.h, _ptr(p), C.c_int(len(p)), C.c_int(int(keep_outliers)), C.c_int(n_iters)))

    def camera(self) -> Camera:
        T = np.zeros(16, dtype=np.float32)
        _chk(self.lib.vo_picp_get_pose(self.h, _ptr(T)))
        cam = self._cam.copy()
        cam.setWorldInCameraPose(T.reshape(4, 4).T)
        return cam

    def _stats(self):
        ci, co, ni = C.c_float(), C.c_float(), C.c_int()
        _chk(self.lib.vo_picp_get_stats(self.h, C.byref(ci), C.byref(co), C.byref(ni)))
        return ci.value, co.value, ni.value

    def chiInliers(self): return self._stats()[0]
    def chiOutliers(self): return self._stats()[1]
    def numInliers(self): return self._stats()[2]

    def system(self):
        """(H with damping, b) of the last round, as the reference leaves _H/_b."""
        H = np.zeros(36, dtype=np.float32)
        b = np.zeros(6, dtype=np.float32)
        _chk(self.lib.vo_picp_get_system(self.h, _ptr(H), _ptr(b)))
        return H.reshape(6, 6).T.copy(), b


class Map:
    """PointCloudVector<3> `map` of vo_complete on the GPU (vo_map_*): update() is PointCloud.h:52-66, the history
    isometry vo_complete.cpp:145-147,175-176."""

    def __init__(self, ctx: Context | None = None, capacity: int = 0):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        h = C.c_void_p()
        _chk(self.lib.vo_map_create(self.ctx.h, C.c_int(capacity), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.vo_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        _chk(self.lib.vo_map_clear(self.h))

    def update(self, points, appearances, T=None):
        """map.update(T * cloud) from host arrays"""
        p = _f32(points, (-1, 3))
        a = _f32(appearances, (-1, 10))
        assert len(p) == len(a)
        _chk(self.lib.vo_map_update(self.h, _ptr(p), _ptr(a), C.c_int(len(p)), _ptr(_colmajor(T, 4)) if T is not None else None))

    def update_dev(self, d_xyz, d_app, n_max, d_n=None, d_T16=None):
        _chk(self.lib.vo_map_update_dev(self.h, C.c_void_p(d_xyz), C.c_void_p(d_app), C.c_int(n_max),
                                        C.c_void_p(d_n) if d_n else None, C.c_void_p(d_T16) if d_T16 else None))

    def history_reset_dev(self, d_X16):
        _chk(self.lib.vo_map_history_reset_dev(self.h, C.c_void_p(d_X16)))

    def history_step_dev(self, d_X16):
        _chk(self.lib.vo_map_history_step_dev(self.h, C.c_void_p(d_X16)))

    @property
    def history_dev(self):
        p = C.c_void_p()
        _chk(self.lib.vo_map_history_dev_ptr(self.h, C.byref(p)))
        return p.value

    def history(self):
        T = np.zeros(16, np.float32)
        _chk(self.lib.vo_map_get_history(self.h, _ptr(T)))
        return T.reshape(4, 4).T.copy()

    def transform(self, T):
        _chk(self.lib.vo_map_transform(self.h, _ptr(_colmajor(T, 4))))

    def __len__(self):
        n = C.c_int()
        _chk(self.lib.vo_map_size(self.h, C.byref(n)))
        return n.value

    def read(self):
        """(points (n, 3), appearances (n, 10)) in entry order"""
        n = len(self)
        p = np.zeros((max(n, 1), 3), np.float32)
        a = np.zeros((max(n, 1), 10), np.float32)
        m = C.c_int()
        _chk(self.lib.vo_map_read(self.h, _ptr(p), _ptr(a), C.c_int(n), C.byref(m)))
        return p[:n].copy(), a[:n].copy()

    # ---- reading the map by appearance (vo_map_lookup*, vo_map_localise*) ----
    def lookup(self, appearances, want_points=False):
        """vo_map_lookup: which entry would update() have found for every row?  Returns (pairs (k, 2) = (query index,
        entry index) in query order, entries (n,) = the entry per query or -1) and, with want_points, the hits' points (k, 3)."""
        a = _f32(appearances, (-1, 10))
        n = len(a)
        pairs = np.zeros((max(n, 1), 2), np.int32)
        ent = np.full(max(n, 1), -1, np.int32)
        xyz = np.zeros((max(n, 1), 3), np.float32)
        k = C.c_int()
        _chk(self.lib.vo_map_lookup(self.h, _ptr(a), C.c_int(n), _ptr(pairs), C.byref(k), _ptr(xyz) if want_points else None, _ptr(ent)))
        out = (pairs[: k.value].copy(), ent[:n].copy())
        return out + (xyz[: k.value].copy(),) if want_points else out

    def lookup_dev(self, d_app, n_max, d_n, d_pairs, d_n_out, d_xyz=None, d_local_pairs=None, d_entries=None):
        """vo_map_lookup_dev on device pointers (ints; d_n and the last three may be None): enqueues and returns"""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.vo_map_lookup_dev(self.h, v(d_app), C.c_int(n_max), v(d_n), v(d_pairs), v(d_n_out), v(d_xyz), v(d_local_pairs),
                                        v(d_entries)))

    def lookup_batch_dev(self, n_frames, d_app, app_stride, n_max, d_n, d_pairs, d_n_out, d_xyz=None, d_local_pairs=None,
                         d_entries=None):
        """vo_map_lookup_batch_dev: n_frames frames against this map in one call (app_stride in rows)"""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.vo_map_lookup_batch_dev(self.h, C.c_int(n_frames), v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n),
                                              v(d_pairs), v(d_n_out), v(d_xyz), v(d_local_pairs), v(d_entries)))

    @staticmethod
    def _ransac(threshold_px, n_hypotheses, seed):
        return RansacParams(int(n_hypotheses), float(threshold_px), int(seed) & 0xFFFFFFFFFFFFFFFF)

    def localise(self, camera: Camera, pixels, appearances, threshold_px=2.0, n_hypotheses=64, seed=0, kernel_threshold=10000.0,
                 n_iters=50, min_inliers=6, T0=None):
        """vo_map_localise: the camera's pose in the map (4x4, p_cam = T p_map) from one frame's pixels (n, 2) and appearances
        (n, 10): lookup -> P3P RANSAC (n_hypotheses == 0: none, T0 is the start) -> n_iters PICP rounds.  Returns (T, stats
        dict); T is T0 (or the identity) unless stats["status"] == 0 (MAP_LOCALISE_STATUS names the others)."""
        uv = _f32(pixels, (-1, 2))
        a = _f32(appearances, (-1, 10))
        assert len(uv) == len(a)
        T = np.zeros(16, np.float32)
        st = MapLocaliseStats()
        prm = self._ransac(threshold_px, n_hypotheses, seed)
        _chk(self.lib.vo_map_localise(self.h, C.c_int(camera._rows), C.c_int(camera._cols), C.c_int(camera._z_near), C.c_int(camera._z_far),
                                      _ptr(_colmajor(camera._K, 3)), _ptr(uv), _ptr(a), C.c_int(len(uv)), C.byref(prm),
                                      C.c_float(kernel_threshold), C.c_int(n_iters), C.c_int(min_inliers),
                                      _ptr(_colmajor(T0, 4)) if T0 is not None else None, _ptr(T), C.byref(st)))
        return T.reshape(4, 4).T.copy(), st.as_dict()

    def localise_dev(self, camera: Camera, d_uv, d_app, n_max, d_n, params: "RansacParams", kernel_threshold, n_iters, min_inliers,
                     d_T0, d_T16_out, d_stats):
        """vo_map_localise_dev on device pointers (ints; d_n and d_T0 may be None): enqueues and returns.  d_T16_out: 16
        floats, d_stats: 32 bytes (MapLocaliseStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.vo_map_localise_dev(self.h, C.c_int(camera._rows), C.c_int(camera._cols), C.c_int(camera._z_near),
                                          C.c_int(camera._z_far), _ptr(_colmajor(camera._K, 3)), v(d_uv), v(d_app), C.c_int(n_max), v(d_n),
                                          C.byref(params), C.c_float(kernel_threshold), C.c_int(n_iters), C.c_int(min_inliers), v(d_T0),
                                          v(d_T16_out), v(d_stats)))

    def localise_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, params: "RansacParams",
                           kernel_threshold, n_iters, min_inliers, d_T0, d_T16_out, d_stats):
        """vo_map_localise_batch_dev on device pointers (strides in pixels / rows)"""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.vo_map_localise_batch_dev(self.h, C.c_int(n_frames), C.c_int(camera._rows), C.c_int(camera._cols),
                                                C.c_int(camera._z_near), C.c_int(camera._z_far), _ptr(_colmajor(camera._K, 3)), v(d_uv),
                                                C.c_size_t(uv_stride), v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n),
                                                C.byref(params), C.c_float(kernel_threshold), C.c_int(n_iters), C.c_int(min_inliers),
                                                v(d_T0), v(d_T16_out), v(d_stats)))

    def localise_batch(self, camera: Camera, frames, threshold_px=2.0, n_hypotheses=64, seed=0, kernel_threshold=10000.0, n_iters=50,
                       min_inliers=6, T0=None):
        """vo_map_localise_batch_dev for a list of host frames (pixels (n, 2), appearances (n, 10)) of any sizes: padded to a
        common n_max, uploaded, localised in ONE call.  T0: one 4x4 per frame, or None.  Returns a list of (T, stats dict)."""
        F = len(frames)
        if F == 0:
            return []
        ctx = self.ctx
        n = np.array([len(_f32(a, (-1, 10))) for _, a in frames], np.int32)
        cap = max(int(n.max()), 1)
        uv = np.zeros((F, cap, 2), np.float32)
        app = np.zeros((F, cap, 10), np.float32)
        for f, (p, a) in enumerate(frames):
            uv[f, : n[f]] = _f32(p, (-1, 2))
            app[f, : n[f]] = _f32(a, (-1, 10))
        t0 = None if T0 is None else np.stack([_colmajor(T, 4) for T in T0]).astype(np.float32)
        ins = [ctx.to_device(uv), ctx.to_device(app), ctx.to_device(n)] + ([ctx.to_device(t0)] if t0 is not None else [])
        outs = [ctx.alloc(F * 64), ctx.alloc(F * 32)]
        try:
            self.localise_batch_dev(camera, F, ins[0], cap, ins[1], cap, cap, ins[2], self._ransac(threshold_px, n_hypotheses, seed),
                                    kernel_threshold, n_iters, min_inliers, ins[3] if t0 is not None else None, outs[0], outs[1])
            T = np.zeros((F, 16), np.float32); ctx.d2h(T, outs[0])
            st = (MapLocaliseStats * F)()
            raw = np.zeros(F * 32, np.uint8); ctx.d2h(raw, outs[1])
            C.memmove(st, raw.ctypes.data, F * 32)
        finally:
            for d in ins + outs:
                ctx.free(d)
        return [(T[f].reshape(4, 4).T.copy(), st[f].as_dict()) for f in range(F)]


    # ---- structure-only refinement (vo_map_refine*) ----
    def refine_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_T16, params: "MapRefineParams",
                         d_status_out, d_xyz_out, d_stats):
        """vo_map_refine_batch_dev on device pointers (ints; d_n, d_status_out and d_xyz_out may be None; strides in pixels /
        rows): enqueues and returns.  d_stats: 48 bytes (MapRefineStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.vo_map_refine_batch_dev(self.h, C.c_int(n_frames), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride),
                                              v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_T16), C.byref(params),
                                              v(d_status_out), v(d_xyz_out), v(d_stats)))

    def refine(self, camera: Camera, frames, poses, n_rounds=10, min_obs=3, huber_px=0.0, damping=0.0):
        """vo_map_refine: every entry re-estimated, in place, from all the rows of `frames` (a list of (pixels (n, 2),
        appearances (n, 10)) of any sizes, padded here to a common n_max) that see it, the poses (4x4, p_cam = T p_map, one
        per frame) fixed.  Returns (status (size,) int32: MAP_REFINE_STATUS names the codes, stats dict)."""
        F = len(frames)
        if F < 1 or F != len(poses):
            raise ValueError("Map.refine: one pose per frame, at least one frame")
        n = np.array([len(_f32(a, (-1, 10))) for _, a in frames], np.int32)
        cap = int(n.max())
        uv = np.zeros((F, max(cap, 1), 2), np.float32)
        app = np.zeros((F, max(cap, 1), 10), np.float32)
        for f, (p, a) in enumerate(frames):
            uv[f, : n[f]] = _f32(p, (-1, 2))
            app[f, : n[f]] = _f32(a, (-1, 10))
        T = np.stack([_colmajor(X, 4) for X in poses]).astype(np.float32)
        status = np.full(max(len(self), 1), -1, np.int32)
        st = MapRefineStats()
        prm = MapRefineParams(int(n_rounds), int(min_obs), float(huber_px), float(damping))
        _chk(self.lib.vo_map_refine(self.h, C.c_int(F), _ptr(_colmajor(camera._K, 3)), _ptr(uv[:, :cap]) if cap else None,
                                    _ptr(app[:, :cap]) if cap else None, _ptr(n), C.c_int(cap), _ptr(T), C.byref(prm), _ptr(status),
                                    C.byref(st)))
        return status[: st.n_entries].copy(), st.as_dict()

    # ---- motion-only refinement and the alternation of the two halves (vo_map_refine_poses*, vo_map_adjust*) ----
    @staticmethod
    def _window(frames, poses, fixed):
        """host frames of any sizes padded to a common n_max: (F, cap, uv, app, n, T (F, 16) column-major, mask or None)"""
        F = len(frames)
        if F < 1 or F != len(poses) or (fixed is not None and len(fixed) != F):
            raise ValueError("one pose (and one mask byte) per frame, at least one frame")
        n = np.array([len(_f32(a, (-1, 10))) for _, a in frames], np.int32)
        cap = int(n.max())
        uv = np.zeros((F, max(cap, 1), 2), np.float32)
        app = np.zeros((F, max(cap, 1), 10), np.float32)
        for f, (p, a) in enumerate(frames):
            uv[f, : n[f]] = _f32(p, (-1, 2))
            app[f, : n[f]] = _f32(a, (-1, 10))
        T = np.ascontiguousarray(np.stack([_colmajor(X, 4) for X in poses]).astype(np.float32))
        mask = None if fixed is None else np.ascontiguousarray(np.asarray(fixed).astype(bool).astype(np.uint8))
        return F, cap, uv, app, n, T, mask

    def refine_poses_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_T16_in, d_fixed,
                               params: "MapPoseRefineParams", d_T16_out, d_status_out, d_H_out, d_stats):
        """vo_map_refine_poses_batch_dev on device pointers (ints; d_n, d_fixed, d_status_out and d_H_out may be None; d_T16_out
        may be d_T16_in; strides in pixels / rows): enqueues and returns.  d_stats: 48 bytes (MapPoseRefineStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.vo_map_refine_poses_batch_dev(self.h, C.c_int(n_frames), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride),
                                                    v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_T16_in), v(d_fixed),
                                                    C.byref(params), v(d_T16_out), v(d_status_out), v(d_H_out), v(d_stats)))

    def refine_poses(self, camera: Camera, frames, poses, fixed=None, n_rounds=10, min_obs=3, huber_px=0.0, damping=0.0, want_H=False):
        """vo_map_refine_poses: every frame's pose (4x4, p_cam = T p_map) re-estimated from all its rows that hit an entry, the
        map fixed; `fixed` (one truth value per frame, or None) holds frames.  Returns (poses (F, 4, 4) float32, status (F,)
        int32: MAP_POSE_STATUS names the codes, stats dict) and, with want_H, the information matrices (F, 6, 6) float64 (NaN
        for a frame that never solved)."""
        F, cap, uv, app, n, T, mask = self._window(frames, poses, fixed)
        status = np.full(F, -1, np.int32)
        H = np.full((F, 36), np.nan, np.float64)
        st = MapPoseRefineStats()
        prm = MapPoseRefineParams(int(n_rounds), int(min_obs), float(huber_px), float(damping))
        _chk(self.lib.vo_map_refine_poses(self.h, C.c_int(F), _ptr(_colmajor(camera._K, 3)), _ptr(uv[:, :cap]) if cap else None,
                                          _ptr(app[:, :cap]) if cap else None, _ptr(n), C.c_int(cap), _ptr(T),
                                          _ptr(mask) if mask is not None else None, C.byref(prm), _ptr(status),
                                          _ptr(H) if want_H else None, C.byref(st)))
        out = (T.reshape(F, 4, 4).transpose(0, 2, 1).copy(), status, st.as_dict())
        return out + (H.reshape(F, 6, 6),) if want_H else out

    def adjust_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_T16, d_fixed,
                         params: "MapAdjustParams", d_pose_status_out, d_point_status_out, d_stats):
        """vo_map_adjust_batch_dev on device pointers: d_T16 and the map in place; d_stats: n_sweeps x 96 bytes (MapAdjustStats)"""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.vo_map_adjust_batch_dev(self.h, C.c_int(n_frames), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride),
                                              v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_T16), v(d_fixed),
                                              C.byref(params), v(d_pose_status_out), v(d_point_status_out), v(d_stats)))

    def adjust(self, camera: Camera, frames, poses, fixed=None, n_sweeps=6, pose_rounds=2, point_rounds=2, min_obs_pose=3,
               min_obs_point=3, huber_px=0.0, damping=0.0):
        """vo_map_adjust: n_sweeps times the pose half (refine_poses, in place on the poses) and then the point half (refine, in
        place on the map).  Hold the gauge with `fixed`: with no frame held the solution drifts.  Returns (poses (F, 4, 4)
        float32, pose status (F,), point status (size,), [per sweep dict(poses=stats dict, points=stats dict)])."""
        F, cap, uv, app, n, T, mask = self._window(frames, poses, fixed)
        pose_status = np.full(F, -1, np.int32)
        point_status = np.full(max(len(self), 1), -1, np.int32)
        st = (MapAdjustStats * int(n_sweeps))() if n_sweeps >= 1 else (MapAdjustStats * 1)()
        prm = MapAdjustParams(int(n_sweeps), int(pose_rounds), int(point_rounds), int(min_obs_pose), int(min_obs_point), float(huber_px),
                              float(damping))
        _chk(self.lib.vo_map_adjust(self.h, C.c_int(F), _ptr(_colmajor(camera._K, 3)), _ptr(uv[:, :cap]) if cap else None,
                                    _ptr(app[:, :cap]) if cap else None, _ptr(n), C.c_int(cap), _ptr(T),
                                    _ptr(mask) if mask is not None else None, C.byref(prm), _ptr(pose_status), _ptr(point_status), st))
        sweeps = [dict(poses=s.poses.as_dict(), points=s.points.as_dict()) for s in st]
        return T.reshape(F, 4, 4).transpose(0, 2, 1).copy(), pose_status, point_status[: st[0].points.n_entries].copy(), sweeps

    # ---- joint adjustment by matrix-free Schur PCG (vox_map_bundle*, include/vo_map_bundle.h) ----
    def bundle_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_T16, d_fixed,
                         params: "MapBundleParams", d_pose_status_out, d_point_status_out, d_rounds_out, d_stats):
        """vox_map_bundle_batch_dev on device pointers: d_T16 and the map in place; d_rounds_out: n_rounds x 40 bytes
        (MapBundleRound) or None; d_stats: 48 bytes (MapBundleStats)"""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.vox_map_bundle_batch_dev(self.h, C.c_int(n_frames), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride),
                                               v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_T16), v(d_fixed),
                                               C.byref(params), v(d_pose_status_out), v(d_point_status_out), v(d_rounds_out), v(d_stats)))

    def bundle(self, camera: Camera, frames, poses, fixed=None, n_rounds=3, n_cg=64, cg_tol=1e-8, lambda0=1e-4, min_obs_pose=3,
               min_obs_point=3, huber_px=0.0):
        """vox_map_bundle: the poses of the free frames and the points of the free landmarks adjusted jointly, in place on the
        map, by n_rounds Levenberg-Marquardt rounds whose reduced camera system is solved by at most n_cg PCG iterations.  Hold
        the gauge with `fixed`.  Returns (poses (F, 4, 4) float32, pose status (F,), point status (size,), [per round dict],
        stats dict: MAP_BUNDLE_STATUS names stats["status"])."""
        F, cap, uv, app, n, T, mask = self._window(frames, poses, fixed)
        pose_status = np.full(F, -1, np.int32)
        point_status = np.full(max(len(self), 1), -1, np.int32)
        rounds = (MapBundleRound * max(int(n_rounds), 1))()
        st = MapBundleStats()
        prm = MapBundleParams(int(n_rounds), int(n_cg), float(cg_tol), float(lambda0), int(min_obs_pose), int(min_obs_point), float(huber_px))
        _chk(self.lib.vox_map_bundle(self.h, C.c_int(F), _ptr(_colmajor(camera._K, 3)), _ptr(uv[:, :cap]) if cap else None,
                                     _ptr(app[:, :cap]) if cap else None, _ptr(n), C.c_int(cap), _ptr(T),
                                     _ptr(mask) if mask is not None else None, C.byref(prm), _ptr(pose_status), _ptr(point_status), rounds,
                                     C.byref(st)))
        return (T.reshape(F, 4, 4).transpose(0, 2, 1).copy(), pose_status, point_status[: st.n_entries].copy(),
                [rounds[k].as_dict() for k in range(max(int(n_rounds), 0))], st.as_dict())


    # ---- culling of landmarks (voe_map_cull*, include/vo_map_cull.h) ----
    def cull_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_T16, params: "MapCullParams",
                       d_verdict_out, d_remap_out, d_entry_out, d_stats):
        """voe_map_cull_batch_dev on device pointers (ints; d_n and the three outputs may be None; strides in pixels / rows):
        enqueues and returns.  d_entry_out: size x 48 bytes (MapCullEntry); d_stats: 48 bytes (MapCullStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_cull_batch_dev(self.h, C.c_int(n_frames), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride),
                                             v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_T16), C.byref(params),
                                             v(d_verdict_out), v(d_remap_out), v(d_entry_out), v(d_stats)))

    def cull(self, camera: Camera, frames, poses, min_obs=3, min_frames=2, max_rms_px=2.0, max_err_px=0.0, min_parallax_deg=0.0,
             drop_unseen=False, dry_run=False):
        """voe_map_cull: every entry judged from all the rows of `frames` (as in refine) that see it, the poses (4x4,
        p_cam = T p_map) given; the entries that fail are taken out of the map, the survivors keep their order.  Returns
        dict(verdict (old size,) int32: MAP_CULL_VERDICT names the codes, remap (old size,) int32: the new index or -1,
        entries: a structured array of MapCullEntry records, stats dict: MAP_CULL_STATUS names stats["status"])."""
        F, cap, uv, app, n, T, _ = self._window(frames, poses, None)
        size = max(len(self), 1)
        verdict = np.full(size, -1, np.int32)
        remap = np.full(size, -2, np.int32)
        entries = np.zeros(size, MAP_CULL_ENTRY_DTYPE)
        st = MapCullStats()
        prm = MapCullParams(int(min_obs), int(min_frames), float(max_rms_px), float(max_err_px), float(min_parallax_deg), int(bool(drop_unseen)),
                            int(bool(dry_run)))
        _chk(self.lib.voe_map_cull(self.h, C.c_int(F), _ptr(_colmajor(camera._K, 3)), _ptr(uv[:, :cap]) if cap else None,
                                   _ptr(app[:, :cap]) if cap else None, _ptr(n), C.c_int(cap), _ptr(T), C.byref(prm), _ptr(verdict),
                                   _ptr(remap), C.c_void_p(entries.ctypes.data), C.byref(st)))
        k = st.n_before
        return dict(verdict=verdict[:k].copy(), remap=remap[:k].copy(), entries=entries[:k].copy(), stats=st.as_dict())


    # ---- landmarks added from the frames' unmapped tracks (voe_map_grow*, include/vo_map_grow.h) ----
    def grow_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_T16, params: "MapGrowParams",
                       d_row_out, d_track_out, track_cap, d_stats):
        """voe_map_grow_batch_dev on device pointers (ints; d_n and the two outputs may be None; strides in pixels / rows):
        enqueues and returns.  d_row_out: n_frames x n_max int32; d_track_out: track_cap x 80 bytes (MapGrowTrack); d_stats: 96
        bytes (MapGrowStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_grow_batch_dev(self.h, C.c_int(n_frames), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride),
                                             v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_T16), C.byref(params),
                                             v(d_row_out), v(d_track_out), C.c_int(track_cap), v(d_stats)))

    def grow(self, camera: Camera, frames, poses, n_rounds=5, min_obs=3, min_frames=3, huber_px=0.0, damping=0.0, max_rms_px=2.0,
             max_err_px=0.0, min_parallax_deg=2.0, max_added=0, dry_run=False, track_cap=None):
        """voe_map_grow: the rows of `frames` (as in refine) that find no entry are grouped into tracks by equal appearance, every
        track is triangulated from all its rows at the poses (4x4, p_cam = T p_map) given, refined and judged by the cull's
        tests; the tracks that pass are appended to the map.  Returns dict(rows (F, n_max) int32: the entry every row is found
        at afterwards, -1 for a dead or NaN row, -2 - t for an open row whose track t was not added; tracks: a structured array
        of MapGrowTrack records (MAP_GROW_VERDICT names the codes; track_cap: room for that many, default one per row); stats
        dict: MAP_GROW_STATUS names stats["status"])."""
        F, cap, uv, app, n, T, _ = self._window(frames, poses, None)
        rows = np.full((F, max(cap, 1)), -9, np.int32)
        track_cap = max(F * cap, 1) if track_cap is None else int(track_cap)
        tracks = np.zeros(max(track_cap, 1), MAP_GROW_TRACK_DTYPE)
        st = MapGrowStats()
        prm = MapGrowParams(int(n_rounds), int(min_obs), int(min_frames), float(huber_px), float(damping), float(max_rms_px), float(max_err_px),
                            float(min_parallax_deg), int(max_added), int(bool(dry_run)))
        _chk(self.lib.voe_map_grow(self.h, C.c_int(F), _ptr(_colmajor(camera._K, 3)), _ptr(uv[:, :cap]) if cap else None,
                                   _ptr(app[:, :cap]) if cap else None, _ptr(n), C.c_int(cap), _ptr(T), C.byref(prm),
                                   _ptr(rows) if cap else None, C.c_void_p(tracks.ctypes.data) if track_cap else None, C.c_int(track_cap),
                                   C.byref(st)))
        return dict(rows=rows[:, :cap].copy(), tracks=tracks[: min(st.n_tracks, track_cap)].copy(), stats=st.as_dict())

    # ---- two maps: alignment by 3-point similarity RANSAC and the merge (voe_map_align*, voe_map_merge*, include/vo_map_align.h) ----
    def size_bound(self):
        """voe_map_size_bound: the host's bound of the size (what sizes the arrays of align_dev / merge_dev); no device work"""
        n = C.c_int()
        _chk(self.lib.voe_map_size_bound(self.h, C.byref(n)))
        return n.value

    def align_dev(self, src: "Map", params: "MapAlignParams", d_S16_out, d_pairs_out, d_n_matches, d_inlier_mask, d_hypothesis_counts,
                  d_stats):
        """voe_map_align_dev on device pointers (ints; the mask and the counts may be None): this map is dst.  Enqueues and
        returns.  d_pairs_out: src.size_bound() x 8 bytes; d_stats: 48 bytes (MapAlignStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_align_dev(self.h, src.h, C.byref(params), v(d_S16_out), v(d_pairs_out), v(d_n_matches), v(d_inlier_mask),
                                        v(d_hypothesis_counts), v(d_stats)))

    def align(self, src: "Map", threshold, n_hypotheses=64, seed=0, with_scale=True, n_refits=1, min_inliers=3, want_counts=False):
        """voe_map_align: the similarity S (4x4, p_self ~ S p_src) between `src` and this map from the landmarks they share, by
        3-point RANSAC and n_refits Umeyama refits over the inliers.  Returns dict(S (4, 4) float32, pairs (k, 2) = (src entry,
        entry of this map), mask (k,) bool: the inliers, stats dict: MAP_ALIGN_STATUS names stats["status"]) and, with
        want_counts, counts (n_hypotheses,) int32.  S is the identity unless the status is OK."""
        n = max(len(src), 1)
        S = np.zeros(16, np.float32)
        pairs = np.zeros((n, 2), np.int32)
        mask = np.zeros(n, np.uint8)
        counts = np.zeros(int(n_hypotheses), np.int32)
        k = C.c_int()
        st = MapAlignStats()
        prm = MapAlignParams(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_hypotheses), int(bool(with_scale)), int(n_refits), int(min_inliers),
                             float(threshold), 0)
        _chk(self.lib.voe_map_align(self.h, src.h, C.byref(prm), _ptr(S), _ptr(pairs), C.byref(k), _ptr(mask),
                                    _ptr(counts) if want_counts else None, C.byref(st)))
        out = dict(S=S.reshape(4, 4).T.copy(), pairs=pairs[: k.value].copy(), mask=mask[: k.value].astype(bool), stats=st.as_dict())
        if want_counts:
            out["counts"] = counts
        return out

    def merge_dev(self, src: "Map", d_S16, policy, d_remap_out, d_stats):
        """voe_map_merge_dev on device pointers (ints; d_S16 and d_remap_out may be None): this map is dst.  d_stats: 16 bytes"""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_merge_dev(self.h, src.h, v(d_S16), C.c_int(int(policy)), v(d_remap_out), v(d_stats)))

    def merge(self, src: "Map", S=None, policy=0):
        """voe_map_merge: src's entries, moved by S (4x4 or None), into this map.  policy: MAP_MERGE_TAKE_SRC (a shared landmark
        takes src's point, as update does) or MAP_MERGE_KEEP_DST (only the entries this map does not hold are appended).
        Returns (remap (len(src),) int32: the entry of this map that src entry i is found at afterwards, or -1; stats dict)."""
        n = max(len(src), 1)
        remap = np.full(n, -2, np.int32)
        st = MapMergeStats()
        _chk(self.lib.voe_map_merge(self.h, src.h, _ptr(_colmajor(S, 4)) if S is not None else None, C.c_int(int(policy)), _ptr(remap),
                                    C.byref(st)))
        return remap[: st.n_src].copy(), st.as_dict()

    # ---- the nearest entry within a radius and the canonical rows (voe_map_nearest*, include/vo_hip.h: NEAREST) ----
    def nearest_batch_dev(self, n_frames, d_app, app_stride, n_max, d_n, params: "MapNearestParams", d_entry_out, d_status_out=None,
                          d_dist2_out=None, d_app_out=None, d_stats=None):
        """voe_map_nearest_batch_dev on device pointers (ints; d_n and every output but d_entry_out may be None; the stride in rows;
        d_app_out may be d_app): enqueues and returns.  d_stats: 32 bytes (MapNearestStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_nearest_batch_dev(self.h, C.c_int(n_frames), v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n),
                                                C.byref(params), v(d_entry_out), v(d_status_out), v(d_dist2_out), v(d_app_out), v(d_stats)))

    def nearest(self, frames, radius, ratio=0.0, unique=False):
        """voe_map_nearest: for every row of every frame ([app] or [(uv, app)]) the nearest entry within `radius` (ratio: the
        second-best test, 0 = off; unique: an entry keeps its closest row per frame), and the rows canonicalised so that the exact
        lookup -- and every map call built on it -- finds that association.  Returns dict(entry, status, dist2: lists of per-frame
        arrays; app: the canonical rows per frame; stats dict).  Status names: MAP_NEAREST_STATUS."""
        apps = [_f32(f[1] if isinstance(f, (tuple, list)) else f, (-1, 10)) for f in frames]
        F = len(apps)
        n = np.array([len(a) for a in apps], np.int32)
        cap = int(n.max()) if F else 0
        app = np.zeros((max(F, 1), max(cap, 1), 10), np.float32)
        for f, a in enumerate(apps):
            app[f, : n[f]] = a
        ent = np.full((max(F, 1), max(cap, 1)), -1, np.int32)
        sta = np.full((max(F, 1), max(cap, 1)), 5, np.int32)
        d2 = np.full((max(F, 1), max(cap, 1)), np.inf, np.float32)
        out = app.copy()
        st = MapNearestStats()
        pr = MapNearestParams(float(radius), float(ratio), int(bool(unique)), 0)
        _chk(self.lib.voe_map_nearest(self.h, C.c_int(F), _ptr(app) if cap else None, _ptr(n), C.c_int(cap), C.byref(pr), _ptr(ent), _ptr(sta),
                                      _ptr(d2), _ptr(out), C.byref(st)))
        cut = lambda a: [a[f, : n[f]].copy() for f in range(F)]
        return dict(entry=cut(ent), status=cut(sta), dist2=cut(d2), app=cut(out), stats=st.as_dict())

    # ---- the nearest entry among those that project near the row's pixel under a pose prior (voe_map_guided*, vo_hip.h: GUIDED) ----
    def guided_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_T16, params: "MapGuidedParams",
                         d_entry_out, d_status_out=None, d_dist2_out=None, d_pix2_out=None, d_app_out=None, d_stats=None):
        """voe_map_guided_batch_dev on device pointers (ints; d_n and every output but d_entry_out may be None; strides in pixels /
        rows; d_T16: n_frames priors of 16 floats, column-major; d_app_out may be d_app): enqueues and returns.  K is the camera's;
        the depth gate is params.z_near / z_far.  d_stats: 48 bytes (MapGuidedStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_guided_batch_dev(self.h, C.c_int(n_frames), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride),
                                               v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_T16), C.byref(params),
                                               v(d_entry_out), v(d_status_out), v(d_dist2_out), v(d_pix2_out), v(d_app_out), v(d_stats)))

    def guided(self, camera: Camera, frames, poses, radius_px, radius, ratio=0.0, unique=False):
        """voe_map_guided: for every row of every frame [(uv, app)] the nearest entry within `radius` among the entries that
        project, under the frame's prior `poses[f]` (4x4, p_cam = T p_map), within `radius_px` of the row's pixel; the camera gives
        K and the depth gate.  Returns dict(entry, status, dist2, pix2: lists of per-frame arrays; app: the canonical rows per
        frame; stats dict).  Status names: MAP_GUIDED_STATUS."""
        F = len(frames)
        assert len(poses) == F
        n = np.array([len(_f32(a, (-1, 10))) for _, a in frames], np.int32)
        cap = int(n.max()) if F else 0
        shape = (max(F, 1), max(cap, 1))
        uv, app = np.zeros(shape + (2,), np.float32), np.zeros(shape + (10,), np.float32)
        for f, (p, a) in enumerate(frames):
            uv[f, : n[f]] = _f32(p, (-1, 2))
            app[f, : n[f]] = _f32(a, (-1, 10))
        T = np.stack([_colmajor(X, 4) for X in poses]).astype(np.float32) if F else np.zeros((1, 16), np.float32)
        ent, sta = np.full(shape, -1, np.int32), np.full(shape, 5, np.int32)
        d2, g2 = np.full(shape, np.inf, np.float32), np.full(shape, np.inf, np.float32)
        out = app.copy()
        st = MapGuidedStats()
        pr = MapGuidedParams(float(radius_px), float(radius), float(ratio), int(bool(unique)), int(camera._z_near), int(camera._z_far))
        _chk(self.lib.voe_map_guided(self.h, C.c_int(F), _ptr(_colmajor(camera._K, 3)), _ptr(uv) if cap else None, _ptr(app) if cap else None,
                                     _ptr(n), C.c_int(cap), _ptr(T), C.byref(pr), _ptr(ent), _ptr(sta), _ptr(d2), _ptr(g2), _ptr(out), C.byref(st)))
        cut = lambda a: [a[f, : n[f]].copy() for f in range(F)]
        return dict(entry=cut(ent), status=cut(sta), dist2=cut(d2), pix2=cut(g2), app=cut(out), stats=st.as_dict())

    # ---- duplicate landmarks fused: mutual nearest in space and appearance (voe_map_fuse*, vo_hip.h: FUSE) ----
    def fuse_batch_dev(self, n_frames, d_app, app_stride, n_max, d_n, params: "MapFuseParams", d_stats, d_partner_out=None, d_dist2_out=None,
                       d_gap2_out=None, d_verdict_out=None, d_remap_out=None, d_app_out=None):
        """voe_map_fuse_batch_dev on device pointers (ints; n_frames == 0 with d_app and d_n None: no frames; every output but
        d_stats may be None; the stride in rows; d_app_out may be d_app): enqueues and returns.  The per-entry outputs hold
        size_bound() words; d_stats: 56 bytes (MapFuseStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_fuse_batch_dev(self.h, C.c_int(n_frames), v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), C.byref(params),
                                             v(d_partner_out), v(d_dist2_out), v(d_gap2_out), v(d_verdict_out), v(d_remap_out), v(d_app_out),
                                             v(d_stats)))

    def fuse(self, radius_xyz, radius, frames=None, position=1, veto_shared_frame=False, dry_run=False):
        """voe_map_fuse: two entries that are each other's nearest in appearance within `radius` among the entries within
        `radius_xyz` in space are one landmark; the higher index is absorbed (position: 0 the survivor keeps its point, 1 the
        midpoint).  frames ([app] or [(uv, app)], or None): with veto_shared_frame a pair seen together in one frame is left
        alone, and the rows that hit an absorbed entry come back with the survivor's bytes.  Returns dict(partner, dist2, gap2,
        verdict, remap: (old size,) arrays; app: the rows per frame, or None; stats dict).  MAP_FUSE_VERDICT names the verdicts,
        MAP_FUSE_STATUS stats["status"]."""
        size = max(len(self), 1)
        partner, verdict, remap = np.full(size, -2, np.int32), np.full(size, -1, np.int32), np.full(size, -2, np.int32)
        d2, g2 = np.full(size, np.nan, np.float32), np.full(size, np.nan, np.float32)
        st = MapFuseStats()
        pr = MapFuseParams(float(radius_xyz), float(radius), int(position), int(bool(veto_shared_frame)), int(bool(dry_run)))
        if frames is None:
            _chk(self.lib.voe_map_fuse(self.h, C.c_int(0), None, None, C.c_int(0), C.byref(pr), _ptr(partner), _ptr(d2), _ptr(g2), _ptr(verdict),
                                       _ptr(remap), None, C.byref(st)))
            out = None
        else:
            apps = [_f32(f[1] if isinstance(f, (tuple, list)) else f, (-1, 10)) for f in frames]
            F = len(apps)
            n = np.array([len(a) for a in apps], np.int32)
            cap = int(n.max()) if F else 0
            app = np.zeros((max(F, 1), max(cap, 1), 10), np.float32)
            for f, a in enumerate(apps):
                app[f, : n[f]] = a
            rows = app.copy()
            _chk(self.lib.voe_map_fuse(self.h, C.c_int(F), _ptr(app) if cap else None, _ptr(n), C.c_int(cap), C.byref(pr), _ptr(partner), _ptr(d2),
                                       _ptr(g2), _ptr(verdict), _ptr(remap), _ptr(rows) if cap else None, C.byref(st)))
            out = [rows[f, : n[f]].copy() for f in range(F)]
        k = st.n_before
        return dict(partner=partner[:k].copy(), dist2=d2[:k].copy(), gap2=g2[:k].copy(), verdict=verdict[:k].copy(), remap=remap[:k].copy(),
                    app=out, stats=st.as_dict())

    # ---- covisibility of frames and the window chosen from it (voe_map_covis*, voe_map_window*, include/vo_map_covis.h) ----
    def words(self):
        """the 32-bit words a bit row needs for this map: enough for size_bound() entries, at least one"""
        return max((self.size_bound() + 31) // 32, 1)

    def covis_batch_dev(self, n_frames, d_app, app_stride, n_max, d_n, n_words, d_bits_out, d_counts_out, d_stats):
        """voe_map_covis_batch_dev on device pointers (ints; d_n and d_counts_out may be None; the stride in rows): enqueues and
        returns.  d_bits_out: n_frames x n_words x 4 bytes; d_counts_out: n_frames x n_frames x 4 bytes; d_stats: 32 bytes."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_covis_batch_dev(self.h, C.c_int(n_frames), v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n),
                                              C.c_int(n_words), v(d_bits_out), v(d_counts_out), v(d_stats)))

    def covisibility(self, frames, want_counts=True, n_words=None):
        """voe_map_covis: which entries every frame sees and how many every two frames share.  frames: [(uv, app)] as in refine,
        or [app].  Returns dict(bits (F, W) uint32: bit e & 31 of word e >> 5 of row f is set when frame f sees entry e, counts
        (F, F) int32 or None, stats dict)."""
        apps = [_f32(f[1] if isinstance(f, (tuple, list)) else f, (-1, 10)) for f in frames]
        F = len(apps)
        n = np.array([len(a) for a in apps], np.int32)
        cap = int(n.max()) if F else 0
        app = np.zeros((max(F, 1), max(cap, 1), 10), np.float32)
        for f, a in enumerate(apps):
            app[f, : n[f]] = a
        W = self.words() if n_words is None else int(n_words)
        bits = np.zeros((max(F, 1), max(W, 1)), np.uint32)
        counts = np.zeros((max(F, 1), max(F, 1)), np.int32) if want_counts else None
        st = MapCovisStats()
        _chk(self.lib.voe_map_covis(self.h, C.c_int(F), _ptr(app[:, :cap]) if cap else None, _ptr(n), C.c_int(cap), C.c_int(W), _ptr(bits),
                                    _ptr(counts) if want_counts else None, C.byref(st)))
        return dict(bits=bits, counts=counts, stats=st.as_dict())

    # ---- a trajectory's correction carried into the map (voe_map_apply_correction*, include/vo_pose_graph.h) ----
    def apply_correction_batch_dev(self, n_frames, d_app, app_stride, n_max, d_n, d_S16_old, d_S16_new, dry_run, d_ref_frame_out, d_stats):
        """voe_map_apply_correction_batch_dev on device pointers (ints; d_n and d_ref_frame_out may be None; the stride in rows):
        enqueues and returns.  d_ref_frame_out: map size x int32; d_stats: 16 bytes (MapApplyStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_apply_correction_batch_dev(self.h, C.c_int(n_frames), None, C.c_size_t(n_max), v(d_app), C.c_size_t(app_stride),
                                                         C.c_int(n_max), v(d_n), v(d_S16_old), v(d_S16_new), C.c_int(int(bool(dry_run))),
                                                         v(d_ref_frame_out), v(d_stats)))

    def apply_correction(self, frames, S_old, S_new, dry_run=False):
        """voe_map_apply_correction: every entry some row of `frames` ([(uv, app)] as in refine, or [app]) sees moves by
        S_new[f]^-1 S_old[f] of its reference frame f -- the frame of its first observation in ascending key -- so that it keeps
        its place in that frame's camera; S_old, S_new: F x 4 x 4 (p_cam = S p_map).  Returns (ref_frame (size,) int32, -1: unseen;
        stats dict: n_entries, n_seen, n_moved).  The rigid poses afterwards are rigid_pose(S_new[f])."""
        apps = [_f32(f[1] if isinstance(f, (tuple, list)) else f, (-1, 10)) for f in frames]
        F = len(apps)
        n = np.array([len(a) for a in apps], np.int32)
        cap = int(n.max()) if F else 0
        app = np.zeros((max(F, 1), max(cap, 1), 10), np.float32)
        for f, a in enumerate(apps):
            app[f, : n[f]] = a
        So = np.ascontiguousarray(np.asarray(S_old, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        Sn = np.ascontiguousarray(np.asarray(S_new, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        assert len(So) == F and len(Sn) == F
        ref = np.full(max(len(self), 1), -2, np.int32)
        st = MapApplyStats()
        _chk(self.lib.voe_map_apply_correction(self.h, C.c_int(F), None, _ptr(app) if cap else None, _ptr(n), C.c_int(cap), _ptr(So), _ptr(Sn),
                                               C.c_int(int(bool(dry_run))), _ptr(ref), C.byref(st)))
        return ref[: st.n_entries].copy(), st.as_dict()

    # ---- loop edges found and measured in the map (voe_map_loops*, include/vo_map_loops.h) ----
    def loops_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_S16, params: "MapLoopsParams",
                        d_edges_out, d_Z16_out, d_weights_out, d_loops_out, d_hist_out, d_ref_frame_out, d_stats):
        """voe_map_loops_batch_dev on device pointers (ints; d_n, d_hist_out and d_ref_frame_out may be None; strides in pixels /
        rows): enqueues and returns.  With L = params.max_loops: d_edges_out L x 2 int32, d_Z16_out L x 16 float32, d_weights_out
        L x 3 float32 -- the three arrays voe_pose_graph_dev takes --, d_loops_out L x 40 bytes (MAP_LOOP_RECORD_DTYPE), d_hist_out
        n_frames x n_frames int32, d_ref_frame_out map size x int32, d_stats 32 bytes (MapLoopsStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_loops_batch_dev(self.h, C.c_int(n_frames), C.c_int(camera._rows), C.c_int(camera._cols), C.c_int(camera._z_near),
                                              C.c_int(camera._z_far), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride), v(d_app),
                                              C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_S16), C.byref(params), v(d_edges_out),
                                              v(d_Z16_out), v(d_weights_out), v(d_loops_out), v(d_hist_out), v(d_ref_frame_out), v(d_stats)))

    def loops_problems_dev(self):
        """voe_map_loops_problems_dev: the device pointers (ints) of what the last loops call on this map left in its workspace:
        dict(world [L][n_max][3] float32, uv [L][n_max][2] float32, pairs [L][n_max][2] int32, n_pairs [L] int32, candidates
        [F][2] int32, inlier_pairs [L][n_max][2] int32, n_inliers [L] int32, T16 [L][16] float32, solver_stats [L][4] float32)"""
        out = (C.c_void_p * 9)()
        _chk(self.lib.voe_map_loops_problems_dev(self.h, C.byref(out)))
        return dict(zip(("world", "uv", "pairs", "n_pairs", "candidates", "inlier_pairs", "n_inliers", "T16", "solver_stats"), (int(o or 0) for o in out)))

    def loops(self, camera: Camera, frames, S, gap=50, ref_window=5, min_shared=12, separation=3, max_loops=8, threshold_px=2.0,
              n_hypotheses=64, seed=0, kernel_threshold=10000.0, n_iters=50, min_inliers=6, w_loop=(1.0, 1.0, 1.0), want_hist=True,
              want_ref_frame=True, n_max=None):
        """voe_map_loops: the loop edges this map shows for `frames` ([(uv, app)] as in refine) with the drifted similarities S
        (F x 4 x 4, p_cam = S p_map).  Frame j's candidate is the i < j - gap whose band -- the entries with a reference frame in
        [i - ref_window, i] -- holds the most entries j sees (at least min_shared); candidates within `separation` frames suppress
        each other; the best max_loops are measured by P3P RANSAC + PICP of frame j against the band of i.  Returns dict(edges
        (L, 2) int32, Z (L, 4, 4) float32, weights (L, 3) float32 -- append them to the odometry edges of pose_graph(): every slot that
        is not OK has weights 0 0 0 and is skipped there --, loops: MAP_LOOP_RECORD_DTYPE records (MAP_LOOP_STATUS names
        "status"), hist (F, F) int32 or None, ref_frame (size,) int32 or None, stats dict).  n_max: the row capacity the frames are
        padded to (default: the longest frame)."""
        F = len(frames)
        n = np.array([len(_f32(a, (-1, 10))) for _, a in frames], np.int32)
        cap = max(int(n.max()) if F else 0, 1) if n_max is None else int(n_max)
        assert F == 0 or int(n.max()) <= cap
        uv = np.zeros((max(F, 1), cap, 2), np.float32)
        app = np.zeros((max(F, 1), cap, 10), np.float32)
        for f, (p, a) in enumerate(frames):
            uv[f, : n[f]] = _f32(p, (-1, 2))
            app[f, : n[f]] = _f32(a, (-1, 10))
        S32 = np.ascontiguousarray(np.asarray(S, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        assert len(S32) == F
        prm = MapLoopsParams(int(gap), int(ref_window), int(min_shared), int(separation), int(max_loops), 0,
                             self._ransac(threshold_px, n_hypotheses, seed), float(kernel_threshold), int(n_iters), int(min_inliers),
                             (C.c_float * 3)(*[float(x) for x in w_loop]), 0)
        L = max(int(max_loops), 1)
        edges, Z, w = np.full((L, 2), -2, np.int32), np.zeros((L, 16), np.float32), np.zeros((L, 3), np.float32)
        rec = np.zeros(L, MAP_LOOP_RECORD_DTYPE)
        hist = np.zeros((max(F, 1), max(F, 1)), np.int32) if want_hist else None
        ref = np.full(max(len(self), 1), -2, np.int32) if want_ref_frame else None
        st = MapLoopsStats()
        _chk(self.lib.voe_map_loops(self.h, C.c_int(F), C.c_int(camera._rows), C.c_int(camera._cols), C.c_int(camera._z_near), C.c_int(camera._z_far),
                                    _ptr(_colmajor(camera._K, 3)), _ptr(uv), _ptr(app), _ptr(n), C.c_int(cap), _ptr(S32), C.byref(prm), _ptr(edges),
                                    _ptr(Z), _ptr(w), _ptr(rec), _ptr(hist) if want_hist else None, _ptr(ref) if want_ref_frame else None,
                                    C.byref(st)))
        return dict(edges=edges, Z=Z.reshape(L, 4, 4).transpose(0, 2, 1).copy(), weights=w, loops=rec, hist=hist,
                    ref_frame=ref[: st.n_entries].copy() if want_ref_frame else None, stats=st.as_dict())

    def window_dev(self, n_frames, n_words, d_bits, d_n, n_max, params: "MapWindowParams", d_role_out, d_n_rows_out, d_fixed_out,
                   d_order_out, d_union_out, d_stats):
        """voe_map_window_dev on device pointers (ints; d_n, d_order_out and d_union_out may be None): enqueues and returns"""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_window_dev(self.h, C.c_int(n_frames), C.c_int(n_words), v(d_bits), v(d_n), C.c_int(n_max), C.byref(params),
                                         v(d_role_out), v(d_n_rows_out), v(d_fixed_out), v(d_order_out), v(d_union_out), v(d_stats)))

    def window(self, bits, query, k_free=8, k_fixed=8, min_shared=15, n_rows=None, n_max=None):
        """voe_map_window: the local window of frame `query` from the bit rows of covisibility().  n_rows: the frames' live rows
        (what n_rows of the result hands on for the window's frames; default: n_max, itself 0 by default, for every frame).
        Returns dict(role (F,) int32: MAP_WINDOW_ROLE names the codes, n_rows (F,) int32 and fixed (F,) uint8: what bundle /
        adjust / cull take over the same frames, order (F,) int32, union (W,) uint32, stats dict: MAP_WINDOW_STATUS names
        stats["status"])."""
        bits = np.ascontiguousarray(np.asarray(bits, np.uint32))
        if bits.ndim != 2:
            raise ValueError("bits: (frames, words)")
        F, W = bits.shape
        n = None if n_rows is None else np.ascontiguousarray(np.asarray(n_rows, np.int32))
        if n is not None and n.shape != (F,):
            raise ValueError("one row count per frame")
        cap = int(n_max) if n_max is not None else (int(n.max()) if n is not None and F else 0)
        role, rows, order = np.full(max(F, 1), -1, np.int32), np.full(max(F, 1), -1, np.int32), np.full(max(F, 1), -2, np.int32)
        fixed, union = np.full(max(F, 1), 255, np.uint8), np.zeros(max(W, 1), np.uint32)
        st = MapWindowStats()
        prm = MapWindowParams(int(query), int(k_free), int(k_fixed), int(min_shared))
        _chk(self.lib.voe_map_window(self.h, C.c_int(F), C.c_int(W), _ptr(bits), _ptr(n) if n is not None else None, C.c_int(cap), C.byref(prm),
                                     _ptr(role), _ptr(rows), _ptr(fixed), _ptr(order), _ptr(union), C.byref(st)))
        return dict(role=role, n_rows=rows, fixed=fixed, order=order, union=union, stats=st.as_dict())

    # ---- keyframes chosen from the bit rows (voe_map_keyframes*, vo_hip.h: KEYFRAMES) ----
    def keyframes_dev(self, n_frames, n_words, d_bits, d_n, n_max, d_flags, params: "MapKeyframesParams", d_verdict_out, d_n_rows_out,
                      d_keep_out, d_step_out, d_order_out, d_seen_out, d_red_out, d_stats):
        """voe_map_keyframes_dev on device pointers (ints; d_n, d_flags and d_order_out may be None): enqueues and returns.  The
        per-frame outputs hold n_frames words (d_keep_out: bytes); d_stats: 32 bytes (MapKeyframesStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_keyframes_dev(self.h, C.c_int(n_frames), C.c_int(n_words), v(d_bits), v(d_n), C.c_int(n_max), v(d_flags),
                                            C.byref(params), v(d_verdict_out), v(d_n_rows_out), v(d_keep_out), v(d_step_out), v(d_order_out),
                                            v(d_seen_out), v(d_red_out), v(d_stats)))

    def keyframes(self, bits, flags=None, min_observers=3, share_permille=900, min_seen=1, max_gap=0, max_dropped=None, n_rows=None,
                  n_max=None):
        """voe_map_keyframes: which frames to keep, from the bit rows of covisibility().  A frame is a candidate when at least
        share_permille / 1000 of the entries it sees are seen by min_observers other kept frames (and it sees min_seen, and with
        max_gap > 0 dropping it leaves no run of more than max_gap missing frames); the best candidate is dropped, the counts
        follow, at most max_dropped times (default: MAP_KEYFRAMES_MAX_STEPS; 0: the analysis alone).  flags (F,) uint8: 0 free,
        1 protected, 2 gone (dropped by an earlier call).  n_rows: the frames' live rows, as in window().  Returns dict(verdict
        (F,) int32: MAP_KEYFRAMES_VERDICT names the codes, n_rows (F,) int32: what refine / bundle / adjust / cull / grow / loops
        take over the same frames, keep (F,) uint8, step (F,) int32, order (F,) int32, seen, red (F,) int32, stats dict)."""
        bits = np.ascontiguousarray(np.asarray(bits, np.uint32))
        if bits.ndim != 2:
            raise ValueError("bits: (frames, words)")
        F, W = bits.shape
        n = None if n_rows is None else np.ascontiguousarray(np.asarray(n_rows, np.int32))
        if n is not None and n.shape != (F,):
            raise ValueError("one row count per frame")
        fl = None if flags is None else np.ascontiguousarray(np.asarray(flags, np.uint8))
        if fl is not None and fl.shape != (F,):
            raise ValueError("one flag per frame")
        cap = int(n_max) if n_max is not None else (int(n.max()) if n is not None and F else 0)
        ints = [np.full(max(F, 1), -7, np.int32) for _ in range(6)]
        keep = np.full(max(F, 1), 255, np.uint8)
        st = MapKeyframesStats()
        prm = MapKeyframesParams(int(min_observers), int(share_permille), int(min_seen), int(max_gap),
                                 MAP_KEYFRAMES_MAX_STEPS if max_dropped is None else int(max_dropped))
        verdict, rows, step, order, seen, red = ints
        _chk(self.lib.voe_map_keyframes(self.h, C.c_int(F), C.c_int(W), _ptr(bits), _ptr(n) if n is not None else None, C.c_int(cap),
                                        _ptr(fl) if fl is not None else None, C.byref(prm), _ptr(verdict), _ptr(rows), _ptr(keep), _ptr(step),
                                        _ptr(order), _ptr(seen), _ptr(red), C.byref(st)))
        return dict(verdict=verdict, n_rows=rows, keep=keep, step=step, order=order, seen=seen, red=red, stats=st.as_dict())

    # ---- single observations pruned (voe_map_prune*, vo_hip.h: PRUNE) ----
    def prune_batch_dev(self, camera: Camera, n_frames, d_uv, uv_stride, d_app, app_stride, n_max, d_n, d_T16, params: "MapPruneParams",
                        d_entry_out, d_status_out, d_sq_out, d_app_out, d_landmark_out, d_frame_out, d_stats):
        """voe_map_prune_batch_dev on device pointers (ints; d_n and every output but d_entry_out and d_stats may be None;
        d_app_out may be d_app; strides in pixels / rows): enqueues and returns.  d_entry_out, d_status_out: n_frames x n_max
        int32; d_sq_out: the same of float64; d_landmark_out: size x 32 bytes (MAP_PRUNE_LANDMARK_DTYPE); d_frame_out: n_frames x
        16 bytes (MAP_PRUNE_FRAME_DTYPE); d_stats: 64 bytes (MapPruneStats)."""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_prune_batch_dev(self.h, C.c_int(n_frames), _ptr(_colmajor(camera._K, 3)), v(d_uv), C.c_size_t(uv_stride),
                                              v(d_app), C.c_size_t(app_stride), C.c_int(n_max), v(d_n), v(d_T16), C.byref(params),
                                              v(d_entry_out), v(d_status_out), v(d_sq_out), v(d_app_out), v(d_landmark_out), v(d_frame_out),
                                              v(d_stats)))

    def prune_dev(self, camera: Camera, d_uv, d_app, n_max, d_n, d_T16, params: "MapPruneParams", d_entry_out, d_status_out, d_sq_out,
                  d_app_out, d_landmark_out, d_frame_out, d_stats):
        """voe_map_prune_dev: prune_batch_dev on one frame"""
        v = lambda d: C.c_void_p(d) if d else None
        _chk(self.lib.voe_map_prune_dev(self.h, _ptr(_colmajor(camera._K, 3)), v(d_uv), v(d_app), C.c_int(n_max), v(d_n), v(d_T16),
                                        C.byref(params), v(d_entry_out), v(d_status_out), v(d_sq_out), v(d_app_out), v(d_landmark_out),
                                        v(d_frame_out), v(d_stats)))

    def prune(self, camera: Camera, frames, poses, max_err_px=0.0, rel_factor=0.0, rel_floor_px=0.0, rel_min_obs=3, unique=True,
              max_share_landmark=1000, max_share_frame=1000):
        """voe_map_prune: every observation of `frames` (as in refine; poses 4x4, p_cam = T p_map) judged on its own: not finite,
        behind the camera, a second row of its frame on one entry (unique), |e| above max_err_px, or |e| above rel_factor times
        its landmark's median (and above rel_floor_px; landmarks with rel_min_obs eligible observations).  A landmark with more
        than max_share_landmark per mille of soft observations, then a frame with more than max_share_frame, is named instead
        and keeps its rows (1000: guard off).  The map is not written.  Returns dict(entry (F, n_max) int32: the entry of a row
        that stays or -1, status (F, n_max) int32: MAP_PRUNE_STATUS names the codes, sq (F, n_max) float64, frames: the list of
        (uv, app) with the pruned rows' first appearance component made NaN -- what the other map calls take --, landmarks and
        frame_records: structured arrays, stats dict)."""
        F, cap, uv, app, n, T, _ = self._window(frames, poses, None)
        rows = max(cap, 1)
        entry = np.full((F, rows), -1, np.int32)
        status = np.full((F, rows), 1, np.int32)
        sq = np.full((F, rows), np.inf, np.float64)
        app_in = np.ascontiguousarray(app[:, :cap]) if cap else None
        app_out = np.zeros((F, rows, 10), np.float32)
        lm = np.zeros(max(len(self), 1), MAP_PRUNE_LANDMARK_DTYPE)
        fr = np.zeros(F, MAP_PRUNE_FRAME_DTYPE)
        st = MapPruneStats()
        prm = MapPruneParams(float(max_err_px), float(rel_factor), float(rel_floor_px), int(rel_min_obs), int(bool(unique)),
                             int(max_share_landmark), int(max_share_frame), 0)
        uv_in = np.ascontiguousarray(uv[:, :cap]) if cap else None
        e2, s2, q2, a2 = (np.ascontiguousarray(x[:, :cap]) for x in (entry, status, sq, app_out))
        _chk(self.lib.voe_map_prune(self.h, C.c_int(F), _ptr(_colmajor(camera._K, 3)), _ptr(uv_in) if cap else None,
                                    _ptr(app_in) if cap else None, _ptr(n), C.c_int(cap), _ptr(T), C.byref(prm), _ptr(e2), _ptr(s2),
                                    _ptr(q2), _ptr(a2), C.c_void_p(lm.ctypes.data), C.c_void_p(fr.ctypes.data), C.byref(st)))
        out_frames = [(np.asarray(frames[f][0], np.float32).reshape(-1, 2).copy(), a2[f, : n[f]].copy()) for f in range(F)]
        return dict(entry=e2, status=s2, sq=q2, frames=out_frames, landmarks=lm[: st.n_entries].copy(), frame_records=fr, stats=st.as_dict())



class MapLocaliseStats(C.Structure):
    """vo_map_localise_stats (include/vo_hip.h)"""
    _fields_ = [("status", C.c_int32), ("n_rows", C.c_int32), ("n_hits", C.c_int32), ("ransac_status", C.c_int32),
                ("ransac_inliers", C.c_int32), ("num_inliers", C.c_int32), ("chi_inliers", C.c_float), ("chi_outliers", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


MAP_LOCALISE_STATUS = ("OK", "FEW_MATCHES", "NO_CONSENSUS", "FEW_INLIERS", "NOT_FINITE")     # VO_MAP_LOCALISE_*


class MapRefineParams(C.Structure):
    """vo_map_refine_params (include/vo_hip.h)"""
    _fields_ = [("n_rounds", C.c_int32), ("min_obs", C.c_int32), ("huber_px", C.c_float), ("damping", C.c_float)]


class MapRefineStats(C.Structure):
    """vo_map_refine_stats (include/vo_hip.h)"""
    _fields_ = [("n_entries", C.c_int32), ("n_obs", C.c_int32), ("by_status", C.c_int32 * 6), ("cost_before", C.c_double),
                ("cost_after", C.c_double)]

    def as_dict(self):
        return dict(n_entries=self.n_entries, n_obs=self.n_obs, by_status=list(self.by_status), cost_before=self.cost_before,
                    cost_after=self.cost_after)


assert C.sizeof(MapRefineParams) == 16 and C.sizeof(MapRefineStats) == 48
MAP_REFINE_STATUS = ("OK", "UNSEEN", "FEW_OBS", "BEHIND", "NOT_FINITE", "COST_ROSE")      # VO_MAP_REFINE_*


class MapPoseRefineParams(C.Structure):
    """vo_map_pose_refine_params (include/vo_map_adjust.h)"""
    _fields_ = [("n_rounds", C.c_int32), ("min_obs", C.c_int32), ("huber_px", C.c_float), ("damping", C.c_float)]


class MapPoseRefineStats(C.Structure):
    """vo_map_pose_refine_stats (include/vo_map_adjust.h)"""
    _fields_ = [("n_frames", C.c_int32), ("n_obs", C.c_int32), ("by_status", C.c_int32 * 6), ("cost_before", C.c_double),
                ("cost_after", C.c_double)]

    def as_dict(self):
        return dict(n_frames=self.n_frames, n_obs=self.n_obs, by_status=list(self.by_status), cost_before=self.cost_before,
                    cost_after=self.cost_after)


class MapAdjustParams(C.Structure):
    """vo_map_adjust_params (include/vo_map_adjust.h)"""
    _fields_ = [("n_sweeps", C.c_int32), ("pose_rounds", C.c_int32), ("point_rounds", C.c_int32), ("min_obs_pose", C.c_int32),
                ("min_obs_point", C.c_int32), ("huber_px", C.c_float), ("damping", C.c_float)]


class MapAdjustStats(C.Structure):
    """vo_map_adjust_stats (include/vo_map_adjust.h): one sweep"""
    _fields_ = [("poses", MapPoseRefineStats), ("points", MapRefineStats)]


assert C.sizeof(MapPoseRefineParams) == 16 and C.sizeof(MapPoseRefineStats) == 48
assert C.sizeof(MapAdjustParams) == 28 and C.sizeof(MapAdjustStats) == 96
MAP_POSE_STATUS = ("OK", "FIXED", "FEW_OBS", "BEHIND", "NOT_FINITE", "COST_ROSE")          # VO_MAP_POSE_*


class MapBundleParams(C.Structure):
    """vox_map_bundle_params (include/vo_map_bundle.h)"""
    _fields_ = [("n_rounds", C.c_int32), ("n_cg", C.c_int32), ("cg_tol", C.c_float), ("lambda0", C.c_float), ("min_obs_pose", C.c_int32),
                ("min_obs_point", C.c_int32), ("huber_px", C.c_float)]


class MapBundleRound(C.Structure):
    """vox_map_bundle_round (include/vo_map_bundle.h): one round"""
    _fields_ = [("cost", C.c_double), ("cost_candidate", C.c_double), ("lambda_", C.c_double), ("residual", C.c_double),
                ("cg_iterations", C.c_int32), ("accepted", C.c_int32)]

    def as_dict(self):
        return dict(cost=self.cost, cost_candidate=self.cost_candidate, lambda_=self.lambda_, residual=self.residual,
                    cg_iterations=self.cg_iterations, accepted=self.accepted)


class MapBundleStats(C.Structure):
    """vox_map_bundle_stats (include/vo_map_bundle.h)"""
    _fields_ = [("status", C.c_int32), ("n_frames", C.c_int32), ("n_entries", C.c_int32), ("n_obs", C.c_int32), ("n_free_frames", C.c_int32),
                ("n_free_points", C.c_int32), ("n_accepted", C.c_int32), ("reserved", C.c_int32), ("cost_before", C.c_double),
                ("cost_after", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


assert C.sizeof(MapBundleParams) == 28 and C.sizeof(MapBundleRound) == 40 and C.sizeof(MapBundleStats) == 48
MAP_BUNDLE_STATUS = ("OK", "NOT_FINITE", "BEHIND", "NOTHING_FREE", "NO_STEP", "COST_ROSE")   # VOX_MAP_BUNDLE_*


class MapCullParams(C.Structure):
    """voe_map_cull_params (include/vo_map_cull.h)"""
    _fields_ = [("min_obs", C.c_int32), ("min_frames", C.c_int32), ("max_rms_px", C.c_float), ("max_err_px", C.c_float),
                ("min_parallax_deg", C.c_float), ("drop_unseen", C.c_int32), ("dry_run", C.c_int32)]


class MapCullEntry(C.Structure):
    """voe_map_cull_entry (include/vo_map_cull.h): one landmark"""
    _fields_ = [("verdict", C.c_int32), ("n_obs", C.c_int32), ("n_frames", C.c_int32), ("reserved", C.c_int32), ("mean_sq_px", C.c_double),
                ("max_sq_px", C.c_double), ("min_z", C.c_double), ("cos_parallax", C.c_double)]


class MapCullStats(C.Structure):
    """voe_map_cull_stats (include/vo_map_cull.h)"""
    _fields_ = [("status", C.c_int32), ("n_before", C.c_int32), ("n_kept", C.c_int32), ("n_obs", C.c_int32), ("by_verdict", C.c_int32 * 8)]

    def as_dict(self):
        return dict(status=self.status, n_before=self.n_before, n_kept=self.n_kept, n_obs=self.n_obs, by_verdict=list(self.by_verdict))


assert C.sizeof(MapCullParams) == 28 and C.sizeof(MapCullEntry) == 48 and C.sizeof(MapCullStats) == 48
MAP_CULL_ENTRY_DTYPE = np.dtype([("verdict", "<i4"), ("n_obs", "<i4"), ("n_frames", "<i4"), ("reserved", "<i4"), ("mean_sq_px", "<f8"),
                                 ("max_sq_px", "<f8"), ("min_z", "<f8"), ("cos_parallax", "<f8")])
assert MAP_CULL_ENTRY_DTYPE.itemsize == 48
MAP_CULL_VERDICT = ("KEPT", "UNSEEN", "FEW_OBS", "FEW_FRAMES", "NOT_FINITE", "BEHIND", "HIGH_ERROR", "LOW_PARALLAX")   # VOE_MAP_CULL_*
MAP_CULL_STATUS = ("OK", "NOTHING_DROPPED")


class MapGrowParams(C.Structure):
    """voe_map_grow_params (include/vo_map_grow.h)"""
    _fields_ = [("n_rounds", C.c_int32), ("min_obs", C.c_int32), ("min_frames", C.c_int32), ("huber_px", C.c_float), ("damping", C.c_float),
                ("max_rms_px", C.c_float), ("max_err_px", C.c_float), ("min_parallax_deg", C.c_float), ("max_added", C.c_int32),
                ("dry_run", C.c_int32)]


class MapGrowTrack(C.Structure):
    """voe_map_grow_track (include/vo_map_grow.h): one track"""
    _fields_ = [("verdict", C.c_int32), ("n_obs", C.c_int32), ("n_frames", C.c_int32), ("entry", C.c_int32), ("first_key", C.c_int32),
                ("refined", C.c_int32), ("reserved", C.c_int32 * 2), ("xyz", C.c_float * 3), ("reserved2", C.c_int32), ("mean_sq_px", C.c_double),
                ("max_sq_px", C.c_double), ("min_z", C.c_double), ("cos_parallax", C.c_double)]


class MapGrowStats(C.Structure):
    """voe_map_grow_stats (include/vo_map_grow.h)"""
    _fields_ = [("status", C.c_int32), ("n_live", C.c_int32), ("n_hits", C.c_int32), ("n_nan", C.c_int32), ("n_open", C.c_int32),
                ("n_tracks", C.c_int32), ("n_added", C.c_int32), ("n_before", C.c_int32), ("n_after", C.c_int32), ("by_verdict", C.c_int32 * 12),
                ("reserved", C.c_int32 * 3)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("by_verdict", "reserved")}
        d["by_verdict"] = list(self.by_verdict)
        return d


assert C.sizeof(MapGrowParams) == 40 and C.sizeof(MapGrowTrack) == 80 and C.sizeof(MapGrowStats) == 96
MAP_GROW_TRACK_DTYPE = np.dtype([("verdict", "<i4"), ("n_obs", "<i4"), ("n_frames", "<i4"), ("entry", "<i4"), ("first_key", "<i4"), ("refined", "<i4"),
                                 ("reserved", "<i4", (2,)), ("xyz", "<f4", (3,)), ("reserved2", "<i4"), ("mean_sq_px", "<f8"), ("max_sq_px", "<f8"),
                                 ("min_z", "<f8"), ("cos_parallax", "<f8")])
assert MAP_GROW_TRACK_DTYPE.itemsize == 80
MAP_GROW_VERDICT = ("ADDED", "FEW_OBS", "FEW_FRAMES", "DEGENERATE", "NOT_FINITE", "BEHIND", "HIGH_ERROR", "LOW_PARALLAX", "NO_ROOM")   # VOE_MAP_GROW_*
MAP_GROW_STATUS = ("OK", "NO_OPEN_ROWS", "NOTHING_ADDED")


class MapAlignParams(C.Structure):
    """voe_map_align_params (include/vo_map_align.h)"""
    _fields_ = [("seed", C.c_uint64), ("n_hypotheses", C.c_int32), ("with_scale", C.c_int32), ("n_refits", C.c_int32),
                ("min_inliers", C.c_int32), ("threshold", C.c_float), ("reserved", C.c_int32)]


class MapAlignStats(C.Structure):
    """voe_map_align_stats (include/vo_map_align.h)"""
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("best_hypothesis", C.c_int32),
                ("best_count", C.c_int32), ("n_valid", C.c_int32), ("refit_kept", C.c_int32), ("reserved", C.c_int32),
                ("scale", C.c_double), ("rms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class MapMergeStats(C.Structure):
    """voe_map_merge_stats (include/vo_map_align.h)"""
    _fields_ = [("n_src", C.c_int32), ("n_shared", C.c_int32), ("n_appended", C.c_int32), ("n_dst_after", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


assert C.sizeof(MapAlignParams) == 32 and C.sizeof(MapAlignStats) == 48 and C.sizeof(MapMergeStats) == 16
MAP_ALIGN_STATUS = ("OK", "FEW_MATCHES", "NO_HYPOTHESIS", "FEW_INLIERS")      # VOE_MAP_ALIGN_*
MAP_ALIGN_MAX_REFITS = 16
MAP_MERGE_TAKE_SRC, MAP_MERGE_KEEP_DST = 0, 1                                   # VOE_MAP_MERGE_*


class MapNearestParams(C.Structure):
    """voe_map_nearest_params (include/vo_hip.h)"""
    _fields_ = [("radius", C.c_float), ("ratio", C.c_float), ("unique", C.c_int32), ("reserved", C.c_int32)]


class MapNearestStats(C.Structure):
    """voe_map_nearest_stats (include/vo_hip.h)"""
    _fields_ = [("n_frames", C.c_int32), ("n_entries", C.c_int32), ("n_live", C.c_int32), ("n_matched", C.c_int32),
                ("n_no_entry", C.c_int32), ("n_ambiguous", C.c_int32), ("n_displaced", C.c_int32), ("n_nan", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


assert C.sizeof(MapNearestParams) == 16 and C.sizeof(MapNearestStats) == 32
MAP_NEAREST_STATUS = ("MATCHED", "NO_ENTRY", "AMBIGUOUS", "DISPLACED", "NAN_ROW", "NOT_LIVE")      # VOE_MAP_NEAREST_*


class MapGuidedParams(C.Structure):
    """voe_map_guided_params (include/vo_hip.h)"""
    _fields_ = [("radius_px", C.c_float), ("radius", C.c_float), ("ratio", C.c_float), ("unique", C.c_int32), ("z_near", C.c_int32),
                ("z_far", C.c_int32), ("reserved", C.c_int32 * 2)]


class MapGuidedStats(C.Structure):
    """voe_map_guided_stats (include/vo_hip.h)"""
    _fields_ = [("n_frames", C.c_int32), ("n_entries", C.c_int32), ("n_live", C.c_int32), ("n_matched", C.c_int32),
                ("n_no_entry", C.c_int32), ("n_ambiguous", C.c_int32), ("n_displaced", C.c_int32), ("n_nan", C.c_int32),
                ("n_in_view", C.c_int64), ("n_gated", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


assert C.sizeof(MapGuidedParams) == 32 and C.sizeof(MapGuidedStats) == 48
MAP_GUIDED_STATUS = MAP_NEAREST_STATUS                                          # VOE_MAP_GUIDED_* = VOE_MAP_NEAREST_*


class MapFuseParams(C.Structure):
    """voe_map_fuse_params (include/vo_hip.h)"""
    _fields_ = [("radius_xyz", C.c_float), ("radius", C.c_float), ("position", C.c_int32), ("veto_shared_frame", C.c_int32),
                ("dry_run", C.c_int32), ("reserved", C.c_int32 * 3)]


class MapFuseStats(C.Structure):
    """voe_map_fuse_stats (include/vo_hip.h)"""
    _fields_ = [("status", C.c_int32), ("n_before", C.c_int32), ("n_after", C.c_int32), ("n_pairs", C.c_int32), ("n_conflicts", C.c_int32),
                ("n_rows_rewritten", C.c_int32), ("by_verdict", C.c_int32 * 6), ("n_gated", C.c_int64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "by_verdict" else getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(MapFuseParams) == 32 and C.sizeof(MapFuseStats) == 56
MAP_FUSE_VERDICT = ("NOT_FINITE", "ALONE", "NOT_MUTUAL", "CONFLICT", "SURVIVOR", "ABSORBED")      # VOE_MAP_FUSE_* (the verdicts)
MAP_FUSE_STATUS = ("OK", "NOTHING_FUSED")                                                        # VOE_MAP_FUSE_* (the call)


class MapKeyframesParams(C.Structure):
    """voe_map_keyframes_params (include/vo_hip.h)"""
    _fields_ = [("min_observers", C.c_int32), ("share_permille", C.c_int32), ("min_seen", C.c_int32), ("max_gap", C.c_int32),
                ("max_dropped", C.c_int32), ("reserved", C.c_int32 * 3)]


class MapKeyframesStats(C.Structure):
    """voe_map_keyframes_stats (include/vo_hip.h)"""
    _fields_ = [("n_frames", C.c_int32), ("n_kept", C.c_int32), ("n_dropped", C.c_int32), ("n_gone", C.c_int32), ("n_protected", C.c_int32),
                ("n_needed", C.c_int32), ("n_blocked", C.c_int32), ("n_empty", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


assert C.sizeof(MapKeyframesParams) == 32 and C.sizeof(MapKeyframesStats) == 32
MAP_KEYFRAMES_VERDICT = ("LEFT", "PROTECTED", "GONE", "DROPPED", "EMPTY", "NEEDED", "GAP")      # VOE_MAP_KEYFRAMES_* (the verdicts)
MAP_KEYFRAMES_FLAG = ("FREE", "PROTECTED", "GONE")                                              # VOE_MAP_KEYFRAMES_* (the flags)
MAP_KEYFRAMES_MAX_STEPS = 1024                                                                  # VOE_MAP_KEYFRAMES_MAX_STEPS


class MapPruneParams(C.Structure):
    """voe_map_prune_params (include/vo_hip.h)"""
    _fields_ = [("max_err_px", C.c_float), ("rel_factor", C.c_float), ("rel_floor_px", C.c_float), ("rel_min_obs", C.c_int32),
                ("unique", C.c_int32), ("max_share_landmark", C.c_int32), ("max_share_frame", C.c_int32), ("reserved", C.c_int32)]


class MapPruneStats(C.Structure):
    """voe_map_prune_stats (include/vo_hip.h)"""
    _fields_ = [("n_frames", C.c_int32), ("n_entries", C.c_int32), ("by_status", C.c_int32 * 10), ("n_landmarks_at_fault", C.c_int32),
                ("n_frames_at_fault", C.c_int32), ("n_obs", C.c_int32), ("n_pruned", C.c_int32)]

    def as_dict(self):
        return dict(n_frames=self.n_frames, n_entries=self.n_entries, by_status=list(self.by_status),
                    n_landmarks_at_fault=self.n_landmarks_at_fault, n_frames_at_fault=self.n_frames_at_fault, n_obs=self.n_obs,
                    n_pruned=self.n_pruned)


assert C.sizeof(MapPruneParams) == 32 and C.sizeof(MapPruneStats) == 64
MAP_PRUNE_LANDMARK_DTYPE = np.dtype([("n_obs", "<i4"), ("n_el", "<i4"), ("n_soft", "<i4"), ("n_pruned", "<i4"), ("at_fault", "<i4"),
                                     ("reserved", "<i4"), ("med_sq", "<f8")])      # voe_map_prune_landmark
MAP_PRUNE_FRAME_DTYPE = np.dtype([("n_obs", "<i4"), ("n_el", "<i4"), ("n_soft", "<i4"), ("at_fault", "<i4")])      # voe_map_prune_frame
assert MAP_PRUNE_LANDMARK_DTYPE.itemsize == 32 and MAP_PRUNE_FRAME_DTYPE.itemsize == 16
MAP_PRUNE_STATUS = ("KEPT", "NOT_LIVE", "MISS", "NOT_FINITE", "BEHIND", "DUPLICATE", "HIGH_ERROR", "RELATIVE", "LANDMARK_AT_FAULT",
                    "FRAME_AT_FAULT")                                                           # VOE_MAP_PRUNE_*


class MapCovisStats(C.Structure):
    """voe_map_covis_stats (include/vo_map_covis.h)"""
    _fields_ = [("n_frames", C.c_int32), ("n_entries", C.c_int32), ("n_hits", C.c_int32), ("n_seen", C.c_int32),
                ("n_entries_seen", C.c_int32), ("reserved", C.c_int32 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class MapWindowParams(C.Structure):
    """voe_map_window_params (include/vo_map_covis.h)"""
    _fields_ = [("query", C.c_int32), ("k_free", C.c_int32), ("k_fixed", C.c_int32), ("min_shared", C.c_int32)]


class MapWindowStats(C.Structure):
    """voe_map_window_stats (include/vo_map_covis.h)"""
    _fields_ = [("status", C.c_int32), ("n_free", C.c_int32), ("n_fixed", C.c_int32), ("n_candidates", C.c_int32),
                ("n_fixed_candidates", C.c_int32), ("n_points", C.c_int32), ("query_seen", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


assert C.sizeof(MapCovisStats) == 32 and C.sizeof(MapWindowParams) == 16 and C.sizeof(MapWindowStats) == 32
MAP_COVIS_MAX_FRAMES = 4096                                                     # VOE_MAP_COVIS_MAX_FRAMES
MAP_WINDOW_ROLE = ("OUTSIDE", "FREE", "FIXED")                                  # VOE_MAP_WINDOW_*
MAP_WINDOW_STATUS = ("OK", "NO_FIXED", "QUERY_UNSEEN")


class PoseGraphParams(C.Structure):
    """voe_pose_graph_params (include/vo_pose_graph.h)"""
    _fields_ = [("n_rounds", C.c_int32), ("n_cg", C.c_int32), ("cg_tol", C.c_float), ("lambda0", C.c_float), ("huber", C.c_float),
                ("with_scale", C.c_int32), ("preconditioner", C.c_int32)]


class PoseGraphRound(C.Structure):
    """voe_pose_graph_round (include/vo_pose_graph.h): one round"""
    _fields_ = [("cost", C.c_double), ("cost_candidate", C.c_double), ("lambda_", C.c_double), ("residual", C.c_double),
                ("cg_iterations", C.c_int32), ("accepted", C.c_int32)]


class PoseGraphStats(C.Structure):
    """voe_pose_graph_stats (include/vo_pose_graph.h)"""
    _fields_ = [("status", C.c_int32), ("n_frames", C.c_int32), ("n_edges", C.c_int32), ("n_live_edges", C.c_int32),
                ("n_free_frames", C.c_int32), ("n_active_frames", C.c_int32), ("n_accepted", C.c_int32), ("reserved", C.c_int32),
                ("cost_before", C.c_double), ("cost_after", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class MapApplyStats(C.Structure):
    """voe_map_apply_stats (include/vo_pose_graph.h)"""
    _fields_ = [("n_entries", C.c_int32), ("n_seen", C.c_int32), ("n_moved", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


assert C.sizeof(MapApplyStats) == 16
assert C.sizeof(PoseGraphParams) == 28 and C.sizeof(PoseGraphRound) == 40 and C.sizeof(PoseGraphStats) == 48
POSE_GRAPH_ROUND_DTYPE = np.dtype([("cost", "<f8"), ("cost_candidate", "<f8"), ("lambda", "<f8"), ("residual", "<f8"),
                                   ("cg_iterations", "<i4"), ("accepted", "<i4")])
assert POSE_GRAPH_ROUND_DTYPE.itemsize == 40
POSE_GRAPH_STATUS = ("OK", "NOT_FINITE", "NOTHING_FREE", "NO_EDGES", "NO_STEP", "COST_ROSE")      # VOE_POSE_GRAPH_*
POSE_GRAPH_PRECONDITIONER = ("CHAIN", "JACOBI")
POSE_GRAPH_EDGE_OK, POSE_GRAPH_EDGE_SKIPPED = 0, 1


def pose_graph_dev(ctx: Context, n_frames, d_S16, n_edges, d_edges, d_Z16, d_weights, d_fixed, params: PoseGraphParams,
                   d_edge_status_out, d_edge_cost_out, d_rounds_out, d_stats):
    """voe_pose_graph_dev on device pointers (ints; d_weights, d_fixed and the three outputs before d_stats may be None): enqueues
    and returns.  d_S16: n_frames x 16 float32, column-major 4x4 each, in place; d_edges: n_edges x 2 int32; d_Z16: n_edges x 16;
    d_edge_cost_out: n_edges doubles; d_rounds_out: n_rounds x 40 bytes (PoseGraphRound); d_stats: 48 bytes (PoseGraphStats)."""
    v = lambda p: C.c_void_p(p or 0)
    _chk(ctx.lib.voe_pose_graph_dev(ctx.h, C.c_int(n_frames), v(d_S16), C.c_int(n_edges), v(d_edges), v(d_Z16), v(d_weights), v(d_fixed),
                                    C.byref(params), v(d_edge_status_out), v(d_edge_cost_out), v(d_rounds_out), v(d_stats)))


def pose_graph(S, edges, Z, weights=None, fixed=None, n_rounds=8, n_cg=8, cg_tol=1e-6, lambda0=1e-4, huber=0.0, with_scale=True,
               preconditioner="CHAIN", ctx: Context | None = None):
    """voe_pose_graph: the similarities S (F x 4 x 4, p_cam = S_f p_world, S = [c R | t]) optimised under the relative-pose edges
    (i, j) with measurements Z (E x 4 x 4, Z_ij ~ S_j S_i^-1), weights (E x 3: translation, rotation, log-scale; None: ones) and
    held frames `fixed` (F booleans or None).  Returns (S_new F x 4 x 4 float32, stats dict, rounds: POSE_GRAPH_ROUND_DTYPE
    records, edge_status int32, edge_cost float64 -- s^2 of every live edge at S_new).  POSE_GRAPH_STATUS names stats["status"]."""
    ctx = ctx or default_context()
    S32 = np.ascontiguousarray(np.asarray(S, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))      # column-major per frame
    F = len(S32)
    e = _i32pairs(edges) if len(edges) else np.zeros((0, 2), np.int32)
    E = len(e)
    Z32 = np.ascontiguousarray(np.asarray(Z, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)) if E else np.zeros((0, 4, 4), np.float32)
    assert len(Z32) == E
    w = _f32(weights, (E, 3)) if weights is not None else None
    fx = np.ascontiguousarray(np.asarray(fixed).astype(np.uint8)) if fixed is not None else None
    assert fx is None or fx.shape == (F,)
    prm = PoseGraphParams(int(n_rounds), int(n_cg), float(cg_tol), float(lambda0), float(huber), int(bool(with_scale)),
                          POSE_GRAPH_PRECONDITIONER.index(preconditioner) if isinstance(preconditioner, str) else int(preconditioner))
    st = PoseGraphStats()
    rounds = np.zeros(max(int(n_rounds), 0), POSE_GRAPH_ROUND_DTYPE)
    es, ec = np.zeros(E, np.int32), np.zeros(E, np.float64)
    nul = C.c_void_p(0)
    _chk(ctx.lib.voe_pose_graph(ctx.h, C.c_int(F), _ptr(S32), C.c_int(E), _ptr(e) if E else nul, _ptr(Z32) if E else nul,
                                _ptr(w) if w is not None and E else nul, _ptr(fx) if fx is not None else nul, C.byref(prm),
                                _ptr(es) if E else nul, _ptr(ec) if E else nul, _ptr(rounds) if len(rounds) else nul, C.byref(st)))
    return S32.transpose(0, 2, 1).copy(), st.as_dict(), rounds, es, ec


def rigid_pose(S):
    """The rigid pose that goes with a similarity S = [c R | t] of the pose graph: [R | t / c], on the host in double.  A map point
    moved by S_new^-1 S_old of its reference frame projects there, under rigid_pose(S_new), where it projected before."""
    S = np.asarray(S, np.float64).reshape(4, 4)
    M = S[:3, :3]
    c = np.cbrt(np.linalg.det(M))
    out = np.eye(4)
    out[:3, :3] = M / c
    out[:3, 3] = S[:3, 3] / c
    return out


def similarity_pose(T, S):
    """The pose of a frame of src's in the map moved by S: T (4x4 rigid, p_cam = T p_src) and S = [c R | t] (4x4, p_dst = S p_src)
    give the rigid T' = [R_T R^T | c t_T - R_T R^T t], on the host in double.  T' p_dst = c T p_src: camera points only scale by c,
    so every projection is unchanged."""
    T, S = np.asarray(T, np.float64).reshape(4, 4), np.asarray(S, np.float64).reshape(4, 4)
    M = S[:3, :3]
    c = np.cbrt(np.linalg.det(M))
    Rn = T[:3, :3] @ (M / c).T
    out = np.eye(4)
    out[:3, :3] = Rn
    out[:3, 3] = c * T[:3, 3] - Rn @ S[:3, 3]
    return out


def triangulate_points(k, X, correspondences, p1_img, p2_img, app2=None, want_pairs=True,
                       ctx: Context | None = None):
    """utils.cpp:51-134.  Returns (triangulated, correspondences_new, appearances)."""
    ctx = ctx or default_context()
    pairs = _i32pairs(correspondences)
    a = _f32(p1_img, (-1, 2))
    b = _f32(p2_img, (-1, 2))
    n = len(pairs)
    xyz = np.zeros((max(n, 1), 3), dtype=np.float32)
    outp = np.zeros((max(n, 1), 2), dtype=np.int32)
    app = _f32(app2, (-1, 10)) if app2 is not None else None
    oapp = np.zeros((max(n, 1), 10), dtype=np.float32) if app is not None else None
    n_out = C.c_int()
    nul = C.c_void_p(0)
    _chk(ctx.lib.vo_triangulate(ctx.h, _ptr(_colmajor(k, 3)), _ptr(_colmajor(X, 4)), _ptr(pairs), C.c_int(n),
                                _ptr(a), C.c_int(len(a)), _ptr(b), C.c_int(len(b)),
                                _ptr(app) if app is not None else nul, _ptr(xyz),
                                _ptr(outp) if want_pairs else nul, _ptr(oapp) if oapp is not None else nul,
                                C.byref(n_out)))
    m = n_out.value
    return xyz[:m].copy(), (outp[:m].copy() if want_pairs else None), (oapp[:m].copy() if oapp is not None else None)


def compute_correspondences_images(appearances1, appearances2, radius=0.1, ctx: Context | None = None):
    """vo_complete.cpp:12-49 -> pairs (ref_idx, curr_idx)."""
    ctx = ctx or default_context()
    a1 = _f32(appearances1, (-1, 10))
    a2 = _f32(appearances2, (-1, 10))
    out = np.zeros((max(min(len(a1), len(a2)), 1), 2), dtype=np.int32)
    n_out = C.c_int()
    _chk(ctx.lib.vo_match_appearances(ctx.h, _ptr(a1), C.c_int(len(a1)), _ptr(a2), C.c_int(len(a2)),
                                      C.c_float(radius), _ptr(out), C.byref(n_out)))
    return out[: n_out.value].copy()


def extract_correspondences_world(correspondences_imgs, correspondences_world, ctx: Context | None = None):
    """vo_complete.cpp:52-66 -> pairs (curr_idx, world_idx)."""
    ctx = ctx or default_context()
    a = _i32pairs(correspondences_imgs)
    b = _i32pairs(correspondences_world)
    out = np.zeros((max(len(a), 1), 2), dtype=np.int32)
    n_out = C.c_int()
    _chk(ctx.lib.vo_join_correspondences(ctx.h, _ptr(a), C.c_int(len(a)), _ptr(b), C.c_int(len(b)), _ptr(out),
                                         C.byref(n_out)))
    return out[: n_out.value].copy()


def transform_points(X, points, ctx: Context | None = None):
    """Isometry3f * point set, PointCloud.h:77-82."""
    ctx = ctx or default_context()
    p = _f32(points, (-1, 3))
    out = np.zeros_like(p)
    _chk(ctx.lib.vo_transform_points(ctx.h, _ptr(_colmajor(X, 4)), _ptr(p), C.c_int(len(p)), _ptr(out)))
    return out


def estimate_transform(k, correspondences, p1_img, p2_img, ctx: Context | None = None):
    """epipolar_utils.cpp:176-213: relative pose (first camera in the frame of the second) from >= 8
    image correspondences; the cheirality vote runs the GPU triangulation kernel."""
    ctx = ctx or default_context()
    pairs = _i32pairs(correspondences)
    a = _f32(p1_img, (-1, 2))
    b = _f32(p2_img, (-1, 2))
    X = np.zeros(16, dtype=np.float32)
    _chk(ctx.lib.vo_estimate_transform(ctx.h, _ptr(_colmajor(k, 3)), _ptr(pairs), C.c_int(len(pairs)), _ptr(a),
                                       C.c_int(len(a)), _ptr(b), C.c_int(len(b)), _ptr(X)))
    return X.reshape(4, 4).T.copy()


class RansacParams(C.Structure):
    """vo_ransac_params (include/vo_hip.h)"""
    _fields_ = [("n_hypotheses", C.c_int), ("threshold_px", C.c_float), ("seed", C.c_uint64)]


class MapLoopsParams(C.Structure):
    """voe_map_loops_params (include/vo_map_loops.h)"""
    _fields_ = [("gap", C.c_int32), ("ref_window", C.c_int32), ("min_shared", C.c_int32), ("separation", C.c_int32), ("max_loops", C.c_int32),
                ("reserved0", C.c_int32), ("ransac", RansacParams), ("kernel_threshold", C.c_float), ("n_iters", C.c_int32),
                ("min_inliers", C.c_int32), ("w_loop", C.c_float * 3), ("reserved1", C.c_int32)]


class MapLoopRecord(C.Structure):
    """voe_map_loop_record (include/vo_map_loops.h): one slot"""
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("c", C.c_int32), ("n_pairs", C.c_int32), ("ransac_status", C.c_int32),
                ("ransac_inliers", C.c_int32), ("num_inliers", C.c_int32), ("status", C.c_int32), ("chi_inliers", C.c_float),
                ("chi_outliers", C.c_float)]


class MapLoopsStats(C.Structure):
    """voe_map_loops_stats (include/vo_map_loops.h)"""
    _fields_ = [("n_frames", C.c_int32), ("n_entries", C.c_int32), ("n_candidates", C.c_int32), ("n_survivors", C.c_int32),
                ("n_slots", C.c_int32), ("n_ok", C.c_int32), ("reserved", C.c_int32 * 2)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


assert C.sizeof(MapLoopsParams) == 72 and C.sizeof(MapLoopRecord) == 40 and C.sizeof(MapLoopsStats) == 32
MAP_LOOP_RECORD_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("c", "<i4"), ("n_pairs", "<i4"), ("ransac_status", "<i4"), ("ransac_inliers", "<i4"),
                                  ("num_inliers", "<i4"), ("status", "<i4"), ("chi_inliers", "<f4"), ("chi_outliers", "<f4")])
assert MAP_LOOP_RECORD_DTYPE.itemsize == 40
MAP_LOOP_STATUS = ("OK", "FEW_MATCHES", "NO_CONSENSUS", "FEW_INLIERS", "NOT_FINITE", "EMPTY")      # VOE_MAP_LOOP_*


def estimate_transform_ransac(k, correspondences, p1_img, p2_img, threshold_px=1.0, n_hypotheses=2048, seed=0,
                              ctx: Context | None = None):
    """estimate_transform behind RANSAC (vo_estimate_transform_ransac): n_hypotheses minimal 8-point fits scored by
    Sampson distance on the GPU, the pose refitted on the best one's inliers -- bit for bit
    estimate_transform(k, correspondences[mask], p1_img, p2_img).  Returns (X, mask (bool, one per pair), n_inliers)."""
    ctx = ctx or default_context()
    pairs = _i32pairs(correspondences)
    a = _f32(p1_img, (-1, 2))
    b = _f32(p2_img, (-1, 2))
    X = np.zeros(16, dtype=np.float32)
    mask = np.zeros(max(len(pairs), 1), dtype=np.uint8)
    n_in = C.c_int()
    prm = RansacParams(int(n_hypotheses), float(threshold_px), int(seed) & 0xFFFFFFFFFFFFFFFF)
    _chk(ctx.lib.vo_estimate_transform_ransac(ctx.h, _ptr(_colmajor(k, 3)), _ptr(pairs), C.c_int(len(pairs)), _ptr(a),
                                              C.c_int(len(a)), _ptr(b), C.c_int(len(b)), C.byref(prm), _ptr(X), _ptr(mask),
                                              C.byref(n_in)))
    return X.reshape(4, 4).T.copy(), mask[: len(pairs)].astype(bool), n_in.value


class EpiRefineParams(C.Structure):
    """vo_epi_refine_params (include/vo_hip.h)"""
    _fields_ = [("n_rounds", C.c_int), ("huber_px", C.c_float)]


class EpiRefineStats(C.Structure):
    """vo_epi_refine_stats (include/vo_hip.h)"""
    _fields_ = [("status", C.c_int32), ("rounds", C.c_int32), ("n_used", C.c_int32), ("n_skipped", C.c_int32),
                ("n_bad", C.c_int32), ("reserved", C.c_int32), ("cost_before", C.c_double), ("cost_after", C.c_double)]

    def as_dict(self):
        return dict(status=self.status, rounds=self.rounds, n_used=self.n_used, n_skipped=self.n_skipped, n_bad=self.n_bad,
                    cost_before=self.cost_before, cost_after=self.cost_after)


EPI_REFINE_STATUS = ("OK", "FEW_PAIRS", "SINGULAR", "COST_ROSE", "BAD_INPUT", "BAD_INDEX")     # VO_EPI_REFINE_*


def refine_transform_dev(ctx: Context, k, d_pairs, n_max, d_n_pairs, d_mask, d_p1, n1, d_p2, n2, X_in, d_X_in, params: EpiRefineParams,
                         d_X_out, d_stats):
    """vo_refine_transform_dev on device pointers (ints; d_n_pairs and d_mask may be None): enqueues and returns.  X_in: a 4x4
    start pose on the host, or None with d_X_in a device pointer to 16 floats (column-major).  d_X_out: 16 floats,
    d_stats: 40 bytes (EpiRefineStats)."""
    v = lambda d: C.c_void_p(d) if d else None
    _chk(ctx.lib.vo_refine_transform_dev(ctx.h, _ptr(_colmajor(k, 3)), v(d_pairs), C.c_int(n_max), v(d_n_pairs), v(d_mask), v(d_p1),
                                         C.c_int(n1), v(d_p2), C.c_int(n2), _ptr(_colmajor(X_in, 4)) if X_in is not None else None,
                                         v(d_X_in), C.byref(params), v(d_X_out), v(d_stats)))


def refine_transform(k, correspondences, p1_img, p2_img, X, n_rounds=10, huber_px=0.0, mask=None, ctx: Context | None = None):
    """Gauss-Newton refit of the relative pose X (4x4, e.g. from estimate_transform[_ransac]) on the Sampson error of the
    pairs (vo_refine_transform): n_rounds plain rounds, Huber weight at huber_px pixels (0: none), only the pairs marked in
    mask (one flag per pair, or None: all).  Returns (X_out (4x4), stats dict): X_out is X bit for bit unless
    stats["status"] == 0 (EPI_REFINE_STATUS names the others)."""
    ctx = ctx or default_context()
    pairs = _i32pairs(correspondences)
    a = _f32(p1_img, (-1, 2))
    b = _f32(p2_img, (-1, 2))
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if len(m) != len(pairs):
            raise ValueError("mask must hold one flag per pair")
    out = np.zeros(16, dtype=np.float32)
    st = EpiRefineStats()
    prm = EpiRefineParams(int(n_rounds), float(huber_px))
    _chk(ctx.lib.vo_refine_transform(ctx.h, _ptr(_colmajor(k, 3)), _ptr(pairs), C.c_int(len(pairs)), _ptr(m) if m is not None else None,
                                     _ptr(a), C.c_int(len(a)), _ptr(b), C.c_int(len(b)), _ptr(_colmajor(X, 4)), C.byref(prm),
                                     _ptr(out), C.byref(st)))
    return out.reshape(4, 4).T.copy(), st.as_dict()


def estimate_pose_ransac(k, rows, cols, z_near, z_far, world, meas, correspondences, threshold_px=1.0, n_hypotheses=2048, seed=0,
                         ctx: Context | None = None):
    """P3P RANSAC over 2D-3D pairs (vo_estimate_pose_ransac): n_hypotheses minimal P3P fits scored by reprojection error on
    the GPU behind Camera::projectPoint's gates.  correspondences = (meas_idx, world_idx), the solver's orientation.  Returns
    (T (4x4, world in camera: the pose a PICP solve starts from), mask (bool, one per pair), n_inliers)."""
    ctx = ctx or default_context()
    pairs = _i32pairs(correspondences)
    w = _f32(world, (-1, 3))
    m = _f32(meas, (-1, 2))
    T = np.zeros(16, dtype=np.float32)
    mask = np.zeros(max(len(pairs), 1), dtype=np.uint8)
    n_in = C.c_int()
    prm = RansacParams(int(n_hypotheses), float(threshold_px), int(seed) & 0xFFFFFFFFFFFFFFFF)
    _chk(ctx.lib.vo_estimate_pose_ransac(ctx.h, C.c_int(rows), C.c_int(cols), C.c_int(z_near), C.c_int(z_far), _ptr(_colmajor(k, 3)),
                                         _ptr(w), C.c_int(len(w)), _ptr(m), C.c_int(len(m)), _ptr(pairs), C.c_int(len(pairs)),
                                         C.byref(prm), _ptr(T), _ptr(mask), C.byref(n_in)))
    return T.reshape(4, 4).T.copy(), mask[: len(pairs)].astype(bool), n_in.value


def estimate_pose_ransac_batch_dev(ctx: Context, n_problems, rows, cols, z_near, z_far, k, d_world, world_stride, n_world, d_meas,
                                   meas_stride, n_meas, d_pairs, pairs_stride, d_n_pairs, params: RansacParams, d_T16, d_inlier_pairs,
                                   d_n_inliers, d_mask, d_counts, d_status):
    """vo_estimate_pose_ransac_batch_dev on device pointers (ints; d_n_pairs, d_mask, d_counts may be None): enqueues and
    returns.  Strides in elements (points, pixels, pairs)."""
    v = lambda d: C.c_void_p(d) if d else None
    _chk(ctx.lib.vo_estimate_pose_ransac_batch_dev(
        ctx.h, C.c_int(n_problems), C.c_int(rows), C.c_int(cols), C.c_int(z_near), C.c_int(z_far), _ptr(_colmajor(k, 3)),
        v(d_world), C.c_size_t(world_stride), C.c_int(n_world), v(d_meas), C.c_size_t(meas_stride), C.c_int(n_meas), v(d_pairs),
        C.c_size_t(pairs_stride), v(d_n_pairs), C.byref(params), v(d_T16), v(d_inlier_pairs), v(d_n_inliers), v(d_mask), v(d_counts),
        v(d_status)))


def estimate_pose_ransac_batch(ctx: Context, problems, k, rows, cols, z_near, z_far, threshold_px=2.0, n_hypotheses=128, seed=0):
    """P3P RANSAC over many 2D-3D problems in ONE call (vo_estimate_pose_ransac_batch_dev).  problems: a list of host problems
    (world (n, 3), meas (m, 2), correspondences (p, 2) = (meas_idx, world_idx)) of any sizes -- padded to common strides and
    uploaded.  Every problem's result is bit for bit that of the single device call on it alone.  Returns, per problem,
    (T (4x4), status (VO_POSE_RANSAC_*: 0 tracked, 1-4 fell back to the identity and every pair), inlier pairs (n, 2) in
    their original order, mask (bool, one per pair)).  The batched default is 128 hypotheses."""
    P = len(problems)
    if P == 0:
        return []
    W = [_f32(w, (-1, 3)) for w, _, _ in problems]
    M = [_f32(m, (-1, 2)) for _, m, _ in problems]
    Q = [_i32pairs(c) for _, _, c in problems]
    nw, nm, npr = max(max(map(len, W)), 1), max(max(map(len, M)), 1), max(max(map(len, Q)), 1)

    def stack(arrs, cap, width, dt):
        out = np.zeros((P, cap, width), dt)
        for i, a in enumerate(arrs):
            out[i, : len(a)] = a
        return out

    n = np.array([len(q) for q in Q], np.int32)
    ins = [ctx.to_device(stack(W, nw, 3, np.float32)), ctx.to_device(stack(M, nm, 2, np.float32)),
           ctx.to_device(stack(Q, npr, 2, np.int32)), ctx.to_device(n)]
    outs = [ctx.alloc(P * 64), ctx.alloc(P * npr * 8), ctx.alloc(max(P * 4, 8)), ctx.alloc(max(P * npr, 8)), ctx.alloc(max(P * 4, 8))]
    try:
        prm = RansacParams(int(n_hypotheses), float(threshold_px), int(seed) & 0xFFFFFFFFFFFFFFFF)
        # the points every problem may index are its own: a stride's padding is never a valid index
        estimate_pose_ransac_batch_dev(ctx, P, rows, cols, z_near, z_far, k, ins[0], nw, nw, ins[1], nm, nm, ins[2], npr, ins[3], prm,
                                       outs[0], outs[1], outs[2], outs[3], None, outs[4])
        T = np.zeros((P, 16), np.float32); ctx.d2h(T, outs[0])
        inl = np.zeros((P, npr, 2), np.int32); ctx.d2h(inl, outs[1])
        nin = np.zeros(P, np.int32); ctx.d2h(nin, outs[2])
        mask = np.zeros((P, npr), np.uint8); ctx.d2h(mask, outs[3])
        st = np.zeros(P, np.int32); ctx.d2h(st, outs[4])
    finally:
        for d in ins + outs:
            ctx.free(d)
    return [(T[p].reshape(4, 4).T.copy(), int(st[p]), inl[p, : nin[p]].copy(), mask[p, : n[p]].astype(bool)) for p in range(P)]


def radius_search(tree_appearances, query_appearances, radius=0.1, ctx: Context | None = None):
    """TreeNode_::fullSearch (eigen_kdtree.h:56-71) for every query: list of int32 arrays, one per query,
    with the indices of ALL tree points closer than `radius` (ascending; the library's order is unspecified)."""
    ctx = ctx or default_context()
    t = _f32(tree_appearances, (-1, 10))
    q = _f32(query_appearances, (-1, 10))
    offsets = np.zeros(len(q) + 1, dtype=np.int32)
    cap = max(2 * len(q), 16)
    while True:
        idx = np.zeros(cap, dtype=np.int32)
        n_total = C.c_int()
        rc = ctx.lib.vo_radius_search(ctx.h, _ptr(t), C.c_int(len(t)), _ptr(q), C.c_int(len(q)), C.c_float(radius),
                                      _ptr(offsets), _ptr(idx), C.c_int(cap), C.byref(n_total))
        if rc == -1 and n_total.value > cap:            # not enough room: the call reports what it needs
            cap = n_total.value
            continue
        _chk(rc)
        break
    return [np.sort(idx[offsets[i]:offsets[i + 1]]) for i in range(len(q))]


class KdTree:
    """The reference's PCA kd-tree in its approximate modes (eigen_kdtree.h:18-52,75-85; vo_kdtree_*): built on the
    host like the TreeNode_ constructor, queried on the GPU.  bestMatchFull / fullSearch are tree-independent:
    compute_correspondences_images / radius_search."""

    def __init__(self, points_appearances, max_points_in_leaf=20, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        p = _f32(points_appearances, (-1, 10))
        h = C.c_void_p()
        _chk(self.lib.vo_kdtree_create(self.ctx.h, _ptr(p), C.c_int(len(p)), C.c_int(max_points_in_leaf), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.vo_kdtree_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        n, nodes, leaves = C.c_int(), C.c_int(), C.c_int()
        _chk(self.lib.vo_kdtree_info(self.h, C.byref(n), C.byref(nodes), C.byref(leaves)))
        return n.value, nodes.value, leaves.value

    def bestMatchFast(self, queries, norm=0.1):
        """index of the best point of each query's leaf within `norm`, or -1 (eigen_kdtree.h:75-85)"""
        q = _f32(queries, (-1, 10))
        out = np.full(max(len(q), 1), -1, dtype=np.int32)
        _chk(self.lib.vo_kdtree_best_match_fast(self.h, _ptr(q), C.c_int(len(q)), C.c_float(norm), _ptr(out)))
        return out[:len(q)].copy()

    def fastSearch(self, queries, norm=0.1):
        """per query the points of its leaf within `norm`, in leaf order (eigen_kdtree.h:40-52)"""
        q = _f32(queries, (-1, 10))
        offsets = np.zeros(len(q) + 1, dtype=np.int32)
        cap = max(2 * len(q), 16)
        while True:
            idx = np.zeros(cap, dtype=np.int32)
            n_total = C.c_int()
            rc = self.lib.vo_kdtree_fast_search(self.h, _ptr(q), C.c_int(len(q)), C.c_float(norm), _ptr(offsets), _ptr(idx),
                                                C.c_int(cap), C.byref(n_total))
            if rc == -1 and n_total.value > cap:
                cap = n_total.value
                continue
            _chk(rc)
            break
        return [idx[offsets[i]:offsets[i + 1]].copy() for i in range(len(q))]
