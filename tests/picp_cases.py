"""Inputs shared by the tests of the PICP solver: correspondences of a generated frame pair, the case matrix that
tests/test_picp_budget_cpu.py (reference side) and tests/test_gpu_picp_system.py (GPU) both walk, and the upload of a batch
of problems for vo_picp_solve_batch_dev.  Test infrastructure only."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np

from picp_budget import N_CU

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_picp_cases_synth", os.path.join(_ROOT, "visual-odometry_amd", "synth.py"))
synth = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(synth)                    # numpy only: the CPU tests need no library

ROWS, COLS, Z_NEAR, Z_FAR = 480, 640, 0, 10
CAP = 4 * N_CU * 256                               # picp_grid_for: at most 4 workgroups per CU; from CAP pairs on threads loop
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 65535, 65536, 65537, 131073, CAP - 1, CAP, CAP + 1, 300001)
FULL = (257, 65537)                                # every pose x setting x K
POSES = ("identity", "small", "general")
SETTINGS = ((10000.0, False), (60.0, False), (60.0, True))


def corr_of(fp):
    """(measurement index, world index) pairs of a generated frame pair's true matches"""
    mp = dict(fp["model_pairs"].tolist())
    return np.array([(c, mp[r]) for r, c in fp["gt_matches"].tolist()], np.int32)


def general_K(K):
    K = np.array(K, np.float32)
    K[0, 1] = 0.7                                  # skew, and a last row entry that is not 1: the non-pinhole instantiation
    K[2, 2] = 1.0009765625
    return K


def general_world(rng, model):
    """move the world by G^-1, G a general isometry: a camera at X G then sees what a camera at X saw before -- the camera
    points are unchanged, the gates still pass, and R is far from I.  -> (world float32, G float64)"""
    G = synth.random_isometry(rng, 1.0, 2.0).astype(np.float64)
    Gi = np.linalg.inv(G)
    world = (model.astype(np.float64) @ Gi[:3, :3].T + Gi[:3, 3]).astype(np.float32)
    return world, G


@functools.lru_cache(maxsize=None)
def frame(n):
    """per size: the frame pair, its pairs, and the three start poses with their worlds"""
    fp = synth.frame_pair(n, seed=3000 + n)
    corr = corr_of(fp)
    assert len(corr) == n
    rng = np.random.default_rng(n)
    small = synth.random_isometry(rng, 0.01, 0.02).astype(np.float32)
    world_g, G = general_world(rng, fp["model"])
    T_g = (synth.random_isometry(rng, 0.01, 0.02).astype(np.float64) @ G).astype(np.float32)
    poses = dict(identity=(np.eye(4, dtype=np.float32), fp["model"]), small=(small, fp["model"]), general=(T_g, world_g))
    return dict(fp=fp, corr=corr, poses=poses, K=dict(pinhole=np.asarray(fp["K"], np.float32), general=general_K(fp["K"])))


def case_ids():
    """the covering set: every size at the general pose with (60, keep), K alternating; every pose x setting x K at FULL;
    and the sizes from 65 535 on at the general pose with (10000, drop) as well -- at thr = 60 a quarter of a million pairs
    always hold a few within the chi^2 band, which leaves the inlier count open by that many, while at thr = 10000 every
    pair is an inlier far from every gate and the count must be n exactly: one pair dropped or visited twice at a grid edge
    cannot hide"""
    ids = []
    for i, n in enumerate(SIZES):
        if n not in FULL:
            ids.append((n, "general", 60.0, True, "general" if i % 2 else "pinhole"))
            if n >= 65535:
                ids.append((n, "general", 10000.0, False, "pinhole" if i % 2 else "general"))
    for n in FULL:
        for pose in POSES:
            for thr, keep in SETTINGS:
                for k in ("pinhole", "general"):
                    ids.append((n, pose, thr, keep, k))
    return ids


def case_name(cid):
    n, pose, thr, keep, k = cid
    return f"{n}-{pose}-thr{int(thr)}-{'keep' if keep else 'drop'}-{k}"


def case(cid):
    """-> dict(K, T0, world, meas, corr, thr, keep): the arguments of picp_budget.system after K and T"""
    n, pose, thr, keep, k = cid
    f = frame(n)
    T0, world = f["poses"][pose]
    return dict(K=f["K"][k], T0=T0, world=world, meas=f["fp"]["cur_pts"], corr=f["corr"], thr=thr, keep=keep)


def system_args(c, T=None):
    return (c["K"], c["T0"] if T is None else T, c["world"], c["meas"], c["corr"], c["thr"], c["keep"], ROWS, COLS, Z_NEAR, Z_FAR)


class Batch:
    """P problems over ONE generated frame pair (so that the oracle has one camera and the test one upload): problem p uses
    the first sizes[p] pairs and starts at T0[p].  `world` replaces the frame's model points (same count), `T0` the small
    random start poses."""

    def __init__(self, vo, ctx, n, sizes, seed, K=None, rng_seed=3, world=None, T0=None):
        self.vo, self.ctx, self.n = vo, ctx, n
        self.fp = vo.synth.frame_pair(n, seed=seed, distractors=n // 50)
        self.pairs = corr_of(self.fp)
        self.sizes = np.array([min(s, len(self.pairs)) for s in sizes], np.int32)
        self.P = len(sizes)
        self.stride = len(self.pairs)
        self.K = np.asarray(self.fp["K"] if K is None else K, np.float32)
        self.world = np.asarray(self.fp["model"] if world is None else world, np.float32)
        assert self.world.shape == self.fp["model"].shape
        rng = np.random.default_rng(rng_seed)
        if T0 is None:
            T0 = np.stack([vo.synth.random_isometry(rng, 0.01, 0.02) for _ in range(self.P)])
        self.T0 = np.asarray(T0, np.float32)
        self.d = [ctx.to_device(np.tile(self.world, (self.P, 1))), ctx.to_device(np.tile(self.fp["cur_pts"], (self.P, 1))),
                  ctx.to_device(np.tile(self.pairs, (self.P, 1))), ctx.to_device(self.sizes),
                  ctx.to_device(np.ascontiguousarray(np.transpose(self.T0, (0, 2, 1))).reshape(self.P, 16))]
        self.d_T, self.d_S = ctx.alloc(self.P * 64), ctx.alloc(self.P * 16)

    def run(self, iters, thr, keep, form=2):
        lib, ctx = self.ctx.lib, self.ctx
        assert lib.vo_picp_batch_set_form(ctx.h, form) == 0
        K = np.ascontiguousarray(self.K.T).ravel()
        n_pts = len(self.world)
        rc = lib.vo_picp_solve_batch_dev(ctx.h, self.P, 480, 640, 0, 10, K.ctypes.data_as(C.c_void_p), C.c_float(thr), int(keep),
                                         C.c_void_p(self.d[0]), C.c_size_t(n_pts), C.c_void_p(self.d[1]), C.c_size_t(len(self.fp["cur_pts"])),
                                         C.c_void_p(self.d[2]), C.c_size_t(self.stride), C.c_void_p(self.d[3]), C.c_void_p(self.d[4]),
                                         iters, C.c_void_p(self.d_T), C.c_void_p(self.d_S))
        assert rc == 0, lib.vo_last_error()
        f, w = C.c_int(), C.c_int()
        assert lib.vo_picp_batch_info(ctx.h, C.byref(f), C.byref(w)) == 0
        T = np.zeros((self.P, 16), np.float32); S = np.zeros((self.P, 4), np.float32)
        ctx.d2h(T, self.d_T); ctx.d2h(S, self.d_S)
        lib.vo_picp_batch_set_form(ctx.h, 0)
        return T, S, f.value, w.value

    def close(self):
        for x in self.d + [self.d_T, self.d_S]:
            self.ctx.free(x)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """round 0 of a case on the reference side: the float64 system with its budgets, and rho of the float32 restatement with
    pairwise sums (picp_budget.system(dt=float32)) against it"""
    import picp_budget as pb
    a = system_args(case(cid))
    ref = pb.system(*a)
    f = pb.system(*a, dt=np.float32)
    r32 = pb.rho_system(ref, f["H"], f["b"], f["chi_in"], f["chi_out"], f["n_in"])
    return ref, r32


@functools.lru_cache(maxsize=None)
def ceiling():
    """C: 4 times the largest rho, over H, b and the chi^2 sums of the whole case matrix, of the reference's formulas
    evaluated in float32 with pairwise sums.  Measured on the reference side only, never on the kernels."""
    return 4.0 * max(reference(cid)[1]["worst"] for cid in case_ids())
