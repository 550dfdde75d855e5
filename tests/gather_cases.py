"""Worker of tests/test_gpu_gather_round.py: runs one fixed set of single-problem solves on cuda:0 and prints, as one JSON line,
what every solve left (pose, H, b, chi of inliers / outliers, inlier count -- as bytes -- or the error a getter returned).
Which form the library takes for them is decided by the environment of this process (VO_PICP_GATHER, ...): the test runs this
file once per setting and compares the lines."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as g  # noqa: E402

SIZES = (257, 300, 8191, 8192, 8193, 50000, 65537)
ITERS = (1, 2, 9)
SPARE = 7          # pairs of the device array beyond the device count (never to be read)


def state(s, vo):
    try:
        T = s.camera().worldInCameraPose()
    except vo.api.VoError as e:
        return ["error", e.code, str(e)]
    H, b = s.system()
    return [T.tobytes().hex(), H.tobytes().hex(), b.tobytes().hex(), float(s.chiInliers()).hex(), float(s.chiOutliers()).hex(),
            s.numInliers()]


def main():
    vo = g.load_package()
    sizes = [int(a) for a in sys.argv[1:]] or SIZES
    ctx = vo.Context(0)
    lib = ctx.lib
    out = {}
    for n in sizes:
        fp = vo.synth.frame_pair(n, seed=9800 + n % 89, noise_px=1.5)
        corr = np.stack([fp["gt_matches"][:n, 1], fp["model_pairs"][fp["gt_matches"][:n, 0], 1]], 1).astype(np.int32)
        assert len(corr) == n
        rng = np.random.default_rng(n)
        d_pairs = ctx.to_device(np.concatenate([corr, np.full((SPARE, 2), -7, np.int32)]))
        d_n = ctx.to_device(np.array([n], np.int32))
        T0 = vo.synth.random_isometry(rng, 0.02, 0.05).astype(np.float32)
        d_T0 = ctx.to_device(np.ascontiguousarray(T0.T).ravel())
        bad = corr.copy()
        bad[1] = (-1, 0)
        bad[n // 2] = (0, 10 ** 9)
        bad[n - 1] = (len(fp["cur_pts"]), 0)
        for pinhole in (True, False):
            K = fp["K"].copy()
            if not pinhole:
                K[0, 1] = 0.7
                K[2, 2] = 1.0009765625
            for keep in (False, True):
                key = "%d/%s/%s/" % (n, "pinhole" if pinhole else "general", "keep" if keep else "drop")
                cam = vo.Camera(fp["rows"], fp["cols"], fp["z_near"], fp["z_far"], K, np.eye(4), ctx=ctx)
                s = vo.PICPSolver(ctx)
                s.setKernelThreshold(40.0 if keep else 10000.0)
                for it in ITERS:
                    s.init(cam, fp["model"], fp["cur_pts"])
                    s.solve(corr, keep, it)                       # host pairs, re-packed (init has replaced the points)
                    out[key + "solve%d" % it] = state(s, vo)
                    # device pairs with a device count below the array's length, behind a pending pose reset
                    vo.api._chk(lib.vo_picp_set_pose_dev(s.h, C.c_void_p(d_T0)))
                    vo.api._chk(lib.vo_picp_solve_dev(s.h, C.c_void_p(d_pairs), C.c_int(n + SPARE), C.c_void_p(d_n),
                                                      C.c_int(int(keep)), C.c_int(it)))
                    out[key + "dev%d" % it] = state(s, vo)
                s.init(cam, fp["model"], fp["cur_pts"])
                s.solve(bad, keep, 2)                             # three pairs index outside the point arrays
                out[key + "bad"] = state(s, vo)
                s.init(cam, fp["model"], fp["cur_pts"])
                s.solve(bad, keep, 1)
                out[key + "bad1"] = state(s, vo)
                s.init(cam, fp["model"], fp["cur_pts"])
                s.solve(corr, keep, 2)                            # ... and the tally does not outlive them
                out[key + "after_bad"] = state(s, vo)
                s.init(cam, fp["model"], fp["cur_pts"])
                for _ in range(9):
                    s.oneRound(corr, keep)
                out[key + "rounds9"] = state(s, vo)
                s.close()
        for p in (d_pairs, d_n, d_T0):
            ctx.free(p)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
