"""Time vo_estimate_pose_ransac_dev at 50k pairs (30 % of the world indices replaced at random, large motion) x {512, 2048,
8192} hypotheses, next to 100 plain PICP rounds (vo_picp_solve_dev) on the same pairs, every array already in device memory
(the form DeviceSequence / SequencePipeline call).

  python tools/pose_ransac_rate.py [--hyp 512,2048,8192] [--reps 30]       -> one JSON line per hypothesis count
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pose_ransac_rate.py --hyp 2048
  python tools/pose_ransac_rate.py --split DIR/*/*kernel_stats.csv        -> the traced run's kernels folded into stages

Stages: gather (the packed records), hypotheses (sample + P3P), scoring, select (selection, mask, scan, compaction) and, for
the solve that follows, picp (its kernels).  The call itself never waits: its wall time is taken to a stream
synchronisation behind it (vo_ctx_synchronize), the same for the solve."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = [("gather", ("pose_gather_kernel",)), ("hypotheses", ("pose_hyp_kernel",)), ("scoring", ("pose_score_kernel",)),
          ("select", ("pose_select_kernel", "pose_mask_kernel", "scan_counts_kernel", "pose_scatter_kernel")),
          ("picp", ("picp",))]


def split(path):
    rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        name = r["Name"]
        calls, total = int(r["Calls"]), float(r["TotalDurationNs"])
        stage = "other"
        for s, keys in STAGES:
            if any(k in name for k in keys):
                stage = s
                break
        o = out.setdefault(stage, {"kernels": {}, "total_ns": 0.0})
        o["kernels"][name.replace("void ", "").split("(")[0]] = {"calls": calls, "avg_us": round(total / calls / 1e3, 2)}
        o["total_ns"] += total
    print(json.dumps({"kernel_stats": os.path.basename(path), "stages": out}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hyp", default="512,2048,8192")
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--frac", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--split", default=None)
    a = ap.parse_args()
    if a.split:
        return split(a.split)
    import ctypes as C

    import numpy as np

    import __graft_entry__ as g
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pose_ransac_restatement as P
    vo = g.load_package()
    ctx = vo.Context(0)
    lib = ctx.lib
    fp, world, meas, pairs, bad, _ = P.tracking_problem(vo, a.n, seed=2001, noise_px=0.5, frac=a.frac, max_angle=0.3, max_t=0.5)
    K = np.ascontiguousarray(np.asarray(fp["K"], np.float32).T).ravel()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    cam = (480, 640, 0, 10)
    n = len(pairs)
    d_w, d_m, d_pairs = ctx.to_device(np.ascontiguousarray(world, np.float32)), ctx.to_device(np.ascontiguousarray(meas, np.float32)), \
        ctx.to_device(pairs)
    d_T, d_inl, d_nin, d_st, d_I, d_n = ctx.alloc(64), ctx.alloc(8 * n), ctx.alloc(16), ctx.alloc(16), ctx.alloc(64), ctx.alloc(16)
    ctx.h2d(d_I, np.eye(4, dtype=np.float32)); ctx.h2d(d_n, np.array([n], np.int32))
    h = C.c_void_p()
    assert lib.vo_picp_create(ctx.h, C.byref(h)) == 0
    assert lib.vo_picp_set_camera(h, *map(C.c_int, cam), p(K), p(np.eye(4, dtype=np.float32))) == 0
    assert lib.vo_picp_set_kernel_threshold(h, C.c_float(10000.0)) == 0
    assert lib.vo_picp_set_points_dev(h, C.c_void_p(d_w), C.c_int(len(world)), C.c_void_p(d_m), C.c_int(len(meas))) == 0

    def timed(f):
        assert lib.vo_ctx_synchronize(ctx.h) == 0
        t = time.perf_counter()
        f()
        assert lib.vo_ctx_synchronize(ctx.h) == 0
        return time.perf_counter() - t

    def solve(dT, dp, dn):
        assert lib.vo_picp_set_pose_dev(h, C.c_void_p(dT)) == 0
        assert lib.vo_picp_solve_dev(h, C.c_void_p(dp), C.c_int(n), C.c_void_p(dn), C.c_int(0), C.c_int(100)) == 0

    for H in [int(x) for x in a.hyp.split(",")]:
        prm = vo.RansacParams(H, 2.0, 0)

        def robust():
            rc = lib.vo_estimate_pose_ransac_dev(ctx.h, *map(C.c_int, cam), p(K), C.c_void_p(d_w), C.c_int(len(world)), C.c_void_p(d_m),
                                                 C.c_int(len(meas)), C.c_void_p(d_pairs), C.c_int(n), None, C.byref(prm),
                                                 C.c_void_p(d_T), C.c_void_p(d_inl), C.c_void_p(d_nin), None, None, C.c_void_p(d_st))
            assert rc == 0, lib.vo_last_error()
        for _ in range(3):
            timed(robust); timed(lambda: solve(d_I, d_pairs, d_n))
        tr = [timed(robust) for _ in range(a.reps)]
        tt = [timed(lambda: (robust(), solve(d_T, d_inl, d_nin))) for _ in range(a.reps)]
        tp = [timed(lambda: solve(d_I, d_pairs, d_n)) for _ in range(a.reps)]
        nin, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
        ctx.d2h(nin, d_nin); ctx.d2h(st, d_st)
        med = lambda v: round(statistics.median(v) * 1e3, 4)
        print(json.dumps({"pairs": n, "mismatched": a.frac, "hypotheses": H, "status": int(st[0]), "inliers": int(nin[0]),
                          "ransac_ms": med(tr), "ransac_ms_min": round(min(tr) * 1e3, 4),
                          "ransac_plus_100_rounds_ms": med(tt), "plain_100_rounds_ms": med(tp),
                          "tracking_ratio_to_plain": round(statistics.median(tt) / statistics.median(tp), 2),
                          "device": ctx.device_info()[0]}), flush=True)
    lib.vo_picp_destroy(h)
    for d in (d_w, d_m, d_pairs, d_T, d_inl, d_nin, d_st, d_I, d_n):
        ctx.free(d)


if __name__ == "__main__":
    main()
