"""Time vo_estimate_pose_ransac_dev at 50k pairs (30 % of the world indices replaced at random, large motion) x {512, 2048,
8192} hypotheses, next to 100 plain PICP rounds (vo_picp_solve_dev) on the same pairs, every array already in device memory
(the form DeviceSequence / SequencePipeline call).

  python tools/pose_ransac_rate.py [--hyp 512,2048,8192] [--reps 30]       -> one JSON line per hypothesis count
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pose_ransac_rate.py --hyp 2048
  python tools/pose_ransac_rate.py --split DIR/*/*kernel_stats.csv        -> the traced run's kernels folded into stages
  python tools/pose_ransac_rate.py --batch 200 [--sizes 127,2000,50000] [--hyp 128,512] [--frames 200x50000]
      vo_estimate_pose_ransac_batch_dev on P problems against a loop of P single calls on the same data (five alternating
      runs per shape, the median run each), then the tracked many-frames call against the plain one (--frames FxN, 50 rounds,
      128 hypotheses; --frames 0 leaves it out): one JSON line per measurement, each stamped (tools/stamp.py)

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

STAGES = [("gather", ("pose_gather_kernel", "pose_gather_batch_kernel")), ("hypotheses", ("pose_hyp_kernel", "pose_hyp_batch_kernel")),
          ("scoring", ("pose_score_kernel", "pose_score_batch_kernel")),
          ("select", ("pose_select_kernel", "pose_mask_kernel", "pose_scatter_kernel", "pose_select_batch_kernel",
                      "pose_mask_batch_kernel", "pose_scatter_batch_kernel")),
          ("picp", ("picp",)), ("match", ("match", "hash", "cell")), ("join", ("join",)), ("triangulate", ("triang",)),
          ("transform", ("transform",)), ("scan", ("scan_counts_kernel",))]


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


def batch_mode(a):
    import ctypes as C

    import numpy as np

    import __graft_entry__ as g
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pose_ransac_restatement as P
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    lib, V, I, S = ctx.lib, C.c_void_p, C.c_int, C.c_size_t
    st = stamp.current()
    cam = (480, 640, 0, 10)
    NP = a.batch

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    def timed(f, reps):
        sync()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        sync()
        return (time.perf_counter() - t) / reps * 1e3

    def alternate(fa, fb, reps):
        """five alternating runs of each: (median ms of a, median ms of b)"""
        fa(); fb()
        ta, tb = [], []
        for _ in range(5):
            ta.append(timed(fa, reps)); tb.append(timed(fb, reps))
        return statistics.median(ta), statistics.median(tb), ta, tb

    for n in [int(x) for x in a.sizes.split(",") if x.strip() and int(x) > 0]:      # (--sizes 0: the frames measurement alone)
        # P problems of n pairs: the same generator, another seed per problem up to 8, then repeated (the timing does not see it)
        base = [P.tracking_problem(vo, n, seed=2001 + i, noise_px=0.5, frac=a.frac, max_angle=0.3, max_t=0.5) for i in range(min(NP, 8))]
        K = np.ascontiguousarray(np.asarray(base[0][0]["K"], np.float32).T).ravel()
        pick = [base[i % len(base)] for i in range(NP)]
        world = np.ascontiguousarray(np.stack([np.asarray(b[1], np.float32) for b in pick]))
        meas = np.ascontiguousarray(np.stack([np.asarray(b[2], np.float32) for b in pick]))
        pairs = np.ascontiguousarray(np.stack([np.asarray(b[3], np.int32) for b in pick]))
        d_w, d_m, d_p = ctx.to_device(world), ctx.to_device(meas), ctx.to_device(pairs)
        d_T, d_inl, d_nin, d_st = ctx.alloc(NP * 64), ctx.alloc(NP * n * 8), ctx.alloc(NP * 4 + 8), ctx.alloc(NP * 4 + 8)
        d_T1, d_inl1, d_nin1, d_st1 = ctx.alloc(NP * 64), ctx.alloc(NP * n * 8), ctx.alloc(NP * 4 + 8), ctx.alloc(NP * 4 + 8)
        for H in [int(x) for x in a.hyp.split(",")]:
            prm = vo.RansacParams(H, 2.0, 0)

            def batched():
                rc = lib.vo_estimate_pose_ransac_batch_dev(ctx.h, I(NP), *map(I, cam), K.ctypes.data_as(V), V(d_w), S(n), I(n), V(d_m), S(n),
                                                           I(n), V(d_p), S(n), None, C.byref(prm), V(d_T), V(d_inl), V(d_nin), None, None,
                                                           V(d_st))
                assert rc == 0, lib.vo_last_error()

            def loop():
                for q in range(NP):
                    rc = lib.vo_estimate_pose_ransac_dev(ctx.h, *map(I, cam), K.ctypes.data_as(V), V(d_w + 12 * n * q), I(n),
                                                         V(d_m + 8 * n * q), I(n), V(d_p + 8 * n * q), I(n), None, C.byref(prm),
                                                         V(d_T1 + 64 * q), V(d_inl1 + 8 * n * q), V(d_nin1 + 4 * q), None, None,
                                                         V(d_st1 + 4 * q))
                    assert rc == 0, lib.vo_last_error()

            reps = max(1, min(a.reps, int(2e8 / (NP * n * H)) + 1))
            tb, tl, rb, rl = alternate(batched, loop, reps)
            get = lambda d, k, dt: (lambda x: (ctx.d2h(x, d), x)[1])(np.zeros(k, dt))
            same = get(d_T, NP * 16, np.float32).tobytes() == get(d_T1, NP * 16, np.float32).tobytes() and \
                np.array_equal(get(d_nin, NP, np.int32), get(d_nin1, NP, np.int32)) and \
                np.array_equal(get(d_st, NP, np.int32), get(d_st1, NP, np.int32))
            print(json.dumps({"measurement": "batched call vs loop of single calls", "problems": NP, "pairs": n, "mismatched": a.frac,
                              "hypotheses": H, "reps_per_run": reps, "batched_ms": round(tb, 4), "loop_ms": round(tl, 4),
                              "loop_over_batched": round(tl / tb, 2), "batched_runs_ms": [round(x, 4) for x in rb],
                              "loop_runs_ms": [round(x, 4) for x in rl], "same_poses_counts_status": bool(same),
                              "fell_back": int((get(d_st, NP, np.int32) != 0).sum()), "device": ctx.device_info()[0], "stamp": st}),
                  flush=True)
        for d in (d_w, d_m, d_p, d_T, d_inl, d_nin, d_st, d_T1, d_inl1, d_nin1, d_st1):
            ctx.free(d)
    if a.frames and a.frames != "0":
        F, n = (int(x) for x in a.frames.lower().split("x"))
        fps = [vo.synth.frame_pair(n, seed=2001 + i, noise_px=0.5) for i in range(min(F, 4))]
        gen = lambda lo, hi: [fps[i % len(fps)] for i in range(lo, hi)]
        plain = vo.BatchPipeline(ctx, gen, n_iters=50, with_appearance=False, n_frames=F, upload_block=50)
        tracked = vo.BatchPipeline(ctx, gen, n_iters=50, with_appearance=False, n_frames=F, upload_block=50,
                                   track_ransac=dict(threshold_px=2.0, n_hypotheses=128, seed=0))
        tt, tp, rt, rp = alternate(tracked.run, plain.run, max(1, a.reps // 6))
        stt, ntr = tracked.track_stats()
        print(json.dumps({"measurement": "tracked many-frames call vs plain", "frames": F, "points": n, "rounds": 50, "hypotheses": 128,
                          "tracked_ms": round(tt, 4), "plain_ms": round(tp, 4), "tracked_frames_per_s": round(F * 1e3 / tt),
                          "plain_frames_per_s": round(F * 1e3 / tp), "tracked_runs_ms": [round(x, 4) for x in rt],
                          "plain_runs_ms": [round(x, 4) for x in rp], "fell_back": int((stt != 0).sum()),
                          "pairs_handed_on_mean": float(ntr.mean()), "device": ctx.device_info()[0], "stamp": st}), flush=True)
        plain.close(); tracked.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--sizes", default="127,2000,50000")
    ap.add_argument("--frames", default="200x50000")
    ap.add_argument("--hyp", default="512,2048,8192")
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--frac", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--split", default=None)
    a = ap.parse_args()
    if a.split:
        return split(a.split)
    if a.batch:
        if a.hyp == "512,2048,8192":
            a.hyp = "128,512"
        return batch_mode(a)
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
