"""Time vo_estimate_transform_ransac_dev at 50k pairs (30 % mismatched) x {512, 2048, 8192} hypotheses, next to the plain
vo_estimate_transform_dev on the same pairs, every array already in device memory (the form DeviceSequence calls).

  python tools/ransac_rate.py [--hyp 512,2048,8192] [--reps 30]            -> one JSON line per hypothesis count
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ransac_rate.py --hyp 2048
  python tools/ransac_rate.py --split DIR/*/*kernel_stats.csv             -> the traced run's kernels folded into stages

Stages: gather (maxima of both images + the float4 pairs), hypotheses (sample + minimal solve), scoring, select (selection,
mask, compaction), refit (vo_estimate_transform_dev's kernels: maxima, A^T A, vote).  Wall times include the call's host
syncs: one read-back after the selection and the refit's two."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = [("gather", ("ransac_gather_kernel",)), ("hypotheses", ("ransac_hyp_kernel",)), ("scoring", ("ransac_score_kernel",)),
          ("select", ("ransac_select_kernel", "ransac_mask_kernel", "scan_counts_kernel", "ransac_scatter_kernel")),
          ("refit", ("epi_ata_kernel", "epi_sum_kernel", "epi_vote_kernel"))]


def split(path):
    rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        name = r["Name"]
        calls, total = int(r["Calls"]), float(r["TotalDurationNs"])
        stage = "other"
        if "epi_max_kernel" in name:
            stage = "maxima"                     # launched twice per call: once in front of the gather, once by the refit
        for s, keys in STAGES:
            if any(k in name for k in keys):
                stage = s
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
    import ransac_restatement as R
    vo = g.load_package()
    ctx = vo.Context(0)
    fp = vo.synth.frame_pair(a.n, seed=2000, noise_px=0.25)
    pairs, _ = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), a.frac)
    K = np.ascontiguousarray(np.asarray(fp["K"], np.float32).T).ravel()
    d_pairs, d_p1, d_p2 = ctx.to_device(pairs), ctx.to_device(fp["ref_pts"]), ctx.to_device(fp["cur_pts"])
    n, n1, n2 = len(pairs), len(fp["ref_pts"]), len(fp["cur_pts"])
    X = np.zeros(16, np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def plain(dp, m):
        t = time.perf_counter()
        rc = ctx.lib.vo_estimate_transform_dev(ctx.h, p(K), C.c_void_p(dp), C.c_int(m), None, C.c_void_p(d_p1), C.c_int(n1),
                                               C.c_void_p(d_p2), C.c_int(n2), p(X))
        assert rc == 0, ctx.lib.vo_last_error()
        return time.perf_counter() - t

    for H in [int(h) for h in a.hyp.split(",")]:
        prm = vo.RansacParams(H, 1.0, 0)
        n_in = C.c_int()

        def robust():
            t = time.perf_counter()
            rc = ctx.lib.vo_estimate_transform_ransac_dev(ctx.h, p(K), C.c_void_p(d_pairs), C.c_int(n), None, C.c_void_p(d_p1),
                                                          C.c_int(n1), C.c_void_p(d_p2), C.c_int(n2), C.byref(prm), p(X), None,
                                                          None, C.byref(n_in))
            assert rc == 0, ctx.lib.vo_last_error()
            return time.perf_counter() - t
        for _ in range(3):
            robust(); plain(d_pairs, n)
        tr = [robust() for _ in range(a.reps)]
        inl = pairs[vo.estimate_transform_ransac(fp["K"], pairs, fp["ref_pts"], fp["cur_pts"], 1.0, H, 0, ctx=ctx)[1]]
        d_inl = ctx.to_device(inl)
        tp = [plain(d_pairs, n) for _ in range(a.reps)]
        tf = [plain(d_inl, len(inl)) for _ in range(a.reps)]
        ctx.free(d_inl)
        med = lambda v: round(statistics.median(v) * 1e3, 4)
        print(json.dumps({"pairs": n, "mismatched": a.frac, "hypotheses": H, "inliers": n_in.value,
                          "ransac_ms": med(tr), "ransac_ms_min": round(min(tr) * 1e3, 4),
                          "plain_ms_all_pairs": med(tp), "plain_ms_inliers_only": med(tf),
                          "ratio_to_plain": round(statistics.median(tr) / statistics.median(tp), 2),
                          "device": ctx.device_info()[0]}), flush=True)
    for d in (d_pairs, d_p1, d_p2):
        ctx.free(d)


if __name__ == "__main__":
    main()
