"""Time vo_refine_transform_dev (10 rounds) next to vo_estimate_transform_dev on the same arrays, at 2000 and 50 000 pairs,
every array already in device memory.  A run is `--calls` calls back to back, each timed on the host clock from the call to
the end of a stream synchronisation; the figure of a size is the median over `--runs` runs of the run's median call, the
two calls' runs alternating in one session.

  python tools/epi_refine_rate.py [--sizes 2000,50000] [--rounds 10] [--huber 0] [--runs 5] [--calls 200] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/epi_refine_rate.py --sizes 50000 --runs 1

One JSON line per size; --out writes the list as a file (profiles/epi_refine_rate.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,50000")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--huber", type=float, default=0.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np

    import __graft_entry__ as g
    vo = g.load_package()
    ctx = vo.Context(0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    results = []
    for n in [int(s) for s in a.sizes.split(",")]:
        fp = vo.synth.frame_pair(n, seed=2000, noise_px=0.5)
        pairs = np.ascontiguousarray(fp["gt_matches"], np.int32)
        K = np.ascontiguousarray(np.asarray(fp["K"], np.float32).T).ravel()
        d_pairs, d_p1, d_p2 = ctx.to_device(pairs), ctx.to_device(fp["ref_pts"]), ctx.to_device(fp["cur_pts"])
        d_out = ctx.alloc(128)
        n1, n2 = len(fp["ref_pts"]), len(fp["cur_pts"])
        X = np.zeros(16, np.float32)
        prm = vo.EpiRefineParams(a.rounds, a.huber)

        def linear():
            t = time.perf_counter()
            rc = ctx.lib.vo_estimate_transform_dev(ctx.h, p(K), C.c_void_p(d_pairs), C.c_int(n), None, C.c_void_p(d_p1), C.c_int(n1),
                                                   C.c_void_p(d_p2), C.c_int(n2), p(X))
            assert rc == 0, ctx.lib.vo_last_error()
            ctx.synchronize()
            return time.perf_counter() - t

        linear()
        X_lin = X.copy()

        def refit():
            t = time.perf_counter()
            rc = ctx.lib.vo_refine_transform_dev(ctx.h, p(K), C.c_void_p(d_pairs), C.c_int(n), None, None, C.c_void_p(d_p1), C.c_int(n1),
                                                 C.c_void_p(d_p2), C.c_int(n2), p(X_lin), None, C.byref(prm), C.c_void_p(d_out),
                                                 C.c_void_p(d_out + 64))
            assert rc == 0, ctx.lib.vo_last_error()
            ctx.synchronize()
            return time.perf_counter() - t

        for _ in range(20):
            refit(); linear()
        tr, tl = [], []
        for _ in range(a.runs):
            tr.append(statistics.median(refit() for _ in range(a.calls)))
            tl.append(statistics.median(linear() for _ in range(a.calls)))
        raw = np.zeros(40, np.uint8)
        ctx.d2h(raw, d_out + 64)
        st = vo.EpiRefineStats.from_buffer_copy(raw.tobytes()).as_dict()
        ms = lambda v: round(statistics.median(v) * 1e3, 4)
        r = {"pairs": n, "rounds": a.rounds, "huber_px": a.huber, "launches": 2 * (a.rounds + 1), "form": "two launches per round",
             "refit_ms": ms(tr), "refit_ms_runs": [round(v * 1e3, 4) for v in tr],
             "linear_ms": ms(tl), "linear_ms_runs": [round(v * 1e3, 4) for v in tl],
             "ratio_to_linear": round(statistics.median(tr) / statistics.median(tl), 3),
             "per_round_us": round(statistics.median(tr) * 1e6 / (a.rounds + 1), 2),
             "status": st["status"], "rounds_done": st["rounds"], "cost_before": st["cost_before"], "cost_after": st["cost_after"],
             "runs": a.runs, "calls_per_run": a.calls, "device": ctx.device_info()[0]}
        print(json.dumps(r), flush=True)
        results.append(r)
        for d in (d_pairs, d_p1, d_p2, d_out):
            ctx.free(d)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
