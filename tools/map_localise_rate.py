"""Time the read-only side of the device map.

  python tools/map_localise_rate.py [--entries 800000] [--rows 50000] [--out profiles/map_localise_rate.json]
      (a) vo_map_lookup_dev of `rows` rows that are ALL present, against a map of about `entries` entries, next to
          vo_map_update_dev of the same rows on the same map (the update performs the same probe plus atomics and a commit; it
          finds every class, so the map does not change): same process, alternating, medians of 5 x 200 calls after warm-up.
      (b) the 121 frames of tests/golden/example_data in ONE vo_map_localise_batch_dev call against 121 vo_map_localise_dev
          calls enqueued back to back with one synchronisation at the end (64 hypotheses, 2 px, 50 rounds).
      One JSON object with the evidence stamp (tools/stamp.py) is written to --out and printed.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/map_localise_rate.py --trace-run
      one batched and 121 single calls alone, for the trace
  python tools/map_localise_rate.py --split DIR/*/*kernel_stats.csv      -> the traced run's kernels folded into stages"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STAGES = [("lookup", ("map_lookup",)), ("ransac", ("pose_",)), ("picp", ("picp", "T16_to_pose12")), ("finish", ("map_localise_finish",)),
          ("scan", ("scan_counts_kernel",)), ("map update", ("map_probe", "map_flag", "map_scan", "map_commit", "map_rehash"))]


def split(path):
    out = {}
    for r in csv.DictReader(open(path)):
        name, calls, total = r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])
        stage = next((s for s, keys in STAGES if any(k in name for k in keys)), "other")
        o = out.setdefault(stage, {"kernels": {}, "total_us": 0.0})
        o["kernels"][name.replace("void ", "").split("(")[0]] = {"calls": calls, "avg_us": round(total / calls / 1e3, 2)}
        o["total_us"] = round(o["total_us"] + total / 1e3, 2)
    print(json.dumps({"kernel_stats": os.path.basename(path), "stages": out}, indent=1))


def example_frames():
    import re

    import numpy as np
    data = os.path.join(ROOT, "tests", "golden", "example_data", "data")
    w = np.loadtxt(os.path.join(data, "world.dat"))
    frames = []
    for f in sorted(x for x in os.listdir(data) if re.search(r"^meas-\d.*\.dat$", x)):
        rows = [[float(v) for v in line.split()[3:15]] for line in open(os.path.join(data, f)).read().splitlines()[3:] if line.split()]
        a = np.array(rows, np.float32).reshape(-1, 12)
        frames.append((a[:, :2].copy(), a[:, 2:].copy()))
    lines = open(os.path.join(data, "camera.dat")).read().splitlines()
    K = np.array([[float(v) for v in ln.split()] for ln in lines[1:4]], np.float32)
    ints = {ln.split()[0]: int(ln.split()[1]) for ln in lines if ln.split() and ln.split()[0] in ("z_near:", "z_far:", "width:", "height:")}
    return w[:, 1:4].astype(np.float32), w[:, 4:14].astype(np.float32), frames, K, (ints["height:"], ints["width:"], ints["z_near:"], ints["z_far:"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=800000)
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_localise_rate.json"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--split", default=None)
    a = ap.parse_args()
    if a.split:
        return split(a.split)
    import numpy as np

    import __graft_entry__ as g
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    lib, V, I, S = ctx.lib, C.c_void_p, C.c_int, C.c_size_t

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    def timed(f, reps):
        sync()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        sync()
        return (time.perf_counter() - t) / reps * 1e6

    def alternate(fa, fb, reps):
        for _ in range(20):
            fa(); fb()
        ta, tb = [], []
        for _ in range(5):
            ta.append(timed(fa, reps)); tb.append(timed(fb, reps))
        return ta, tb

    res = {"device": ctx.device_info()[0], "stamp": stamp.current()}
    # ---- (b) the example frames: one batched call against 121 single calls
    w_pts, w_app, frames, K, cam = example_frames()
    m = vo.Map(ctx)
    m.update(w_pts, w_app)
    F, cap = len(frames), max(len(p) for p, _ in frames)
    uv = np.zeros((F, cap, 2), np.float32); app = np.zeros((F, cap, 10), np.float32)
    n = np.array([len(p) for p, _ in frames], np.int32)
    for f, (p, q) in enumerate(frames):
        uv[f, : n[f]] = p; app[f, : n[f]] = q
    d_uv, d_app, d_n, d_T, d_st = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(n), ctx.alloc(64 * F), ctx.alloc(32 * F)
    Kc = np.ascontiguousarray(K.T).ravel()
    prm = vo.RansacParams(64, 2.0, 0)

    def batched():
        rc = lib.vo_map_localise_batch_dev(m.h, I(F), *map(I, cam), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n),
                                           C.byref(prm), C.c_float(10000.0), I(50), I(6), None, V(d_T), V(d_st))
        assert rc == 0, lib.vo_last_error()

    def singles():
        for f in range(F):
            rc = lib.vo_map_localise_dev(m.h, *map(I, cam), Kc.ctypes.data_as(V), V(d_uv + 8 * cap * f), V(d_app + 40 * cap * f), I(cap),
                                         V(d_n + 4 * f), C.byref(prm), C.c_float(10000.0), I(50), I(6), None, V(d_T + 64 * f),
                                         V(d_st + 32 * f))
            assert rc == 0, lib.vo_last_error()

    if a.trace_run:
        batched(); singles(); sync()
        return
    tb, ts = alternate(batched, singles, 10)
    st = np.zeros((F, 8), np.int32); ctx.d2h(st, d_st)
    res["localise_example_frames"] = {
        "frames": F, "rows_per_frame": [int(n.min()), int(n.max())], "hypotheses": 64, "threshold_px": 2.0, "rounds": 50,
        "batched_call_us": round(statistics.median(tb), 1), "single_calls_us": round(statistics.median(ts), 1),
        "single_over_batched": round(statistics.median(ts) / statistics.median(tb), 2),
        "batched_runs_us": [round(x, 1) for x in tb], "single_runs_us": [round(x, 1) for x in ts], "calls_per_run": 10,
        "statuses_all_ok": bool((st[:, 0] == 0).all())}
    m.close()
    for d in (d_uv, d_app, d_n, d_T, d_st):
        ctx.free(d)
    # ---- (a) lookup against update: `rows` rows, all present, in a map of `entries` entries
    rng = np.random.default_rng(1)
    E, R = a.entries, a.rows
    big_app = rng.uniform(-1, 1, (E, 10)).astype(np.float32)
    big_pts = rng.uniform(-5, 5, (E, 3)).astype(np.float32)
    # room for 64 more clouds: the host's bound of the size grows by a cloud per update and is refreshed from the device (one
    # small read-back) only when it would pass the capacity -- once in 64 calls here; the lookup probes the same table
    m = vo.Map(ctx, capacity=E + 64 * R)
    for lo in range(0, E, R):
        m.update(big_pts[lo: lo + R], big_app[lo: lo + R])
    size = len(m)
    pick = rng.permutation(E)[:R]
    d_q, d_p = ctx.to_device(big_app[pick]), ctx.to_device(big_pts[pick])
    d_pairs, d_cnt, d_xyz = ctx.alloc(8 * R), ctx.alloc(16), ctx.alloc(12 * R)

    def lookup():
        assert lib.vo_map_lookup_dev(m.h, V(d_q), I(R), None, V(d_pairs), V(d_cnt), None, None, None) == 0

    def lookup_gather():
        assert lib.vo_map_lookup_dev(m.h, V(d_q), I(R), None, V(d_pairs), V(d_cnt), V(d_xyz), None, None) == 0

    def update():
        assert lib.vo_map_update_dev(m.h, V(d_p), V(d_q), I(R), None, None) == 0

    tl, tu = alternate(lookup, update, a.calls)
    tg, _ = alternate(lookup_gather, update, a.calls)
    cnt = np.zeros(4, np.int32); ctx.d2h(cnt, d_cnt)
    res["lookup_vs_update"] = {
        "map_entries": size, "map_entries_after": len(m), "map_capacity": E + 64 * R, "rows": R, "rows_found": int(cnt[0]), "calls_per_run": a.calls,
        "lookup_us": round(statistics.median(tl), 2), "update_us": round(statistics.median(tu), 2),
        "lookup_with_gather_us": round(statistics.median(tg), 2),
        "lookup_over_update": round(statistics.median(tl) / statistics.median(tu), 3),
        "lookup_runs_us": [round(x, 2) for x in tl], "update_runs_us": [round(x, 2) for x in tu],
        "lookup_with_gather_runs_us": [round(x, 2) for x in tg]}
    m.close()
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
