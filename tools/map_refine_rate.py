"""Time the structure-only refinement of the device map.

  python tools/map_refine_rate.py [--big-frames 200] [--big-visible 50000] [--out profiles/map_refine_rate.json]
      Two shapes: the 121 frames of tests/golden/example_data against the map of world.dat, and synth.sequence(n_frames,
      n_visible) against its own map, both pushed off by a seeded amount and refined out of place (the map stays, every call
      does the same work).  Per shape, medians of 5 runs after warm-up, every run ending in a synchronise:
        call_us          vo_map_refine_batch_dev, 10 rounds
        call_0_rounds_us the same with n_rounds = 0: lookup + lists + ONE evaluation + statistics
        lookup_us        vo_map_lookup_batch_dev alone with the entry of every position
        round_us         (call_us - call_0_rounds_us) / 10: what a round adds
      and from them observations per second and the bytes a round moves per observation, against the 12 B (4 B key + 8 B
      pixel) the kernel's source implies.  The CPU restatement's time is recorded for scale.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/map_refine_rate.py --trace-run
      three calls per shape alone, for the trace
  python tools/map_refine_rate.py --split DIR/*/*kernel_stats.csv      -> the traced run's kernels folded into lookup / lists / refine"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = [("lookup", ("map_lookup",)), ("lists", ("map_refine_count", "map_refine_offsets", "map_refine_scatter", "map_refine_order")),
          ("refine", ("map_refine_kernel",)), ("statistics", ("map_refine_stats",)), ("scan", ("scan_counts_kernel",))]
BYTES_PER_OBS_ROUND = 12                                      # map_refine_kernel: 4 B key + 8 B pixel; the pose comes from LDS


def split(path):
    out = {}
    for r in csv.DictReader(open(path)):
        name, calls, total = r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])
        stage = next((s for s, keys in STAGES if any(k in name for k in keys)), "other")
        o = out.setdefault(stage, {"kernels": {}, "total_us": 0.0})
        o["kernels"][name.replace("void ", "").split("(")[0]] = {"calls": calls, "avg_us": round(total / calls / 1e3, 2)}
        o["total_us"] = round(o["total_us"] + total / 1e3, 2)
    print(json.dumps({"kernel_stats": os.path.basename(path), "stages": out}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big-frames", type=int, default=200)
    ap.add_argument("--big-visible", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_refine_rate.json"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--split", default=None)
    a = ap.parse_args()
    if a.split:
        return split(a.split)
    import numpy as np

    import __graft_entry__ as g
    import map_refine_restatement as R
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

    def shape(name, K, start, app_map, frames, poses, truth, calls):
        F, cap = len(frames), max(len(p) for p, _ in frames)
        uv = np.zeros((F, cap, 2), np.float32); app = np.full((F, cap, 10), np.nan, np.float32)
        n = np.array([len(p) for p, _ in frames], np.int32)
        for f, (p, q) in enumerate(frames):
            uv[f, : n[f]] = p; app[f, : n[f]] = q
        T = np.stack([np.ascontiguousarray(np.asarray(X, np.float32).T).ravel() for X in poses])
        M = len(start)
        m = vo.Map(ctx, capacity=M)
        for lo in range(0, M, 100000):
            m.update(start[lo: lo + 100000], app_map[lo: lo + 100000])
        assert len(m) == M
        d_uv, d_app, d_n, d_T = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(n), ctx.to_device(T)
        d_status, d_xyz, d_stats = ctx.alloc(4 * M), ctx.alloc(12 * M), ctx.alloc(64)
        d_pairs, d_hits, d_ent = ctx.alloc(8 * F * cap), ctx.alloc(4 * F), ctx.alloc(4 * F * cap)
        Kc = np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()

        def call(n_rounds):
            prm = vo.MapRefineParams(n_rounds, 3, 0.0, 0.0)
            rc = lib.vo_map_refine_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T),
                                             C.byref(prm), V(d_status), V(d_xyz), V(d_stats))
            assert rc == 0, lib.vo_last_error()

        def lookup():
            assert lib.vo_map_lookup_batch_dev(m.h, I(F), V(d_app), S(cap), I(cap), V(d_n), V(d_pairs), V(d_hits), None, None, V(d_ent)) == 0

        if a.trace_run:
            for _ in range(3):
                call(10)
            sync()
            return None
        for _ in range(3):
            call(10); call(0); lookup()
        t10, t0, tl = [], [], []
        for _ in range(5):                                    # alternating, so that a drift of the machine hits all three alike
            t10.append(timed(lambda: call(10), calls)); t0.append(timed(lambda: call(0), calls)); tl.append(timed(lookup, calls))
        call(10); sync()
        st = vo.MapRefineStats(); raw = np.zeros(48, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 48)
        status = np.zeros(M, np.int32); ctx.d2h(status, d_status)
        xyz = np.zeros((M, 3), np.float32); ctx.d2h(xyz, d_xyz)
        ok = status == 0
        err = float(np.linalg.norm(xyz[ok].astype(np.float64) - truth[ok], axis=1).max()) if ok.any() else None
        med = statistics.median
        per_round = (med(t10) - med(t0)) / 10.0
        out = {"frames": F, "n_max": int(cap), "map_entries": M, "observations": st.n_obs, "by_status": list(st.by_status), "rounds": 10,
               "largest_distance_to_truth_of_ok": err, "calls_per_run": calls,
               "call_us": round(med(t10), 1), "call_0_rounds_us": round(med(t0), 1), "lookup_us": round(med(tl), 1),
               "lists_one_evaluation_statistics_us": round(med(t0) - med(tl), 1), "round_us": round(per_round, 2),
               "observations_per_second_whole_call": round(st.n_obs / (med(t10) * 1e-6)),
               "observation_rounds_per_second": round(st.n_obs / (per_round * 1e-6)) if per_round > 0 else None,
               "bytes_per_observation_per_round_source": BYTES_PER_OBS_ROUND,
               "round_GBps_at_source_bytes": round(st.n_obs * BYTES_PER_OBS_ROUND / (per_round * 1e-6) / 1e9, 2) if per_round > 0 else None,
               "call_runs_us": [round(x, 1) for x in t10], "call_0_rounds_runs_us": [round(x, 1) for x in t0],
               "lookup_runs_us": [round(x, 1) for x in tl]}
        m.close()
        for d in (d_uv, d_app, d_n, d_T, d_status, d_xyz, d_stats, d_pairs, d_hits, d_ent):
            ctx.free(d)
        return out

    res = {"device": ctx.device_info()[0], "stamp": stamp.current(), "per_observation_terms": "double",
           "note": "the split into lookup / lists / refine kernels comes from a kernel trace (--trace-run, --split), not from these host timings"}
    P = R.example_problem()
    start = R.perturbed(P["world_pts"])
    res["example_data"] = shape("example", P["K"], start, P["world_app"], P["frames"], P["poses"], P["world_pts"], a.calls * 5)
    if not a.trace_run:
        t = time.perf_counter()
        R.refine(P["K"], start, P["world_app"], P["frames"], P["poses"])
        res["example_data"]["cpu_restatement_s"] = round(time.perf_counter() - t, 3)
    s = vo.synth.sequence(n_frames=a.big_frames, n_visible=a.big_visible)
    poses = [np.linalg.inv(vo.synth.planar_pose(*x) @ vo.synth.CAM_IN_ROBOT) for x in s["gt"]]
    big_start = R.perturbed(s["world_xyz"], 1, 0.05)
    frames = [(f["pts"], f["app"]) for f in s["frames"]]
    res["synthetic_sequence"] = shape("sequence", s["K"], big_start, s["world_app"], frames, poses, s["world_xyz"], max(a.calls // 4, 3))
    if not a.trace_run:
        # the restatement on a sample of 300 landmarks with >= 3 observations (the ids are known: no lookup), scaled by observations
        obs = {}
        for f, fr in enumerate(s["frames"]):
            for i, e in enumerate(fr["ids"][:2000]):
                obs.setdefault(int(e), []).append((f, i))
        sample = [e for e, v in obs.items() if len(v) >= 3][:300]
        T = np.stack([np.asarray(X, np.float32).astype(np.float64) for X in poses])
        t = time.perf_counter()
        n_obs = 0
        for e in sample:
            fs = np.array([f for f, _ in obs[e]])
            uvs = np.stack([s["frames"][f]["pts"][i] for f, i in obs[e]])
            R.refine_point(s["K"].astype(np.float64), T[fs, :3, :3], T[fs, :3, 3], uv=uvs, p0=big_start[e], n_rounds=10, huber=0.0, damping=0.0)
            n_obs += len(fs)
        dt = time.perf_counter() - t
        res["synthetic_sequence"]["cpu_restatement_sample"] = {"landmarks": len(sample), "observations": n_obs, "seconds": round(dt, 3),
                                                               "scaled_to_all_observations_s": round(dt / max(n_obs, 1) * res["synthetic_sequence"]["observations"], 1)}
    if a.trace_run:
        return
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
