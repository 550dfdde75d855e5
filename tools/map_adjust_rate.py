"""Time the pose half of the map's adjustment and one sweep of the alternation.

  python tools/map_adjust_rate.py [--big-frames 200] [--big-visible 50000] [--out profiles/map_adjust_rate.json]
      Two shapes: the 121 frames of tests/golden/example_data against the map of world.dat, and synth.sequence(n_frames,
      n_visible) against its own map; poses and points pushed off by a seeded amount.  Per shape, medians of 5 runs after
      warm-up, every run ending in a synchronise:
        poses_us           vo_map_refine_poses_batch_dev, 10 rounds, out of place (the input stays: every call does the same work)
        poses_0_rounds_us  the same with n_rounds = 0: lookup + ONE evaluation + statistics
        round_us           (poses_us - poses_0_rounds_us) / 10: what a round adds
        sweep_us           vo_map_adjust_batch_dev, one sweep of 2 + 2 rounds, in place (poses and map move on from call to call;
                           the launches and their sizes stay the same)
        localise_us        vo_map_localise_batch_dev with n_hypotheses = 0 and 10 rounds from the same start poses, for context: it
                           minimises the solver's gated float32 cost, not this one
      The CPU restatement's time for the pose half is recorded for scale (on the second shape: a sample of frames, scaled)."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big-frames", type=int, default=200)
    ap.add_argument("--big-visible", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_adjust_rate.json"))
    a = ap.parse_args()
    import numpy as np

    import __graft_entry__ as g
    import map_pose_refine_restatement as P
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

    def shape(K, cam, start_pts, app_map, frames, start_poses, calls):
        F, cap = len(frames), max(len(p) for p, _ in frames)
        uv = np.zeros((F, cap, 2), np.float32); app = np.full((F, cap, 10), np.nan, np.float32)
        n = np.array([len(p) for p, _ in frames], np.int32)
        for f, (p, q) in enumerate(frames):
            uv[f, : n[f]] = p; app[f, : n[f]] = q
        T = np.stack([np.ascontiguousarray(np.asarray(X, np.float32).T).ravel() for X in start_poses])
        fixed = np.zeros(F, np.uint8); fixed[0] = fixed[-1] = 1
        M = len(start_pts)
        m = vo.Map(ctx, capacity=M)
        for lo in range(0, M, 100000):
            m.update(start_pts[lo: lo + 100000], app_map[lo: lo + 100000])
        assert len(m) == M
        d_uv, d_app, d_n, d_T, d_fixed = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(n), ctx.to_device(T), ctx.to_device(fixed)
        d_T2, d_Tout, d_status, d_stats = ctx.to_device(T), ctx.alloc(64 * F), ctx.alloc(4 * F), ctx.alloc(64)
        d_adj, d_lst = ctx.alloc(96), ctx.alloc(32 * F)
        Kc = np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()

        def poses(n_rounds):
            prm = vo.MapPoseRefineParams(n_rounds, 3, 0.0, 0.0)
            rc = lib.vo_map_refine_poses_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T),
                                                   V(d_fixed), C.byref(prm), V(d_Tout), V(d_status), None, V(d_stats))
            assert rc == 0, lib.vo_last_error()

        def sweep():
            prm = vo.MapAdjustParams(1, 2, 2, 3, 3, 0.0, 0.0)
            rc = lib.vo_map_adjust_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T2),
                                             V(d_fixed), C.byref(prm), None, None, V(d_adj))
            assert rc == 0, lib.vo_last_error()

        rp = vo.RansacParams(0, 2.0, 0)

        def localise():
            rc = lib.vo_map_localise_batch_dev(m.h, I(F), *map(I, cam), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n),
                                               C.byref(rp), C.c_float(10000.0), I(10), I(6), V(d_T), V(d_Tout), V(d_lst))
            return rc

        refused = None
        if localise() != 0:                                   # (the batched solver has limits of its own: then the context figure is missing)
            refused = lib.vo_last_error().decode(errors="replace")
        for _ in range(3):
            poses(10); poses(0)
            if refused is None:
                localise()
        t10, t0, tl, ts = [], [], [], []
        for _ in range(5):                                    # alternating, so that a drift of the machine hits all alike
            t10.append(timed(lambda: poses(10), calls)); t0.append(timed(lambda: poses(0), calls))
            if refused is None:
                tl.append(timed(localise, calls))
        print("pose half timed", flush=True)
        poses(10); sync()
        st = vo.MapPoseRefineStats(); raw = np.zeros(48, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 48)
        sweep(); sync()                                       # (sizes the workspaces)
        for _ in range(5):
            ts.append(timed(sweep, max(calls // 4, 2)))
        med = statistics.median
        per_round = (med(t10) - med(t0)) / 10.0
        out = {"frames": F, "n_max": int(cap), "map_entries": M, "observations": st.n_obs, "by_status": list(st.by_status), "rounds": 10,
               "calls_per_run": calls, "poses_us": round(med(t10), 1), "poses_0_rounds_us": round(med(t0), 1), "round_us": round(per_round, 2),
               "observation_rounds_per_second": round(st.n_obs / (per_round * 1e-6)) if per_round > 0 else None,
               "sweep_2_plus_2_rounds_us": round(med(ts), 1), "localise_no_ransac_10_rounds_us": round(med(tl), 1) if tl else "not measured: " + str(refused),
               "poses_runs_us": [round(x, 1) for x in t10], "poses_0_rounds_runs_us": [round(x, 1) for x in t0],
               "sweep_runs_us": [round(x, 1) for x in ts], "localise_runs_us": [round(x, 1) for x in tl]}
        m.close()
        for d in (d_uv, d_app, d_n, d_T, d_fixed, d_T2, d_Tout, d_status, d_stats, d_adj, d_lst):
            ctx.free(d)
        return out

    res = {"device": ctx.device_info()[0], "stamp": stamp.current(), "per_observation_terms": "double",
           "measured": "every *_us figure below, on the device named above; cpu_restatement_* on the host of the same run",
           "not_measured": "no kernel trace or counter run was taken: the split of a call into lookup / rounds is the 0-round difference alone"}
    E = R.example_problem()
    start = P.push(E["poses"], 6, 0.01, 0.005)
    pts = R.perturbed(E["world_pts"], 5, 0.02)
    d = __import__("map_localise_restatement").example_data()
    res["example_data"] = shape(E["K"], d["cam"], pts, E["world_app"], E["frames"], start, a.calls * 5)
    t = time.perf_counter()
    P.refine_poses(E["K"], pts, E["world_app"], E["frames"], start)
    res["example_data"]["cpu_restatement_poses_s"] = round(time.perf_counter() - t, 3)
    print("example data done", flush=True)
    s = vo.synth.sequence(n_frames=a.big_frames, n_visible=a.big_visible)
    print("sequence made", flush=True)
    truth = [np.linalg.inv(vo.synth.planar_pose(*x) @ vo.synth.CAM_IN_ROBOT) for x in s["gt"]]
    big_start = P.push(truth, 2, 0.01, 0.005)
    big_pts = R.perturbed(s["world_xyz"], 1, 0.02)
    frames = [(f["pts"], f["app"]) for f in s["frames"]]
    res["synthetic_sequence"] = shape(s["K"], (s["rows"], s["cols"], s["z_near"], s["z_far"]), big_pts, s["world_app"], frames, big_start,
                                      max(a.calls // 4, 3))
    # the restatement on 3 frames (the ids are known: no lookup), scaled by observations
    t = time.perf_counter()
    n_obs = 0
    for f in range(min(3, len(frames))):
        ids = np.asarray(s["frames"][f]["ids"])
        P.refine_pose(s["K"].astype(np.float64), big_start[f], s["frames"][f]["pts"], big_pts[ids], 10, 0.0, 0.0)
        n_obs += len(ids)
    dt = time.perf_counter() - t
    res["synthetic_sequence"]["cpu_restatement_sample"] = {"frames": min(3, len(frames)), "observations": n_obs, "seconds": round(dt, 3),
                                                           "scaled_to_all_observations_s": round(dt / max(n_obs, 1) * res["synthetic_sequence"]["observations"], 1)}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
