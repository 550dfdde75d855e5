"""Time the joint adjustment (vox_map_bundle_batch_dev) beside the alternation.

  python tools/map_bundle_rate.py [--big-frames 200] [--big-visible 50000] [--out profiles/map_bundle_rate.json]
      Two shapes, the window of tools/map_adjust_rate.py: the 121 frames of tests/golden/example_data against the map of
      world.dat, and synth.sequence(n_frames, n_visible) against its own map; poses and points pushed off by the same seeded
      amounts, the first and the last frame held.  Every run restores the start (poses and map points, outside the timed
      span), synchronises, makes ONE call and synchronises again; medians of 5 runs:
        round_n_cg_{1,16,64}_us   one round with cg_tol = 0, so that PCG takes all n_cg iterations (the record's count is checked)
        cg_iteration_us           (round_n_cg_64_us - round_n_cg_16_us) / 48: what one PCG iteration adds
        zero_rounds_us            n_rounds = 0: lookup, lists, the start's evaluation and the end's
        alternation_6_sweeps_us   vo_map_adjust_batch_dev, 6 sweeps of 2 + 2 rounds, and the total cost it reaches
        joint_to_that_cost        the fewest rounds (n_cg 64, cg_tol 1e-8, lambda0 1e-4) after which the joint call's cost is below
                                  the alternation's, that call's time and cost -- or, if 6 rounds do not get there, what they reach
      Costs are the calls' own: cost_after of the joint call; for the alternation, cost_before of a 0-round joint call on the state
      it left (the same evaluation)."""
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
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_bundle_rate.json"))
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

    def shape(K, start_pts, app_map, frames, start_poses):
        F, cap = len(frames), max(len(p) for p, _ in frames)
        uv = np.zeros((F, cap, 2), np.float32); app = np.full((F, cap, 10), np.nan, np.float32)
        n = np.array([len(p) for p, _ in frames], np.int32)
        for f, (p, q) in enumerate(frames):
            uv[f, : n[f]] = p; app[f, : n[f]] = q
        T = np.stack([np.ascontiguousarray(np.asarray(X, np.float32).T).ravel() for X in start_poses])
        fixed = np.zeros(F, np.uint8); fixed[0] = fixed[-1] = 1
        start_pts = np.ascontiguousarray(start_pts, np.float32)
        M = len(start_pts)
        m = vo.Map(ctx, capacity=M)
        for lo in range(0, M, 100000):
            m.update(start_pts[lo: lo + 100000], app_map[lo: lo + 100000])
        assert len(m) == M
        d_xyz = C.c_void_p()
        assert lib.vo_map_dev_ptrs(m.h, C.byref(d_xyz), None, None) == 0
        d_uv, d_app, d_n, d_T, d_fixed = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(n), ctx.to_device(T), ctx.to_device(fixed)
        d_rounds, d_stats, d_adj = ctx.alloc(40 * 8), ctx.alloc(64), ctx.alloc(96 * 6)
        Kc = np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()

        def restore():
            ctx.h2d(d_T, T); ctx.h2d(d_xyz.value, start_pts)

        def bundle(n_rounds, n_cg, cg_tol=1e-8):
            prm = vo.MapBundleParams(n_rounds, n_cg, cg_tol, 1e-4, 3, 3, 0.0)
            rc = lib.vox_map_bundle_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T),
                                              V(d_fixed), C.byref(prm), None, None, V(d_rounds), V(d_stats))
            assert rc == 0, lib.vo_last_error()

        def alternation():
            prm = vo.MapAdjustParams(6, 2, 2, 3, 3, 0.0, 0.0)
            rc = lib.vo_map_adjust_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T),
                                             V(d_fixed), C.byref(prm), None, None, V(d_adj))
            assert rc == 0, lib.vo_last_error()

        def stats():
            st = vo.MapBundleStats(); raw = np.zeros(48, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 48)
            return st.as_dict()

        def rounds(k):
            rec = (vo.MapBundleRound * k)(); raw = np.zeros(40 * k, np.uint8); ctx.d2h(raw, d_rounds); C.memmove(rec, raw.ctypes.data, 40 * k)
            return [rec[i].as_dict() for i in range(k)]

        def timed(f):
            runs = []
            for _ in range(6):                                # the first run warms up (and sizes the workspaces)
                restore(); sync()
                t = time.perf_counter()
                f()
                sync()
                runs.append((time.perf_counter() - t) * 1e6)
            return round(statistics.median(runs[1:]), 1), [round(x, 1) for x in runs[1:]]

        out = {"frames": F, "n_max": int(cap), "map_entries": M}
        out["zero_rounds_us"], out["zero_rounds_runs_us"] = timed(lambda: bundle(0, 1))
        st = stats()
        out.update(observations=st["n_obs"], free_frames=st["n_free_frames"], free_points=st["n_free_points"], cost_start=st["cost_before"])
        for n_cg in (1, 16, 64):
            out[f"round_n_cg_{n_cg}_us"], out[f"round_n_cg_{n_cg}_runs_us"] = timed(lambda: bundle(1, n_cg, 0.0))
            out[f"round_n_cg_{n_cg}_iterations_taken"] = rounds(1)[0]["cg_iterations"]
        out["cg_iteration_us"] = round((out["round_n_cg_64_us"] - out["round_n_cg_16_us"]) / 48.0, 2)
        out["alternation_6_sweeps_us"], out["alternation_6_sweeps_runs_us"] = timed(alternation)
        bundle(0, 1); sync()                                  # evaluates the state the alternation left
        target = stats()["cost_before"]
        out["alternation_6_sweeps_cost"] = target
        reached = None
        for k in range(1, 7):
            us, runs = timed(lambda: bundle(k, 64))
            st, rec = stats(), rounds(k)
            reached = {"rounds": k, "us": us, "runs_us": runs, "cost": st["cost_after"], "status": vo.MAP_BUNDLE_STATUS[st["status"]],
                       "cg_iterations": [r["cg_iterations"] for r in rec], "accepted": [r["accepted"] for r in rec],
                       "below_the_alternation": bool(st["cost_after"] < target)}
            if reached["below_the_alternation"]:
                break
        out["joint_to_that_cost"] = reached
        m.close()
        for d in (d_uv, d_app, d_n, d_T, d_fixed, d_rounds, d_stats, d_adj):
            ctx.free(d)
        return out

    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: wall time of one call between two synchronises, host launches included",
           "not_measured": "no kernel trace or counter run was taken: the cost of a PCG iteration is the difference of two calls"}
    E = R.example_problem()
    res["example_data"] = shape(E["K"], R.perturbed(E["world_pts"], 5, 0.02), E["world_app"], E["frames"], P.push(E["poses"], 6, 0.01, 0.005))
    print("example data done", flush=True)
    if not a.skip_big:
        s = vo.synth.sequence(n_frames=a.big_frames, n_visible=a.big_visible)
        print("sequence made", flush=True)
        truth = [np.linalg.inv(vo.synth.planar_pose(*x) @ vo.synth.CAM_IN_ROBOT) for x in s["gt"]]
        frames = [(f["pts"], f["app"]) for f in s["frames"]]
        res["synthetic_sequence"] = shape(s["K"], R.perturbed(s["world_xyz"], 1, 0.02), s["world_app"], frames, P.push(truth, 2, 0.01, 0.005))
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
