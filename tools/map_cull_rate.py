"""Time the culling of landmarks (voe_map_cull_batch_dev) beside the parent's one pass over the same
observations.

  python tools/map_cull_rate.py [--big-frames 200] [--big-visible 50000] [--skip-big] [--out profiles/map_cull_rate.json]
      Two shapes: the 121 frames of tests/golden/example_data against the map of world.dat, and synth.sequence(n_frames,
      n_visible) against its own map, both with their ground-truth poses; as many landmarks as 5 % of the map, drawn (seeded)
      from those that at least three rows see, are pushed off by 0.3 per coordinate.  Every run restores the map (clear +
      update, outside the timed span), synchronises, makes ONE call and synchronises again; medians of 5 runs after one that
      warms up and sizes the workspaces:
        dry_run_us               dry_run = 1, min_obs = 1, min_frames = 1, max_rms_px = 1, the parallax test off
        dry_run_parallax_us      the same with min_parallax_deg = 1: the pairwise pass on top
        full_cull_us             dry_run = 0, the parallax test off: the staging copy, the copy back and the rehash on top
        refine_zero_rounds_us    the yardstick: vo_map_refine_batch_dev with n_rounds = 0 on the same inputs -- the same lookup,
                                 the same lists and one pass over the observations
      and, from the entry records of a dry run: observations, sum_n_obs_sq (what the pairwise pass grows with), the counts by
      verdict, and the bytes a rehash touches (12 bytes x the table's capacity)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_cull_rate.json"))
    a = ap.parse_args()
    import numpy as np

    import __graft_entry__ as g
    import map_refine_restatement as R
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    lib, V, I, S = ctx.lib, C.c_void_p, C.c_int, C.c_size_t

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    def shape(K, pts, app_map, frames, poses, seed):
        F, cap = len(frames), max(len(p) for p, _ in frames)
        uv = np.zeros((F, cap, 2), np.float32); app = np.full((F, cap, 10), np.nan, np.float32)
        n = np.array([len(p) for p, _ in frames], np.int32)
        for f, (p, q) in enumerate(frames):
            uv[f, : n[f]] = p; app[f, : n[f]] = q
        T = np.stack([np.ascontiguousarray(np.asarray(X, np.float32).T).ravel() for X in poses])
        pts, app_map = np.ascontiguousarray(pts, np.float32).copy(), np.ascontiguousarray(app_map, np.float32)
        M = len(pts)
        m = vo.Map(ctx, capacity=M)

        def restore():
            m.clear()
            for lo in range(0, M, 100000):
                m.update(pts[lo: lo + 100000], app_map[lo: lo + 100000])

        restore()
        assert len(m) == M
        d_uv, d_app, d_n, d_T = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(n), ctx.to_device(T)
        d_entry, d_stats = ctx.alloc(48 * M + 16), ctx.alloc(64)
        Kc = np.ascontiguousarray(np.asarray(K, np.float32).T).ravel()

        def cull(dry, parallax, entries=False):
            prm = vo.MapCullParams(1, 1, 1.0, 0.0, parallax, 0, int(dry))
            rc = lib.voe_map_cull_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T),
                                            C.byref(prm), None, None, V(d_entry) if entries else None, V(d_stats))
            assert rc == 0, lib.vo_last_error()

        def yardstick():
            prm = vo.MapRefineParams(0, 3, 0.0, 0.0)
            rc = lib.vo_map_refine_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T),
                                             C.byref(prm), None, None, V(d_stats))
            assert rc == 0, lib.vo_last_error()

        def stats():
            st = vo.MapCullStats(); raw = np.zeros(48, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 48)
            return st.as_dict()

        def timed(f, restoring=False):
            runs = []
            for _ in range(6):                                # the first run warms up (and sizes the workspaces)
                if restoring:
                    restore()
                sync()
                t = time.perf_counter()
                f()
                sync()
                runs.append((time.perf_counter() - t) * 1e6)
            return round(statistics.median(runs[1:]), 1), [round(x, 1) for x in runs[1:]]

        # the landmarks pushed: 5 % of the map's size, among those with three observations, found by a dry run on the clean map
        cull(True, 0.0, entries=True); sync()
        ent = np.zeros(M, vo.MAP_CULL_ENTRY_DTYPE); ctx.d2h(ent, d_entry)
        rng = np.random.default_rng(seed)
        well = np.nonzero(ent["n_obs"] >= 3)[0]
        who = rng.choice(well, min(len(well), max(M // 20, 1)), replace=False)
        pts[who] += np.float32(0.3)
        restore()
        out = {"frames": F, "n_max": int(cap), "map_entries": M, "landmarks_with_3_observations": int(len(well)), "pushed": int(len(who)),
               "sum_n_obs_sq": int((ent["n_obs"].astype(np.int64) ** 2).sum()), "largest_n_obs": int(ent["n_obs"].max())}
        out["dry_run_us"], out["dry_run_runs_us"] = timed(lambda: cull(True, 0.0), restoring=True)
        st = stats()
        out.update(observations=st["n_obs"], by_verdict=st["by_verdict"], would_keep=st["n_kept"])
        out["dry_run_parallax_us"], out["dry_run_parallax_runs_us"] = timed(lambda: cull(True, 1.0), restoring=True)
        out["by_verdict_with_parallax"] = stats()["by_verdict"]
        out["full_cull_us"], out["full_cull_runs_us"] = timed(lambda: cull(False, 0.0), restoring=True)
        st = stats()
        out.update(kept=st["n_kept"], dropped_fraction=round(1.0 - st["n_kept"] / M, 4), status=vo.MAP_CULL_STATUS[st["status"]])
        assert len(m) == st["n_kept"]
        restore()
        out["refine_zero_rounds_us"], out["refine_zero_rounds_runs_us"] = timed(yardstick, restoring=True)
        tcap = 1024
        while tcap < 2 * M + 2 * (M >> 2):
            tcap <<= 1
        out["rehash_bytes"] = 12 * tcap
        out["staging_bytes_each_way"] = 52 * out["kept"]
        m.close()
        for d in (d_uv, d_app, d_n, d_T, d_entry, d_stats):
            ctx.free(d)
        return out

    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: wall time of one call between two synchronises, host launches included",
           "not_measured": "no kernel trace or counter run was taken: what the pairwise pass, the staging copy and the rehash cost is the "
                           "difference of two calls, not a kernel's own time"}
    E = R.example_problem()
    res["example_data"] = shape(E["K"], E["world_pts"], E["world_app"], E["frames"], E["poses"], 1)
    print("example data done", flush=True)
    if not a.skip_big:
        s = vo.synth.sequence(n_frames=a.big_frames, n_visible=a.big_visible)
        print("sequence made", flush=True)
        truth = [np.linalg.inv(vo.synth.planar_pose(*x) @ vo.synth.CAM_IN_ROBOT) for x in s["gt"]]
        frames = [(f["pts"], f["app"]) for f in s["frames"]]
        res["synthetic_sequence"] = shape(s["K"], s["world_xyz"], s["world_app"], frames, truth, 2)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
