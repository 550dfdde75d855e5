"""Time the growing of the map (voe_map_grow_batch_dev) beside the nearest existing call on the same
window, vo_map_refine_batch_dev: the same lookup, the same list building, the same rounds.

  python tools/map_grow_rate.py --case open10|empty [--frames 200] [--visible 50000] [--runs 3] [--out profiles/map_grow_timing_<case>.json]
      synth.sequence(frames, visible) with its ground-truth poses against its own map.
        open10   a seeded tenth of the landmarks is taken out of the map: about 10 % of the rows are open
        empty    the map is empty: every row is open
      Every run restores the map (clear + update, outside the timed span), synchronises, makes ONE call and synchronises again;
      the median of `runs` runs after one that warms up and sizes the workspaces:
        grow_us                  the defaults of Map.grow (5 rounds, min_obs = min_frames = 3, 2 px, 2 degrees), no optional output
        grow_zero_rounds_us      the same with n_rounds = 0: the linear point alone
        grow_dry_run_us          the defaults with dry_run = 1: no append
        refine_us                the yardstick: vo_map_refine_batch_dev with 5 rounds, min_obs = 3 on the WHOLE map and the same window
  python tools/map_grow_rate.py --merge a.json b.json --out profiles/map_grow_timing.json     (no device: joins the parts)"""
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
    ap.add_argument("--case", choices=("open10", "empty"), default="open10")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--visible", type=int, default=50000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--merge", nargs="*")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        parts = [json.load(open(p)) for p in a.merge]
        res = {k: parts[0][k] for k in ("device", "stamp", "measured", "not_measured")}
        res["cases"] = {p["case"]: p["result"] for p in parts}
        assert len({json.dumps(p["stamp"], sort_keys=True) for p in parts}) == 1, "the parts were measured on different sources"
        open(a.out or os.path.join(ROOT, "profiles", "map_grow_timing.json"), "w").write(json.dumps(res, indent=1) + "\n")
        return
    import numpy as np

    import __graft_entry__ as g
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    lib, V, I, S = ctx.lib, C.c_void_p, C.c_int, C.c_size_t

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    s = vo.synth.sequence(n_frames=a.frames, n_visible=a.visible)
    print("sequence made", flush=True)
    poses = [np.linalg.inv(vo.synth.planar_pose(*x) @ vo.synth.CAM_IN_ROBOT) for x in s["gt"]]
    frames = [(f["pts"], f["app"]) for f in s["frames"]]
    F, cap = len(frames), max(len(p) for p, _ in frames)
    uv = np.zeros((F, cap, 2), np.float32); app = np.full((F, cap, 10), np.nan, np.float32)
    n = np.array([len(p) for p, _ in frames], np.int32)
    for f, (p, q) in enumerate(frames):
        uv[f, : n[f]] = p; app[f, : n[f]] = q
    T = np.stack([np.ascontiguousarray(np.asarray(X, np.float32).T).ravel() for X in poses])
    pts, app_map = np.ascontiguousarray(s["world_xyz"], np.float32), np.ascontiguousarray(s["world_app"], np.float32)
    M = len(pts)
    keep = np.ones(M, bool)
    if a.case == "open10":
        keep[np.random.default_rng(1).choice(M, M // 10, replace=False)] = False
    m = vo.Map(ctx, capacity=M)

    def restore(which):
        m.clear()
        idx = np.nonzero(which)[0]
        for lo in range(0, len(idx), 100000):
            m.update(pts[idx[lo: lo + 100000]], app_map[idx[lo: lo + 100000]])

    d_uv, d_app, d_n, d_T, d_stats = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(n), ctx.to_device(T), ctx.alloc(128)
    Kc = np.ascontiguousarray(np.asarray(s["K"], np.float32).T).ravel()

    def grow(n_rounds=5, dry=False):
        prm = vo.MapGrowParams(n_rounds, 3, 3, 0.0, 0.0, 2.0, 0.0, 2.0, 0, int(dry))
        rc = lib.voe_map_grow_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T), C.byref(prm),
                                        None, None, I(0), V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def yardstick():
        prm = vo.MapRefineParams(5, 3, 0.0, 0.0)
        rc = lib.vo_map_refine_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(cap), V(d_app), S(cap), I(cap), V(d_n), V(d_T),
                                         C.byref(prm), None, None, V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def stats():
        st = vo.MapGrowStats(); raw = np.zeros(96, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 96)
        return st.as_dict()

    def timed(f, which):
        runs = []
        for _ in range(a.runs + 1):                           # the first run warms up (and sizes the workspaces)
            restore(which)
            sync()
            t = time.perf_counter()
            f()
            sync()
            runs.append((time.perf_counter() - t) * 1e6)
        return round(statistics.median(runs[1:]), 1), [round(x, 1) for x in runs[1:]]

    start = keep if a.case == "open10" else np.zeros(M, bool)
    out = {"frames": F, "n_max": int(cap), "rows": int(n.sum()), "world_entries": M, "map_entries_before": int(start.sum())}
    out["grow_us"], out["grow_runs_us"] = timed(grow, start)
    st = stats()
    out.update(status=vo.MAP_GROW_STATUS[st["status"]], n_live=st["n_live"], n_hits=st["n_hits"], n_open=st["n_open"], n_tracks=st["n_tracks"],
               n_added=st["n_added"], n_after=st["n_after"], by_verdict=st["by_verdict"], open_fraction=round(st["n_open"] / max(st["n_live"], 1), 4))
    assert len(m) == st["n_after"]
    print("grow timed", flush=True)
    out["grow_zero_rounds_us"], out["grow_zero_rounds_runs_us"] = timed(lambda: grow(0), start)
    out["grow_dry_run_us"], out["grow_dry_run_runs_us"] = timed(lambda: grow(5, True), start)
    print("variants timed", flush=True)
    out["refine_us"], out["refine_runs_us"] = timed(yardstick, np.ones(M, bool))
    res = {"device": ctx.device_info()[0], "stamp": stamp.current(), "case": a.case, "result": out,
           "measured": "every *_us figure, on the device named: wall time of one call between two synchronises, host launches included",
           "not_measured": "no kernel trace or counter run was taken: no figure here is a kernel's own time"}
    text = json.dumps(res, indent=1)
    print(text)
    path = a.out or os.path.join(ROOT, "profiles", f"map_grow_timing_{a.case}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
