"""Time voe_map_nearest_batch_dev beside the exact lookup and beside the only route the library had
before it.

  python tools/map_nearest_rate.py [--frames 200] [--rows 50000] [--entries 800000] [--sigma 0.005] [--out profiles/map_nearest_timing.json]
      A map of `entries` random appearances U(-1, 1)^10; every frame holds `rows` rows, each a copy of a (seeded) entry pushed by
      N(0, sigma).  Every run synchronises, makes ONE call and synchronises again.  The figures alternate within every round --
      nearest, index, lookup, matcher, nearest, ... -- and are the medians of 5 rounds after one that warms up and sizes the
      workspaces:
        nearest_us          the call over all frames (radius 0.1, ratio 0.8, unique 0): index build + search + finish
        nearest_unique_us   the same with unique 1 (the claim words and their memsets on top)
        index_us            the same call on ONE frame of ONE row: the index build, and launches of a search that has nothing to do
        search_us           nearest_us - index_us: the search and the finishing launch over all rows
        lookup_us           (a) the exact floor: vo_map_lookup_batch_dev of the CLEAN rows at the same shape
        matcher_8_us        (b) the parent's route: vo_match_appearances_dev(map's appearances, frame's rows) for 8 frames, one
                            call each; matcher_scaled_us = matcher_8_us * frames / 8 (the calls are independent and equal in
                            size, so the scaling is linear by construction)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--entries", type=int, default=800000)
    ap.add_argument("--sigma", type=float, default=0.005)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_nearest_timing.json"))
    a = ap.parse_args()
    import numpy as np

    import __graft_entry__ as g
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    lib, V, I, S = ctx.lib, C.c_void_p, C.c_int, C.c_size_t

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    F, N, M = a.frames, a.rows, a.entries
    rng = np.random.default_rng(7)
    app_map = rng.uniform(-1, 1, (M, 10)).astype(np.float32)
    m = vo.Map(ctx, capacity=M)
    for lo in range(0, M, 100000):
        m.update(np.zeros((len(app_map[lo: lo + 100000]), 3), np.float32), app_map[lo: lo + 100000])
    assert len(m) == M
    d_app, d_clean = ctx.alloc(40 * F * N + 16), ctx.alloc(40 * F * N + 16)
    for f in range(F):                                        # frame by frame: the host never holds all rows
        ids = rng.integers(0, M, N)
        ctx.h2d(d_clean + 40 * f * N, app_map[ids])
        ctx.h2d(d_app + 40 * f * N, (app_map[ids] + rng.normal(0, a.sigma, (N, 10))).astype(np.float32))
    print("frames made", flush=True)
    d_ent, d_st, d_d2, d_out, d_stats = ctx.alloc(4 * F * N + 16), ctx.alloc(4 * F * N + 16), ctx.alloc(4 * F * N + 16), ctx.alloc(40 * F * N + 16), ctx.alloc(64)
    d_pairs, d_cnt = ctx.alloc(8 * F * N + 16), ctx.alloc(4 * F + 16)
    px, pa, ph = V(), V(), V()
    assert lib.vo_map_dev_ptrs(m.h, C.byref(px), C.byref(pa), C.byref(ph)) == 0
    K = min(8, F)

    def nearest(unique, frames=F, rows=N):
        prm = vo.MapNearestParams(0.1, 0.8, unique, 0)
        rc = lib.voe_map_nearest_batch_dev(m.h, I(frames), V(d_app), S(N), I(rows), None, C.byref(prm), V(d_ent), V(d_st), V(d_d2), V(d_out), V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def lookup():
        rc = lib.vo_map_lookup_batch_dev(m.h, I(F), V(d_clean), S(N), I(N), None, V(d_pairs), V(d_cnt), None, None, V(d_ent))
        assert rc == 0, lib.vo_last_error()

    def matcher():
        for f in range(K):
            rc = lib.vo_match_appearances_dev(ctx.h, pa, I(M), V(d_app + 40 * f * N), I(N), C.c_float(0.1), V(d_pairs + 8 * f * N), V(d_cnt + 4 * f))
            assert rc == 0, lib.vo_last_error()

    what = {"nearest_us": lambda: nearest(0), "index_us": lambda: nearest(0, 1, 1), "lookup_us": lookup, "matcher_8_us": matcher,
            "nearest_unique_us": lambda: nearest(1)}
    runs = {k: [] for k in what}
    for r in range(6):                                        # the first round warms up (and sizes the workspaces)
        for k, f in what.items():
            sync()
            t = time.perf_counter()
            f()
            sync()
            runs[k].append((time.perf_counter() - t) * 1e6)
    out = {"frames": F, "rows_per_frame": N, "map_entries": M, "sigma": a.sigma, "radius": 0.1, "ratio": 0.8, "matcher_frames": K}
    for k in what:
        out[k] = round(statistics.median(runs[k][1:]), 1)
        out[k.replace("_us", "_runs_us")] = [round(x, 1) for x in runs[k][1:]]
    nearest(0)
    sync()
    st = vo.MapNearestStats(); raw = np.zeros(32, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 32)
    out["nearest_stats"] = st.as_dict()
    cnt = np.zeros(K, np.int32); ctx.d2h(cnt, d_cnt)
    out["matcher_pairs_per_frame"] = cnt.tolist()
    out["search_us"] = round(out["nearest_us"] - out["index_us"], 1)
    out["matcher_scaled_us"] = round(out["matcher_8_us"] * F / K, 1)
    out["nearest_over_lookup"] = round(out["nearest_us"] / out["lookup_us"], 2)
    out["matcher_scaled_over_nearest"] = round(out["matcher_scaled_us"] / out["nearest_us"], 2)
    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: wall time of one call (the matcher: 8 calls) between two synchronises, host launches included",
           "not_measured": "no kernel trace or counter run was taken: search_us is a difference of two calls, matcher_scaled_us a product",
           "shape": out}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
