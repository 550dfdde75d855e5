"""Time voe_map_guided_batch_dev beside voe_map_nearest_batch_dev and the exact lookup, on the same arrays
in the same session.

  python tools/map_guided_rate.py [--frames 200] [--rows 50000] [--px 8] [--sigma 0.005] [--rounds 5] [--z_vis 5] [--out profiles/map_guided_timing.json]
      synth.sequence with `frames` frames of about `rows` visible landmarks each against its own map (every landmark of the
      sequence, its true position).  Every appearance is pushed by N(0, sigma); the priors are the true poses pushed by a fixed
      motion (0.01, -0.005, 0.01 in translation, 0.002 rad about the camera's y: a few pixels).  Every run synchronises, makes ONE
      call and synchronises again.  The figures alternate within every round -- guided, nearest, lookup, guided, ... -- and are the
      medians of `rounds` rounds after one that warms up and sizes the workspaces:
        guided_us           voe_map_guided_batch_dev over all frames (radius_px, radius 0.1, ratio 0.8, unique 0): per group of
                            frames the index (box, count, scan, place) and the search, then the finish
        guided_unique_us    the same with unique 1 (the claim words and their memsets on top)
        guided_zvis_us      guided_us with z_far = z_vis, the depth beyond which the sequence makes no row, in place of the camera
                            file's z_far (26, which the generator sets for another purpose): the landmarks between the two depths
                            project into the image, nobody measures them, and every one of them inside a row's window is tested
        nearest_us          voe_map_nearest_batch_dev on the same pushed rows (radius 0.1, ratio 0.8, unique 0)
        lookup_us           the exact floor: vo_map_lookup_batch_dev of the CLEAN rows at the same shape
      and from the call's statistics n_gated / n_live (entries tested per row) and n_in_view / n_frames (records per frame)."""
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
    ap.add_argument("--px", type=float, default=8.0)
    ap.add_argument("--sigma", type=float, default=0.005)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--z_vis", type=int, default=5, help="the depth beyond which synth.sequence makes no row")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_guided_timing.json"))
    a = ap.parse_args()
    import numpy as np

    import __graft_entry__ as g
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    lib, V, I, S = ctx.lib, C.c_void_p, C.c_int, C.c_size_t

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    seq = vo.synth.sequence(n_frames=a.frames, n_visible=a.rows)
    F, M = len(seq["frames"]), len(seq["world_xyz"])
    N = max(len(fr["ids"]) for fr in seq["frames"])
    print(f"sequence made: {F} frames, {M} landmarks, n_max {N}", flush=True)
    m = vo.Map(ctx, capacity=M)
    for lo in range(0, M, 100000):
        m.update(seq["world_xyz"][lo: lo + 100000], seq["world_app"][lo: lo + 100000])
    assert len(m) == M
    rng = np.random.default_rng(7)
    bump = np.eye(4)
    c, s = np.cos(0.002), np.sin(0.002)
    bump[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    bump[:3, 3] = (0.01, -0.005, 0.01)
    H = seq["H"].astype(np.float64)
    T = np.zeros((F, 16), np.float32)
    n = np.zeros(F, np.int32)
    d_app, d_clean, d_uv = ctx.alloc(40 * F * N + 16), ctx.alloc(40 * F * N + 16), ctx.alloc(8 * F * N + 16)
    for f, fr in enumerate(seq["frames"]):                    # frame by frame: the host never holds all rows
        k = len(fr["ids"])
        n[f] = k
        app = np.zeros((N, 10), np.float32); app[:k] = fr["app"]
        uv = np.zeros((N, 2), np.float32); uv[:k] = fr["pts"]
        ctx.h2d(d_clean + 40 * f * N, app)
        app[:k] = (fr["app"] + rng.normal(0, a.sigma, (k, 10))).astype(np.float32)
        ctx.h2d(d_app + 40 * f * N, app)
        ctx.h2d(d_uv + 8 * f * N, uv)
        T[f] = np.ascontiguousarray((bump @ np.linalg.inv(vo.synth.planar_pose(*seq["gt"][f]) @ H)).T).reshape(16)
    d_T, d_n = ctx.to_device(T), ctx.to_device(n)
    K = np.ascontiguousarray(np.asarray(seq["K"], np.float32).T).reshape(9)
    R = F * N
    d_ent, d_st, d_d2, d_g2, d_out, d_stats = (ctx.alloc(4 * R + 16), ctx.alloc(4 * R + 16), ctx.alloc(4 * R + 16), ctx.alloc(4 * R + 16),
                                              ctx.alloc(40 * R + 16), ctx.alloc(64))
    d_pairs, d_cnt = ctx.alloc(8 * R + 16), ctx.alloc(4 * F + 16)
    print("frames uploaded", flush=True)

    def guided(unique, z_far=int(seq["z_far"])):
        prm = vo.MapGuidedParams(a.px, 0.1, 0.8, unique, int(seq["z_near"]), z_far)
        rc = lib.voe_map_guided_batch_dev(m.h, I(F), K.ctypes.data_as(V), V(d_uv), S(N), V(d_app), S(N), I(N), V(d_n), V(d_T), C.byref(prm), V(d_ent),
                                          V(d_st), V(d_d2), V(d_g2), V(d_out), V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def nearest():
        prm = vo.MapNearestParams(0.1, 0.8, 0, 0)
        rc = lib.voe_map_nearest_batch_dev(m.h, I(F), V(d_app), S(N), I(N), V(d_n), C.byref(prm), V(d_ent), V(d_st), V(d_d2), V(d_out), V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def lookup():
        rc = lib.vo_map_lookup_batch_dev(m.h, I(F), V(d_clean), S(N), I(N), V(d_n), V(d_pairs), V(d_cnt), None, None, V(d_ent))
        assert rc == 0, lib.vo_last_error()

    what = {"guided_us": lambda: guided(0), "nearest_us": nearest, "lookup_us": lookup, "guided_unique_us": lambda: guided(1),
            "guided_zvis_us": lambda: guided(0, a.z_vis)}
    runs = {k: [] for k in what}
    for r in range(a.rounds + 1):                             # the first round warms up (and sizes the workspaces)
        for k, f in what.items():
            sync()
            t = time.perf_counter()
            f()
            sync()
            runs[k].append((time.perf_counter() - t) * 1e6)
    out = {"frames": F, "rows_per_frame_max": N, "rows": int(n.sum()), "map_entries": M, "sigma": a.sigma, "radius_px": a.px, "radius": 0.1, "ratio": 0.8,
           "prior_push": "t (0.01, -0.005, 0.01), 0.002 rad about y"}
    for k in what:
        out[k] = round(statistics.median(runs[k][1:]), 1)
        out[k.replace("_us", "_runs_us")] = [round(x, 1) for x in runs[k][1:]]
    guided(0)
    sync()
    st = vo.MapGuidedStats(); raw = np.zeros(48, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 48)
    out["guided_stats"] = st.as_dict()
    out["gated_per_live_row"] = round(st.n_gated / max(st.n_live, 1), 3)
    out["in_view_per_frame"] = round(st.n_in_view / F, 1)
    guided(0, a.z_vis)
    sync()
    ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 48)
    out["guided_zvis_stats"] = st.as_dict()
    out["z_far"], out["z_vis"] = int(seq["z_far"]), a.z_vis
    out["zvis_gated_per_live_row"] = round(st.n_gated / max(st.n_live, 1), 3)
    out["zvis_in_view_per_frame"] = round(st.n_in_view / F, 1)
    out["guided_zvis_over_lookup"] = round(out["guided_zvis_us"] / out["lookup_us"], 2)
    out["nearest_over_guided_zvis"] = round(out["nearest_us"] / out["guided_zvis_us"], 2)
    out["guided_over_lookup"] = round(out["guided_us"] / out["lookup_us"], 2)
    out["nearest_over_guided"] = round(out["nearest_us"] / out["guided_us"], 2)
    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: wall time of one call between two synchronises, host launches included",
           "not_measured": "this tool takes no kernel trace: how guided_us divides between the index and the search is not in this file",
           "shape": out}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
