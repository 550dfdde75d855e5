#!/usr/bin/env python3
"""Times voe_map_loops_batch_dev on the device at 200 frames x 50 000 rows on the synthetic sequence's map (the shape of
profiles/pose_graph_timing.json's apply and of profiles/map_grow_timing.json), next to the calls it is made of on the same arrays
in the same session: vo_map_lookup_batch_dev, voe_map_covis_batch_dev without and with the pair counts, and a dry-run
voe_map_apply_correction_batch_dev.  The sequence never returns to a place it has left, so the gap is 10 frames instead of 50:
a landmark stays in view for about 25 frames, and the candidates are the frames that still see what a frame 11 and more behind
them saw first.  The poses are the ground truth (no drift): every slot measures.  max_loops 1 and 8 separate the measurement from
the search.  A call's time is the wall time from the enqueue to the end of a stream synchronise, after 2 warm-up calls, over 8
calls: median and range.  Gates nothing.

    python tools/map_loops_rate.py            -> profiles/map_loops_timing.json
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import __graft_entry__ as g  # noqa: E402


def main(n_frames=200, n_visible=50000, warm=2, reps=8):
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    s = vo.synth.sequence(n_frames=n_frames, n_visible=n_visible)
    poses = [np.linalg.inv(vo.synth.planar_pose(*x) @ vo.synth.CAM_IN_ROBOT) for x in s["gt"]]
    F, cap = len(s["frames"]), max(len(f["app"]) for f in s["frames"])
    app = np.full((F, cap, 10), np.nan, np.float32)
    uv = np.zeros((F, cap, 2), np.float32)
    n = np.array([len(f["app"]) for f in s["frames"]], np.int32)
    for f, fr in enumerate(s["frames"]):
        app[f, : n[f]], uv[f, : n[f]] = fr["app"], fr["pts"]
    pts, app_map = np.ascontiguousarray(s["world_xyz"], np.float32), np.ascontiguousarray(s["world_app"], np.float32)
    M = len(pts)
    m = vo.Map(ctx, capacity=M)
    for lo in range(0, M, 100000):
        m.update(pts[lo: lo + 100000], app_map[lo: lo + 100000])
    cam = vo.Camera(s["rows"], s["cols"], s["z_near"], s["z_far"], s["K"], np.eye(4), ctx=ctx)
    S = np.stack([np.ascontiguousarray(np.asarray(X, np.float32).T).ravel() for X in poses])
    d_uv, d_app, d_n, d_S = ctx.to_device(uv), ctx.to_device(app), ctx.to_device(n), ctx.to_device(S)
    W = m.words()
    Lmax = 8
    d_pairs, d_nout, d_ent = ctx.alloc(8 * F * cap), ctx.alloc(4 * F + 16), ctx.alloc(4 * F * cap)
    d_bits, d_counts, d_cst, d_ast = ctx.alloc(4 * F * W), ctx.alloc(4 * F * F), ctx.alloc(32), ctx.alloc(16)
    d_edges, d_Z, d_w, d_rec, d_st = ctx.alloc(8 * Lmax), ctx.alloc(64 * Lmax), ctx.alloc(12 * Lmax), ctx.alloc(40 * Lmax), ctx.alloc(32)
    V, I, Zt = C.c_void_p, C.c_int, C.c_size_t

    def params(max_loops):
        return vo.MapLoopsParams(10, 5, 12, 3, max_loops, 0, vo.RansacParams(64, 2.0, 0), 10000.0, 50, 6, (C.c_float * 3)(1.0, 1.0, 1.0), 0)

    calls = {
        "lookup": lambda: ctx.lib.vo_map_lookup_batch_dev(m.h, I(F), V(d_app), Zt(cap), I(cap), V(d_n), V(d_pairs), V(d_nout), None, None, V(d_ent)),
        "covis_bits": lambda: m.covis_batch_dev(F, d_app, cap, cap, d_n, W, d_bits, None, d_cst),
        "covis_counts": lambda: m.covis_batch_dev(F, d_app, cap, cap, d_n, W, d_bits, d_counts, d_cst),
        "apply_dry_run": lambda: m.apply_correction_batch_dev(F, d_app, cap, cap, d_n, d_S, d_S, True, None, d_ast),
        "loops_1": lambda: m.loops_batch_dev(cam, F, d_uv, cap, d_app, cap, cap, d_n, d_S, params(1), d_edges, d_Z, d_w, d_rec, None, None, d_st),
        "loops_8": lambda: m.loops_batch_dev(cam, F, d_uv, cap, d_app, cap, cap, d_n, d_S, params(8), d_edges, d_Z, d_w, d_rec, None, None, d_st),
    }
    out = {}
    for name, f in calls.items():
        times = []
        for k in range(warm + reps):
            ctx.synchronize()
            t = time.perf_counter()
            f()
            ctx.synchronize()
            if k >= warm:
                times.append(1e3 * (time.perf_counter() - t))
        out[name] = dict(ms_median=float(np.median(times)), ms_min=float(min(times)), ms_max=float(max(times)))
        print(f"{name:14s} {out[name]['ms_median']:8.3f} ms ({out[name]['ms_min']:.3f} .. {out[name]['ms_max']:.3f})")
    rec = np.zeros(Lmax, vo.MAP_LOOP_RECORD_DTYPE)
    ctx.d2h(rec, d_rec)
    st = vo.MapLoopsStats()
    raw = np.zeros(32, np.uint8)
    ctx.d2h(raw, d_st)
    C.memmove(C.byref(st), raw.ctypes.data, 32)
    cst = np.zeros(8, np.int32)
    ctx.d2h(cst, d_cst)
    print(st.as_dict(), [(int(r["i"]), int(r["j"]), int(r["c"]), int(r["n_pairs"]), int(r["num_inliers"]), vo.MAP_LOOP_STATUS[int(r["status"])]) for r in rec])
    name, ncu = ctx.device_info()
    res = dict(what="wall time of enqueue + synchronise per call, 2 warm-up calls, 8 timed, every call on the same device arrays in one session; "
                    "loops_L: voe_map_loops_batch_dev with gap 10, ref_window 5, min_shared 12, separation 3, max_loops L, 64 hypotheses, 50 rounds, "
                    "no histogram or reference-frame output",
               device=name, n_cu=ncu, stamp=stamp.current(), not_measured="no kernel trace or counter run: the stages of a call are not separated "
               "beyond what the differences between the rows say", n_frames=F, n_max=cap, rows=int(n.sum()), n_entries=int(st.n_entries),
               n_entries_seen=int(cst[4]), n_words=W, stats=st.as_dict(),
               slots=[dict(i=int(r["i"]), j=int(r["j"]), c=int(r["c"]), n_pairs=int(r["n_pairs"]), ransac_inliers=int(r["ransac_inliers"]),
                           num_inliers=int(r["num_inliers"]), status=vo.MAP_LOOP_STATUS[int(r["status"])]) for r in rec], calls=out)
    with open(os.path.join(ROOT, "profiles", "map_loops_timing.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
