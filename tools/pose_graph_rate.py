#!/usr/bin/env python3
"""Times voe_pose_graph_dev on the device: the example graph (121 frames, 124 edges) and synthetic chains of 1 000 and 10 000
frames with 1 % loop edges (a scale drift of e^3 over the whole chain), CHAIN against JACOBI.  JACOBI's n_cg is doubled from CHAIN's until its final cost is within 1 % of
CHAIN's (or 256 is reached): iterations and milliseconds at equal final cost.  A call's time is the wall time from the enqueue to
the end of a stream synchronise, after 3 warm-up calls, over 10 calls: median and range.  Per PCG iteration the call enqueues
three launches; at the example's size their cost is launch latency, reported as the time per iteration.  `launches` counts the
kernel launches of a call (8 at the start, 3 (n_cg + 2) per round, 3 at the end); the memset in front of them is not among them.
Then voe_map_apply_correction_batch_dev at 200 frames x 50 000 rows on the synthetic sequence's map (the shape of
profiles/map_grow_timing.json), next to vo_map_lookup_batch_dev on the same arrays: the lookup is the floor of the apply.
Gates nothing.

    python tools/pose_graph_rate.py            -> profiles/pose_graph_timing.json
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import __graft_entry__ as g  # noqa: E402
import pose_graph_cases as Cc  # noqa: E402
import pose_graph_restatement as P  # noqa: E402


def timed(vo, ctx, case, n_cg, preconditioner, warm=3, reps=10):
    S0 = np.ascontiguousarray(np.asarray(case["S"], np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
    e = np.asarray(case["edges"], np.int32)
    Z = np.ascontiguousarray(np.asarray(case["Z"], np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
    d_S, d_e, d_Z, d_f = ctx.to_device(S0), ctx.to_device(e), ctx.to_device(Z), ctx.to_device(np.asarray(case["fixed"], np.uint8))
    R = int(case["n_rounds"])
    d_r, d_st = ctx.alloc(40 * R + 16), ctx.alloc(64)
    prm = vo.PoseGraphParams(R, int(n_cg), float(case["cg_tol"]), float(case["lambda0"]), 0.0, 1, P.PRECONDITIONER.index(preconditioner))
    times = []
    for k in range(warm + reps):
        ctx.h2d(d_S, S0)
        ctx.synchronize()
        t = time.perf_counter()
        vo.pose_graph_dev(ctx, len(S0), d_S, len(e), d_e, d_Z, None, d_f, prm, None, None, d_r, d_st)
        ctx.synchronize()
        if k >= warm:
            times.append(1e3 * (time.perf_counter() - t))
    rounds = np.zeros(R, vo.POSE_GRAPH_ROUND_DTYPE)
    ctx.d2h(rounds, d_r)
    st = vo.PoseGraphStats()
    raw = np.zeros(48, np.uint8)
    ctx.d2h(raw, d_st)
    C.memmove(C.byref(st), raw.ctypes.data, 48)
    for d in (d_S, d_e, d_Z, d_f, d_r, d_st):
        ctx.free(d)
    iters = int(rounds["cg_iterations"].sum())
    return dict(preconditioner=preconditioner, n_cg=int(n_cg), status=vo.POSE_GRAPH_STATUS[st.status], cost_before=st.cost_before,
                cost_after=st.cost_after, accepted=int(st.n_accepted), cg_iterations=iters, launches=8 + R * 3 * (int(n_cg) + 2) + 3,
                ms_median=float(np.median(times)), ms_min=float(min(times)), ms_max=float(max(times)))


def apply_timing(vo, ctx, n_frames=200, n_visible=50000, warm=2, reps=8):
    s = vo.synth.sequence(n_frames=n_frames, n_visible=n_visible)
    poses = [np.linalg.inv(vo.synth.planar_pose(*x) @ vo.synth.CAM_IN_ROBOT) for x in s["gt"]]
    F, cap = len(s["frames"]), max(len(f["app"]) for f in s["frames"])
    app = np.full((F, cap, 10), np.nan, np.float32)
    n = np.array([len(f["app"]) for f in s["frames"]], np.int32)
    for f, fr in enumerate(s["frames"]):
        app[f, : n[f]] = fr["app"]
    pts, app_map = np.ascontiguousarray(s["world_xyz"], np.float32), np.ascontiguousarray(s["world_app"], np.float32)
    M = len(pts)
    m = vo.Map(ctx, capacity=M)
    for lo in range(0, M, 100000):
        m.update(pts[lo: lo + 100000], app_map[lo: lo + 100000])
    S_old = np.stack([np.ascontiguousarray(np.asarray(X, np.float32).T).ravel() for X in poses])
    S_new = np.stack([np.ascontiguousarray((np.diag([1.0 + 1e-4 * f] * 3 + [1.0]) @ np.asarray(X, np.float64)).astype(np.float32).T).ravel()
                      for f, X in enumerate(poses)])
    d_app, d_n, d_So, d_Sn = ctx.to_device(app), ctx.to_device(n), ctx.to_device(S_old), ctx.to_device(S_new)
    d_pairs, d_nout, d_ent, d_st = ctx.alloc(8 * F * cap), ctx.alloc(4 * F + 16), ctx.alloc(4 * F * cap), ctx.alloc(16)
    V, I, Z = C.c_void_p, C.c_int, C.c_size_t

    def lookup():
        assert ctx.lib.vo_map_lookup_batch_dev(m.h, I(F), V(d_app), Z(cap), I(cap), V(d_n), V(d_pairs), V(d_nout), None, None, V(d_ent)) == 0

    def apply():
        m.apply_correction_batch_dev(F, d_app, cap, cap, d_n, d_So, d_Sn, False, None, d_st)

    out = {}
    for name, f in (("lookup", lookup), ("apply", apply)):
        times = []
        for k in range(warm + reps):
            ctx.synchronize()
            t = time.perf_counter()
            f()
            ctx.synchronize()
            if k >= warm:
                times.append(1e3 * (time.perf_counter() - t))
        out[name] = dict(ms_median=float(np.median(times)), ms_min=float(min(times)), ms_max=float(max(times)))
    st = np.zeros(4, np.int32)
    ctx.d2h(st, d_st)
    out.update(n_frames=F, n_max=cap, rows=int(n.sum()), n_entries=int(st[0]), n_seen=int(st[1]), n_moved=int(st[2]))
    print(f"apply: {F} frames x {cap} rows, map of {M}: lookup {out['lookup']['ms_median']:.3f} ms, apply {out['apply']['ms_median']:.3f} ms "
          f"({out['apply']['ms_min']:.3f} .. {out['apply']['ms_max']:.3f}); {int(st[1])} seen, {int(st[2])} moved")
    return out


def main():
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    graphs = {"example_121": Cc.example_graph()[0]}
    for F in (1000, 10000):
        graphs["chain_%d" % F] = dict(Cc.graph(F, [(k, F - 1 - k) for k in range(F // 100)], seed=F, drift=3.0 / F)[0], **dict(P.DEFAULT))
    out = {}
    for name, case in graphs.items():
        chain = timed(vo, ctx, case, 8, "CHAIN")
        rows, n_cg = [chain], 8
        while True:
            j = timed(vo, ctx, case, n_cg, "JACOBI")
            rows.append(j)
            if j["cost_after"] <= 1.01 * chain["cost_after"] or n_cg >= 256:
                break
            n_cg *= 2
        for r in rows:
            r["us_per_launch"] = 1e3 * r["ms_median"] / r["launches"]
            print(f"{name:12s} {r['preconditioner']:6s} n_cg {r['n_cg']:3d}: {r['status']}, cost {r['cost_before']:.4g} -> {r['cost_after']:.6g}, "
                  f"{r['cg_iterations']} iterations, {r['ms_median']:.3f} ms ({r['ms_min']:.3f} .. {r['ms_max']:.3f}), {r['launches']} launches, "
                  f"{r['us_per_launch']:.2f} us each")
        out[name] = dict(n_frames=len(case["S"]), n_edges=len(case["edges"]), n_rounds=int(case["n_rounds"]), rows=rows)
    name, ncu = ctx.device_info()
    res = dict(what="voe_pose_graph_dev, wall time of enqueue + synchronise per call, 3 warm-up calls, 10 timed; JACOBI's n_cg doubled until its "
                    "final cost is within 1 % of CHAIN's at n_cg = 8 (or 256)",
               device=name, n_cu=ncu, stamp=stamp.current(), not_measured="no kernel trace or counter run", graphs=out,
               apply=apply_timing(vo, ctx))
    with open(os.path.join(ROOT, "profiles", "pose_graph_timing.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
