"""Time the alignment and the merge of two device maps (voe_map_align_dev, voe_map_merge_dev) beside
the two calls they are made of or modelled on, at the same sizes and in the same session.

  python tools/map_align_rate.py [--src 50000] [--dst 800000] [--hypotheses 256] [--out profiles/map_align_timing.json]
      dst: a map of --dst random landmarks; src: --src of them (a tenth pushed off) moved by the inverse of a planted similarity,
      plus 5 % entries of its own.  Every run synchronises, makes ONE call and synchronises again (wall time, host launches
      included); medians of 5 runs after one that warms up and sizes the workspaces.  The merges restore dst first (clear +
      update, outside the timed span).
        align_us            voe_map_align_dev, n_refits = 1, every optional output
        align_no_refit_us   the same with n_refits = 0
        merge_take_src_us   voe_map_merge_dev, VOE_MAP_MERGE_TAKE_SRC, with the remap
        merge_keep_dst_us   voe_map_merge_dev, VOE_MAP_MERGE_KEEP_DST, with the remap
        lookup_us           the yardstick: vo_map_lookup_dev of src's appearances on dst (the first three launches of either call)
        update_us           vo_map_update_dev of src's rows into dst (what TAKE_SRC is made of)
        p3p_ransac_us       the other yardstick: vo_estimate_pose_ransac_batch_dev, one problem of --src pairs, --hypotheses"""
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
    ap.add_argument("--src", type=int, default=50000)
    ap.add_argument("--dst", type=int, default=800000)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_align_timing.json"))
    a = ap.parse_args()
    import numpy as np

    import __graft_entry__ as g
    import map_align_cases as Cc
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    lib, V, I = ctx.lib, C.c_void_p, C.c_int

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    def timed(call, before=None, runs=5):
        out = []
        for k in range(runs + 1):
            if before:
                before()
            sync()
            t0 = time.perf_counter()
            call()
            sync()
            if k:
                out.append((time.perf_counter() - t0) * 1e6)
        return round(statistics.median(out), 1), [round(x, 1) for x in out]

    n_own = a.src // 20
    n_shared = a.src - n_own
    c = Cc.planted(n_shared, 7, n_src_only=n_own, n_dst_only=a.dst - n_shared, n_pushed=n_shared // 10, extent=50.0, threshold=0.05,
                   n_hypotheses=a.hypotheses)
    dst, src = vo.Map(ctx, capacity=a.dst + a.src), vo.Map(ctx, capacity=a.src)

    def restore():
        dst.clear()
        for lo in range(0, a.dst, 100000):
            dst.update(c["dst_pts"][lo: lo + 100000], c["dst_app"][lo: lo + 100000])
        assert len(dst) == a.dst

    restore()
    src.update(c["src_pts"], c["src_app"])
    assert len(src) == a.src
    n_max = src.size_bound()
    d_S, d_pairs, d_nm, d_mask = ctx.alloc(64), ctx.alloc(8 * n_max), ctx.alloc(16), ctx.alloc(n_max)
    d_counts, d_stats, d_remap, d_ms = ctx.alloc(4 * a.hypotheses), ctx.alloc(64), ctx.alloc(4 * n_max), ctx.alloc(16)

    def align(n_refits):
        prm = vo.MapAlignParams(1, a.hypotheses, 1, n_refits, 3, 0.05, 0)
        dst.align_dev(src, prm, d_S, d_pairs, d_nm, d_mask, d_counts, d_stats)

    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: wall time of one call between two synchronises, host launches "
                       "included; medians of 5 runs after a warm-up",
           "not_measured": "no kernel trace or counter run was taken: what a single kernel of a call costs is not known",
           "src_entries": a.src, "dst_entries": a.dst, "n_hypotheses": a.hypotheses}
    res["align_us"], res["align_runs_us"] = timed(lambda: align(1))
    st = vo.MapAlignStats()
    raw = np.zeros(48, np.uint8); ctx.d2h(raw, d_stats)
    C.memmove(C.byref(st), raw.ctypes.data, 48)
    res["align_stats"] = st.as_dict()
    assert st.status == 0 and st.n_matches == n_shared and st.n_inliers == n_shared - n_shared // 10, st.as_dict()
    res["align_no_refit_us"], res["align_no_refit_runs_us"] = timed(lambda: align(0))
    S = np.zeros(16, np.float32); ctx.d2h(S, d_S)
    x, ap_, n = V(), V(), V()
    assert lib.vo_map_dev_ptrs(src.h, C.byref(x), C.byref(ap_), C.byref(n)) == 0
    res["lookup_us"], res["lookup_runs_us"] = timed(lambda: dst.lookup_dev(ap_.value, n_max, n.value, d_pairs, d_nm))
    for key, policy in (("merge_take_src_us", vo.MAP_MERGE_TAKE_SRC), ("merge_keep_dst_us", vo.MAP_MERGE_KEEP_DST)):
        res[key], res[key.replace("_us", "_runs_us")] = timed(lambda: dst.merge_dev(src, d_S, policy, d_remap, d_ms), before=restore)
        ms = np.zeros(4, np.int32); ctx.d2h(ms, d_ms)
        res[key.replace("_us", "_stats")] = dict(n_src=int(ms[0]), n_shared=int(ms[1]), n_appended=int(ms[2]), n_dst_after=int(ms[3]))
        assert ms.tolist() == [a.src, n_shared, n_own, a.dst + n_own], ms
    res["update_us"], res["update_runs_us"] = timed(lambda: dst.update_dev(x.value, ap_.value, n_max, n.value, d_S), before=restore)

    # the P3P yardstick: one problem of a.src exact 2D-3D pairs
    rng = np.random.default_rng(3)
    K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    world = np.stack([rng.uniform(-2, 2, a.src), rng.uniform(-1.5, 1.5, a.src), rng.uniform(4, 9, a.src)], 1).astype(np.float32)
    meas = (world @ K.T)
    meas = (meas[:, :2] / meas[:, 2:]).astype(np.float32)
    pairs = np.stack([np.arange(a.src), np.arange(a.src)], 1).astype(np.int32)
    d_w, d_m, d_p = ctx.to_device(world), ctx.to_device(meas), ctx.to_device(pairs)
    d_T, d_ip, d_ni, d_st = ctx.alloc(64), ctx.alloc(8 * a.src), ctx.alloc(16), ctx.alloc(16)
    prm = vo.RansacParams(a.hypotheses, 2.0, 1)
    res["p3p_ransac_us"], res["p3p_ransac_runs_us"] = timed(lambda: vo.estimate_pose_ransac_batch_dev(
        ctx, 1, 480, 640, 0, 100, K, d_w, a.src, a.src, d_m, a.src, a.src, d_p, a.src, None, prm, d_T, d_ip, d_ni, None, None, d_st))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_us") or k.endswith("stats")}, indent=1))


if __name__ == "__main__":
    main()
