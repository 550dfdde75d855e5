"""Time the choice of keyframes (voe_map_keyframes_dev) beside the covisibility that feeds it and the
window that reads the same bit rows.

  python tools/map_keyframes_rate.py [--frames 200] [--rows 50000] [--rounds 3] [--out profiles/map_keyframes_timing.json]
      synth.sequence with `frames` frames of about `rows` visible landmarks each against its own map (every landmark of the
      sequence: 1.87 M at the defaults).  Every run synchronises, makes ONE call and synchronises again; the calls alternate
      within a round, and the figures are medians of `rounds` rounds after one that warms up and sizes the workspaces:
        covis_without_counts_us   voe_map_covis_batch_dev without the matrix: the bit rows the other calls read
        window_us                 voe_map_window_dev on them (query: the middle frame, 8 / 8 / 15)
        keyframes_<k>_us          voe_map_keyframes_dev, min_observers 3, 900 per mille, frames 0 and the last protected, max_dropped
                                  k in 0, 16, 128; with the frames each dropped
        keyframes_idle_<k>_us     the same with min_observers = frames: no frame is a candidate, so the first step raises the
                                  device's done flag and the other k - 1 steps are launches that return at once
      and from them us_per_step_<k> (the steps that looked for a candidate, over the analysis-only call) and us_per_idle_step."""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_keyframes_timing.json"))
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
    W = m.words()
    n = np.zeros(F, np.int32)
    d_app = ctx.alloc(40 * F * N + 16)
    for f, fr in enumerate(seq["frames"]):                    # frame by frame: the host never holds all rows
        k = len(fr["ids"])
        n[f] = k
        app = np.zeros((N, 10), np.float32); app[:k] = fr["app"]
        ctx.h2d(d_app + 40 * f * N, app)
    d_n = ctx.to_device(n)
    flags = np.zeros(F, np.uint8); flags[[0, F - 1]] = 1
    d_flags = ctx.to_device(flags)
    d_bits, d_stats = ctx.alloc(4 * F * W + 16), ctx.alloc(64)
    d_role, d_rows, d_fixed, d_wstats = ctx.alloc(4 * F + 16), ctx.alloc(4 * F + 16), ctx.alloc(F + 16), ctx.alloc(64)
    d_out = [ctx.alloc(4 * F + 16) for _ in range(6)]
    d_keep, d_kstats = ctx.alloc(F + 16), ctx.alloc(64)
    wprm = vo.MapWindowParams(F // 2, min(8, F), min(8, F), 15)
    print("frames uploaded", flush=True)

    def covis():
        rc = lib.voe_map_covis_batch_dev(m.h, I(F), V(d_app), S(N), I(N), V(d_n), I(W), V(d_bits), None, V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def window():
        rc = lib.voe_map_window_dev(m.h, I(F), I(W), V(d_bits), V(d_n), I(N), C.byref(wprm), V(d_role), V(d_rows), V(d_fixed), None, None, V(d_wstats))
        assert rc == 0, lib.vo_last_error()

    def keyframes(min_observers, budget):
        prm = vo.MapKeyframesParams(min_observers, 900, 1, 0, budget)
        rc = lib.voe_map_keyframes_dev(m.h, I(F), I(W), V(d_bits), V(d_n), I(N), V(d_flags), C.byref(prm), V(d_out[0]), V(d_out[1]), V(d_keep),
                                       V(d_out[2]), V(d_out[3]), V(d_out[4]), V(d_out[5]), V(d_kstats))
        assert rc == 0, lib.vo_last_error()

    def kstats():
        sync()
        st = vo.MapKeyframesStats(); raw = np.zeros(32, np.uint8); ctx.d2h(raw, d_kstats); C.memmove(C.byref(st), raw.ctypes.data, 32)
        return st.as_dict()

    budgets = (0, 16, 128)
    what = {"covis_without_counts_us": covis, "window_us": window}
    what.update({f"keyframes_{b}_us": (lambda b=b: keyframes(3, b)) for b in budgets})
    what.update({f"keyframes_idle_{b}_us": (lambda b=b: keyframes(F, b)) for b in budgets[1:]})
    runs = {k: [] for k in what}
    covis()
    for r in range(a.rounds + 1):                             # the first round warms up (and sizes the workspaces)
        for k, f in what.items():
            sync()
            t = time.perf_counter()
            f()
            sync()
            runs[k].append((time.perf_counter() - t) * 1e6)
    out = {"frames": F, "rows_per_frame_max": N, "rows": int(n.sum()), "map_entries": M, "words_per_row": W, "bytes_of_bit_rows": 4 * F * W,
           "min_observers": 3, "share_permille": 900, "protected": [0, F - 1]}
    for k in what:
        out[k] = round(statistics.median(runs[k][1:]), 1)
        out[k.replace("_us", "_runs_us")] = [round(x, 1) for x in runs[k][1:]]
    for b in budgets:
        keyframes(3, b)
        out[f"keyframes_{b}_stats"] = kstats()
    keyframes(F, budgets[-1])
    out["keyframes_idle_stats"] = kstats()
    out["us_per_idle_step"] = round((out["keyframes_idle_128_us"] - out["keyframes_idle_16_us"]) / (budgets[-1] - 16), 2)
    for b in budgets[1:]:                                     # the steps that looked for a candidate: the drops, and the one that found none
        real = min(out[f"keyframes_{b}_stats"]["n_dropped"] + 1, b)
        out[f"steps_{b}"] = real
        out[f"us_per_step_{b}"] = round((out[f"keyframes_{b}_us"] - out["keyframes_0_us"] - (b - real) * out["us_per_idle_step"]) / real, 2)
    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: wall time of one call between two synchronises, host launches included",
           "not_measured": "this tool takes no kernel trace: how a step divides between its two launches is not in this file; us_per_step_<k> "
                           "is a difference of medians -- the call over the analysis-only call, less the idle steps -- and no kernel's own time",
           "shape": out}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
