"""Time the covisibility of frames and the window chosen from it (voe_map_covis_batch_dev, voe_map_window_dev, DESIGN.md
section 4.18) beside the call's own first launches.

  python tools/map_covis_rate.py [--frames 200] [--rows 50000] [--entries 800000] [--out profiles/map_covis_timing.json]
      A map of `entries` random appearances; frame f holds `rows` rows drawn (seeded) from the entries within 2 x rows of
      f * entries / frames, so that near frames share about a quarter of their rows and far ones none.  Every run synchronises,
      makes ONE call and synchronises again; medians of 5 runs after one that warms up and sizes the workspaces:
        covis_with_counts_us     voe_map_covis_batch_dev with the matrix
        covis_without_counts_us  the same without it: lookup, memset, bit pass, the population counts
        count_pass_us            the difference of the two medians: the tiled count pass
        window_us                voe_map_window_dev on the bits (query: the middle frame, 8 / 8 / 15)
        lookup_us                the yardstick: vo_map_lookup_batch_dev of the same frames with its entry output
        memset_us                the yardstick: a device memset of the bit array
      and the tile arithmetic of the count pass for the shape."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_covis_timing.json"))
    a = ap.parse_args()
    import numpy as np

    import __graft_entry__ as g
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    lib, V, I, S = ctx.lib, C.c_void_p, C.c_int, C.c_size_t
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    lib.vo_ctx_stream.restype = C.c_void_p
    stream = V(lib.vo_ctx_stream(ctx.h))

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    F, N, M = a.frames, a.rows, a.entries
    rng = np.random.default_rng(7)
    app_map = rng.uniform(-1, 1, (M, 10)).astype(np.float32)
    m = vo.Map(ctx, capacity=M)
    for lo in range(0, M, 100000):
        m.update(np.zeros((len(app_map[lo: lo + 100000]), 3), np.float32), app_map[lo: lo + 100000])
    assert len(m) == M
    W = m.words()
    d_app = ctx.alloc(40 * F * N + 16)
    for f in range(F):                                        # frame by frame: the host never holds all rows
        pool = ((f * M) // F + np.arange(-2 * N, 2 * N)) % M
        ids = rng.choice(pool, N, replace=False)
        ctx.h2d(d_app + 40 * f * N, app_map[ids])
    print("frames made", flush=True)
    d_bits, d_counts, d_stats = ctx.alloc(4 * F * W + 16), ctx.alloc(4 * F * F + 16), ctx.alloc(64)
    d_pairs, d_cnt, d_ent = ctx.alloc(8 * F * N + 16), ctx.alloc(4 * F + 16), ctx.alloc(4 * F * N + 16)
    d_role, d_rows, d_fixed, d_wstats = ctx.alloc(4 * F + 16), ctx.alloc(4 * F + 16), ctx.alloc(F + 16), ctx.alloc(64)
    prm = vo.MapWindowParams(F // 2, min(8, F), min(8, F), 15)

    def covis(counts):
        rc = lib.voe_map_covis_batch_dev(m.h, I(F), V(d_app), S(N), I(N), None, I(W), V(d_bits), V(d_counts) if counts else None, V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def window():
        rc = lib.voe_map_window_dev(m.h, I(F), I(W), V(d_bits), None, I(N), C.byref(prm), V(d_role), V(d_rows), V(d_fixed), None, None, V(d_wstats))
        assert rc == 0, lib.vo_last_error()

    def lookup():
        rc = lib.vo_map_lookup_batch_dev(m.h, I(F), V(d_app), S(N), I(N), None, V(d_pairs), V(d_cnt), None, None, V(d_ent))
        assert rc == 0, lib.vo_last_error()

    def memset():
        assert hip.hipMemsetAsync(V(d_bits), I(0), S(4 * F * W), stream) == 0

    def timed(f):
        runs = []
        for _ in range(6):                                    # the first run warms up (and sizes the workspaces)
            sync()
            t = time.perf_counter()
            f()
            sync()
            runs.append((time.perf_counter() - t) * 1e6)
        return round(statistics.median(runs[1:]), 1), [round(x, 1) for x in runs[1:]]

    out = {"frames": F, "rows_per_frame": N, "map_entries": M, "words_per_row": W}
    out["covis_with_counts_us"], out["covis_with_counts_runs_us"] = timed(lambda: covis(True))
    out["covis_without_counts_us"], out["covis_without_counts_runs_us"] = timed(lambda: covis(False))
    out["count_pass_us"] = round(out["covis_with_counts_us"] - out["covis_without_counts_us"], 1)
    st = vo.MapCovisStats(); raw = np.zeros(32, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 32)
    out["covis_stats"] = st.as_dict()
    out["window_us"], out["window_runs_us"] = timed(window)
    ws = vo.MapWindowStats(); ctx.d2h(raw, d_wstats); C.memmove(C.byref(ws), raw.ctypes.data, 32)
    out["window_stats"] = ws.as_dict()
    out["lookup_us"], out["lookup_runs_us"] = timed(lookup)
    out["memset_us"], out["memset_runs_us"] = timed(memset)
    E = 32                                                    # COVIS_TILE (visual-odometry_amd/csrc/covis_rules.h)
    T = (F + E - 1) // E
    out["tile_arithmetic"] = {"tile_edge": E, "tiles_launched": T * (T + 1) // 2, "word_ands": F * (F + 1) // 2 * W,
                              "word_ands_launched": T * (T + 1) // 2 * E * E * W, "bytes_of_B_read": T * (T + 1) // 2 * 2 * E * W * 4,
                              "bytes_of_B": 4 * F * W}
    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: wall time of one call between two synchronises, host launches included",
           "not_measured": "no kernel trace or counter run was taken: the count pass's share is the difference of two calls, not a kernel's own time",
           "shape": out}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
