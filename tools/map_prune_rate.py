"""Time the pruning of observations (voe_map_prune_batch_dev) beside the cull's dry run -- the yardstick:
the same lookup, the same lists and one pass per landmark -- and beside the exact lookup alone, in ONE session.

  python tools/map_prune_rate.py [--frames 200] [--rows 50000] [--calls 20] [--share 0.01] [--out profiles/map_prune_timing.json]
      synth.sequence with `frames` frames of about `rows` visible landmarks each against its own map (every landmark of the
      sequence: 1.87 M at the defaults) at the ground-truth poses; `share` of every frame's rows are re-pointed: they get the
      appearance of a random other landmark (seeded).  The calls alternate within a round; every call lies between two events
      on the context's stream, and the figures are medians of `calls` rounds after two that warm up and size the workspaces:
        prune_us              every output given, the rows out of place (80 B per live row move in the finishing launch)
        prune_in_place_us     d_app_out = d_app, the rows restored right after the call (outside every timed span): only
                              the pruned rows are written
        prune_bare_us         d_entry_out and the statistics alone
        cull_dry_run_us       voe_map_cull_batch_dev, dry_run = 1, min_obs = min_frames = 1, max_err_px as the prune's
        lookup_us             vo_map_lookup_batch_dev with the entries alone
      and stream_80B_per_row_us: what 80 B per live row cost at the bandwidth a hipMemcpyAsync device-to-device of the rows
      reaches in the same session (40 B read + 40 B written per row: the copy itself)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--share", type=float, default=0.01)
    ap.add_argument("--max-err-px", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_prune_timing.json"))
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
    ev = [V(), V()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def sync():
        assert lib.vo_ctx_synchronize(ctx.h) == 0

    def timed(f):
        """one call between two events on the context's stream, in microseconds"""
        sync()
        assert hip.hipEventRecord(ev[0], stream) == 0
        f()
        assert hip.hipEventRecord(ev[1], stream) == 0
        assert hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return ms.value * 1e3

    seq = vo.synth.sequence(n_frames=a.frames, n_visible=a.rows)
    F, M = len(seq["frames"]), len(seq["world_xyz"])
    N = max(len(fr["ids"]) for fr in seq["frames"])
    print(f"sequence made: {F} frames, {M} landmarks, n_max {N}", flush=True)
    m = vo.Map(ctx, capacity=M)
    for lo in range(0, M, 100000):
        m.update(seq["world_xyz"][lo: lo + 100000], seq["world_app"][lo: lo + 100000])
    assert len(m) == M
    rng = np.random.default_rng(1)
    n = np.zeros(F, np.int32)
    d_uv, d_app, d_app0, d_app_out = ctx.alloc(8 * F * N + 16), ctx.alloc(40 * F * N + 16), ctx.alloc(40 * F * N + 16), ctx.alloc(40 * F * N + 16)
    n_wrong = 0
    for f, fr in enumerate(seq["frames"]):                    # frame by frame: the host never holds all rows
        k = len(fr["ids"])
        n[f] = k
        uv = np.zeros((N, 2), np.float32); uv[:k] = fr["pts"]
        app = np.zeros((N, 10), np.float32); app[:k] = fr["app"]
        who = rng.choice(k, int(round(a.share * k)), replace=False)
        app[who] = seq["world_app"][rng.integers(0, M, len(who))]
        n_wrong += len(who)
        ctx.h2d(d_uv + 8 * f * N, uv)
        ctx.h2d(d_app + 40 * f * N, app)
        ctx.h2d(d_app0 + 40 * f * N, app)
    T = np.stack([np.ascontiguousarray(np.asarray(np.linalg.inv(vo.synth.planar_pose(*x) @ vo.synth.CAM_IN_ROBOT), np.float32).T).ravel() for x in seq["gt"]])
    d_n, d_T = ctx.to_device(n), ctx.to_device(np.ascontiguousarray(T[:F]))
    Kc = np.ascontiguousarray(np.asarray(seq["K"], np.float32).T).ravel()
    rows = F * N
    d_entry, d_status, d_sq = ctx.alloc(4 * rows + 16), ctx.alloc(4 * rows + 16), ctx.alloc(8 * rows + 16)
    d_lm, d_fr, d_stats, d_cstats = ctx.alloc(32 * M + 16), ctx.alloc(16 * F + 16), ctx.alloc(64), ctx.alloc(64)
    d_pairs, d_cnt = ctx.alloc(8 * rows + 16), ctx.alloc(4 * F + 16)
    print(f"frames uploaded: {int(n.sum())} live rows, {n_wrong} re-pointed", flush=True)
    prm = vo.MapPruneParams(a.max_err_px, 0.0, 0.0, 3, 1, 500, 300, 0)
    cprm = vo.MapCullParams(1, 1, 0.0, a.max_err_px, 0.0, 0, 1)

    def prune(app_out, full=True):
        o = (lambda d: V(d)) if full else (lambda d: None)
        rc = lib.voe_map_prune_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(N), V(d_app), S(N), I(N), V(d_n), V(d_T), C.byref(prm), V(d_entry),
                                         o(d_status), o(d_sq), V(app_out) if app_out else None, o(d_lm), o(d_fr), V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def cull():
        rc = lib.voe_map_cull_batch_dev(m.h, I(F), Kc.ctypes.data_as(V), V(d_uv), S(N), V(d_app), S(N), I(N), V(d_n), V(d_T), C.byref(cprm), None, None,
                                        None, V(d_cstats))
        assert rc == 0, lib.vo_last_error()

    def lookup():
        m.lookup_batch_dev(F, d_app, N, N, d_n, d_pairs, d_cnt, d_entries=d_entry)

    def copy_rows(dst=None):
        assert hip.hipMemcpyAsync(V(dst or d_app_out), V(d_app0), S(40 * rows), I(3), stream) == 0

    def restore():
        copy_rows(d_app)
        sync()

    what = {"prune_us": lambda: prune(d_app_out), "prune_in_place_us": lambda: prune(d_app), "prune_bare_us": lambda: prune(None, full=False),
            "cull_dry_run_us": cull, "lookup_us": lookup, "copy_rows_d2d_us": copy_rows}
    runs = {k: [] for k in what}
    for r in range(a.calls + 2):                              # the first two rounds warm up (and size the workspaces)
        for k, f in what.items():
            runs[k].append(timed(f))
            if k == "prune_in_place_us":                      # every call of a round sees the window prune_us saw
                restore()
    out = {"frames": F, "rows_per_frame_max": N, "rows": int(n.sum()), "rows_repointed": n_wrong, "map_entries": M, "max_err_px": a.max_err_px,
           "unique": 1, "max_share_landmark": 500, "max_share_frame": 300, "timed_calls": a.calls}
    for k in what:
        out[k] = round(statistics.median(runs[k][2:]), 1)
        out[k.replace("_us", "_min_max_us")] = [round(min(runs[k][2:]), 1), round(max(runs[k][2:]), 1)]
    prune(d_app_out); sync()
    st = vo.MapPruneStats(); raw = np.zeros(64, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 64)
    out["prune_stats"] = st.as_dict()
    cull(); sync()
    cs = vo.MapCullStats(); raw = np.zeros(48, np.uint8); ctx.d2h(raw, d_cstats); C.memmove(C.byref(cs), raw.ctypes.data, 48)
    out["cull_stats"] = cs.as_dict()
    live = int(n.sum())
    out["stream_80B_per_row_us"] = round(out["copy_rows_d2d_us"] * live / rows, 1)
    out["prune_over_cull_dry_run_us"] = round(out["prune_us"] - out["cull_dry_run_us"], 1)
    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: the time between two events on the context's stream around one call, "
                       "host launches included; medians of `timed_calls` calls that alternate in one session",
           "not_measured": "this tool takes no kernel trace: how a call divides between its launches comes from a rocprofv3 --kernel-trace --stats "
                           "run of its own (DESIGN.md section 4.27 quotes it where one was taken)",
           "shape": out}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
