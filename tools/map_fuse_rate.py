"""Time voe_map_fuse_batch_dev on a large map with planted duplicates, the same call under dry_run (the
search without the compaction), and voe_map_cull_batch_dev dropping the same number of entries in the same session.

  python tools/map_fuse_rate.py [--frames 200] [--rows 50000] [--dup 0.1] [--radius_xyz 0.04] [--rounds 3] [--out profiles/map_fuse_timing.json]
      The map is every landmark of synth.sequence(frames, rows) -- 1.87 M at the defaults -- and `dup` of them entered a second
      time BEHIND the landmarks: the point pushed by U(-0.015, 0.015), the appearance by N(0, 0.005).  The sequence's appearances
      are distinct, so radius 0.1 pairs the copies alone; what the spatial gate lets through beside them is the map's own density
      (n_gated per entry is reported: the figure belongs to it).  The fuse is called WITHOUT frames.  Every run synchronises, makes
      ONE call and synchronises again; a call that changes the map is preceded by a restore (clear + update, not timed).  The
      figures alternate within every round and are the medians of `rounds` rounds after one that warms up and sizes the workspaces:
        fuse_us        voe_map_fuse_batch_dev, position 1: index, search, verdicts, compaction, rehash
        fuse_dry_us    the same with dry_run 1: index, search and verdicts; compaction and rehash return at once
        cull_us        voe_map_cull_batch_dev with drop_unseen on ONE frame that holds a row for every landmark and none for the
                       copies (every threshold off, one camera far behind the map): the lookup of that frame, the lists, the
                       score, and the SAME compaction and rehash dropping the same entries
        cull_dry_us    the same with dry_run 1: what the cull spends in front of the compaction
      fuse_us - fuse_dry_us and cull_us - cull_dry_us both estimate compaction + rehash; fuse_dry_us is the join."""
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
    ap.add_argument("--dup", type=float, default=0.1)
    ap.add_argument("--radius_xyz", type=float, default=0.04)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_fuse_timing.json"))
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
    P, A = seq["world_xyz"], seq["world_app"]
    L = len(P)
    D = int(round(a.dup * L))
    rng = np.random.default_rng(11)
    ch = np.sort(rng.permutation(L)[:D])
    pts = np.concatenate([P, (P[ch] + rng.uniform(-0.015, 0.015, (D, 3))).astype(np.float32)])
    app = np.concatenate([A, (A[ch] + rng.normal(0, 0.005, (D, 10))).astype(np.float32)])
    M = L + D
    print(f"map made: {L} landmarks + {D} copies", flush=True)
    m = vo.Map(ctx, capacity=M)

    def restore():
        m.clear()
        for lo in range(0, M, 100000):
            m.update(pts[lo: lo + 100000], app[lo: lo + 100000])

    restore()
    assert len(m) == M
    d_partner, d_verdict, d_remap, d_stats = ctx.alloc(4 * M + 16), ctx.alloc(4 * M + 16), ctx.alloc(4 * M + 16), ctx.alloc(64)
    # the cull's frame: a row for every landmark, none for the copies; one camera 1000 behind the map, so that every z is positive
    d_rows, d_uv = ctx.to_device(A), ctx.to_device(np.zeros((L, 2), np.float32))
    T = np.eye(4, dtype=np.float32)
    T[2, 3] = 1000.0
    d_T = ctx.to_device(np.ascontiguousarray(T.T).reshape(16))
    K = np.ascontiguousarray(np.asarray(seq["K"], np.float32).T).reshape(9)
    d_cstats = ctx.alloc(64)

    def fuse(dry):
        prm = vo.MapFuseParams(a.radius_xyz, 0.1, 1, 0, dry)
        rc = lib.voe_map_fuse_batch_dev(m.h, I(0), None, S(0), I(0), None, C.byref(prm), V(d_partner), None, None, V(d_verdict), V(d_remap), None, V(d_stats))
        assert rc == 0, lib.vo_last_error()

    def cull(dry):
        prm = vo.MapCullParams(1, 1, 0.0, 0.0, 0.0, 1, dry)
        rc = lib.voe_map_cull_batch_dev(m.h, I(1), K.ctypes.data_as(V), V(d_uv), S(L), V(d_rows), S(L), I(L), None, V(d_T), C.byref(prm), V(d_verdict),
                                        V(d_remap), None, V(d_cstats))
        assert rc == 0, lib.vo_last_error()

    what = {"fuse_us": (lambda: fuse(0), True), "fuse_dry_us": (lambda: fuse(1), False), "cull_us": (lambda: cull(0), True),
            "cull_dry_us": (lambda: cull(1), False)}
    runs = {k: [] for k in what}
    for r in range(a.rounds + 1):                             # the first round warms up (and sizes the workspaces)
        for k, (f, changes) in what.items():
            sync()
            t = time.perf_counter()
            f()
            sync()
            runs[k].append((time.perf_counter() - t) * 1e6)
            if changes:
                assert len(m) == L, (k, len(m))
                restore()
        print(f"round {r} done", flush=True)
    out = {"landmarks": L, "copies": D, "map_entries": M, "radius_xyz": a.radius_xyz, "radius": 0.1, "position": 1, "frames": 0,
           "push": "points U(-0.015, 0.015), appearances N(0, 0.005)"}
    for k in what:
        out[k] = round(statistics.median(runs[k][1:]), 1)
        out[k.replace("_us", "_runs_us")] = [round(x, 1) for x in runs[k][1:]]
    fuse(1)
    sync()
    st = vo.MapFuseStats(); raw = np.zeros(56, np.uint8); ctx.d2h(raw, d_stats); C.memmove(C.byref(st), raw.ctypes.data, 56)
    out["fuse_stats"] = st.as_dict()
    out["n_gated_per_entry"] = round(st.n_gated / max(st.n_before, 1), 4)
    out["pairs_are_the_planted"] = bool(st.n_pairs == D and st.n_after == L)
    out["fuse_minus_dry_us"] = round(out["fuse_us"] - out["fuse_dry_us"], 1)
    out["cull_minus_dry_us"] = round(out["cull_us"] - out["cull_dry_us"], 1)
    out["fuse_minus_cull_us"] = round(out["fuse_us"] - out["cull_us"], 1)
    res = {"device": ctx.device_info()[0], "stamp": stamp.current(),
           "measured": "every *_us figure below, on the device named above: wall time of one call between two synchronises, host launches included",
           "not_measured": "no kernel trace and no counters: how fuse_dry_us divides between the index build and the search is not in this file; no "
                           "call with frames (lookup, lists, veto, rows); no other density, radius_xyz or share of copies",
           "shape": out}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
