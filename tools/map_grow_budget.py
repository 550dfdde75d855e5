#!/usr/bin/env python3
"""The budget of tests/test_gpu_map_grow.py, measured on the CPU alone: per case of tests/map_grow_cases.py the distance of the
float64 restatement's double point and mean_sq_px between the forward and the reversed order of summation, with the counts the
CPU test pins; and for the example data the distances of the added points to world.dat, which set the default bound of
apps/grow_map -> profiles/map_grow_budget.json.  Usage: python tools/map_grow_budget.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import map_grow_cases as Gc  # noqa: E402


def record(name):
    r = Gc.reference(name)
    st = r["stats"]
    return dict(status=int(st["status"]), n_open=int(st["n_open"]), n_tracks=int(st["n_tracks"]), n_added=int(st["n_added"]),
                by_verdict=st["by_verdict"], sum_n_obs_sq=r["sum_n_obs_sq"], n_rounding=int(r["rounding"].sum()), **Gc.spreads(name))


def distances(name):
    """the distances of the added points of an example-data case to world.dat, matched by appearance"""
    c, r = Gc.case(name), Gc.reference(name)
    key = {a.tobytes(): k for k, a in enumerate(c["truth_app"])}
    d = np.array([np.linalg.norm(p.astype(np.float64) - c["truth"][key[a.tobytes()]].astype(np.float64)) for p, a in r["added_rows"]])
    return dict(n_added=len(d), median=float(np.median(d)), largest=float(d.max()))


def downstream():
    """the cost per observation (sum of |e|^2 over all observations of all frames, no Huber) of world.dat and of the map the
    restatement grows back after the cull of the 40 pushed landmarks: what a bundle of either starts from"""
    import map_cull_restatement as Q
    c, r = Gc.case("example_after_cull"), Gc.reference("example_after_cull")
    out = {}
    for name, (pts, app) in (("world", (c["truth"], c["truth_app"])), ("grown", (r["points"], r["app"]))):
        s = Q.cull(c["K"], pts, app, c["frames"], c["poses"], min_obs=1, min_frames=1, max_rms_px=0.0, dry_run=True)
        out[name + "_cost_per_observation"] = float((s["mean_sq_px"] * s["n_obs"]).sum() / s["n_obs"].sum())
        out[name + "_observations"] = int(s["n_obs"].sum())
    return out


if __name__ == "__main__":
    out = dict(what="per case: point_order_rel -- the largest distance of a track's DOUBLE point between the forward-order and the "
                    "reversed-order float64 runs, relative to its largest coordinate; mean_order_rel -- the same for mean_sq_px, relative; "
                    "n_rounding -- tracks whose double point lies within 8 a-priori bounds of a float32 midpoint.  The GPU test allows "
                    "4 x the spread plus twice the restatement's a-priori rounding bound (tests/map_grow_restatement.py).  example: "
                    "the distances of the added points to world.dat; apps/grow_map's default bound is 2 x the largest of "
                    "example_from_empty_two_views.  downstream: the cost per observation a bundle starts from, on world.dat and on "
                    "the map grown back after the cull of the 40 pushed landmarks (example_after_cull)",
               cases={n: record(n) for n in Gc.CASES},
               example={n: distances(n) for n in ("example_from_empty", "example_from_empty_two_views", "example_removed", "example_after_cull")},
               downstream=downstream())
    with open(os.path.join(ROOT, "profiles", "map_grow_budget.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1)[:3000])
