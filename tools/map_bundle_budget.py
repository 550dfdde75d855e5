#!/usr/bin/env python3
"""The budget of tests/test_gpu_map_bundle.py, measured on the CPU alone: per case the distance between the float64
restatement's forward-order and reversed-order runs (tests/map_bundle_restatement.py), in pixels, with the statuses and counts
the CPU test pins -> profiles/map_bundle_budget.json.  Usage: python tools/map_bundle_budget.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import map_bundle_cases as Bc  # noqa: E402


def record(name):
    r = Bc.reference(name)
    poses, points = Bc.reach(name)
    return dict(status=int(r["status"]), n_obs=int(r["stats"]["n_obs"]), n_free_frames=int(r["stats"]["n_free_frames"]),
                n_free_points=int(r["stats"]["n_free_points"]), accepted=[int(x["accepted"]) for x in r["rounds"]],
                cg_iterations=[int(x["cg_iterations"]) for x in r["rounds"]], reach_pose_px=poses, reach_point_px=points)


if __name__ == "__main__":
    out = dict(what="distance between the forward-order and the reversed-order float64 runs, largest over the free frames "
                    "(H-norm in the final U_f) and over the free landmarks (in the final V_j); the GPU test allows 4 x this plus "
                    "the half ulps of the stored float32 entries", cases={n: record(n) for n in Bc.CASES})
    with open(os.path.join(ROOT, "profiles", "map_bundle_budget.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["cases"], indent=1))
