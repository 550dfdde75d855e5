#!/usr/bin/env python3
"""The budget of tests/test_gpu_map_cull.py, measured on the CPU alone: per case of tests/map_cull_cases.py the distance of the
float64 restatement's mean_sq_px between the forward and the reversed order of summation, and what another expression order
(sums taken z, y, x; the ray normalised by a reciprocal) moves in mean_sq_px, max_sq_px, min_z and cos_parallax, with the counts
the CPU test pins -> profiles/map_cull_budget.json.  Usage: python tools/map_cull_budget.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import map_cull_cases as Cc  # noqa: E402


def record(name):
    r = Cc.reference(name)
    return dict(status=int(r["stats"]["status"]), n_before=int(r["stats"]["n_before"]), n_kept=int(r["stats"]["n_kept"]),
                n_obs=int(r["stats"]["n_obs"]), by_verdict=r["stats"]["by_verdict"], sum_n_obs_sq=r["sum_n_obs_sq"], **Cc.spreads(name))


if __name__ == "__main__":
    out = dict(what="per case: mean_order_rel -- the largest relative distance of an entry's mean_sq_px between the forward-order and "
                    "the reversed-order float64 runs; *_expr_* -- the largest distance between two expression orders (relative for "
                    "mean_sq_px and max_sq_px, absolute for min_z and cos_parallax).  The GPU test allows 4 x the spread plus twice "
                    "the restatement's a-priori rounding bound of the statistic (tests/map_cull_restatement.py)",
               cases={n: record(n) for n in Cc.CASES})
    with open(os.path.join(ROOT, "profiles", "map_cull_budget.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["cases"], indent=1))
