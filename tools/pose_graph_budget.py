#!/usr/bin/env python3
"""Measures, on the CPU alone, how far the restatement of voe_pose_graph* moves when every sum over the edges is taken in the
opposite order: per case of tests/pose_graph_cases.py and per frame, sqrt(d^T H_ff d) between the two double states.  Four
times that, plus half an ulp of each stored float32 entry, is the ceiling tests/test_gpu_pose_graph.py holds the device to; no
device value goes into it.  Writes profiles/pose_graph_budget.json; tests/test_pose_graph_cpu.py re-measures it.

    python tools/pose_graph_budget.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import pose_graph_cases as Cc  # noqa: E402
import pose_graph_restatement as P  # noqa: E402


def main():
    cases = {}
    for name in Cc.CASES:
        ref = Cc.reference(name)
        reach = Cc.reach(name)
        hu = P.half_ulp(ref, ref["S_out"])
        cases[name] = dict(status=P.STATUS[ref["status"]], n_frames=int(ref["stats"]["n_frames"]), n_edges=int(ref["stats"]["n_edges"]),
                           accepted="".join(str(r["accepted"]) for r in ref["rounds"]), reach_max=float(reach.max(initial=0.0)),
                           half_ulp_max=float(hu.max(initial=0.0)))
        print(f"{name:28s} {cases[name]['status']:12s} reach {cases[name]['reach_max']:.3g}  half ulps {cases[name]['half_ulp_max']:.3g}")
    out = dict(what="per case: the largest distance, over the frames, between the forward-order and the reversed-order run of "
                    "tests/pose_graph_restatement.py, in sqrt(d^T H_ff d); the GPU test's ceiling is 4 x reach_max + the half ulps of the stored state",
               measured_on="the CPU alone (NumPy float64)", numpy=np.__version__, cases=cases)
    path = os.path.join(ROOT, "profiles", "pose_graph_budget.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
