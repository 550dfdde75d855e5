#!/usr/bin/env python3
"""Runs every case of tests/map_loops_cases.py through voe_map_loops_batch_dev on the device and records, per case, how far Z lies
from rule 8 of include/vo_map_loops.h evaluated in float64 from the device's own float32 pose, in float32 ulps of the largest term
summed into the entry.  Both sides compute in double from the same float32 inputs, so the bound tests/test_gpu_map_loops.py holds
is one ulp -- the final rounding -- whatever this file says; it records what was seen.  Writes profiles/map_loops_budget.json.

    python tools/map_loops_budget.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as g  # noqa: E402
import map_loops_cases as Lc  # noqa: E402
import map_loops_restatement as L  # noqa: E402
from map_loops_dev import LoopsDev  # noqa: E402


def main():
    import stamp
    vo = g.load_package()
    ctx = vo.Context(0)
    cases = {}
    for name in Lc.CASES:
        d = LoopsDev(vo, ctx, Lc.case(name))
        try:
            d.clear_out()
            assert d.call() == 0, ctx.lib.vo_last_error()
            got, rec, _ = d.got()
            log = {}
            bad = L.compare(Lc.reference(name), got, log)
            cases[name] = dict(n_frames=d.F, n_max=d.n_max, max_loops=d.L, statuses=[L.STATUS[int(r["status"])] for r in rec], z_ulp_max=log["z_ulp"],
                               differences=bad)
            print(f"{name:14s} Z within {log['z_ulp']:.3f} ulp; {cases[name]['statuses']}; {bad or 'equal to the restatement'}")
        finally:
            d.close()
    out = dict(what="per case: the largest |Z_device - Z_rule8| over the OK slots' entries, in float32 ulps of the largest term summed into the entry; "
                    "rule 8 evaluated in float64 (tests/map_loops_restatement.edge_Z) from the device's own float32 pose and the float32 S_i",
               bound_ulp=1.0, device=ctx.device_info()[0], stamp=stamp.current(), cases=cases)
    path = os.path.join(ROOT, "profiles", "map_loops_budget.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
