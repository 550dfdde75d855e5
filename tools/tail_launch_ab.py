#!/usr/bin/env python3
"""A/B of the tail launch (picp_tail_kernel) on ONE GPU in one session (DESIGN.md section 8's rule): builds alternate run by run.

    python tools/tail_launch_ab.py --parent PATH --change PATH --out FILE

Every run is a fresh child `python bench.py ...` with VO_HIP_LIB set; the first child that fails ends the script.
  headline     five plain runs per build
  iters_100    --iters 100, three per build
  ten_rounds   --iters 10 --steps 1000, five per build: the tail form is not chosen, the round kernels must cost what they did
  loop_price   the change with VO_PICP_TAIL_FROM=2 at --iters 10 --steps 1000: rounds 3 .. 9 run inside the tail launch, seven
               grid barriers in place of seven kernel boundaries; us per in-launch round = launched round + difference / 7
  m_sweep      one headline run of the change at VO_PICP_TAIL_FROM 12, 16, 24
  outputs      --dump-outputs per build, compared byte for byte
  sequence     one --full --legs sequence line per build (100 rounds per frame), recorded only
Everything but the headline runs with --no-extras (the headline figure does not depend on the other legs)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import stamp  # noqa: E402
from tools.cycle_skip_ab import alternating, bench, row, summary  # noqa: E402

LAUNCHED_ROUND_US = 3.45      # the slope of the step between 50 and 100 real rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--change", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--skip-sequence", action="store_true")
    a = ap.parse_args()
    libs = [("parent", os.path.abspath(a.parent)), ("change", os.path.abspath(a.change))]
    change = libs[1][1]
    out = {"what": "python bench.py per build, builds alternating run by run on one MI355X in one session; value = PICP iterations/s; "
                   "all parts but the headline with --no-extras",
           "rule": "kept if the slowest run of the change beats the fastest run of the parent in the same session",
           "builds": [n for n, _ in libs]}

    def save():
        out["stamp"] = stamp.current()
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    out["headline"] = alternating(libs, [], 5)
    h = out["headline"]
    out["headline"]["accepted"] = h["change"]["min"] > h["parent"]["max"]
    out["headline"]["median_ratio"] = h["change"]["median"] / h["parent"]["median"]
    save()
    out["iters_100"] = alternating(libs, ["--no-extras", "--iters", "100"], 3)
    save()
    ten = ["--no-extras", "--iters", "10", "--steps", "1000"]
    out["ten_rounds"] = alternating(libs, ten, 5)
    t = out["ten_rounds"]
    out["ten_rounds"]["change_median_within_parent_spread"] = abs(t["change"]["median"] - t["parent"]["median"]) <= t["parent"]["spread"]
    save()
    loop = summary([row(bench(change, ten, {"VO_PICP_TAIL_FROM": "2"})) for _ in range(3)])
    diff = loop["median_us_per_step"] - t["parent"]["median_us_per_step"]
    out["loop_price"] = {"tail_from_2": loop, "us_more_than_parent_step": diff, "in_launch_rounds": 7,
                         "us_per_in_launch_round": LAUNCHED_ROUND_US + diff / 7, "launched_round_us": LAUNCHED_ROUND_US}
    save()
    out["m_sweep"] = {m: row(bench(change, ["--no-extras"], {"VO_PICP_TAIL_FROM": m})) for m in ("12", "16", "24")}
    save()
    dumps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, path in libs:
            d = os.path.join(tmp, name)
            bench(path, ["--steps", "20", "--warmup", "2", "--dump-outputs", d])
            dumps[name] = {f: open(os.path.join(d, f), "rb").read().hex() for f in sorted(os.listdir(d))}
    out["outputs"] = {"files": sorted(dumps["parent"]), "identical": dumps["parent"] == dumps["change"]}
    save()
    if not a.skip_sequence:
        out["sequence"] = {name: bench(path, ["--full", "--legs", "sequence", "--steps", "20", "--warmup", "2"], timeout=600).get("sequence")
                           for name, path in libs}
        save()
    print(json.dumps({k: out[k] for k in ("outputs", "loop_price", "m_sweep")}, indent=1))
    print(json.dumps({k: {b: {x: out[k][b][x] for x in ("median", "min", "max", "median_us_per_step")} for b in ("parent", "change")}
                      for k in ("headline", "iters_100", "ten_rounds")}, indent=1))


if __name__ == "__main__":
    main()
