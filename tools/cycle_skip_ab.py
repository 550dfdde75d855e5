#!/usr/bin/env python3
"""A/B of the cycle skip on ONE GPU in one session (DESIGN.md section 8's rule): builds alternate run by run.

    python tools/cycle_skip_ab.py --lib parent=PATH --lib change=PATH [--lib NAME=PATH ...] --out FILE

Every run is a fresh child `python bench.py ...` with VO_HIP_LIB set; the first child that fails ends the script.
  headline     five plain runs per build
  iters_100    --iters 100 (the slope of the step time between 50 and 100 rounds is the cost of a skipped launch)
  ten_rounds   --iters 10 --steps 1000, five per build: nothing can be skipped, the cost of control word and detector
  outputs      --dump-outputs per build, compared byte for byte with the first build's
  sequence     one --full --legs sequence line per build (100 rounds per frame), recorded only"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import stamp  # noqa: E402


def bench(lib, extra, env_extra=None, timeout=300):
    env = dict(os.environ, VO_HIP_LIB=lib, **(env_extra or {}))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra], capture_output=True, text=True, env=env, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench.py {' '.join(extra)} on {lib} ended with {r.returncode}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def row(d):
    return {"value": d["value"], "ms_per_step": d["ms_per_step"], "launch_us": d["roofline"]["launch_us"]}


def summary(rows):
    v = [r["value"] for r in rows]
    return {"runs": rows, "median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v),
            "median_us_per_step": statistics.median(r["ms_per_step"] for r in rows) * 1e3}


def alternating(libs, extra, reps):
    rows = {name: [] for name, _ in libs}
    for i in range(reps):
        for name, path in libs:
            rows[name].append(row(bench(path, extra)))
            print(name, extra, rows[name][-1], flush=True)
    return {name: summary(r) for name, r in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True, help="NAME=PATH, the parent first")
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-sequence", action="store_true")
    ap.add_argument("--only", default=None, help="headline or ten_rounds: that part alone")
    a = ap.parse_args()
    libs = [(x.split("=", 1)[0], os.path.abspath(x.split("=", 1)[1])) for x in a.lib]
    out = {"what": "python bench.py per build, builds alternating run by run on one MI355X in one session; value = PICP iterations/s",
           "rule": "kept if the slowest run of the change beats the fastest run of the parent in the same session",
           "builds": [n for n, _ in libs]}

    def save():
        out["stamp"] = stamp.current()
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    if a.only:
        out[a.only] = alternating(libs, {"headline": [], "ten_rounds": ["--iters", "10", "--steps", "1000"]}[a.only], a.reps)
        save()
        return
    out["headline"] = alternating(libs, [], a.reps)
    save()
    out["iters_100"] = alternating(libs, ["--iters", "100"], 3)
    save()
    out["ten_rounds"] = alternating(libs, ["--iters", "10", "--steps", "1000"], a.reps)
    save()
    dumps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, path in libs:
            d = os.path.join(tmp, name)
            bench(path, ["--steps", "20", "--warmup", "2", "--dump-outputs", d])
            dumps[name] = {f: open(os.path.join(d, f), "rb").read().hex() for f in sorted(os.listdir(d))}
    first = libs[0][0]
    out["outputs"] = {"files": sorted(dumps[first]), "identical_to_" + first: {n: dumps[n] == dumps[first] for n, _ in libs}}
    save()
    if not a.skip_sequence:
        out["sequence"] = {name: bench(path, ["--full", "--legs", "sequence", "--steps", "20", "--warmup", "2"], timeout=600).get("sequence")
                           for name, path in libs}
        save()
    print(json.dumps({k: out[k] for k in ("outputs",)}))


if __name__ == "__main__":
    main()
