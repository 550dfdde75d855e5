#!/usr/bin/env python3
"""A/B of the early form of the tail launch on ONE GPU in one session: builds alternate run by run.

    python tools/tail_early_ab.py --parent PATH --change PATH --out FILE [--model-us X] [--parts a,b,...]

Every run is a fresh child `python bench.py ...` with VO_HIP_LIB set; the first child that fails ends the script.
  headline     five plain runs per build; accepted if the slowest run of the change beats the fastest run of the parent;
               --model-us: the step model written down before the measurement, the gap to the median step is recorded
  capture      one headline run of the change with VO_PICP_TAIL_LOG=1: at which solve of the handle each graph was captured;
               the early form's must fall inside the untimed steps (bench.py's pre-warm plus warm-up)
  iters_100    --iters 100, three per build
  ten_rounds   --iters 10 --steps 1000, five per build: the form is not eligible, the median must lie within the parent's
               max - min spread
  parts        the change's headline with VO_PICP_TAIL_EARLY=0 (the parent's forms in the change's build), three runs
  outputs      --dump-outputs per build, and of the change forced into the early form (VO_PICP_TAIL_EARLY=1 at
               VO_PICP_TAIL_FROM=9: the dump's few steps never reach the tier on their own), compared byte for byte
  sequence     --full --legs sequence, two per build, alternating: frames never repeat, the form stays off
Everything but the headline runs with --no-extras.  The file is rewritten after every part, parts already in it are kept: the
script may be run part by part."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import stamp  # noqa: E402
from tools.cycle_skip_ab import alternating, bench, row, summary  # noqa: E402

PARTS = ("headline", "capture", "iters_100", "ten_rounds", "parts", "outputs", "sequence")


def capture_log(lib, untimed):
    env = dict(os.environ, VO_HIP_LIB=lib, VO_PICP_TAIL_LOG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-extras"], capture_output=True, text=True, env=env, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("bench.py with VO_PICP_TAIL_LOG=1 ended with %d" % r.returncode)
    caps = [{"rounds": int(a), "tail_from": int(b), "early": bool(e), "at_solve": int(c)}
            for a, b, e, c in re.findall(r"graph of (\d+) rounds, tail_from (\d+)( \(early form\))?, captured at solve (\d+)", r.stderr)]
    early = [c for c in caps if c["early"]]
    return {"captures": caps, "untimed_steps": untimed, "early_form_captured": bool(early),
            "all_inside_the_untimed_steps": all(c["at_solve"] <= untimed for c in caps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--change", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--model-us", type=float, default=None, help="the step model's headline step of the change, us")
    ap.add_argument("--untimed", type=int, default=120, help="bench.py's pre-warm plus warm-up steps")
    ap.add_argument("--parts", default=",".join(PARTS))
    a = ap.parse_args()
    libs = [("parent", os.path.abspath(a.parent)), ("change", os.path.abspath(a.change))]
    change = libs[1][1]
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out.update({"what": "python bench.py per build, builds alternating run by run on one MI355X in one session; value = PICP iterations/s; "
                        "all parts but the headline with --no-extras",
                "rule": "kept if the slowest run of the change beats the fastest run of the parent in the same session",
                "builds": [n for n, _ in libs]})

    def save():
        out["stamp"] = stamp.current()
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for part in a.parts.split(","):
        if part == "headline":
            h = alternating(libs, [], 5)
            h["accepted"] = h["change"]["min"] > h["parent"]["max"]
            h["median_ratio"] = h["change"]["median"] / h["parent"]["median"]
            if a.model_us is not None:
                h["model_us_per_step"] = a.model_us
                h["median_minus_model_us"] = h["change"]["median_us_per_step"] - a.model_us
            out[part] = h
        elif part == "capture":
            out[part] = capture_log(change, a.untimed)
        elif part == "iters_100":
            out[part] = alternating(libs, ["--no-extras", "--iters", "100"], 3)
        elif part == "ten_rounds":
            t = alternating(libs, ["--no-extras", "--iters", "10", "--steps", "1000"], 5)
            t["change_median_within_parent_spread"] = abs(t["change"]["median"] - t["parent"]["median"]) <= t["parent"]["spread"]
            out[part] = t
        elif part == "parts":
            out[part] = {"early_off": summary([row(bench(change, ["--no-extras"], {"VO_PICP_TAIL_EARLY": "0"})) for _ in range(3)])}
        elif part == "outputs":
            dumps = {}
            with tempfile.TemporaryDirectory() as tmp:
                for name, path, env in [(n, p, None) for n, p in libs] + [("change_forced_early", change, {"VO_PICP_TAIL_EARLY": "1", "VO_PICP_TAIL_FROM": "9"})]:
                    d = os.path.join(tmp, name)
                    bench(path, ["--steps", "20", "--warmup", "2", "--dump-outputs", d], env)
                    dumps[name] = {f: open(os.path.join(d, f), "rb").read().hex() for f in sorted(os.listdir(d))}
            out[part] = {"files": sorted(dumps["parent"]), "identical": dumps["parent"] == dumps["change"],
                         "forced_early_identical": dumps["parent"] == dumps["change_forced_early"]}
        elif part == "sequence":
            runs = {name: [] for name, _ in libs}
            for _ in range(2):
                for name, path in libs:
                    runs[name].append(bench(path, ["--full", "--legs", "sequence", "--steps", "20", "--warmup", "2"], timeout=600).get("sequence"))
            fps = {name: [r["frames_per_sec"] for r in rs] for name, rs in runs.items()}
            out[part] = {"runs": runs, "frames_per_sec": fps,
                         "change_median_within_parent_spread": abs(statistics.median(fps["change"]) - statistics.median(fps["parent"]))
                         <= max(fps["parent"]) - min(fps["parent"])}
        else:
            raise SystemExit("unknown part " + part)
        save()
        print(part, json.dumps(out[part])[:1500], flush=True)


if __name__ == "__main__":
    main()
