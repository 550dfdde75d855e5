#!/usr/bin/env python3
"""A/B of the submission form of learned tail-form solves ("Between two steps") on ONE GPU in one session:
builds alternate run by run.  The parent is the build of the commit this branches from, never a switch of the new build.

    python tools/tail_submit_ab.py --parent PATH --change PATH --out FILE [--model-us X] [--parts a,b,...]

Every run is a fresh child `python bench.py ...` with VO_HIP_LIB set; the first child that fails ends the script.
  headline     five plain runs per build; accepted if the slowest run of the change beats the fastest run of the parent;
               --model-us: the step model written down before the measurement, the gap to the median step is recorded
  ring_m12     the same with VO_PICP_TAIL_EARLY=0 (the learned ring form at M = 12): whether that tier is in the rule
  default_m    the tier the rule leaves on the graph, in the change's build alone: VO_PICP_TAIL_FROM=16 (skip-path solves at the
               default M) with VO_PICP_TAIL_SUBMIT=graph against =plain, five each, alternating
  capture      one headline run of the change with VO_PICP_TAIL_LOG=1: which graphs the handle captured and at which solve it
               first submitted plainly; both must fall inside the untimed steps (bench.py's pre-warm plus warm-up)
  ten_rounds   --iters 10 --steps 1000, five per build: no tail form, the median must lie within the parent's max - min
  outputs      --dump-outputs per build, and of the change forced plain into the early form (VO_PICP_TAIL_SUBMIT=plain,
               VO_PICP_TAIL_EARLY=1 at VO_PICP_TAIL_FROM=9: the dump's few steps never reach the tier on their own), byte for byte
  sequence     --full --legs sequence, two per build, alternating: frames never repeat, the form stays off (sequence_second_call:
               the same once more under that name, where the first call's medians lay outside the parent's two-run spread)
  host_loop    the change alone: wall time of bench.py's enqueue loop (set_pose_dev + solve_dev per step, 200 steps behind 120
               untimed) before the final barrier, per step, beside the device time of the same steps -- three children
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

PARTS = ("headline", "ring_m12", "default_m", "capture", "ten_rounds", "outputs", "sequence", "host_loop")


def capture_log(lib, untimed):
    env = dict(os.environ, VO_HIP_LIB=lib, VO_PICP_TAIL_LOG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-extras"], capture_output=True, text=True, env=env, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("bench.py with VO_PICP_TAIL_LOG=1 ended with %d" % r.returncode)
    caps = [{"rounds": int(a), "tail_from": int(b), "early": bool(e), "at_solve": int(c)}
            for a, b, e, c in re.findall(r"graph of (\d+) rounds, tail_from (\d+)( \(early form\))?, captured at solve (\d+)", r.stderr)]
    first = [{"at_solve": int(a), "rounds": int(b), "tail_from": int(c), "early": bool(e)}
             for a, b, c, e in re.findall(r"solve (\d+) of the handle is its first submitted as plain launches: (\d+) rounds, tail_from (\d+)( \(early form\))?", r.stderr)]
    return {"captures": caps, "first_plain": first, "untimed_steps": untimed,
            "all_inside_the_untimed_steps": all(c["at_solve"] <= untimed for c in caps + first)}


def host_loop():
    """child: bench.py's loop on the library VO_HIP_LIB names; one JSON line"""
    import time
    import torch
    import __graft_entry__ as entry
    vo = entry.load_package()
    stream = torch.cuda.Stream(device="cuda:0")
    ctx = vo.Context(0, stream.cuda_stream)
    fp = vo.synth.frame_pair(50000, seed=2000)
    pipe = vo.FramePipeline(ctx, fp, n_iters=50, kernel_threshold=10000.0)
    with torch.cuda.stream(stream):
        pipe.match(); pipe.join(); pipe.transform()
        ctx.synchronize()
        for _ in range(120):
            pipe.picp()
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        steps = 200
        ev0.record(stream)
        t0 = time.perf_counter()
        for _ in range(steps):
            pipe.picp()
        t1 = time.perf_counter()
        ev1.record(stream)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    g, p = C_submit(vo, pipe)
    print(json.dumps({"host_us_per_step": (t1 - t0) * 1e6 / steps, "device_us_per_step": ev0.elapsed_time(ev1) * 1e3 / steps,
                      "wall_us_per_step_with_barrier": (t2 - t0) * 1e6 / steps, "graph_solves": g, "plain_solves": p}))
    pipe.close()


def C_submit(vo, pipe):
    import ctypes as C
    g, p = C.c_ulonglong(), C.c_ulonglong()
    if not hasattr(pipe.lib, "voe_picp_submit_info"):
        return None, None
    pipe.lib.voe_picp_submit_info(pipe.solver, C.byref(g), C.byref(p))
    return g.value, p.value


def main():
    if sys.argv[1:] == ["--host-loop"]:
        return host_loop()
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

    def tier(extra, reps=5):
        h = alternating(libs, extra, reps)
        h["accepted"] = h["change"]["min"] > h["parent"]["max"]
        h["median_ratio"] = h["change"]["median"] / h["parent"]["median"]
        return h

    for part in a.parts.split(","):
        if part == "headline":
            h = tier([])
            if a.model_us is not None:
                h["model_us_per_step"] = a.model_us
                h["median_minus_model_us"] = h["change"]["median_us_per_step"] - a.model_us
            out[part] = h
        elif part == "ring_m12":
            os.environ["VO_PICP_TAIL_EARLY"] = "0"
            try:
                out[part] = tier(["--no-extras"])
            finally:
                del os.environ["VO_PICP_TAIL_EARLY"]
        elif part == "default_m":
            rows = {"graph": [], "plain": []}
            for _ in range(5):
                for form in rows:
                    rows[form].append(row(bench(change, ["--no-extras"], {"VO_PICP_TAIL_FROM": "16", "VO_PICP_TAIL_SUBMIT": form})))
            d = {f: summary(r) for f, r in rows.items()}
            d["plain_slowest_beats_graph_fastest"] = d["plain"]["min"] > d["graph"]["max"]
            out[part] = d
        elif part == "capture":
            out[part] = capture_log(change, a.untimed)
        elif part == "ten_rounds":
            t = alternating(libs, ["--no-extras", "--iters", "10", "--steps", "1000"], 5)
            t["change_median_within_parent_spread"] = abs(t["change"]["median"] - t["parent"]["median"]) <= t["parent"]["spread"]
            out[part] = t
        elif part == "outputs":
            dumps = {}
            forced = {"VO_PICP_TAIL_SUBMIT": "plain", "VO_PICP_TAIL_EARLY": "1", "VO_PICP_TAIL_FROM": "9"}
            with tempfile.TemporaryDirectory() as tmp:
                for name, path, env in [(n, p, None) for n, p in libs] + [("change_forced_plain_early", change, forced)]:
                    d = os.path.join(tmp, name)
                    bench(path, ["--steps", "20", "--warmup", "2", "--dump-outputs", d], env)
                    dumps[name] = {f: open(os.path.join(d, f), "rb").read().hex() for f in sorted(os.listdir(d))}
            out[part] = {"files": sorted(dumps["parent"]), "identical": dumps["parent"] == dumps["change"],
                         "forced_plain_early_identical": dumps["parent"] == dumps["change_forced_plain_early"]}
        elif part in ("sequence", "sequence_second_call"):
            runs = {name: [] for name, _ in libs}
            for _ in range(2):
                for name, path in libs:
                    runs[name].append(bench(path, ["--full", "--legs", "sequence", "--steps", "20", "--warmup", "2"], timeout=600).get("sequence"))
            fps = {name: [r["frames_per_sec"] for r in rs] for name, rs in runs.items()}
            out[part] = {"runs": runs, "frames_per_sec": fps,
                         "change_median_within_parent_spread": abs(statistics.median(fps["change"]) - statistics.median(fps["parent"]))
                         <= max(fps["parent"]) - min(fps["parent"])}
        elif part == "host_loop":
            rows = []
            for _ in range(3):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-loop"], capture_output=True, text=True,
                                   env=dict(os.environ, VO_HIP_LIB=change), timeout=300, cwd=ROOT)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-4000:])
                    raise SystemExit("the host loop ended with %d" % r.returncode)
                rows.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
            out[part] = {"runs": rows, "median_host_us_per_step": statistics.median(x["host_us_per_step"] for x in rows),
                         "median_device_us_per_step": statistics.median(x["device_us_per_step"] for x in rows)}
        else:
            raise SystemExit("unknown part " + part)
        save()
        print(part, json.dumps(out[part])[:1500], flush=True)


if __name__ == "__main__":
    main()
