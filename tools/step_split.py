#!/usr/bin/env python3
"""Where one headline step goes, kernel by kernel, from a rocprofv3 kernel trace of bench.py --no-extras.

usage: tools/step_split.py <dir with *kernel_trace.csv> [--json out.json]

A step ends with the finishing launch (picp_round_kernel<true, true, ...>) -- or, where the tail launch closes the solve
(picp_tail_kernel with no finishing launch behind it), with the tail launch; "finish" below is then that launch.  Everything
between the end of one finishing launch and the start of the next step's first PRE round (picp_round_kernel<true, false, ...>, or the tally instantiation
of round 1) is the FIXED part of a step:
it is listed launch by launch (gap in front of the kernel, kernel time).  The rounds are summarised start to start.  All
figures are medians over the steps of the trace that have the most common launch sequence (the timed region).  The tracer
itself stretches the gaps between plain launches (host-side cost per launch); kernel times and the gaps inside a graph
replay are what the untraced run sees.
"""
import csv
import glob
import json
import statistics
import sys
from collections import Counter


def short(name):
    name = name.replace("void ", "").replace("vo::", "")
    i = name.find("(")
    return (name if i < 0 else name[:i]).strip()


def load(d):
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under " + d)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    return rows


def main():
    d = sys.argv[1]
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    rows = load(d)
    # (round 1 of a solve, or the finishing launch of a one-round solve, is the instantiation that also takes the tally of
    # dropped pairs: picp_tally_round_kernel<FINISH, ...>)
    is_finish = lambda n: n.startswith(("picp_round_kernel<true, true", "picp_tally_round_kernel<true"))
    is_round = lambda n: n.startswith(("picp_round_kernel<true, false", "picp_tally_round_kernel<false"))
    # the one launch that stands for the rounds behind round M (picp_tail_kernel): between the last PRE round and the finish
    is_tail = lambda n: n.startswith("picp_tail_kernel")
    # its early form (picp_tail_kernel<PINHOLE, KEEP, true>) computes the repeating pose, finds the repeat and closes in one
    # launch: the headline step is then round 0, nine round launches and the tail -- 11 launches against 14
    is_early_tail = lambda n: is_tail(n) and n.replace(" ", "").endswith(",true>")
    # the tail launch closes the solve where the launch behind it is not a finishing launch
    tail_next = [rows[k + 1][2] for k in range(len(rows) - 1) if is_tail(rows[k][2])]
    tail_closes = bool(tail_next) and sum(1 for n in tail_next if not is_finish(n)) * 2 > len(tail_next)
    is_end = lambda n: is_tail(n) if tail_closes else is_finish(n)
    steps, cur, prev_end = [], [], None
    for s, e, n in rows:
        cur.append((s, e, n))
        if is_end(n):
            if prev_end is not None:
                steps.append((prev_end, cur))
            prev_end, cur = e, []
    sig = lambda st: tuple(n for _, _, n in st[1])
    common, count = Counter(sig(st) for st in steps).most_common(1)[0]
    steps = [st for st in steps if sig(st) == common]
    med = lambda xs: statistics.median(xs) / 1e3 if xs else float("nan")
    first_round = next(i for i, n in enumerate(common) if is_round(n))
    res = {"steps_used": len(steps), "launches_per_step": len(common), "tail_launch_closes_the_step": tail_closes,
           "tail_form": "early" if any(is_early_tail(n) for n in common) else ("plain" if any(is_tail(n) for n in common) else "none"),
           "launch_sequence": list(common), "fixed": [], "unit": "us"}
    print("%d steps of %d launches each (tail launch: %s)" % (len(steps), len(common), res["tail_form"]))
    print("fixed part (end of the finishing launch -> start of the first PRE round):")
    fixed_total = []
    for k in range(first_round + 1):
        gaps, durs = [], []
        for pe, st in steps:
            before = pe if k == 0 else st[k - 1][1]
            gaps.append(st[k][0] - before)
            durs.append(st[k][1] - st[k][0])
        if k < first_round:
            print("  gap %7.2f  kernel %7.2f  %s" % (med(gaps), med(durs), common[k]))
            res["fixed"].append({"kernel": common[k], "gap_before": med(gaps), "kernel_time": med(durs)})
        else:
            print("  gap %7.2f  (then the first PRE round starts)" % med(gaps))
            res["fixed"].append({"kernel": "(first PRE round starts)", "gap_before": med(gaps), "kernel_time": 0.0})
    for pe, st in steps:
        fixed_total.append(st[first_round][0] - pe)
    rr, rk, rg = [], [], []
    fin_gap, fin_dur, total = [], [], []
    tail_gap, tail_dur = [], []
    n_rounds = sum(1 for n in common if is_round(n))
    per_round = [([], []) for _ in range(n_rounds)]      # per round launch of the step: kernel times, start to next start
    for pe, st in steps:
        rounds = [x for x in st if is_round(x[2])]
        behind = [x for x in st if is_round(x[2]) or is_tail(x[2]) or x is st[-1]]
        for k, (a, b) in enumerate(zip(rounds, behind[1:])):
            per_round[k][0].append(a[1] - a[0])
            per_round[k][1].append(b[0] - a[0])
        for a, b in zip(rounds, rounds[1:]):
            rr.append(b[0] - a[0])
            rg.append(b[0] - a[1])
        rk += [e - s for s, e, _ in rounds]
        for k, x in enumerate(st):
            if is_tail(x[2]):
                tail_gap.append(x[0] - st[k - 1][1])
                tail_dur.append(x[1] - x[0])
        fin_gap.append(st[-1][0] - st[-2][1])
        fin_dur.append(st[-1][1] - st[-1][0])
        total.append(st[-1][1] - pe)
    # A round launch that finds its pose already seen returns at once: told from a real one by its kernel time (below half of
    # round 2's, the first plain round).  Their span: the sum of their start-to-next-start times.
    ktime = [med(k) for k, _ in per_round]
    span = [med(s) for _, s in per_round]
    real_time = ktime[1] if len(ktime) > 1 else float("nan")
    returning = [k for k in range(n_rounds) if ktime[k] < 0.5 * real_time]
    res.update({"round_launches": [{"round": k + 1, "kernel_time": ktime[k], "start_to_next_start": span[k]} for k in range(n_rounds)],
                "returning_launches": len(returning), "returning_span": sum(span[k] for k in returning),
                "real_launches": n_rounds - len(returning), "real_span": sum(span[k] for k in range(n_rounds) if k not in returning),
                "tail_launches_per_step": sum(1 for n in common if is_tail(n)), "tail_gap": med(tail_gap), "tail_kernel_time": med(tail_dur)})
    res.update({"fixed_total": med(fixed_total), "pre_rounds_per_step": n_rounds, "round_start_to_start": med(rr),
                "round_kernel_time": med(rk), "round_gap": med(rg), "finish_gap": med(fin_gap), "finish_kernel_time": med(fin_dur),
                "step_total": med(total)})
    print("  fixed part in all          %7.2f us" % res["fixed_total"])
    print("PRE rounds per step: %d ; start to start %.2f us (kernel %.2f + gap %.2f)"
          % (n_rounds, res["round_start_to_start"], res["round_kernel_time"], res["round_gap"]))
    print("of them returning at once: %d, span %.2f us; real: %d, span %.2f us"
          % (res["returning_launches"], res["returning_span"], res["real_launches"], res["real_span"]))
    if res["tail_launches_per_step"]:
        print("tail launch: gap %.2f us, kernel %.2f us" % (res["tail_gap"], res["tail_kernel_time"]))
    print("finishing launch: gap %.2f us, kernel %.2f us" % (res["finish_gap"], res["finish_kernel_time"]))
    print("step, finish end to finish end: %.2f us" % res["step_total"])
    if out_json:
        json.dump(res, open(out_json, "w"), indent=1)


if __name__ == "__main__":
    main()
