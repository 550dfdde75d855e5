#!/usr/bin/env python3
"""Where the fast solver's pose trajectory first repeats ("rounds that have already occurred").

    VO_PICP_CYCLE=0 python tools/cycle_first_repeat.py [--seeds 2000-2007] [--points 50000] [--rounds 100] [--out FILE]

For every seed the pair synth.frame_pair(points, seed) goes through bench.py's own route (match, join, transform), then the
solver runs n_iters = 1 .. rounds from the identity with cycle detection off and the pose is fetched each time: pose k is the
pose after k rounds, pose 0 the identity.  "k = j" is the first k whose pose equals, bit for bit, the pose of an earlier round
j (the most recent one).  Written per seed for the first 50 and the first `rounds` rounds."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402
from tools import stamp  # noqa: E402


def first_repeat(poses, upto):
    """poses[k]: bytes of the pose after k rounds.  (k, j) of the first repeat within rounds 0..upto, or None."""
    for k in range(1, min(upto, len(poses) - 1) + 1):
        for j in range(k - 1, -1, -1):
            if poses[j] == poses[k]:
                return k, j
    return None


def trajectory(vo, ctx, fp, rounds):
    pipe = vo.FramePipeline(ctx, fp, n_iters=1, kernel_threshold=10000.0)
    pipe.match(); pipe.join(); pipe.transform()
    ctx.synchronize()
    poses = [np.eye(4, dtype=np.float32).tobytes()]
    for n in range(1, rounds + 1):
        pipe.n_iters = n
        pipe.picp()
        poses.append(np.ascontiguousarray(pipe.pose(), np.float32).tobytes())
    pipe.close()
    return poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="2000-2007")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lo, _, hi = a.seeds.partition("-")
    seeds = range(int(lo), int(hi or lo) + 1)
    vo = graft.load_package()
    ctx = vo.Context(0)
    out = {"what": "first bitwise repeat of the pose in the fast solver's own trajectory, detection off: k = j reads pose after "
                   "round k equals pose after round j (pose 0 = identity); bench.py's route (match, join, transform, solve_dev)",
           "points": a.points, "rounds": a.rounds, "cycle_env": os.environ.get("VO_PICP_CYCLE"), "seeds": {}}
    for s in seeds:
        poses = trajectory(vo, ctx, vo.synth.frame_pair(a.points, seed=s), a.rounds)
        row = {}
        for upto in sorted({50, a.rounds}):
            r = first_repeat(poses, upto)
            row[f"within_{upto}"] = None if r is None else {"k": r[0], "j": r[1], "period": r[0] - r[1]}
        out["seeds"][str(s)] = row
        print(s, row, flush=True)
    out["stamp"] = stamp.current()
    line = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    else:
        print(line)


if __name__ == "__main__":
    main()
