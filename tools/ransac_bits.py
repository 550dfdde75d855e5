#!/usr/bin/env python3
"""The bits both RANSAC front ends return at the sizes where the code they share (ransac_common.h: scoring tile, mask tail,
scatter, selection) takes different paths, recorded once as the fixture of tests/test_gpu_ransac_bits.py: a change that keeps
arithmetic and operand order must return every one of them unchanged.  Counts are integers and every float here is computed
by one thread, so nothing depends on scheduling.

Inputs: those of tests/test_gpu_ransac_sizes.py (synth.frame_pair of 300 000 pairs, seeds 4200 / 4300, 30 % of the second
indices replaced, a wild in-range tail behind the live pairs where n_max > live, call seed n_hyp + live).  Calls: tests/
ransac_dev.py, dev_call(..., always_read=True) for the epipolar form and Dev for the P3P form.

Cases (n_hyp, live pairs, n_max): one hypothesis in one partial workgroup; the edges of the 64-hypothesis block, the 256-pair
mask / scatter workgroup and the 1024-pair scoring tile; the selection loop past 1024 threads; live counts below the
capacity; the second pass of the gather loop's 1024 workgroups; and, P3P only, 3 live pairs: the fallback (status not OK, the
mask is every live pair, the pose the identity).

Recorded per case: the SHA-256 of the inputs' bytes (a changed input generator shows as that, not as a kernel difference),
the SHA-256 of counts[n_hyp] (the -1 entries included) and mask[n_max], and
  epipolar: return code, n_inliers, X -- the compacted pairs stay in the context's workspace; X is the refit of exactly those
            pairs in their compacted order (vo_estimate_transform_dev on them), n_inliers their count;
  P3P:      status, T16, the compacted pairs and their count.

usage (GPU box, repo root, on the commit whose bits are the reference):
    tools/ransac_bits.py --commit $(git rev-parse HEAD) [--out tests/golden/ransac_bits.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SHARED = [(64, 256, 256), (65, 257, 257), (127, 1023, 1023), (1025, 1025, 1025), (64, 1025, 4097), (4097, 257, 511),
          (65, 262145, 262145)]
EPI_CASES = [(1, 9, 9)] + SHARED
POSE_CASES = [(1, 4, 4)] + SHARED + [(64, 3, 256)]
FIXTURE = os.path.join(ROOT, "tests", "golden", "ransac_bits.json")


def cid(case):
    return "-".join(str(v) for v in case)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def inputs(vo):
    """the two problems of tests/test_gpu_ransac_sizes.py (its epi_data and pose_data fixtures)"""
    import pose_ransac_restatement as P
    import ransac_restatement as R
    fp = vo.synth.frame_pair(300000, seed=4200, noise_px=0.25)
    pairs, _ = R.corrupt(fp["gt_matches"], len(fp["cur_pts"]), 0.3, seed=4)
    epi = dict(K=fp["K"], p1=fp["ref_pts"], p2=fp["cur_pts"], pairs=pairs)
    fp, world, meas, pairs, _, _ = P.tracking_problem(vo, 300000, seed=4300, noise_px=0.5, frac=0.3, max_angle=0.3, max_t=0.5)
    pose = dict(K=fp["K"], world=np.asarray(world, np.float32), meas=np.asarray(meas, np.float32), pairs=pairs)
    return dict(epi=epi, pose=pose)


def _buffer(pairs, n, n_max, n1, n2, seed):
    import test_gpu_ransac_sizes as sizes
    pr = np.ascontiguousarray(pairs[:n], np.int32)
    return sizes._wild_tail(pr, n_max, n1, n2, seed + 1) if n_max > n else pr


def epi_bits(vo, ctx, d, case):
    """-> {inputs, rc, n_inliers, X, mask, counts} of one vo_estimate_transform_ransac_dev call"""
    import test_gpu_ransac_sizes as sizes
    from ransac_dev import dev_call
    n_hyp, n, n_max = case
    seed = n_hyp + n
    buf = _buffer(d["pairs"], n, n_max, len(d["p1"]), len(d["p2"]), seed)
    rc, X, mask, counts, n_in = dev_call(vo, ctx, d["K"], buf, d["p1"], d["p2"], n_hyp, sizes.EPI_THR, seed,
                                         n_live=n if n_max > n else None, always_read=True)
    return dict(inputs=sha(np.asarray(d["K"], np.float32), buf, d["p1"], d["p2"], np.array([n_hyp, n, n_max, seed], np.int64)),
                rc=int(rc), n_inliers=int(n_in), X=sha(X.astype(np.float32)), mask=sha(mask), counts=sha(counts))


def pose_bits(vo, ctx, d, case):
    """-> {inputs, status, n_pairs, T16, pairs, mask, counts} of one vo_estimate_pose_ransac_dev call"""
    import test_gpu_ransac_sizes as sizes
    from ransac_dev import Dev
    n_hyp, n, n_max = case
    seed = n_hyp + n
    buf = _buffer(d["pairs"], n, n_max, len(d["meas"]), len(d["world"]), seed)
    dev = Dev(vo, ctx, d["K"], d["world"], d["meas"], buf)
    try:
        dev.set_live(n)
        rc = dev.call(n_hyp=n_hyp, thr=sizes.POSE_THR, seed=seed)
        assert rc == 0, rc
        T, inl, nin, mask, counts, st = dev.results(n_hyp)
    finally:
        dev.close()
    return dict(inputs=sha(np.asarray(d["K"], np.float32), buf, d["world"], d["meas"], np.array([n_hyp, n, n_max, seed], np.int64)),
                status=int(st), n_pairs=int(nin), T16=sha(T.astype(np.float32)), pairs=sha(inl), mask=sha(mask), counts=sha(counts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None, help="hash of the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    import __graft_entry__ as g
    vo = g.load_package()
    ctx = vo.Context(0)
    data = inputs(vo)
    cases = {"epipolar": {}, "p3p": {}}
    for case in EPI_CASES:
        cases["epipolar"][cid(case)] = epi_bits(vo, ctx, data["epi"], case)
        print("epipolar", case, cases["epipolar"][cid(case)], flush=True)
    for case in POSE_CASES:
        cases["p3p"][cid(case)] = pose_bits(vo, ctx, data["pose"], case)
        print("p3p", case, cases["p3p"][cid(case)], flush=True)
    rep = {"what": "SHA-256 of the inputs' and of each output array's bytes, and the scalars, of both RANSAC front ends' device "
                   "calls (n_hyp-live-n_max); written by tools/ransac_bits.py",
           "commit": commit, "device": str(ctx.device_info()[0]), "library": os.path.basename(vo.LIB_PATH), "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
