#!/usr/bin/env python3
"""The bits a PICP solve returns at the sizes where the round kernels take different paths, recorded once as the fixture of
tests/test_gpu_round_chain.py: a change of picp_round_body that keeps arithmetic, operand order and summation order must
return every one of them unchanged.

Cases: tests/picp_cases.py, selected as tests/test_gpu_round_rows.py does (cid_of): 257 pairs (2 partial rows), 8 193 (33
rows, a partial row group), 65 537 (a second pass of 256 rows) and 300 001 (the grid cap: threads loop over several
correspondences).  1, 2 and 18 rounds each (gathering round -> tally round -> plain rounds and the wrap of the 16-slot ring).
Recorded per case and round count: pose, H, b, the chi^2 sums and the inlier count, as the hex of their bytes.

usage (GPU box, repo root, on the commit whose bits are the reference):
    tools/round_bits.py --commit $(git rev-parse HEAD) [--out tests/golden/picp_round_bits.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = (257, 8193, 65537, 300001)
ROUNDS = (1, 2, 18)
FIXTURE = os.path.join(ROOT, "tests", "golden", "picp_round_bits.json")


def solve_bits(vo, ctx, n, rounds=ROUNDS):
    """-> {str(k): {T, H, b, chi_in, chi_out, n_in as hex}} of a closed solve of k rounds on the case of n pairs"""
    import picp_cases as pc
    import test_gpu_round_rows as rows
    c = pc.case(rows.cid_of(n))
    out = {}
    for k in rounds:
        s = vo.PICPSolver(ctx)
        s.setKernelThreshold(c["thr"])
        s.init(vo.Camera(pc.ROWS, pc.COLS, pc.Z_NEAR, pc.Z_FAR, c["K"], c["T0"], ctx=ctx), c["world"], c["meas"])
        s.solve(c["corr"], c["keep"], k)
        H, b = s.system()
        rec = dict(T=s.camera().worldInCameraPose().astype(np.float32), H=np.asarray(H), b=np.asarray(b),
                   chi_in=np.float32(s.chiInliers()), chi_out=np.float32(s.chiOutliers()), n_in=np.int32(s.numInliers()))
        s.close()
        out[str(k)] = {key: np.asarray(v).tobytes().hex() for key, v in rec.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None, help="hash of the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    import __graft_entry__ as g
    vo = g.load_package()
    ctx = vo.Context(0)
    cases = {}
    for n in SIZES:
        cases[str(n)] = solve_bits(vo, ctx, n)
        print(f"{n} pairs: rounds {sorted(cases[str(n)], key=int)} recorded", flush=True)
    rep = {"what": "bytes (hex) of pose, H, b, chi^2 sums and inlier count of closed PICP solves; written by tools/round_bits.py",
           "commit": commit, "device": str(ctx.device_info()[0]), "library": os.path.basename(vo.LIB_PATH),
           "sizes": list(SIZES), "rounds": list(ROUNDS), "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
