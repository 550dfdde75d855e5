"""The fetch of the previous launch's partial rows at the head of a PICP round (picp_round_body, step (1)) at the sizes
where it can go wrong: one row, a partial group of 32 rows (1, 2, 31, 33 rows), whole groups (32), a partial 256-row pass
(255), a whole one (256), a second pass (257, 1024) and the grid cap with threads looping (1024 rows for 300 001 pairs).
1, 2 and 18 rounds each: the rows of a gathering round 0 read by the tally kernel, the plain round kernel behind it, and
the wrap of the 16-slot ring.

Per case a closed solve must equal the same number of vo_picp_one_round calls bit for bit (pose, H, b, statistics), and the
last round's H, b and chi^2 sums are held entry by entry to tests/picp_budget.py's float64 values at the pose that round
linearised at, within picp_cases.ceiling() roundings of each entry's own budget and under the decision-band rule of
tests/test_gpu_picp_system.py (both from the reference side).  A row lost or read twice moves the sums by a whole
workgroup's terms, hundreds of times that ceiling: asserted once below on a copy of the expected values.

256 pairs are one workgroup, which the solver runs in its one-launch form; VO_PICP_SMALL=0 (read once per process) keeps them
on the round kernels, so that one case runs in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import picp_budget as pb
import picp_cases as pc

pytestmark = pytest.mark.gpu

# (pairs, partial rows on a 256-CU device)
SIZES = ((256, 1), (257, 2), (7936, 31), (8192, 32), (8193, 33), (65280, 255), (65536, 256), (65537, 257), (262144, 1024),
         (300001, 1024))
ROUNDS = (1, 2, 18)                               # 18 wraps the 16-slot ring
BLOCK, MAX_BLOCKS = 256, 2048                     # PICP_BLOCK, PICP_MAX_BLOCKS (csrc/vo_internal.h)


def rows_of(n, n_cu):
    """picp_grid_for (csrc/picp.hip): one workgroup per 256 pairs, at most 4 per CU"""
    return max(1, min((n + BLOCK - 1) // BLOCK, 4 * n_cu if n_cu > 0 else 1024, MAX_BLOCKS))


def cid_of(n):
    """general pose (R far from I); the settings and K alternate over the sizes: (60, keep) weighs kept outliers, at
    (10000, drop) every pair that passes the gates is an inlier and, from round 2 on, the count must be n exactly"""
    i = [s for s, _ in SIZES].index(n)
    thr, keep = ((60.0, True), (10000.0, False))[i % 2]
    return (n, "general", thr, keep, ("pinhole", "general")[(i // 2) % 2])


def _solver(vo, ctx, c):
    s = vo.PICPSolver(ctx)
    s.setKernelThreshold(c["thr"])
    s.init(vo.Camera(pc.ROWS, pc.COLS, pc.Z_NEAR, pc.Z_FAR, c["K"], c["T0"], ctx=ctx), c["world"], c["meas"])
    return s


def _read(s):
    H, b = s.system()
    out = dict(T=s.camera().worldInCameraPose().astype(np.float32), H=H, b=b, chi_in=np.float32(s.chiInliers()),
               chi_out=np.float32(s.chiOutliers()), n_in=np.int32(s.numInliers()))
    s.close()
    return {k: np.asarray(v).tobytes().hex() for k, v in out.items()}


def run_case(vo, ctx, n):
    """-> {rounds k: dict(closed, chain, before)}: the closed solve of k rounds, k vo_picp_one_round calls, and the pose after
    k - 1 rounds (what round k linearised at), every array as the hex of its bytes"""
    c = pc.case(cid_of(n))
    out = {}
    for k in ROUNDS:
        s = _solver(vo, ctx, c)
        s.solve(c["corr"], c["keep"], k)
        closed = _read(s)
        s = _solver(vo, ctx, c)
        for _ in range(k):
            s.oneRound(c["corr"], c["keep"])
        chain = _read(s)
        before = None
        if k > 1:
            s = _solver(vo, ctx, c)
            s.solve(c["corr"], c["keep"], k - 1)
            before = _read(s)["T"]
        out[str(k)] = dict(closed=closed, chain=chain, before=before)
    return out


def _arr(rec, key, dtype=np.float32, shape=None):
    a = np.frombuffer(bytes.fromhex(rec[key]), dtype)
    return a.reshape(shape) if shape else a


def _hold(ref, got, C, what):
    """test_gpu_picp_system's check of one read-back system: every entry within C roundings of its own float64 budget, the
    ambiguous correspondences decided one way for all of H, b, the chi^2 sums and the count"""
    H, b = _arr(got, "H", shape=(6, 6)), _arr(got, "b")
    ci, co, ni = _arr(got, "chi_in")[0], _arr(got, "chi_out")[0], int(_arr(got, "n_in", np.int32)[0])
    assert ref["n_amb"] <= pb.amb_cap(ref["n"]), f"unsuitable input {what}: {ref['n_amb']} ambiguous correspondences"
    assert np.array_equal(H, H.T), f"{what}: H is not symmetric bit for bit"
    r = pb.rho_system(ref, H, b, ci, co, ni, damping=1.0)
    print(f"{what}: rho H {r['H']:.3g} b {r['b']:.3g} chi_in {r['chi_in']:.3g} chi_out {r['chi_out']:.3g}  n_in {ni} (float64 {ref['n_in']}, "
          f"{ref['n_amb']} ambiguous)  C {C:.3g}")
    assert abs(ni - ref["n_in"]) <= ref["n_amb"], f"{what}: {ni} inliers, float64 {ref['n_in']}, {ref['n_amb']} ambiguous"
    assert r["n_in_ok"], f"{what}: no decision of the ambiguous correspondences gives {ni} inliers"
    assert r["worst"] <= C, f"{what}: {r}"


@pytest.mark.parametrize("n,rows", SIZES, ids=[f"{n}-pairs-{r}-rows" for n, r in SIZES])
def test_round_rows(vo, ctx, n, rows):
    assert rows_of(n, ctx.device_info()[1]) == rows, f"{n} pairs are {rows_of(n, ctx.device_info()[1])} rows on this device, not {rows}"
    if n <= BLOCK:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n)], capture_output=True, text=True,
                           env=dict(os.environ, VO_PICP_SMALL="0"), timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        res = json.loads(r.stdout.strip().splitlines()[-1])
    else:
        res = run_case(vo, ctx, n)
    C = pc.ceiling()
    cid = cid_of(n)
    c = pc.case(cid)
    for k in ROUNDS:
        rec = res[str(k)]
        what = f"{pc.case_name(cid)} ({rows} rows) round {k}"
        assert rec["closed"] == rec["chain"], f"{what}: the closed solve and {k} single rounds differ: {rec}"
        if k == 1:
            ref = pc.reference(cid)[0]
        else:
            T_at = _arr(rec, "before", shape=(4, 4))
            assert np.isfinite(T_at).all()
            ref = pb.system(*pc.system_args(c, T_at))
        assert np.isfinite(_arr(rec["closed"], "T")).all()
        _hold(ref, rec["closed"], C, what)


def test_a_lost_or_doubled_row_is_far_outside_the_ceiling():
    """what the check above is worth against the fault it is for, on the expected values alone (no GPU): one of 1024 rows --
    a workgroup's 256 pairs -- left out of, or added twice to, the float64 sums of the largest case that does not loop"""
    n, rows = SIZES[8]
    assert n == rows * BLOCK
    C = pc.ceiling()
    cid = cid_of(n)
    c = pc.case(cid)
    ref = pc.reference(cid)[0]
    for row in (0, rows // 2 + 1, rows - 1):
        part = dict(c, corr=c["corr"][row * BLOCK:(row + 1) * BLOCK])
        f = pb.system(*pc.system_args(part))
        assert f["n_in"] + f["n_out"] > 0
        for sign, name in ((-1.0, "lost"), (1.0, "doubled")):
            H = ref["H"] + sign * f["H"] + np.eye(6)
            rs = pb.rho_system(ref, H, ref["b"] + sign * f["b"], ref["chi_in"] + sign * f["chi_in"], ref["chi_out"] + sign * f["chi_out"],
                               damping=1.0)                                # the sums alone, the count not looked at
            print(f"row {row} of {rows} {name}: rho H {rs['H']:.3g} b {rs['b']:.3g} chi_in {rs['chi_in']:.3g} chi_out {rs['chi_out']:.3g}  C {C:.3g}")
            # H(0, 0) sums squares, so its budget is its value (up to the kept outliers' weights) and 1/1024 of it is
            # 2^14 roundings of that budget; the chi^2 sums carry the pixel magnitudes in their budget and see far less
            assert rs["H"] > 10 * C, (row, name, rs)
        assert f["n_in"] > ref["n_amb"], (row, f["n_in"], ref["n_amb"])    # and the inlier count moves by more than is open


if __name__ == "__main__":                          # the child process of the one-workgroup case
    import __graft_entry__ as g
    _vo = g.load_package()
    print(json.dumps(run_case(_vo, _vo.Context(0), int(sys.argv[1]))))
