"""The yardstick of tests/test_gpu_picp_system.py, checked without a GPU (tests/picp_budget.py, tests/picp_cases.py).

  * the float64 restatement against the float64 oracle: two independent statements of one formula;
  * the ceiling C of the statistic rho, measured on the reference's formulas in float32 with pairwise sums over the whole
    case matrix (the table is printed; o32's sequential sums beside it for comparison -- they grow with n and bound nothing);
  * planted faults: what the check catches, by how much, and -- where it cannot see a fault -- that too, which is the reason
    for the poses and sizes of the case matrix."""
import numpy as np
import pytest

import np_restatement as npr
import picp_budget as pb
import picp_cases as pc
from oracle.oracle import Camera as OCam

CASES = pc.case_ids()
GENERAL = [c for c in CASES if c[1] == "general"]


def _oracle(o, c, iters=1):
    return o.picp_solve(OCam(pc.ROWS, pc.COLS, pc.Z_NEAR, pc.Z_FAR, c["K"], c["T0"]), c["world"], c["meas"], c["corr"], iters,
                        c["thr"], c["keep"])


def test_case_matrix():
    assert pc.CAP == 262144 and len(CASES) == len(set(CASES)) == 14 + 7 + 2 * 18
    assert {c[0] for c in GENERAL if c[2:4] == (60.0, True)} == set(pc.SIZES)
    for n in pc.FULL:
        assert len([c for c in CASES if c[0] == n]) == 18


def test_restatement_equals_float64_oracle(o64):
    """H64, b64 and the statistics of round 0 against o64 to n 2^-52 A_X per entry -- what two float64 summation orders can
    differ by -- the decisions exactly; and against np_restatement.linearize, the matrix-product form of the same formulas"""
    for cid in CASES:
        c = pc.case(cid)
        ref = pc.reference(cid)[0]
        r = _oracle(o64, c)
        n = max(ref["n"], 1)
        eps = n * 2.0 ** -52
        assert int(r["stats"][0, 2]) == ref["n_in"], cid
        assert (np.abs(r["H"][0] - ref["H"]) <= eps * ref["A_H"]).all(), cid
        assert (np.abs(r["b"][0] - ref["b"]) <= eps * ref["A_b"]).all(), cid
        assert abs(r["stats"][0, 0] - ref["chi_in"]) <= eps * ref["A_chi_in"], cid
        assert abs(r["stats"][0, 1] - ref["chi_out"]) <= eps * ref["A_chi_out"], cid
        if cid[0] <= 65537:
            H, b, ci, co, ni = npr.linearize(*pc.system_args(c))
            assert ni == ref["n_in"]
            assert (np.abs(H - ref["H"]) <= 4 * eps * ref["A_H"]).all() and (np.abs(b - ref["b"]) <= 4 * eps * ref["A_b"]).all(), cid
            assert abs(ci - ref["chi_in"]) <= eps * ref["A_chi_in"] and abs(co - ref["chi_out"]) <= eps * ref["A_chi_out"], cid


def test_ambiguous_share_is_inside_the_cap():
    for cid in CASES:
        ref = pc.reference(cid)[0]
        assert ref["n_amb"] <= pb.amb_cap(cid[0]), f"unsuitable input {pc.case_name(cid)}: {ref['n_amb']} ambiguous correspondences"


def test_ceiling_from_the_reference_side(o32):
    """prints rho of both float32 restatements per case and C = 4 max rho(pairwise).  rho of a correct float32 evaluation is
    about the number of roundings on the longest chain (pc 3, ph 3, 1 / z 1, g 2, Jp K 2, skew 2, J^T J 2, lambda 1, the sum):
    the measured maximum must sit below that count, 24, or the budget is not what it claims"""
    C = pc.ceiling()
    print(f"\n{'case':44s} {'n_in':>7s} {'n_out':>7s} {'amb':>3s} | pairwise float32: H b chi_in chi_out | sequential float32 (o32): H b chi_in chi_out")
    worst = 0.0
    for cid in CASES:
        ref, r32 = pc.reference(cid)
        o = _oracle(o32, pc.case(cid))
        ro = pb.rho_system(ref, o["H"][0], o["b"][0], o["stats"][0, 0], o["stats"][0, 1], int(o["stats"][0, 2]))
        worst = max(worst, r32["worst"])
        f = lambda r: " ".join(f"{r[k]:8.2f}" for k in ("H", "b", "chi_in", "chi_out"))
        print(f"{pc.case_name(cid):44s} {ref['n_in']:7d} {ref['n_out']:7d} {ref['n_amb']:3d} | {f(r32)} | {f(ro)}")
        assert r32["n_in_ok"] and ro["n_in_ok"], cid
    print(f"largest pairwise-float32 rho {worst:.3f}  ->  C = {C:.3f}")
    assert C == 4.0 * worst and 0.25 < worst < 24.0


@pytest.mark.parametrize("cid", GENERAL, ids=pc.case_name)
def test_planted_faults_are_caught(cid):
    C = pc.ceiling()
    c = pc.case(cid)
    ref = pc.reference(cid)[0]
    a = pc.system_args(c)
    line = [pc.case_name(cid)]
    for fault in pb.VALUE_FAULTS:
        if fault == "lambda_one" and not (c["keep"] and ref["n_out"] > 0):
            continue
        f = pb.system(*a, fault=fault)
        r = pb.rho_system(ref, f["H"], f["b"], f["chi_in"], f["chi_out"], f["n_in"])
        line.append(f"{fault}: H {r['H']:.3g} b {r['b']:.3g}")
        assert max(r["H"], r["b"]) > 10 * C, (cid, fault, r)
    assert ref["n_in"] - pb.system(*a, fault="drop_block")["n_in"] > 0, "unsuitable input: no inlier among the last 256 pairs"
    for fault in pb.COVERAGE_FAULTS:
        f = pb.system(*a, fault=fault)
        dn = abs(f["n_in"] - ref["n_in"])
        r = pb.rho_system(ref, f["H"], f["b"], f["chi_in"], f["chi_out"], f["n_in"])
        rs = pb.rho_system(ref, f["H"], f["b"], f["chi_in"], f["chi_out"])          # the sums alone, the count not looked at
        line.append(f"{fault}: dn {dn} amb {ref['n_amb']} sums {rs['worst']:.3g}")
        if fault == "drop_last_inlier":
            # one term: caught by the count where no correspondence is ambiguous.  Where some are, an inlier fewer is what
            # the default arithmetic may legitimately report, and one term of 65 535 or more is inside the budget of the sums
            # (asserted: the fault is NOT seen there) -- which is why every size also has a case without ambiguous pairs
            assert dn == 1
            if ref["n_amb"] == 0:
                assert not r["n_in_ok"], (cid, fault, r)
            elif r["n_in_ok"] and r["worst"] <= C:
                assert cid[0] >= 65535 and rs["worst"] <= C, (cid, fault, r)
                line.append("(not seen)")
        else:
            assert dn > ref["n_amb"], (cid, fault, dn)
            assert not r["n_in_ok"] or r["worst"] > C, (cid, fault, r)
    print(" | ".join(line))


def test_every_size_has_a_case_whose_count_is_exact():
    for n in pc.SIZES:
        assert any(pc.reference(c)[0]["n_amb"] == 0 for c in GENERAL if c[0] == n), n


def test_what_the_check_cannot_see():
    """why the case matrix has general poses and reads the inlier count"""
    C = pc.ceiling()
    # (1) at the identity the camera point IS the world point: a Jacobian built from the world point changes nothing at all
    for cid in [c for c in CASES if c[1] == "identity"]:
        ref = pc.reference(cid)[0]
        f = pb.system(*pc.system_args(pc.case(cid)), fault="world_point")
        assert np.array_equal(f["H"], ref["H"]) and np.array_equal(f["b"], ref["b"]), cid
    # (2) a solver that returns no H and b (the batched forms) is held through its one-step pose: the same fault moves the step
    # by `ratio` bounds (picp_budget.step; > 1 fails).  At the small start poses the fault is worth a fraction of what it is
    # at a general pose -- hence the general start poses of the batched tests, where every case must show it (the margin is printed: the step is a far blunter view of H than H itself)
    def ratio(cid):
        c = pc.case(cid)
        ref = pc.reference(cid)[0]
        f = pb.system(*pc.system_args(c), fault="world_point")
        st = pb.step(ref, c["T0"], C)
        dx = np.linalg.solve(f["H"] + np.eye(6), -f["b"])
        return float((np.abs(dx - st["dx"]) / st["tol"]).max())
    for n in pc.FULL:
        for thr, keep in pc.SETTINGS:
            for k in ("pinhole", "general"):
                rs, rg = ratio((n, "small", thr, keep, k)), ratio((n, "general", thr, keep, k))
                print(f"world point, step of {n}-thr{int(thr)}-{'keep' if keep else 'drop'}-{k}: {rs:.3g} bounds at the small pose, {rg:.3g} at the general pose")
                assert rg > 2 and rg > 5 * rs, (n, thr, keep, k, rs, rg)
    # (3) one term of 262 145 is inside the budget of the sums: a dropped correspondence is caught by the count, not by rho
    cid = (pc.CAP + 1, "general", 60.0, True, "pinhole")
    ref = pc.reference(cid)[0]
    f = pb.system(*pc.system_args(pc.case(cid)), fault="drop_last_inlier")
    r = pb.rho_system(ref, f["H"], f["b"], f["chi_in"], f["chi_out"])
    print(f"last inlier dropped at {pc.case_name(cid)}: rho of the sums alone {r['worst']:.3g} (C = {C:.3g}), count {f['n_in'] - ref['n_in']}")
    assert r["chi_in"] < C and f["n_in"] == ref["n_in"] - 1
