"""The yardstick of tests/test_gpu_picp_tail.py, checked without a GPU (tests/picp_budget.py: tail, check_tail, tail32;
tests/picp_cases.py: the large-step and tiny cases, ceiling_tail).

The solver's tail -- LDL^T of the 6x6 system, three sin / cos, R = Rx Ry Rz, T <- v2t(dx) T -- is a pure function of the float32
H (damping included) and b it solved and of the pose before the round.  picp_budget.tail gives its float64 value and a bound
without any sum over correspondences: C_LDLT 2^-24 |H^-1| (|R^T| |R|) |dx| plus the C_POSE composition term.

  * the input conditions of the large-step cases, on the float64 first step: which angles exceed 0.5 rad (the tail takes
    sincosf for all three when any does, its polynomial otherwise) and at least MIN_INLIERS float64 inliers;
  * the float32 restatement of the tail stays inside the bound on every case, old and new (the table is printed), and
    ceiling_tail() = min(1, 4 x its largest ratio) -- from the reference side only;
  * planted faults: what each is worth against ceiling_tail() on small-step and large-step cases, asserted caught where it is
    caught and asserted NOT seen where it is not (test_what_the_check_cannot_see)."""
import numpy as np
import pytest

import picp_budget as pb
import picp_cases as pc

OLD, NEW = pc.case_ids(), pc.tail_case_ids()
LARGE = [c for c in NEW if c[1] in pc.LARGE]
TINY = [c for c in NEW if c[1] not in pc.LARGE]
SMALL_STEP = [c for c in OLD if c[1] == "general" and c[0] in (257, 4097, 65537)] + TINY
# faults that move the pose by whole terms: caught on every case.  (stale_pose needs a pose one round older: _second_round)
GROSS = ("swap_angles", "compose_order", "drop_translation", "b_sign")
GRID = np.arange(0.5, 1.6001, 0.025)              # step angles about z the wrong-branch scan walks


def _first_angles(cid):
    return pc.tail_reference(cid)["tail"]["dx"][3:]


def _worth(H, b, T_at, fault, T_prev=None):
    return pb.check_tail(H, b, T_at, pb.tail32(H, b, T_at, fault=fault, T_prev=T_prev))


@pytest.fixture(scope="module")
def second_round():
    """cid -> (H32, b32, T1, T0): the float32 restatement's system at T1 = float32(v2t(dx64) T0), the pose after the first
    round.  The round a stale pose can show in: the pose one round older is T0."""
    cache = {}

    def get(cid):
        if cid not in cache:
            c = pc.case(cid)
            T1 = pc.tail_reference(cid)["tail"]["T1"].astype(np.float32)
            f = pb.system(*pc.system_args(c, T1), dt=np.float32)
            cache[cid] = ((f["H"] + np.eye(6, dtype=np.float32)).astype(np.float32), f["b"].astype(np.float32), T1, c["T0"])
        return cache[cid]
    return get


def test_tail_cases_beside_the_matrix():
    assert len(NEW) == len(set(NEW)) == 5 * 3 + 1 + 5 and not set(NEW) & set(OLD)
    assert len({pc.case_name(c) for c in OLD + NEW}) == len(OLD) + len(NEW)
    assert {c[0] for c in LARGE} == set(pc.LARGE_SIZES) and {c[0] for c in TINY} == set(pc.TINY_SIZES)
    for n in pc.LARGE_SIZES:
        assert {c[4] for c in LARGE if c[0] == n} == {"pinhole", "general"}
    assert all(c[2:4] == (10000.0, False) for c in NEW)


def test_tail_is_the_part_of_step_without_the_system_budget():
    """tail() and step() share their code: with exact H and b (A_X = E_X = 0) step()'s bound IS tail()'s, bit for bit"""
    for cid in (OLD[0], (4097, "general", 60.0, True, "general"), LARGE[0], LARGE[-1]):
        r = pc.tail_reference(cid)
        T0 = pc.case(cid)["T0"]
        H = r["H"].astype(np.float64)
        z6 = np.zeros((6, 6))
        ref = dict(H=H - np.eye(6), b=r["b"].astype(np.float64), A_H=z6 - np.eye(6), A_b=np.zeros(6), E_H=z6, E_b=np.zeros(6))
        assert np.array_equal(ref["H"] + np.eye(6), H)
        st, t = pb.step(ref, T0, 7.0), r["tail"]
        assert np.array_equal(st["dx"], t["dx"]) and np.array_equal(st["T1"], t["T1"])
        assert np.array_equal(st["tol"], t["tol"]) and np.array_equal(st["tol_system"], t["tol_ldlt"])
        assert np.array_equal(st["tol_pose"], t["tol_pose"]) and np.array_equal(t["tol"], t["tol_ldlt"] + t["tol_pose"])


def test_dx_of_inverts_the_composition():
    rng = np.random.default_rng(5)
    from np_restatement import v2t_euler
    for _ in range(50):
        dx = np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-1.4, 1.4, 3)])
        T0 = v2t_euler(np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)]))
        assert np.abs(pb.dx_of(v2t_euler(dx) @ T0, T0) - dx).max() < 1e-13


def test_large_step_inputs():
    """conditions on the INPUT, from the float64 step of the reference side: the angle pattern each kind is for, and enough
    inliers that the step is a step of the data and not of the damping"""
    seen = set()
    for cid in LARGE:
        ref = pc.reference(cid)[0]
        dx = np.linalg.solve(ref["H"] + np.eye(6), -ref["b"])            # the float64 step of the float64 system
        a32 = _first_angles(cid)                                         # and of the float32 system the tail is held on
        print(f"{pc.case_name(cid):40s} inliers {ref['n_in']:6d} of {cid[0]:6d}  step angles {np.round(dx[3:], 3)}  |t| {np.abs(dx[:3]).max():.3g}")
        assert ref["n_in"] >= pc.MIN_INLIERS, f"unsuitable input {pc.case_name(cid)}: {ref['n_in']} inliers"
        assert ref["n_amb"] <= pb.amb_cap(cid[0])
        for ang in (dx[3:], a32):
            assert pc.large_conditions(cid[1], ang), f"unsuitable input {pc.case_name(cid)}: step angles {ang}"
        assert np.abs(dx[3:] - a32).max() < 1e-3
        # which branch the kernel takes must not hang on a rounding: no angle within 0.02 of the switch
        assert (np.abs(np.abs(a32) - 0.5) > 0.02).all(), (cid, a32)
        seen.add(cid[1])
    assert seen == set(pc.LARGE)
    for cid in SMALL_STEP:
        assert np.abs(_first_angles(cid)).max() < 0.05, cid


def test_ceiling_tail_from_the_reference_side():
    """prints the ratio of the float32 restatement of the tail per case and ceiling_tail().  A correct float32 evaluation
    must stay inside the bound (ratio <= 1) whatever the conditioning: the one- to three-pair problems are there for that"""
    worst = 0.0
    print(f"\n{'case':44s} {'cond(H)':>9s} {'max angle':>9s} | tail32 / bound   ldlt share")
    for cid in OLD + NEW:
        r = pc.tail_reference(cid)
        t = r["tail"]
        worst = max(worst, r["ratio"])
        print(f"{pc.case_name(cid):44s} {np.linalg.cond(r['H'].astype(np.float64)):9.3g} {np.abs(t['dx'][3:]).max():9.3f} | {r['ratio']:8.4f}"
              f"         {float((t['tol_ldlt'] / t['tol']).max()):6.3f}")
        assert r["ratio"] <= 1.0, (cid, r["ratio"])
    Ct = pc.ceiling_tail()
    print(f"largest tail32 / bound {worst:.4f}  ->  ceiling_tail() = {Ct:.4f}")
    assert Ct == min(1.0, 4.0 * worst) and 0.0 < worst < 0.25


def _angle_where_the_polynomial_shows():
    """the smallest step angle (about z, on GRID) from which on the small-angle polynomial used beyond its range exceeds
    ceiling_tail(): the system of a large-step case, b chosen so that the step has that angle"""
    Ct = pc.ceiling_tail()
    cid = (4097, "large-z", 10000.0, False, "general")
    r = pc.tail_reference(cid)
    T0 = pc.case(cid)["T0"]
    rows = []
    for th in GRID:
        dx = r["tail"]["dx"].copy(); dx[5] = th
        b = (-(r["H"].astype(np.float64) @ dx)).astype(np.float32)
        rows.append((float(th), _worth(r["H"], b, T0, None), _worth(r["H"], b, T0, "poly_everywhere")))
    above = [i for i, row in enumerate(rows) if row[2] > Ct]
    first = next(i for i in above if all(j in above for j in range(i, len(rows))))
    return rows[first][0], rows


def test_wrong_branch_case():
    """the 0.5 rad switch is no accuracy cliff: the polynomial stays inside the ceiling far beyond it.  The scan finds the angle
    from which on it does not; a Gauss-Newton step of a pure roll is about sin(roll) and never gets there, a roll seen from
    closer (the scale multiplies the step) does: large-roll is that case, with its inlier floor like every large-step case.
    A kernel that took the polynomial at 0.5 < angle < that angle would not be seen (test_what_the_check_cannot_see)."""
    Ct = pc.ceiling_tail()
    th, rows = _angle_where_the_polynomial_shows()
    for row in rows:
        print(f"step angle {row[0]:.3f}: tail32 / bound {row[1]:.4f}   polynomial everywhere {row[2]:.4f}")
    print(f"the polynomial beyond its range exceeds ceiling_tail() = {Ct:.4f} from a step angle of {th:.3f} rad on")
    assert 0.5 < th < 1.6
    for cid in [c for c in LARGE if c[1] in pc.WRONG_BRANCH]:
        r = pc.tail_reference(cid)
        a = _first_angles(cid)
        w = _worth(r["H"], r["b"], pc.case(cid)["T0"], "poly_everywhere")
        print(f"{pc.case_name(cid)}: step angles {np.round(a, 3)}, {pc.reference(cid)[0]['n_in']} inliers, polynomial everywhere {w:.3g} = {w / Ct:.3g} ceilings")
        assert np.abs(a).max() >= th and w > Ct and pc.reference(cid)[0]["n_in"] >= pc.MIN_INLIERS
    assert [c for c in LARGE if c[1] in pc.WRONG_BRANCH]


@pytest.mark.parametrize("cid", SMALL_STEP + LARGE, ids=pc.case_name)
def test_planted_faults_are_caught(cid, second_round):
    """every fault of TAIL_FAULTS in units of ceiling_tail(), in round 1 and (stale_pose) in round 2.  The four gross faults
    and the stale pose are caught on every small-step and every large-step case; the reciprocal and the polynomial are
    reported here and asserted where they belong (test_wrong_branch_case, test_what_the_check_cannot_see)."""
    Ct = pc.ceiling_tail()
    r = pc.tail_reference(cid)
    T0 = pc.case(cid)["T0"]
    line = [f"{pc.case_name(cid)}: clean {r['ratio'] / Ct:.3g}"]
    for fault in pb.TAIL_FAULTS:
        if fault == "stale_pose":
            continue
        w = _worth(r["H"], r["b"], T0, fault)
        line.append(f"{fault} {w / Ct:.3g}")
        if fault in GROSS:
            # caught = over the ceiling; from 3 pairs on by orders of magnitude (below, cond(H) of 1e5 widens the bound)
            assert w > (10 * Ct if cid[0] >= 3 else Ct), (cid, fault, w, Ct)
    if cid[0] <= 65537:
        H, b, T1, Tp = second_round(cid)
        assert pb.check_tail(H, b, T1, pb.tail32(H, b, T1)) <= Ct
        w = _worth(H, b, T1, "stale_pose", T_prev=Tp)
        line.append(f"stale_pose (round 2) {w / Ct:.3g}")
        assert w > (10 * Ct if cid[0] >= 3 else Ct), (cid, "stale_pose", w, Ct)
    print(" | ".join(line) + "   [x ceiling_tail]")


def test_what_the_check_cannot_see(second_round):
    """what passes the tail check although it is wrong, and why that is accepted"""
    Ct = pc.ceiling_tail()
    # (1) the polynomial below the angle test_wrong_branch_case finds: at every large-step case but large-roll a tail that
    # always took the polynomial stays under the ceiling -- its error at 0.5 ... 0.8 rad is an ulp or two of the sine
    th, _ = _angle_where_the_polynomial_shows()
    for cid in [c for c in LARGE if c[1] not in pc.WRONG_BRANCH]:
        r = pc.tail_reference(cid)
        assert 0.5 < np.abs(_first_angles(cid)).max() < th or cid[1] == "large-mid"
        w = _worth(r["H"], r["b"], pc.case(cid)["T0"], "poly_everywhere")
        assert w <= Ct, (cid, w, Ct)
    # (2) a reciprocal 2e-6 (17 ulp) off: LDL^T with D^-1 wrong by a relative delta solves a system whose D is wrong by
    # delta -- a backward error of delta |R^T| |R|, the form of the bound itself, and 2e-6 = 34 x 2^-24 is of the order of
    # C_LDLT = 19.  It sits AT the ceiling: over it on some cases, under it on others, nowhere by a factor of 3.  Counted,
    # and held to be invisible in general
    seen, ws = 0, []
    for cid in SMALL_STEP + LARGE:
        r = pc.tail_reference(cid)
        ws.append(_worth(r["H"], r["b"], pc.case(cid)["T0"], "recip_17ulp"))
        seen += ws[-1] > Ct
    print(f"recip_17ulp: over ceiling_tail() on {seen} of {len(ws)} cases; worth {min(ws) / Ct:.3g} ... {max(ws) / Ct:.3g} ceilings")
    assert 0 < len(ws) - seen and max(ws) < 3 * Ct
    # (3) a stale pose once the solver stands still: the pose one round older IS the pose
    cid = (257, "general", 60.0, True, "general")
    H, b, T1, _ = second_round(cid)
    assert np.array_equal(pb.tail32(H, b, T1, fault="stale_pose", T_prev=T1), pb.tail32(H, b, T1))
    # (4) the batched forms return no H and b: picp_budget.check_step holds their step with the budget of an n-term sum on
    # top of this bound -- the share of the tail in that bound, at the 4097-pair large-step cases
    C = pc.ceiling()
    for cid in [c for c in LARGE if c[0] == 4097]:
        st = pb.step(pc.reference(cid)[0], pc.case(cid)["T0"], C)
        t = pc.tail_reference(cid)["tail"]
        share = float((t["tol"] / st["tol"]).max())
        print(f"{pc.case_name(cid)}: the tail's bound is {share:.3g} of check_step's")
        assert share < 0.5


def test_host_build_of_the_tail_sources():
    """csrc/vo_math.h's own ldlt6_solve_ordered (FMA updates), sincos_small / sincosf under the kernel's one branch,
    v2t_from_sincos and the composition, compiled for the host and put together as picp_tail_direct puts them together
    (tests/hostcheck/hostcheck.cpp: hc_picp_tail_fast), on every case: inside ceiling_tail() like the restatement.  What the
    GPU adds to this is the Newton reciprocal, the cross-lane data movement and where the old pose comes from."""
    import ctypes as C
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    so, src = os.path.join(here, "hostcheck", "libvo_hostcheck.so"), os.path.join(here, "hostcheck", "hostcheck.cpp")
    hdr = os.path.join(here, "..", "visual-odometry_amd", "csrc", "vo_math.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so, src])
    hc = C.CDLL(so)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    Ct = pc.ceiling_tail()
    worst = 0.0
    for cid in OLD + NEW:
        r = pc.tail_reference(cid)
        T0 = np.asarray(pc.case(cid)["T0"], np.float32)
        out = np.zeros(16, np.float32)
        hc.hc_picp_tail_fast(p(np.ascontiguousarray(r["H"].T).ravel()), p(r["b"]), p(np.ascontiguousarray(T0.T).ravel()), p(out))
        w = pb.check_tail(r["H"], r["b"], T0, out.reshape(4, 4).T)
        worst = max(worst, w)
        assert w <= Ct, (cid, w, Ct)
    print(f"host build of the tail: largest step / bound {worst:.4f} (ceiling_tail() {Ct:.4f})")
