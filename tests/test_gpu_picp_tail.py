"""The default-arithmetic PICP solver's tail -- what turns the summed H and b into the next pose -- against float64.

tests/test_gpu_picp_system.py holds H, b and the chi^2 sums entry by entry; the pose was so far compared with the float32
oracle after whole chains, at 1e-4.  Here every round read back is held on its own: vo_picp_get_system returns the float32 H
(damping included) and b the tail solved, the pose before the round is known (the start pose, the previous read-back, or a
twin handle's solve(k - 1): same data, same bits), and the tail is a pure function of the three.  picp_budget.check_tail
compares the step the GPU pose took, dx_of(T_out, T_at), with H^-1 (-b) in float64, in units of a bound that holds no sum over
correspondences (C_LDLT 2^-24 |H^-1| (|R^T| |R|) |dx| plus the composition's roundings); the result must not exceed
picp_cases.ceiling_tail(), which comes from the reference side alone (tests/test_picp_tail_cpu.py prints it, and what a swapped
angle, a composition the wrong way round, a dropped translation, a stale pose, a 17-ulp reciprocal or the polynomial beyond its
range is worth in it).

What is read where: round 1 and rounds 2, 16, 17, 18 of every case of the matrix and of the large-step and tiny cases -- the
one-launch kernel's in-launch pose hand-over below 4097 pairs, above it the slot of the 16-slot ring a non-finishing round
reads its old pose from, across the wrap; the reference's call pattern (a getter after every oneRound: the finishing launch's
tail and the gather-in-round-0 launch); oneRound calls enqueued ahead through the eight-round graph window.  The large-step
cases take sincosf (an angle above 0.5 rad) or the polynomial at the top of its range, large-roll an angle the polynomial would
be wrong at.  The batched forms return no H and b: see test_batched_forms_take_large_steps.

Measured (MI355X, profiles/picp_tail_budget.json): ceiling_tail() = 0.607; the largest ratio over 78 cases x 5 rounds, the 20
calls and the 9 chains enqueued ahead is 0.112; the batched forms' step is within 0.020 of check_step's bound.

With VO_PICP_TAIL_JSON=<path> in the environment the measured ratios are also written there (profiles/picp_tail_budget.json is
such a run)."""
import atexit
import json
import os

import numpy as np
import pytest

import picp_budget as pb
import picp_cases as pc

pytestmark = pytest.mark.gpu

ROUNDS = (2, 16, 17, 18)                  # 16 is the last round before the slot ring wraps, 17 the first after
ENV = ("VO_PICP_SHARE", "VO_PICP_HELP_KEEP", "VO_PICP_HELP_G", "VO_PICP_HELP_SLACK", "VO_PICP_HELP_ABSENT", "VO_PICP_HELP_SCHEDULE")
CALLS_CASE = (4097, "large-z", 10000.0, False, "general")
AHEAD_CASES = ((4097, "large-x", 10000.0, False, "general"), (65537, "large-two", 10000.0, False, "pinhole"),
               (65537, "general", 60.0, True, "general"))          # round-kernel sizes: only their rounds are left open
RECORD = {"single": {}, "calls": {}, "ahead": {}, "batched": {}}


def _dump():
    path = os.environ.get("VO_PICP_TAIL_JSON")
    if not path or not any(RECORD.values()):
        return
    flat = [v for part in ("single", "calls", "ahead") for rec in RECORD[part].values() for v in rec.values()]
    out = dict(what="max |dx_of(T_gpu, T_at) - H^-1 (-b)| / bound per case and round, H and b the float32 system the GPU read back; "
                    "see tests/picp_budget.py: tail, check_tail", ceiling_tail=pc.ceiling_tail(), C_LDLT=pb.C_LDLT, C_POSE=pb.C_POSE,
               cpu_float32_restatement={pc.case_name(c): pc.tail_reference(c)["ratio"] for c in pc.case_ids() + pc.tail_case_ids()},
               gpu=RECORD, gpu_max_ratio=max(flat) if flat else None, gpu_rounds_held=len(flat),
               batched_max_step_over_bound=max([v["step_over_bound"] for rec in RECORD["batched"].values() for v in rec.values()], default=None))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


atexit.register(_dump)


@pytest.fixture(autouse=True)
def _clean_env():
    saved = {k: os.environ.pop(k, None) for k in ENV}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _solver(vo, ctx, c):
    s = vo.PICPSolver(ctx)
    s.setKernelThreshold(c["thr"])
    s.init(vo.Camera(pc.ROWS, pc.COLS, pc.Z_NEAR, pc.Z_FAR, c["K"], c["T0"], ctx=ctx), c["world"], c["meas"])
    return s


def _pose(s):
    return s.camera().worldInCameraPose().copy()


def _hold(H, b, T_at, T, what):
    """one round's tail: the pose T the GPU left against the float64 step of the H and b it read back, from T_at -> ratio"""
    Ct = pc.ceiling_tail()
    assert np.isfinite(H).all() and np.isfinite(b).all() and np.isfinite(T_at).all() and np.isfinite(T).all(), what
    assert np.array_equal(H, H.T), f"{what}: H is not symmetric bit for bit"
    r = pb.check_tail(H, b, T_at, T)
    t = pb.tail(H, b, T_at)
    print(f"{what}: step / bound {r:.4f} (ceiling {Ct:.4f})  largest step angle {np.abs(t['dx'][3:]).max():.3g}  cond(H) {np.linalg.cond(H.astype(np.float64)):.3g}")
    assert r <= Ct, (what, r, Ct, pb.dx_of(T, T_at), t["dx"], t["tol"])
    return r


def _twin_pose(vo, ctx, c, rounds):
    """the pose a handle of its own leaves after solve(rounds): what round `rounds` + 1 of the same data starts from"""
    if rounds == 0:
        return np.array(c["T0"], np.float32)
    t = _solver(vo, ctx, c)
    t.solve(c["corr"], c["keep"], rounds)
    T = _pose(t)
    t.close()
    return T


@pytest.mark.parametrize("cid", pc.case_ids() + pc.tail_case_ids(), ids=pc.case_name)
def test_single_problem_tail(vo, ctx, cid):
    c = pc.case(cid)
    name = pc.case_name(cid)
    rec = {}
    s = _solver(vo, ctx, c)
    s.oneRound(c["corr"], c["keep"])
    H, b = s.system()
    T = _pose(s)
    s.close()
    rec["round1"] = _hold(H, b, c["T0"], T, f"{name} round 1")
    if cid[1] in pc.LARGE:
        # the step the GPU's own system asks for has the angles the case is for (the reference side asserts the same of float64)
        assert pc.large_conditions(cid[1], pb.tail(H, b, c["T0"])["dx"][3:]), name
    for k in ROUNDS:
        T_at = _twin_pose(vo, ctx, c, k - 1)
        s = _solver(vo, ctx, c)
        s.solve(c["corr"], c["keep"], k)
        H, b = s.system()
        T = _pose(s)
        s.close()
        rec[f"round{k}"] = _hold(H, b, T_at, T, f"{name} round {k}")
    RECORD["single"][name] = rec


def test_reference_call_pattern(vo, ctx):
    """oneRound x 20 with system() and camera() after every call: each call is a gather-in-round-0 launch closed by the
    finishing launch, and the pose before it is the previous read-back.  A large-step case: the first rounds take sincosf,
    the later ones the polynomial."""
    c = pc.case(CALLS_CASE)
    s = _solver(vo, ctx, c)
    T_at = np.array(c["T0"], np.float32)
    rec, angles = {}, []
    for k in range(1, 21):
        s.oneRound(c["corr"], c["keep"])
        H, b = s.system()
        T = _pose(s)
        angles.append(float(np.abs(pb.tail(H, b, T_at)["dx"][3:]).max()))
        rec[f"call{k}"] = _hold(H, b, T_at, T, f"{pc.case_name(CALLS_CASE)} call {k}")
        T_at = T
    s.close()
    assert angles[0] > 0.5 and min(angles) < 0.5            # both branches were taken
    RECORD["calls"][pc.case_name(CALLS_CASE)] = rec


@pytest.mark.parametrize("k", [3, 9, 17])
@pytest.mark.parametrize("cid", AHEAD_CASES, ids=pc.case_name)
def test_rounds_enqueued_ahead(vo, ctx, cid, k):
    """oneRound x k, then the getters: the calls after the first go out ahead of their comparison, through the eight-round
    graph window; the last round's tail is held from a twin handle's solve(k - 1)"""
    c = pc.case(cid)
    T_at = _twin_pose(vo, ctx, c, k - 1)
    s = _solver(vo, ctx, c)
    for _ in range(k):
        s.oneRound(c["corr"], c["keep"])
    assert s.chainInfo()[0] == k
    H, b = s.system()
    T = _pose(s)
    assert s.chainInfo()[0] == 0
    s.close()
    RECORD["ahead"].setdefault(pc.case_name(cid), {})[f"calls{k}"] = _hold(H, b, T_at, T, f"{pc.case_name(cid)} {k} calls ahead")


@pytest.mark.parametrize("form", ["rounds", "workgroup", "helpers"])
def test_batched_forms_take_large_steps(vo, ctx, form):
    """P = 6 large-step problems of 24 000 pairs, one per kind, one round.  The batched forms return no H and b, so this is
    picp_budget.check_step (ratio <= 1), whose bound carries the rounding budget of an n-term sum: it proves that the sincosf
    path of picp_batch_kernel / picp_batch_shared_kernel / the batched round kernels runs and is not grossly wrong there
    (a swapped angle or a composition the wrong way round is thousands of bounds), NOT that the tail is right to the ulp -- that
    needs H and b out of vo_picp_solve_batch_dev.  The ratio is recorded."""
    C = pc.ceiling()
    thr, keep = 10000.0, False
    B = pc.large_batch()
    b = pc.Batch(vo, ctx, pc.BATCH_N, [pc.BATCH_N] * len(pc.BATCH_KINDS), seed=pc.BATCH_SEED, world=B["world"], T0=B["T0"])
    try:
        assert np.array_equal(b.pairs, B["pairs"]) and np.array_equal(b.fp["cur_pts"], B["fp"]["cur_pts"]) and b.sizes.min() == pc.BATCH_N
        if form == "workgroup":
            os.environ["VO_PICP_SHARE"] = "0"
        T, S, got_form, wgs = b.run(1, thr, keep, form=1 if form == "rounds" else 2)
        os.environ.pop("VO_PICP_SHARE", None)
        assert got_form == dict(rounds=1, workgroup=2, helpers=4)[form], (form, got_form)
        if form == "helpers":
            assert wgs > b.P
        rec = {}
        for p, kind in enumerate(pc.BATCH_KINDS):
            ref = pb.system(b.K, b.T0[p], b.world, b.fp["cur_pts"], b.pairs, thr, keep, pc.ROWS, pc.COLS, pc.Z_NEAR, pc.Z_FAR)
            what = f"{form} problem {p} ({kind})"
            assert ref["n_amb"] <= pb.amb_cap(pc.BATCH_N) and ref["n_in"] >= pc.MIN_INLIERS, f"unsuitable input {what}"
            Tp = T[p].reshape(4, 4).T
            r = pb.check_step(ref, b.T0[p], Tp, S[p], C)
            assert pc.large_conditions(kind, r["dx"][3:]), f"unsuitable input {what}: step angles {r['dx'][3:]}"
            rec[kind] = dict(step_over_bound=r["ratio"], rho_chi=r["stats"], n_in=int(S[p, 2]), n_in64=ref["n_in"], ambiguous=ref["n_amb"],
                             largest_step_angle=float(np.abs(r["dx"][3:]).max()))
            print(f"{what}: step / bound {r['ratio']:.3g}  rho chi {r['stats']:.3g}  step angles {np.round(r['dx'][3:], 3)}  n_in {int(S[p, 2])} (float64 {ref['n_in']})")
            assert abs(int(S[p, 2]) - ref["n_in"]) <= ref["n_amb"] and r["n_in_ok"], what
            assert r["stats"] <= C, (what, rec[kind])
            assert r["ratio"] <= 1.0, (what, rec[kind], r["dx"], r["dx_got"], r["tol"])
        RECORD["batched"][form] = rec
    finally:
        b.close()
