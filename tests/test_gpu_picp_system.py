"""The default-arithmetic PICP solver's H, b, chi^2 sums and inlier count against float64, entry by entry.

Every entry of the system the solver read back (vo_picp_get_system) is held to tests/picp_budget.py's float64 value within
C roundings of its OWN budget -- the entry's formula with every factor by its absolute value -- not within a fraction of the
largest entry; C comes from the reference side alone (picp_cases.ceiling, tests/test_picp_budget_cpu.py), never from the
kernels.  The poses are general (R far from I: at the identity every part of the Jacobian that goes through the pose is
invisible), the sizes sit on the single-problem path's own edges (one-workgroup kernel, 255 / 256 / 257 partial rows, the
grid cap of 4 workgroups per CU after which threads loop), and the rounds read back go past the wrap of the 16-slot
hand-off ring.  The batched forms return no H and b: they are held through the pose after ONE round (picp_budget.step).

Measured (MI355X, profiles/picp_system_budget.json): C = 18.0; the largest rho over 57 cases x 5 rounds is 3.6 (H), b and the
chi^2 sums stay below 1; at most 5 ambiguous correspondences in a case; the batched forms' step is within 0.0025 of its bound
(the bound is a worst case over n terms: a blunt view next to H itself -- tests/test_picp_budget_cpu.py prints what a fault
is worth in it).

With VO_PICP_BUDGET_JSON=<path> in the environment the measured figures are also written there (profiles/
picp_system_budget.json is such a run)."""
import atexit
import json
import os

import numpy as np
import pytest

import picp_budget as pb
import picp_cases as pc

pytestmark = pytest.mark.gpu

ROUNDS = (2, 16, 17, 18)                  # 16 is the last round before the slot ring wraps, 17 the first after
BATCH_SIZES = [0, 3, 255, 256, 257, 767, 768, 769, 2000, 6143, 6144, 6148, 9217, 12288, 18431, 18432, 18435, 10 ** 9,
               257, 18432, 10 ** 9]       # the last three repeat earlier ones: same data in one call, same bits
TWINS = ((18, 4), (19, 15), (20, 17))
ENV = ("VO_PICP_SHARE", "VO_PICP_HELP_KEEP", "VO_PICP_HELP_G", "VO_PICP_HELP_SLACK", "VO_PICP_HELP_ABSENT")
RECORD = {"single": {}, "batched": {}}


def _dump():
    path = os.environ.get("VO_PICP_BUDGET_JSON")
    if path and (RECORD["single"] or RECORD["batched"]):
        out = dict(what="rho = max |X_gpu - X_float64| / (2^-24 A_X) per case; see tests/picp_budget.py", C=pc.ceiling(),
                   band_ulp=pb.BAND, cases={})
        from oracle.oracle import Camera as OCam, Oracle
        o32 = Oracle(32)
        for cid in pc.case_ids():
            ref, r32 = pc.reference(cid)
            c = pc.case(cid)
            o = o32.picp_solve(OCam(pc.ROWS, pc.COLS, pc.Z_NEAR, pc.Z_FAR, c["K"], c["T0"]), c["world"], c["meas"], c["corr"], 1, c["thr"], c["keep"])
            ro = pb.rho_system(ref, o["H"][0], o["b"][0], o["stats"][0, 0], o["stats"][0, 1], int(o["stats"][0, 2]))
            out["cases"][pc.case_name(cid)] = dict(
                n=cid[0], n_in=ref["n_in"], n_out=ref["n_out"], ambiguous=ref["n_amb"], ambiguous_cap=pb.amb_cap(cid[0]),
                cpu_float32_pairwise={k: r32[k] for k in ("H", "b", "chi_in", "chi_out")},
                cpu_float32_sequential_o32={k: ro[k] for k in ("H", "b", "chi_in", "chi_out")},
                gpu=RECORD["single"].get(pc.case_name(cid)))
        out["batched"] = RECORD["batched"]
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


def _read(s):
    H, b = s.system()
    return H, b, s.chiInliers(), s.chiOutliers(), s.numInliers(), s.camera().worldInCameraPose().copy()


def _hold(ref, got, C, what):
    """one read-back system against the float64 budget at the pose it was linearised at -> the rho record"""
    H, b, ci, co, ni, _ = got
    assert ref["n_amb"] <= pb.amb_cap(ref["n"]), f"unsuitable input {what}: {ref['n_amb']} ambiguous correspondences"
    assert np.array_equal(H, H.T), f"{what}: H is not symmetric bit for bit"
    r = pb.rho_system(ref, H, b, ci, co, ni, damping=1.0)
    rec = dict(H=r["H"], b=r["b"], chi_in=r["chi_in"], chi_out=r["chi_out"], n_in=int(ni), n_in64=ref["n_in"], ambiguous=ref["n_amb"])
    print(f"{what}: rho H {r['H']:.3g} b {r['b']:.3g} chi_in {r['chi_in']:.3g} chi_out {r['chi_out']:.3g}  n_in {ni} (float64 {ref['n_in']}, "
          f"{ref['n_amb']} ambiguous)  C {C:.3g}")
    assert abs(int(ni) - ref["n_in"]) <= ref["n_amb"], f"{what}: {ni} inliers, float64 {ref['n_in']}, {ref['n_amb']} ambiguous"
    assert r["n_in_ok"], f"{what}: no decision of the ambiguous correspondences gives {ni} inliers"
    assert r["worst"] <= C, f"{what}: {rec}"
    return rec


def test_device_is_the_one_the_case_matrix_was_built_for(ctx):
    assert ctx.device_info()[1] == pb.N_CU


@pytest.mark.parametrize("cid", pc.case_ids(), ids=pc.case_name)
def test_single_problem_system(vo, ctx, cid):
    C = pc.ceiling()
    c = pc.case(cid)
    name = pc.case_name(cid)
    rec = {}
    # round 1, from T0
    s = _solver(vo, ctx, c)
    s.oneRound(c["corr"], c["keep"])
    got = _read(s)
    s.close()
    rec["round1"] = _hold(pc.reference(cid)[0], got, C, f"{name} round 1")
    # rounds 2, 16, 17, 18: a twin handle's solve(k - 1) gives the pose round k linearised at
    for k in ROUNDS:
        t = _solver(vo, ctx, c)
        t.solve(c["corr"], c["keep"], k - 1)
        T_at = t.camera().worldInCameraPose().copy()
        t.close()
        s = _solver(vo, ctx, c)
        s.solve(c["corr"], c["keep"], k)
        got = _read(s)
        s.close()
        assert np.isfinite(T_at).all() and np.isfinite(got[5]).all()
        rec[f"round{k}"] = _hold(pb.system(*pc.system_args(c, T_at)), got, C, f"{name} round {k}")
    RECORD["single"][name] = rec


def _batch(vo, ctx, general_k, seed=7100):
    """P problems on one 24 000-pair frame whose world was moved by G^-1: problem p starts at small_p G"""
    n = 24000
    fp = vo.synth.frame_pair(n, seed=seed, distractors=n // 50)
    rng = np.random.default_rng(seed)
    world, G = pc.general_world(rng, fp["model"])
    T0 = np.stack([(vo.synth.random_isometry(rng, 0.01, 0.02).astype(np.float64) @ G) for _ in BATCH_SIZES]).astype(np.float32)
    for p, q in TWINS:
        T0[p] = T0[q]
    K = pc.general_K(fp["K"]) if general_k else None
    return pc.Batch(vo, ctx, n, BATCH_SIZES, seed=seed, K=K, world=world, T0=T0)


@pytest.mark.parametrize("keep", [False, True], ids=["drop", "keep"])
@pytest.mark.parametrize("general_k", [False, True], ids=["pinhole", "general"])
@pytest.mark.parametrize("form", ["rounds", "workgroup", "helpers"])
def test_batched_forms_one_step(vo, ctx, form, general_k, keep):
    C = pc.ceiling()
    thr = 60.0
    b = _batch(vo, ctx, general_k)
    try:
        assert [int(b.sizes[p]) for p, q in TWINS] == [int(b.sizes[q]) for p, q in TWINS] and b.sizes[17] == len(b.pairs) > 18435
        if form == "workgroup":
            os.environ["VO_PICP_SHARE"] = "0"
        T, S, got_form, wgs = b.run(1, thr, keep, form=1 if form == "rounds" else 2)
        os.environ.pop("VO_PICP_SHARE", None)
        assert got_form == dict(rounds=1, workgroup=2, helpers=4)[form], (form, got_form)
        if form == "helpers":
            assert wgs > b.P
        rec = {}
        for p in range(b.P):
            args = (b.K, b.T0[p], b.world, b.fp["cur_pts"], b.pairs[: b.sizes[p]], thr, keep, pc.ROWS, pc.COLS, pc.Z_NEAR, pc.Z_FAR)
            ref = pb.system(*args)
            what = f"{form} {'general' if general_k else 'pinhole'} {'keep' if keep else 'drop'} problem {p} ({b.sizes[p]} pairs)"
            assert ref["n_amb"] <= pb.amb_cap(max(int(b.sizes[p]), 1)), f"unsuitable input {what}: {ref['n_amb']} ambiguous"
            assert S[p, 3] == 0.0 and S[p, 2] == np.floor(S[p, 2])
            r = pb.check_step(ref, b.T0[p], T[p].reshape(4, 4).T, S[p], C)
            rec[p] = dict(pairs=int(b.sizes[p]), step_over_bound=r["ratio"], rho_chi=r["stats"], n_in=int(S[p, 2]), n_in64=ref["n_in"],
                          ambiguous=ref["n_amb"])
            print(f"{what}: step / bound {r['ratio']:.3g}  rho chi {r['stats']:.3g}  n_in {int(S[p, 2])} (float64 {ref['n_in']}, {ref['n_amb']} ambiguous)")
            assert abs(int(S[p, 2]) - ref["n_in"]) <= ref["n_amb"] and r["n_in_ok"], what
            assert r["stats"] <= C, (what, rec[p])
            assert r["ratio"] <= 1.0, (what, rec[p], r["dx"], r["dx_got"], r["tol"])
        for p, q in TWINS:                                   # same data in one call: same bits, wherever the problem sits
            assert T[p].tobytes() == T[q].tobytes() and S[p].tobytes() == S[q].tobytes(), (p, q)
        assert np.array_equal(T[0].reshape(4, 4).T, b.T0[0]) and not S[0].any()      # no correspondence: the pose stays
        RECORD["batched"][f"{form}-{'general' if general_k else 'pinhole'}-{'keep' if keep else 'drop'}"] = rec
        # zero rounds: the poses come back untouched
        if form == "workgroup":
            os.environ["VO_PICP_SHARE"] = "0"
        T0r, S0r, _, _ = b.run(0, thr, keep, form=1 if form == "rounds" else 2)
        assert np.array_equal(T0r.reshape(-1, 4, 4).transpose(0, 2, 1), b.T0) and not S0r.any()
    finally:
        b.close()
