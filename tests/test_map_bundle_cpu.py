"""CPU checks behind vox_map_bundle*: the ABI of the second namespace on a machine without a device, the float64 restatement
(tests/map_bundle_restatement.py) -- its terms against the two halves' restatements, its PCG against a dense solve of the
explicitly formed reduced system, planted faults against the measure the GPU test uses, the descent against the alternation
-- and the cases of the GPU test (no marginal decision, the budget re-measured)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import map_bundle_cases as Bc
import map_bundle_restatement as B
import map_pose_refine_cases as Cs
import map_pose_refine_restatement as P
import map_refine_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vox_map_bundle_batch_dev", "vox_map_bundle")
BUDGET = os.path.join(ROOT, "profiles", "map_bundle_budget.json")


# ---- ABI: the second namespace ----
def _declared_vox(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(vox_[a-z0-9_]+)\s*\(", txt))


def test_the_vox_symbols_exported_are_those_the_header_declares(vo):
    import shutil
    import subprocess
    lib = vo.load_library()
    for n in NEW:
        assert hasattr(lib, n), n
    assert _declared_vox("vo_map_bundle.h") == set(NEW)
    assert not _declared_vox("vo_hip.h") and not _declared_vox("vo_map_adjust.h")
    assert open(os.path.join(ROOT, "include", "vo_hip.h")).read().count('#include "vo_map_bundle.h"') == 1
    assert lib.vo_abi_version() == 1
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (vox_[a-z0-9_]+)$", out, flags=re.M)) == set(NEW)      # unversioned, and nothing else
        assert not re.findall(r" T (vox_[a-z0-9_]+)@", out, flags=re.M)
    assert "vox_" not in open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "vo_map_adjust.map")).read()


def test_structs_statuses_and_python_names(vo):
    assert C.sizeof(vo.MapBundleParams) == 28 and C.sizeof(vo.MapBundleRound) == 40 and C.sizeof(vo.MapBundleStats) == 48
    assert vo.MapBundleRound.cg_iterations.offset == 32 and vo.MapBundleStats.cost_before.offset == 32 and vo.MapBundleParams.huber_px.offset == 24
    assert vo.MAP_BUNDLE_STATUS == ("OK", "NOT_FINITE", "BEHIND", "NOTHING_FREE", "NO_STEP", "COST_ROSE")
    hdr = open(os.path.join(ROOT, "include", "vo_map_bundle.h")).read()
    for k, name in enumerate(vo.MAP_BUNDLE_STATUS):
        assert re.search(r"#define VOX_MAP_BUNDLE_%s\s+%d\b" % (name, k), hdr), name
    assert (B.OK, B.NOT_FINITE, B.BEHIND, B.NOTHING_FREE, B.NO_STEP, B.COST_ROSE) == tuple(range(6))
    assert "the gauge is free" in hdr and "A SECOND NAMESPACE" in hdr and "ONE workgroup" in hdr and "VOX_MAP_BUNDLE_MAX_STEPS 65536" in hdr
    for n in ("bundle", "bundle_batch_dev"):
        assert hasattr(vo.Map, n)
    hpp = open(os.path.join(ROOT, "include", "vo", "localise.hpp")).read()
    assert "struct BundleOptions" in hpp and " bundle(" in hpp
    src = open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "map_bundle.hip")).read()
    assert "atomicAdd(double" not in src and "cooperative" not in src.lower() and "unsafeAtomicAdd" not in src


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the failure path is not reachable")
def test_new_symbols_refuse_without_a_device(vo):
    lib = vo.load_library()
    z, i, s = None, C.c_int, C.c_size_t
    Kp = np.eye(3, dtype=np.float32).ctypes.data_as(C.c_void_p)
    prm, st = vo.MapBundleParams(2, 8, 1e-8, 1e-4, 3, 3, 0.0), vo.MapBundleStats()
    assert lib.vox_map_bundle_batch_dev(z, i(1), Kp, z, s(1), z, s(1), i(1), z, z, z, C.byref(prm), z, z, z, z) == -1
    assert b"null map" in lib.vo_last_error()
    assert lib.vox_map_bundle(z, i(1), Kp, z, z, z, i(1), z, z, C.byref(prm), z, z, z, C.byref(st)) == -1
    assert b"null map" in lib.vo_last_error()


# ---- the restatement ----
def test_terms_are_those_of_the_two_halves():
    """summed per frame, Jc, w, e and rho give evaluate of the pose half; summed per landmark, Jp gives evaluate of the point half"""
    c = Bc.case("huber_noisy")
    pr = B.Problem(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], c["fixed"], 3, 3)
    T, pts = pr.T0.astype(np.float64), pr.pts0.astype(np.float64)
    e, w, rho, Jc, Jp, z = B.terms(pr.K, T, pts, pr.of, pr.oe, pr.uv, 1.0)
    for f in range(pr.F):
        k = pr.of == f
        H, b, cost, zz = P.evaluate(pr.K, T[f], pr.uv[k], pts[pr.oe[k]], 1.0)
        assert np.allclose(np.einsum("nka,nkb->ab", w[k, None, None] * Jc[k], Jc[k]), H, rtol=1e-12, atol=1e-12 * np.abs(H).max())
        assert np.allclose(np.einsum("nka,nk->a", w[k, None, None] * Jc[k], e[k]), b, rtol=1e-10, atol=1e-10 * np.abs(b).max()) and abs(rho[k].sum() - cost) <= 1e-12 * cost
        assert np.allclose(zz, z[k], rtol=1e-14)
    for j in (0, 17, 64):
        k = pr.oe == j
        H, b, cost, _ = R.evaluate(pr.K, T[pr.of[k], :3, :3], T[pr.of[k], :3, 3], pr.uv[k], pts[j], 1.0)
        assert np.allclose(np.einsum("nka,nkb->ab", w[k, None, None] * Jp[k], Jp[k]), H, rtol=1e-12, atol=1e-12 * np.abs(H).max())
        assert np.allclose(np.einsum("nka,nk->a", w[k, None, None] * Jp[k], e[k]), b, rtol=1e-10, atol=1e-10 * np.abs(b).max())
    assert (w < 1).any() and (w == 1).any()                   # the Huber weight is at work on this case


@pytest.mark.parametrize("name", list(Bc.CASES))
def test_pcg_solve_against_the_dense_solve(name):
    """The two passes ARE the reduced camera system: S p by apply_S equals the explicitly formed S times p to rounding on every
    case, and where PCG is run to convergence the whole call lands where numpy.linalg.solve on the formed S lands."""
    c, ref = Bc.case(name), Bc.reference(name)
    if ref["status"] in (B.NOT_FINITE, B.BEHIND, B.NOTHING_FREE) or c["params"]["n_rounds"] == 0:
        assert not any(r["accepted"] for r in ref["rounds"])
        return
    pr = ref["problem"]
    L = B.linearise(pr, pr.T0.astype(np.float64), pr.pts0.astype(np.float64), float(np.float32(c["params"]["huber_px"])), 1e-4)
    S, ff = B.dense_S(pr, L)
    if len(ff):
        p = np.zeros((pr.F, 6)); p[ff] = np.random.default_rng(1).normal(size=(len(ff), 6))
        q = B.apply_S(pr, L, p)
        assert np.abs(q[ff].ravel() - S @ p[ff].ravel()).max() <= 1e-11 * np.abs(S).max() * np.abs(p).max()
        assert np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max() and np.linalg.eigvalsh(S).min() > 0
    kw = dict(n_cg=6 * max(len(ff), 1) + 6, cg_tol=1e-13)
    conv, dense = Bc.run(c, **kw), Bc.run(c, solver="dense", **kw)
    assert [r["accepted"] for r in conv["rounds"]] == [r["accepted"] for r in dense["rounds"]]
    for a, b in zip(conv["rounds"], dense["rounds"]):
        assert abs(a["cost_candidate"] - b["cost_candidate"]) <= 1e-7 * abs(b["cost_candidate"]) + 1e-9, (name, a, b)
    dp, dq = B.distance(dense, conv)
    base = B.distance(dense, dense)[0]                        # (the measure's own floor: a pose that is not exactly orthonormal)
    print(f"{name}: PCG to convergence lies {dp:.3g} px (poses; floor {base:.3g}) and {dq:.3g} px (points) from the dense solve")
    assert dp <= base + 1e-7 and dq <= 1e-8                  # (measured: the floor itself, and 1.2e-11 px at the most)


def test_one_round_is_the_damped_joint_normal_equations_step():
    """the candidate of one round equals the step of the full (poses + points) damped normal equations solved densely"""
    c = Bc.case("hand")
    r = Bc.run(c, n_rounds=1, n_cg=40, cg_tol=1e-14)
    pr = r["problem"]
    T, pts = pr.T0.astype(np.float64), pr.pts0.astype(np.float64)
    e, w, _, Jc, Jp, _ = B.terms(pr.K, T, pts, pr.of, pr.oe, pr.uv, 0.0)
    ff, fp = np.nonzero(pr.free_f)[0], np.nonzero(pr.free_p)[0]
    n = 6 * len(ff) + 3 * len(fp)
    J = np.zeros((2 * len(pr.of), n))
    for k in range(len(pr.of)):
        if pr.free_f[pr.of[k]]:
            a = 6 * int(np.searchsorted(ff, pr.of[k])); J[2 * k: 2 * k + 2, a: a + 6] = Jc[k]
        a = 6 * len(ff) + 3 * int(np.searchsorted(fp, pr.oe[k])); J[2 * k: 2 * k + 2, a: a + 3] = Jp[k]
    H = J.T @ J
    lam = float(np.float32(1e-4))
    H[np.arange(n), np.arange(n)] *= 1 + lam
    step = -np.linalg.solve(H, J.T @ e.ravel())
    for a, f in enumerate(ff):
        assert np.abs(r["T64"][f] - P.v2t(step[6 * a: 6 * a + 6]) @ T[f]).max() < 1e-9
    assert np.abs(r["P64"][fp] - (pts[fp] + step[6 * len(ff):].reshape(-1, 3))).max() < 1e-9
    assert r["rounds"][0]["accepted"] == 1


SETTINGS = ((1, 60), (4, 60), (1, 2), (4, 2))                 # (n_rounds, n_cg) tried in this order for a planted fault


def test_planted_faults_are_seen():
    """Each fault is seen by the MEASURE of the GPU test, far above its ceiling, on a run that stays OK under the fault.  One round
    is tried first (a faulty step that still lowers the cost is accepted, and a converged faulty solver could reach the same fixed
    point); a fault whose first step raises the cost and is rejected is run for four rounds, where the raised damping lets a step
    through; W^T in pass B, where PCG on a matrix that is not symmetric hands out a useless step, with two PCG iterations.  The
    reference is the clean run under the same settings.  The control -- the preconditioner from U_f alone, without the Schur term
    -- is no fault: PCG converges to the same step."""
    c = Bc.case("huber_noisy")
    pr = Bc.reference("huber_noisy")["problem"]
    clean = {}
    for n_rounds, n_cg in SETTINGS:
        kw = dict(n_rounds=n_rounds, n_cg=n_cg, cg_tol=1e-12)
        ref, rev = Bc.run(c, **kw), Bc.run(c, reverse=True, **kw)
        assert ref["status"] == B.OK and rev["status"] == B.OK
        clean[n_rounds, n_cg] = (kw, ref, B.distance(ref, rev))

    def ratio(r, ref, reach):
        """the stored float32 state's distance to the float64 state over the ceiling: the worst frame, the worst landmark"""
        a = max(P.h_norm(P.pose_delta(ref["T64"][f], r["poses"][f]), ref["U"][f]) / (4 * reach[0] + P.half_ulp_px(r["poses"][f], ref["U"][f]))
                for f in np.nonzero(pr.free_f)[0])
        b = max(B.point_norm(r["points"][j].astype(np.float64) - ref["P64"][j], ref["V"][j]) /
                (4 * reach[1] + B.half_ulp_point_px(r["points"][j], ref["V"][j])) for j in np.nonzero(pr.free_p)[0])
        return a, b

    for key, (kw, ref, reach) in clean.items():
        got = ratio(ref, ref, reach)
        print(f"clean, {key}: forward against reversed {reach[0]:.3g} / {reach[1]:.3g} px; the stored state {got[0]:.3g}, {got[1]:.3g} x the ceiling")
        assert max(got) <= 1.0
    for fault in B.FAULTS + B.CONTROLS:
        for key in SETTINGS:
            kw, ref, reach = clean[key]
            r = Bc.run(c, fault=fault, **kw)
            if r["status"] == B.OK:
                break
        seen = ratio(r, ref, reach)
        print(f"{fault}: (n_rounds, n_cg) = {key}, status {r['status']}, {seen[0]:.3g} (poses), {seen[1]:.3g} (points) x the ceiling, PCG iterations",
              [x["cg_iterations"] for x in r["rounds"]])
        assert r["status"] == B.OK, fault
        if fault in B.CONTROLS:
            assert key == SETTINGS[0] and max(seen) <= 1.0
        else:
            assert max(seen) > 100.0, fault


@pytest.mark.parametrize("name,rounds", [("example", 2), ("hand", 3)])
def test_the_joint_solver_descends_faster_than_the_alternation(name, rounds):
    """the total cost (total_cost of the pose half's restatement, on the float32 state each call hands out) after `rounds` joint
    rounds is below the alternation's after 6 sweeps of 2 + 2 rounds -- both computed by the committed restatements"""
    c = Cs.example_adjust() if name == "example" else Cs.hand_adjust()
    alt = P.adjust(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], c["fixed"], n_sweeps=6, pose_rounds=2, point_rounds=2)
    joint = B.bundle(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], c["fixed"], n_rounds=rounds)
    cost = P.total_cost(c["K"], joint["points"], c["map_app"], c["frames"], joint["poses"])
    print(f"{name}: start {alt['costs'][0]:.6g}; alternation after 6 sweeps {alt['costs'][-1]:.6g}; joint per round",
          " ".join(f"{r['cost_candidate']:.6g}" for r in joint["rounds"]), f"; stored {cost:.6g}")
    assert joint["status"] == B.OK and all(r["accepted"] for r in joint["rounds"])
    assert cost < alt["costs"][-1] < alt["costs"][0]
    assert abs(cost - joint["stats"]["cost_after"]) <= 1e-9 * cost


def test_rules_on_the_small_cases():
    r = Bc.reference("rejected_then_accepted")
    assert [x["accepted"] for x in r["rounds"]] == [0, 1, 1] and r["rounds"][0]["cost_candidate"] > 10 * r["rounds"][0]["cost"]
    assert abs(r["rounds"][1]["lambda_"] - 10 * r["rounds"][0]["lambda_"]) < 1e-12 and r["rounds"][1]["cost"] == r["rounds"][0]["cost"]
    assert r["status"] == B.OK and r["stats"]["n_accepted"] == 2
    for name, status in (("nan_pixel", B.NOT_FINITE), ("nan_point", B.NOT_FINITE), ("camera_turned_away", B.BEHIND), ("nothing_free", B.NOTHING_FREE)):
        r, c = Bc.reference(name), Bc.case(name)
        assert r["status"] == status and r["points"].tobytes() == np.asarray(c["map_pts"], np.float32).tobytes()
        assert all(a.tobytes() == np.asarray(b, np.float32).tobytes() for a, b in zip(r["poses"], c["poses"]))
    r = Bc.reference("zero_rounds")
    assert r["status"] == B.OK and r["rounds"] == [] and r["stats"]["cost_after"] == r["stats"]["cost_before"]
    r = Bc.reference("every_frame_held")
    assert r["stats"]["n_free_frames"] == 0 and [x["cg_iterations"] for x in r["rounds"]] == [0, 0] and r["status"] == B.OK
    assert (r["pose_status"] == B.POSE_FIXED).all() and all(a.tobytes() == b.tobytes() for a, b in zip(r["poses"], r["problem"].T0))
    r = Bc.reference("poses_alone")
    assert r["stats"]["n_free_points"] == 0 and [x["cg_iterations"] for x in r["rounds"]] == [1, 1]
    assert r["points"].tobytes() == r["problem"].pts0.tobytes()
    assert [x["cg_iterations"] for x in Bc.reference("one_cg_iteration")["rounds"]] == [1, 1, 1]
    assert [x["cg_iterations"] for x in Bc.reference("hand")["rounds"]] == [12, 12, 12]      # 12 unknowns: the exact count


def test_gpu_cases_cover_the_edges():
    r = Bc.reference("frame_edges")
    n = r["problem"].n_obs_f.tolist()
    assert n == [1, 2, 3, 16, 16, 0, 17, 63, 64, 65, 255, 256, 257, 1025] and Bc.case("frame_edges")["n_rows"][5] == 0      # frame 3: two rows of one landmark
    assert any(len(a) > k for (_, a), k in zip(Bc.case("frame_edges")["frames"], Bc.case("frame_edges")["n_rows"]))              # garbage behind live rows
    assert r["pose_status"].tolist() == [B.POSE_FEW_OBS] * 2 + [B.POSE_OK] * 3 + [B.POSE_FEW_OBS] + [B.POSE_OK] * 7 + [B.POSE_FIXED]
    assert Bc.reference("frame_edges_no_row_counts")["problem"].n_obs_f.tolist() == Bc.FRAME_HITS and Bc.case("frame_edges_no_row_counts")["n_rows"] is None
    r = Bc.reference("landmark_edges")
    assert sorted(set(r["problem"].n_obs_p.tolist())) == Bc.LANDMARK_SEEN_BY == [1, 2, 3, 15, 16, 17, 33]
    assert sorted(set(r["point_status"].tolist())) == [B.POINT_OK, B.POINT_FEW_OBS]
    assert [len(Bc.case(k)["frames"]) for k in ("one_frame", "two_frames_one_held", "hand", "frames_257")] == [1, 2, 3, 257]
    assert Bc.reference("frames_257")["stats"]["n_free_frames"] > 128 and B.POINT_UNSEEN in Bc.reference("frames_257")["point_status"]
    pr = Bc.reference("two_groups")["problem"]
    assert not set(pr.oe[pr.of < 3]) & set(pr.oe[pr.of >= 3])
    assert Bc.case("huber_noisy")["params"]["huber_px"] == 1.0 and Bc.case("one_cg_iteration")["params"]["n_cg"] == 1
    src = open(os.path.join(ROOT, "visual-odometry_amd", "csrc", "map_bundle.hip")).read()
    assert re.search(r"constexpr int BB = (\d+);", src).group(1) == "256" and re.search(r"constexpr int BG = (\d+);", src).group(1) == "16"


@pytest.mark.parametrize("name", list(Bc.CASES))
def test_gpu_cases_take_no_marginal_decision_and_have_the_recorded_budget(name):
    r, rv = Bc.reference(name), Bc.reference(name, True)
    assert not r["marginal"] and not rv["marginal"]
    assert rv["status"] == r["status"] and [x["accepted"] for x in rv["rounds"]] == [x["accepted"] for x in r["rounds"]]
    assert [x["cg_iterations"] for x in rv["rounds"]] == [x["cg_iterations"] for x in r["rounds"]]
    assert (r["status"] == B.OK and r["stats"]["n_accepted"] > 0) == (name in Bc.WRITES)
    rec = json.load(open(BUDGET))["cases"][name]
    assert rec["status"] == r["status"] and rec["n_obs"] == r["stats"]["n_obs"] and rec["accepted"] == [x["accepted"] for x in r["rounds"]]
    assert rec["cg_iterations"] == [x["cg_iterations"] for x in r["rounds"]]
    assert rec["n_free_frames"] == r["stats"]["n_free_frames"] and rec["n_free_points"] == r["stats"]["n_free_points"]
    reach = Bc.reach(name)
    print(name, "forward against reversed:", reach, "recorded", rec["reach_pose_px"], rec["reach_point_px"])
    for got, want in zip(reach, (rec["reach_pose_px"], rec["reach_point_px"])):
        assert abs(got - want) <= 0.05 * want + 1e-18          # (the same numpy gives the same figure; another one may round otherwise)
