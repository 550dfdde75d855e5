"""CPU checks behind voe_pose_graph*: the ABI of the seventh extension header -- by the voe_ rule -- on a machine without a
device, the float64 restatement (tests/pose_graph_restatement.py) against finite differences and on the example trajectory (the
measured reason for the CHAIN default, asserted), the cases of the GPU test (no marginal decision, no case where the order of
the sums decides, the budget re-measured), planted faults against the measure the GPU test uses, and the host refusals under the
host sanitizers."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import pose_graph_cases as Cc
import pose_graph_restatement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "profiles", "pose_graph_budget.json")


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---- ABI: the seventh header, by rule ----
def test_the_voe_rule_holds_with_the_seventh_header(vo):
    lib = vo.load_library()
    hip = _read("include", "vo_hip.h")
    assert hip.count('#include "vo_pose_graph.h"') == 1 and hip.index('#include "vo_map_grow.h"') < hip.index('#include "vo_pose_graph.h"')
    declared = {}
    for h in ["vo_hip.h"] + re.findall(r'^#include "([a-z0-9_]+\.h)"', hip, flags=re.M):
        for n in re.findall(r"\b(voe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _read("include", h), flags=re.S)):
            declared[n] = h
    assert declared["voe_pose_graph_dev"] == declared["voe_pose_graph"] == "vo_pose_graph.h"
    assert declared["voe_map_apply_correction_batch_dev"] == declared["voe_map_apply_correction"] == "vo_pose_graph.h"
    for n in declared:
        assert hasattr(lib, n), f"{n} is declared in include/{declared[n]} but not exported"
    assert lib.vo_abi_version() == 1
    import shutil
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", vo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert set(re.findall(r" T (voe_[a-z0-9_]+)$", out, flags=re.M)) == set(declared)      # unversioned, and nothing else
    assert "voe_" not in _read("visual-odometry_amd", "csrc", "vo_map_adjust.map")
    mk = _read("visual-odometry_amd", "csrc", "Makefile")
    assert "pose_graph.hip" in mk and "vo_pose_graph.h" in mk
    apps = _read("apps", "Makefile")
    assert "bin/close_loop" in apps and "vo_pose_graph.h" in apps
    hpp = _read("include", "vo", "pose_graph.hpp")
    assert "class PoseGraph" in hpp and " optimise(" in hpp and " addEdge(" in hpp and '#include "pose_graph.hpp"' in _read("include", "vo", "vo.hpp")
    loc = _read("include", "vo", "localise.hpp")
    assert " applyCorrection(" in loc and "inline Isometry3f rigid_pose(const Similarity3f& S)" in loc
    assert C.sizeof(vo.MapApplyStats) == 16 and hasattr(vo.Map, "apply_correction") and hasattr(vo.Map, "apply_correction_batch_dev")
    names = re.search(r"pose_graph_status_name\(int status\) \{\s*static const char\* names\[\] = \{([^}]*)\}", hpp).group(1)
    assert tuple(re.findall(r'"([A-Z_]+)"', names)) == vo.POSE_GRAPH_STATUS


def test_structs_statuses_and_python_names(vo):
    assert C.sizeof(vo.PoseGraphParams) == 28 and C.sizeof(vo.PoseGraphRound) == 40 and C.sizeof(vo.PoseGraphStats) == 48
    assert vo.PoseGraphParams.with_scale.offset == 20 and vo.PoseGraphParams.preconditioner.offset == 24
    assert vo.PoseGraphRound.cg_iterations.offset == 32 and vo.PoseGraphStats.cost_before.offset == 32
    assert vo.POSE_GRAPH_ROUND_DTYPE.itemsize == 40
    assert [vo.POSE_GRAPH_ROUND_DTYPE.fields[k][1] for k in vo.POSE_GRAPH_ROUND_DTYPE.names] == [getattr(vo.PoseGraphRound, k).offset for k, _ in vo.PoseGraphRound._fields_]
    assert vo.POSE_GRAPH_STATUS == P.STATUS and vo.POSE_GRAPH_PRECONDITIONER == P.PRECONDITIONER
    hdr = _read("include", "vo_pose_graph.h")
    for names in (vo.POSE_GRAPH_STATUS, vo.POSE_GRAPH_PRECONDITIONER):
        for k, name in enumerate(names):
            assert re.search(r"#define VOE_POSE_GRAPH_%s\s+%d\b" % (name, k), hdr), name
    assert re.search(r"#define VOE_POSE_GRAPH_EDGE_SKIPPED\s+1\b", hdr) and P.EDGE_SKIPPED == 1
    assert "static_assert(sizeof(voe_pose_graph_params) == 28 && sizeof(voe_pose_graph_round) == 40 && sizeof(voe_pose_graph_stats) == 48" in \
        _read("visual-odometry_amd", "csrc", "capi_map.hip")
    import inspect
    d = {k: v.default for k, v in inspect.signature(vo.pose_graph).parameters.items() if v.default is not inspect.Parameter.empty}
    assert {k: d[k] for k in P.DEFAULT} == P.DEFAULT
    S = np.eye(4)
    S[:3, :3] = 2.0 * P.rot_xyz(np.array([0.1, -0.2, 0.3]))
    S[:3, 3] = (1.0, 2.0, 3.0)
    T = vo.rigid_pose(S)
    assert np.allclose(T[:3, :3], S[:3, :3] / 2.0, atol=1e-15) and np.allclose(T[:3, 3], S[:3, 3] / 2.0, atol=1e-15)
    p = np.array([0.3, -0.4, 5.0])
    a, b = S[:3, :3] @ p + S[:3, 3], T[:3, :3] @ p + T[:3, 3]
    assert np.allclose(a[:2] / a[2], b[:2] / b[2], atol=1e-15)      # the same projection: camera points only scale


# ---- the restatement itself ----
def test_the_jacobians_are_the_derivatives_of_the_residual():
    """J_i and J_j of the header against central differences of r under the header's left update, at a residual that is not small
    in translation and scale (where G's last column and Ad's matter) and small in rotation (where the inverse left Jacobian of the
    rotation is I to first order)"""
    S = np.stack([Cc._sim(1.3, [0.2, -0.4, 0.9], [1.0, -2.0, 0.5]), Cc._sim(0.8, [-0.5, 0.3, 0.2], [0.3, 0.7, -1.1])])
    Z = (Cc._sim(1.1, [1e-4, -2e-4, 1.5e-4], [0.3, -0.2, 0.25]) @ S[1] @ np.linalg.inv(S[0]))[None]
    e, w3 = np.array([[0, 1]]), np.ones((1, 3))
    M, t = P.mats(S)
    ev = P.evaluate(M, t, e, Z[:, :3, :3], Z[:, :3, 3], w3, 0.0)
    A, _ = P.ad_matrices(ev["MA"], ev["tA"])
    G = P.g_matrix(ev["tE"])
    J = {0: -(G @ A)[0], 1: G[0]}
    for side in (0, 1):
        num = np.zeros((7, 7))
        for k in range(7):
            rs = []
            for h in (1e-6, -1e-6):
                x = np.zeros(7)
                x[k] = h
                M2, t2 = M.copy(), t.copy()
                M2[side], t2[side] = P.apply_update(M[side], t[side], x, True)
                rs.append(P.evaluate(M2, t2, e, Z[:, :3, :3], Z[:, :3, 3], w3, 0.0)["r"][0])
            num[:, k] = (rs[0] - rs[1]) / 2e-6
        assert np.abs(num - J[side]).max() < 5e-4 * max(1.0, np.abs(J[side]).max()), (side, np.abs(num - J[side]).max())
    # Ad^-1 as the header writes it is the inverse of Ad for a similarity
    A, Ai = P.ad_matrices(M, t)
    assert np.abs(A @ Ai - np.eye(7)).max() < 1e-13


def test_chain_is_the_exact_inverse_of_the_chains_matrix():
    """on a graph of odometry edges alone, at zero residual and lambda 0, CHAIN solves the system in one iteration"""
    g, gt = Cc.graph(12, [], seed=21, noise=0.0, rot_noise=0.0, t_noise=0.0, drift=0.0)
    S = gt.copy()
    rng = np.random.default_rng(1)
    S[5] = Cc._sim(1.01, 0.01 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)) @ S[5]      # one frame off: two edges pull
    r = P.run(S=S, edges=g["edges"], Z=np.array([gt[j] @ np.linalg.inv(gt[i]) for i, j in g["edges"]]), fixed=g["fixed"], n_rounds=1, n_cg=8,
              cg_tol=1e-4, lambda0=0.0)
    assert r["rounds"][0]["cg_iterations"] <= 3 and r["rounds"][0]["accepted"] == 1, r["rounds"]
    j = P.run(S=S, edges=g["edges"], Z=np.array([gt[j] @ np.linalg.inv(gt[i]) for i, j in g["edges"]]), fixed=g["fixed"], n_rounds=1, n_cg=8,
              cg_tol=1e-4, lambda0=0.0, preconditioner="JACOBI")
    assert j["rounds"][0]["cg_iterations"] > r["rounds"][0]["cg_iterations"]


@pytest.fixture(scope="module")
def example():
    case, gt = Cc.example_graph()
    runs = dict(dense=P.run(**case, solver="dense"), chain=P.run(**case), jacobi=P.run(**dict(case, preconditioner="JACOBI")))
    return case, gt, runs


def test_example_descent_and_the_reason_for_the_default(example):
    """The example trajectory (121 frames, 124 edges) with the committed seed: CHAIN with n_cg = 8 lands within 1 % of the dense
    solve's final cost, JACOBI with the same n_cg does not -- the measured reason for the default, asserted.  The median
    camera-centre error falls below a fifth (the bar of the close-loop demonstration)."""
    case, gt, runs = example
    assert len(case["S"]) == 121 and len(case["edges"]) == 124 and case["n_cg"] == 8 and case["n_rounds"] == 8
    before = Cc.centre_errors(case["S"], gt)
    for name, r in runs.items():
        after = Cc.centre_errors(r["S_out"], gt)
        print(f"{name}: {P.STATUS[r['status']]}, cost {r['stats']['cost_before']:.4g} -> {r['stats']['cost_after']:.6g}, centre error max "
              f"{before.max():.3f} -> {after.max():.3f}, median {np.median(before):.3f} -> {np.median(after):.3f}, PCG iterations "
              f"{[x['cg_iterations'] for x in r['rounds']]}")
        assert r["status"] == 0
    dense, chain, jacobi = (runs[k]["stats"]["cost_after"] for k in ("dense", "chain", "jacobi"))
    assert abs(chain - dense) <= 0.01 * dense
    assert not abs(jacobi - dense) <= 0.01 * dense and jacobi > 2 * dense
    after = Cc.centre_errors(runs["chain"]["S_out"], gt)
    assert np.median(after) < np.median(before) / 5 and after.max() < before.max() / 5
    assert np.array_equal(runs["chain"]["S_out"][0], np.asarray(case["S"], np.float32)[0])       # the held frame


# ---- the cases of the GPU test ----
@pytest.mark.parametrize("name", list(Cc.CASES))
def test_case_takes_no_marginal_decision_and_does_not_hang_on_the_order_of_sums(name):
    """no accept within 1e-6 relative, no PCG stop within a factor 2 of cg_tol; and the reversed-order run of the restatement
    passes the GPU test's own comparison -- a case where the restatement's two orders disagree could not tell a right kernel from a
    wrong one"""
    ref = Cc.reference(name)
    assert not [x for x in ref["margins"]["accept"] if x < 1e-6], ref["margins"]["accept"]
    assert not [x for x in ref["margins"]["stop"] if 0.5 < x < 2], ref["margins"]["stop"]
    assert Cc.compare(name, Cc.as_got(ref)) == []
    assert Cc.compare(name, Cc.as_got(Cc.reference(name, reverse=True))) == []


def test_the_cases_cover_what_they_are_there_for():
    st = {n: P.STATUS[Cc.reference(n)["status"]] for n in Cc.CASES}
    assert st["n1"] == st["no_edges"] == "NO_EDGES" and st["all_held"] == "NOTHING_FREE" and st["nan_z"] == "NOT_FINITE"
    assert {len(Cc.CASES[n]["S"]) for n in Cc.CASES} >= {1, 2, 3, 255, 256, 257, 513}
    for deg in (15, 16, 17, 65):
        e = Cc.CASES["hub%d" % deg]["edges"]
        assert int((e == 3).sum()) == deg
    acc = [r["accepted"] for r in Cc.reference("far_start")["rounds"]]
    assert 0 in acc and 1 in acc and acc.index(0) < len(acc) - 1 - acc[::-1].index(1)         # a rejected round, accepted ones behind it
    sk = Cc.reference("skipped")
    assert sk["edge_status"][Cc.N_GOOD_BEFORE_SKIPPED:].tolist() == [1] * 7 and not sk["edge_status"][:Cc.N_GOOD_BEFORE_SKIPPED].any()
    fl = Cc.reference("false_loop")
    assert int(np.argmax(fl["edge_cost"])) == Cc.FALSE_LOOP_EDGE
    assert Cc.reference("rounds0")["S_out"].tobytes() == np.asarray(Cc.CASES["rounds0"]["S"], np.float32).tobytes()
    assert {Cc.CASES[n]["preconditioner"] for n in Cc.CASES} == {"CHAIN", "JACOBI"} and {Cc.CASES[n]["with_scale"] for n in Cc.CASES} == {True, False}
    mo = Cc.CASES["missing_odometry"]["edges"].tolist()
    assert [10, 11] not in mo and [9, 10] in mo
    # the rigid graph keeps every frame's scale
    rg = Cc.reference("rigid")
    assert np.allclose(np.cbrt(P.det3(rg["state"][0])), np.cbrt(P.det3(P.mats(Cc.CASES["rigid"]["S"])[0])), rtol=1e-12)


@pytest.mark.parametrize("fault", P.FAULTS)
def test_every_planted_fault_is_seen_by_the_gpu_tests_measure(fault):
    seen = [n for n in Cc.CASES if Cc.compare(n, Cc.as_got(Cc.reference(n, fault=fault)))]
    print(fault, "seen on", seen)
    assert seen


def test_the_budget_is_the_restatements_own(vo):
    rec = json.load(open(BUDGET))["cases"]
    assert set(rec) == set(Cc.CASES)
    for name in Cc.CASES:
        ref = Cc.reference(name)
        fresh = float(Cc.reach(name).max(initial=0.0))
        assert rec[name]["status"] == P.STATUS[ref["status"]] and rec[name]["accepted"] == "".join(str(r["accepted"]) for r in ref["rounds"])
        # rounding noise: it may differ between two builds of NumPy, but a recorded reach far above a fresh one would loosen the ceiling
        assert rec[name]["reach_max"] <= 16 * fresh + 1e-13, (name, rec[name]["reach_max"], fresh)
        assert 4 * rec[name]["reach_max"] <= 0.01 * rec[name]["half_ulp_max"] + 1e-13      # the ceiling is the float32 rounding of the stored state


# ---- the refusals that need no HIP, under the host sanitizers ----
def test_pose_graph_refusals_under_the_host_sanitizers(tmp_path):
    """visual-odometry_amd/csrc/map_checks.h: pose_graph_check in a stand-alone program under AddressSanitizer and UBSan, each row
    against the code and the whole message"""
    exe = str(tmp_path / "pose_graph_checks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "visual-odometry_amd", "csrc"),
                           os.path.join(ROOT, "tests", "hostcheck", "pose_graph_checks_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("pose_graph_checks_check: all ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("-> ok") >= 40 and "FAILED" not in r.stdout
