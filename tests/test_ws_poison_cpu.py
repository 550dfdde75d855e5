"""What tests/test_gpu_ws_poison.py rests on, without a GPU: the parser of the hook VO_WS_POISON as a stand-alone program built
with the host sanitizers, and the comparisons of its part (b) shown to bite.  For every family whose restatement takes a planted
`fault=`, the UNFAULTED restatement, dressed as the device's outputs, passes the comparison the GPU test uses, and one FAULTED
restatement of the same case does not: no kernel has to be broken to know that a poisoned workspace that changed a result would be
seen."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import map_bundle_cases as Bc
import map_cull_cases as Qc
import map_fuse_cases as Fc
import map_fuse_restatement as Fr
import map_grow_cases as Gc
import map_guided_cases as Uc
import map_guided_restatement as U
import map_keyframes_cases as Kc
import map_keyframes_restatement as K
import map_loops_cases as Lc
import map_loops_restatement as L
import map_nearest_cases as Nc
import map_nearest_restatement as N
import map_pose_refine_cases as Pc
import map_pose_refine_restatement as P
import map_refine_cases as Rc
import map_refine_restatement as R
import pose_graph_cases as PGc
import test_gpu_map_bundle as TB
import test_gpu_map_cull as TQ
import test_gpu_map_grow as TG
import test_gpu_map_pose_refine as TP
import test_gpu_map_refine as TR
from map_pose_refine_dev import colmajor16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_of_the_parser(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed to build tests/hostcheck/ws_poison_check.cpp"
    exe = str(tmp_path / "ws_poison_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "visual-odometry_amd", "csrc"), os.path.join(ROOT, "tests", "hostcheck", "ws_poison_check.cpp"), "-o", exe],
                   check=True)
    env = {k: v for k, v in os.environ.items() if k != "VO_WS_POISON"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ws_poison_check: ok" in r.stdout


# ---- the comparisons that return a list of differences -----------------------------------------------------------------------------
LISTED = [
    ("nearest", lambda f: [N.compare(Nc.reference(n), Nc.reference(n, fault=f)) for n in Nc.CASES], "tie_to_higher"),
    ("guided", lambda f: [U.compare(Uc.reference(n), Uc.reference(n, fault=f)) for n in Uc.CASES if n != "frames14"], "tie_to_higher"),
    ("fuse", lambda f: [Fr.compare(Fc.reference(n), Fc.reference(n, fault=f)) for n in Fc.CASES], "higher_survives"),
    ("keyframes", lambda f: [K.compare(Kc.reference(n, k), Kc.reference(n, k, fault=f)) for n in ("words_1", "frames_63") for k in range(len(Kc.case(n)["runs"]))],
     "tie_to_highest"),
    ("loops", lambda f: [L.compare(Lc.reference(n), L.as_got(Lc.reference(n, fault=f))) for n in ("small13", "content64")], "tie_reversed"),
    ("pose_graph", lambda f: [PGc.compare(n, PGc.as_got(PGc.reference(n, fault=f))) for n in ("n3", "hub17")], "right_update"),
]


@pytest.mark.parametrize("family,diffs,fault", LISTED, ids=[x[0] for x in LISTED])
def test_a_faulted_restatement_fails_the_comparison(family, diffs, fault):
    assert all(d == [] for d in diffs(None)), family               # the restatement against itself: no difference
    assert any(d != [] for d in diffs(fault)), (family, fault)


# ---- the comparisons that assert: the restatement dressed as the device's outputs ------------------------------------------------
def _refine(vo, name, fault):
    c = Rc.case(name)
    r = Rc.reference(name) if fault is None else R.refine(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], fault=fault,
                                                          **dict(c["params"], **({"n_rows": c["n_rows"]} if c["n_rows"] is not None else {})))
    TR._compare(name, r["status"], r["points"], np.asarray(c["map_pts"], np.float32), r["stats"])


def _poses(vo, name, fault):
    c = Pc.case(name)
    kw = dict(c["params"], **({"n_rows": c["n_rows"]} if c["n_rows"] is not None else {}))
    r = Pc.reference(name) if fault is None else P.refine_poses(c["K"], c["map_pts"], c["map_app"], c["frames"], c["poses"], c.get("fixed"), fault=fault, **kw)
    start = colmajor16(c["poses"])
    T16 = start.copy()
    ok = (r["status"] == P.OK) & (c["params"]["n_rounds"] > 0)
    T16[ok] = colmajor16(r["poses"])[ok]
    H = np.full((len(start), 36), -7.0)
    solved = np.isfinite(r["H"]).all((1, 2))
    H[solved] = r["H"][solved].transpose(0, 2, 1).reshape(-1, 36)
    TP._compare(name, T16, r["status"], H, r["stats"], start)


def _bundle(vo, name, fault):
    c = Bc.case(name)
    r = Bc.reference(name) if fault is None else Bc.run(c, fault=fault)
    d = types.SimpleNamespace(bstats=lambda raw: raw, rounds=lambda raw: raw)
    start16, pts0 = colmajor16(c["poses"]), np.asarray(c["map_pts"], np.float32)
    wrote = r["status"] == 0 and r["stats"]["n_accepted"] > 0
    T16 = colmajor16(r["poses"]) if wrote else start16
    pts = np.asarray(r["points"], np.float32) if wrote else pts0
    TB._compare(name, d, (T16, pts, r["pose_status"], r["point_status"], r["rounds"], dict(r["stats"], status=r["status"])), start16, pts0)


def _cull(vo, name, fault):
    r = Qc.reference(name) if fault is None else Qc.run(Qc.case(name), fault=fault)
    ent = np.zeros(len(r["verdict"]), vo.MAP_CULL_ENTRY_DTYPE)
    for k in ("verdict", "n_obs", "n_frames", "mean_sq_px", "max_sq_px", "min_z", "cos_parallax"):
        ent[k] = r[k]
    d = types.SimpleNamespace(cstats=lambda raw: raw)
    TQ._compare(name, d, (r["verdict"], r["remap"], ent, r["stats"]))


def _grow(vo, name, fault):
    r = Gc.reference(name) if fault is None else Gc.run(Gc.case(name), fault=fault)
    n = r["stats"]["n_tracks"]
    tr = np.zeros(n, vo.MAP_GROW_TRACK_DTYPE)
    for k in ("verdict", "n_obs", "n_frames", "entry", "first_key", "refined", "xyz", "mean_sq_px", "max_sq_px", "min_z", "cos_parallax"):
        tr[k] = r[k][:n]
    d = types.SimpleNamespace(gstats=lambda raw: raw, track_cap=max(n, 1))
    TG._compare(name, d, (r["rows"], tr, r["stats"]))


ASSERTED = [("refine", _refine, "map_of_255", "translation_dropped"), ("pose_refine", _poses, "edges", "angles_swapped"),
            ("bundle", _bundle, "hand", "sign_in_Jp"), ("cull", _cull, "precedence", "mean_over_16"), ("grow", _grow, "verdicts", "tracks_by_last_key")]


@pytest.mark.parametrize("family,dress,name,fault", ASSERTED, ids=[x[0] for x in ASSERTED])
def test_a_faulted_restatement_fails_the_asserting_comparison(vo, family, dress, name, fault):
    dress(vo, name, None)                                         # the restatement itself passes: the dressing is right
    with pytest.raises(AssertionError):
        dress(vo, name, fault)
