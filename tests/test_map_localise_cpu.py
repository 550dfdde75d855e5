"""CPU checks behind vo_map_lookup* / vo_map_localise*: the float64 restatement (tests/map_localise_restatement.py) on the
example data, where the answer is known exactly -- every measurement row is a bitwise copy of its landmark's row in world.dat
and trajectory.dat holds every robot pose -- and the ABI of the new entry points on a machine without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_localise_restatement as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vo_map_lookup_dev", "vo_map_lookup_batch_dev", "vo_map_lookup", "vo_map_localise_dev", "vo_map_localise_batch_dev",
       "vo_map_localise")


@pytest.fixture(scope="module")
def data():
    return M.example_data()


def test_lookup_of_every_frame_returns_the_files_ids(data):
    assert len(data["frames"]) == 121 and len(data["world_app"]) == 1000
    assert len({r.tobytes() for r in data["world_app"]}) == 1000              # distinct landmark rows
    tab = M.table(data["world_app"])
    rows = 0
    for uv, app, ids in data["frames"]:
        ent, pairs, xyz = M.lookup(data["world_app"], app, data["world_pts"], tab=tab)
        assert np.array_equal(ent, ids)
        assert np.array_equal(pairs, np.stack([np.arange(len(ids)), ids], 1))
        assert xyz.tobytes() == data["world_pts"][ids].tobytes()
        rows += len(ids)
    assert rows == 10012 and min(len(f[2]) for f in data["frames"]) == 14


def test_lookup_rules():
    rng = np.random.default_rng(0)
    m = rng.standard_normal((6, 10)).astype(np.float32)
    m[1, 3] = 0.0
    m[2] = m[0]                                   # a later equal row is never the answer
    m[4, 7] = np.nan                              # a NaN entry is never found
    q = np.stack([m[0], m[1], m[4], m[5], m[3] + 1])
    q[1, 3] = -0.0                                # -0 equals +0
    ent, pairs, _ = M.lookup(m, q)
    assert ent.tolist() == [0, 1, -1, 5, -1] and pairs.tolist() == [[0, 0], [1, 1], [3, 5]]
    assert M.lookup(m, q, n_live=1)[0].tolist() == [0, -1, -1, -1, -1]


def test_localising_every_frame_from_scratch_recovers_the_trajectory(data):
    """64 hypotheses, 2 px, seed 0, then 50 rounds on the winner's inliers: within 1e-4 of trajectory.dat on all 121 frames
    (measured 4.72e-5, the rounding of the text files)."""
    tab = M.table(data["world_app"])
    worst = 0.0
    for (uv, app, ids), gt in zip(data["frames"], data["gt"]):
        T, status, info = M.localise(data["K"], data["cam"], data["world_pts"], data["world_app"], uv, app, 2.0, 64, 0, 10000.0, 50, 6,
                                     tab=tab)
        assert status == M.OK and info["n_hits"] == len(ids)
        worst = max(worst, float(np.abs(M.robot_pose(T, data["C"]) - gt).max()))
    print("largest pose difference:", worst)
    assert worst < 1e-4


def _declared():
    txt = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", txt))


def test_new_symbols_are_declared_and_exported(vo):
    lib = vo.load_library()
    for n in NEW:
        assert n in _declared(), n
        assert hasattr(lib, n), n
    for n in ("Map", "MapLocaliseStats", "MAP_LOCALISE_STATUS"):
        assert hasattr(vo, n)
    for n in ("lookup", "localise", "localise_batch"):
        assert hasattr(vo.Map, n)
    assert C.sizeof(vo.MapLocaliseStats) == 32
    hpp = open(os.path.join(ROOT, "include", "vo", "localise.hpp")).read()
    assert "class DeviceMap" in hpp and '"localise.hpp"' in open(os.path.join(ROOT, "include", "vo", "vo.hpp")).read()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the failure path is not reachable")
def test_new_symbols_refuse_without_a_device(vo):
    """no context can exist here (VO_ERR_NO_DEVICE), hence no map: every new entry point refuses the null handle"""
    lib = vo.load_library()
    h = C.c_void_p()
    assert lib.vo_ctx_create(0, None, C.byref(h)) == -2 and not h.value
    m = C.c_void_p()
    assert lib.vo_map_create(None, 0, C.byref(m)) == -1 and not m.value
    z, i = None, C.c_int
    prm = vo.RansacParams(64, 2.0, 0)
    K = np.eye(3, dtype=np.float32)
    n_out = C.c_int(-1)
    st = vo.MapLocaliseStats()
    T = np.zeros(16, np.float32)
    kp, tp = K.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
    assert lib.vo_map_lookup_dev(z, z, i(0), z, z, z, z, z, z) == -1 and b"null map" in lib.vo_last_error()
    assert lib.vo_map_lookup_batch_dev(z, i(1), z, C.c_size_t(0), i(0), z, z, z, z, z, z) == -1
    assert lib.vo_map_lookup(z, z, i(0), z, C.byref(n_out), z, z) == -1
    assert lib.vo_map_localise_dev(z, i(480), i(640), i(0), i(5), kp, z, z, i(1), z, C.byref(prm), C.c_float(1e4), i(50), i(6), z, z,
                                   z) == -1
    assert lib.vo_map_localise_batch_dev(z, i(1), i(480), i(640), i(0), i(5), kp, z, C.c_size_t(1), z, C.c_size_t(1), i(1), z,
                                         C.byref(prm), C.c_float(1e4), i(50), i(6), z, z, z) == -1
    assert lib.vo_map_localise(z, i(480), i(640), i(0), i(5), kp, z, z, i(1), C.byref(prm), C.c_float(1e4), i(50), i(6), z, tp,
                               C.byref(st)) == -1
    assert b"null map" in lib.vo_last_error()
    with pytest.raises(vo.VoError):
        vo.Map()
