"""The workspace contract ("The workspace contract"): a call reads nothing from a workspace that the same call has
not written first.  Every workspace is a grow-only DevBuf that nothing ever clears; the test hook VO_WS_POISON=<byte> makes
DevBuf::ensure fill the whole buffer with the byte before the call that sized it runs, so a read of anything the call has not
written reads the byte instead of whatever a fresh allocation happened to hold.

  (a) the hook reaches the device: the one place where workspace bytes are legitimately visible (voe_map_loops_problems_dev);
  (b) every map family under the bytes 0x00 (what a counter wants to find), 0xFF (what the tables and claim words call "empty")
      and 0xA5 (neither), on a fresh handle per run: the family's own comparison against its cached restatement, the bytes of the
      unpoisoned call on another fresh handle, and the map afterwards against that twin's;
  (c) reuse WITHOUT the hook -- what poison overwrites: a handle that has run every call on the full window of
      tests/map_state_cases.py, and the neighbours that share a buffer, then runs the call under test on a shorter window with
      other row counts; against a fresh twin that runs the short call alone, byte for byte and with guards;
  (d) the context's workspaces under the three bytes, against the oracles their own tests use.

The comparisons are those of the families' own tests; tests/test_ws_poison_cpu.py shows on the CPU that each of them fails on a
faulted restatement.  The environment is flipped in-process and restored in a `finally`.  Nothing here captures a graph."""
import contextlib
import ctypes as C
import os
import time

import numpy as np
import pytest

import map_align_cases as Ac
import map_align_restatement as A
import map_bundle_cases as Bc
import map_covis_cases as Cc
import map_cull_cases as Qc
import map_fuse_cases as Fc
import map_fuse_restatement as Fr
import map_grow_cases as Grc
import map_guided_cases as Gc
import map_guided_restatement as G
import map_keyframes_cases as Kc
import map_keyframes_restatement as K
import map_loops_cases as Lc
import map_loops_restatement as L
import map_nearest_cases as Nc
import map_nearest_restatement as N
import map_pose_refine_cases as Pc
import map_refine_cases as Rc
import map_state_cases as S
import map_states as MS
import pose_graph_cases as PGc
import ransac_restatement as Rr
import test_gpu_epi_refine as TER
import test_gpu_epi_sizes as TES
import test_gpu_map_align as TA
import test_gpu_map_apply_correction as TAp
import test_gpu_map_bundle as TB
import test_gpu_map_covis as TCv
import test_gpu_map_cull as TQ
import test_gpu_map_grow as TG
import test_gpu_map_pose_refine as TP
import test_gpu_map_refine as TR
import test_gpu_pose_graph as TPG
import test_gpu_pose_ransac_batch as TPB
import test_gpu_ransac_sizes as TRS
import test_gpu_sizes as TS
from map_align_dev import AlignDev
from map_bundle_dev import BundleDev
from map_covis_dev import CovisDev
from map_cull_dev import CullDev
from map_fuse_dev import FuseDev
from map_grow_dev import GrowDev
from map_guided_dev import GuidedDev
from map_keyframes_dev import KeyframesDev
from map_loops_dev import LoopsDev
from map_nearest_dev import NearestDev
from map_pose_refine_dev import PoseDev
from map_refine_dev import RefineDev
from map_states import Outs, Win, i32
from oracle.oracle import Camera as OCam
from ransac_batch_dev import BatchDev, single_results
from ransac_batch_dev import same as same_problem
from test_gpu_epi_refine import noisy  # noqa: F401  (the fixture of its parity test)

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0xA5)
byte_ids = pytest.mark.parametrize("byte", BYTES, ids=lambda b: "0x%02X" % b)


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    print(f"\n[time] {request.node.name}: {time.perf_counter() - t0:.2f} s")


@contextlib.contextmanager
def poison(byte):
    """VO_WS_POISON for the calls inside; None: the variable unset (the twin's run)"""
    old = os.environ.get("VO_WS_POISON")
    try:
        if byte is None:
            os.environ.pop("VO_WS_POISON", None)
        else:
            os.environ["VO_WS_POISON"] = "0x%02X" % byte
        yield
    finally:
        if old is None:
            os.environ.pop("VO_WS_POISON", None)
        else:
            os.environ["VO_WS_POISON"] = old


def same(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- (a) the hook reaches the device ----------------------------------------------------------------------------------------------
def test_the_hook_reaches_the_device(vo, ctx):
    """voe_map_loops_batch_dev of `one_loop` under 0xA5 on a fresh map: loops_pairs_kernel (map_loops.hip) writes the gathered
    points of a slot only for its `count` pairs, so the rows of d_world_xyz behind d_n_pairs[0] still hold what ensure() left --
    every byte 0xA5.  Without the hook the same call gives the same outputs."""
    c = Lc.case("one_loop")
    with poison(0xA5):
        d = LoopsDev(vo, ctx, c)
        try:
            d.clear_out()
            assert d.call() == 0, ctx.lib.vo_last_error()
            out = d.outputs()
            pr = d.problems()
            n = int(pr["n_pairs"][0])
            assert 6 <= n < d.n_max, (n, d.n_max)                 # a filled slot with rows behind its pairs
            tail = pr["world"][0, n:].view(np.uint8)
            assert tail.size > 0 and (tail == 0xA5).all(), np.unique(tail)
            assert not (pr["world"][0, :n].view(np.uint8) == 0xA5).all()
        finally:
            d.close()
    with poison(None):
        t = LoopsDev(vo, ctx, c)
        try:
            t.clear_out()
            assert t.call() == 0, ctx.lib.vo_last_error()
            assert same(t.outputs(), out)
            w = t.problems()["world"][0, n:].view(np.uint8)
            print(f"behind the {n} pairs of slot 0 without the hook: bytes {np.unique(w).tolist()[:8]}")
        finally:
            t.close()


# ---- (b) every family on a fresh handle under the three bytes ----------------------------------------------------------------
# The families whose harness and comparison have one shape: Dev(vo, ctx, case) / clear_out / call / outputs / got / map_state and
# compare(reference, got) -> list of differences.  Byte-compared: poison adds no tolerance.
_twins = {}


def _uniform_run(vo, ctx, Dev, case, byte):
    """(outputs with their guard words, got, the map afterwards) of one call on a fresh handle; the map is BUILT under the byte as
    well (vo_map_update's scratch)"""
    d = None
    try:
        with poison(byte):
            d = Dev(vo, ctx, case)
            d.clear_out()
            assert d.call() == 0, ctx.lib.vo_last_error()
            out = d.outputs()
            got = d.got()[0] if Dev is LoopsDev else d.got(out)   # (the loops' problems live in the workspace: read before anything else runs)
        with poison(None):
            state = d.map_state()
    finally:
        if d is not None:
            d.close()
    return out, got, state


def _uniform(vo, ctx, family, Dev, cases, compare, name, byte):
    c, ref = cases.case(name), cases.reference(name)
    key = (family, name)
    if key not in _twins:                                         # the unpoisoned call on a fresh handle: once per case
        _twins[key] = _uniform_run(vo, ctx, Dev, c, None)
    t_out, _, t_state = _twins[key]
    out, got, state = _uniform_run(vo, ctx, Dev, c, byte)
    bad = compare(ref, got)
    assert bad == [], bad
    assert same(out, t_out), f"{family} {name}: the outputs under 0x{byte:02X} are not the unpoisoned call's"
    assert same(state, t_state), f"{family} {name}: the map after the call under 0x{byte:02X} is not the unpoisoned twin's"


@byte_ids
@pytest.mark.parametrize("name", list(Nc.CASES))
def test_nearest(vo, ctx, name, byte):
    _uniform(vo, ctx, "nearest", NearestDev, Nc, N.compare, name, byte)


@byte_ids
@pytest.mark.parametrize("name", list(Gc.CASES))
def test_guided(vo, ctx, name, byte):
    _uniform(vo, ctx, "guided", GuidedDev, Gc, G.compare, name, byte)


@byte_ids
@pytest.mark.parametrize("name", list(Fc.CASES))
def test_fuse(vo, ctx, name, byte):
    _uniform(vo, ctx, "fuse", FuseDev, Fc, Fr.compare, name, byte)


@byte_ids
@pytest.mark.parametrize("name", list(Lc.CASES))
def test_loops(vo, ctx, name, byte):
    """the integers byte for byte; Z within the one ulp of its largest term that tests/test_gpu_map_loops.py allows -- and every
    output, the float ones included, the bytes of the unpoisoned call"""
    log = {}

    def compare(ref, got):
        bad = L.compare(ref, got, log)
        return bad if bad or log["z_ulp"] <= 1.0 else [("z_ulp", log["z_ulp"])]
    _uniform(vo, ctx, "loops", LoopsDev, Lc, compare, name, byte)


@byte_ids
@pytest.mark.parametrize("name", list(Kc.CASES))
def test_keyframes(vo, ctx, name, byte):
    c = Kc.case(name)
    res = {}
    for b in (None, byte):
        if b is None and ("keyframes", name) in _twins:
            res[b] = _twins[("keyframes", name)]
            continue
        with poison(b):
            d = KeyframesDev(vo, ctx, c)
            try:
                runs = []
                for prm in c["runs"]:
                    d.clear_out()
                    assert d.call(prm) == 0, ctx.lib.vo_last_error()
                    runs.append(d.results())
                bits = d.bits()
                stats = [d.stats(r["stats_raw"]) for r in runs]
            finally:
                d.close()
        res[b] = (runs, stats, bits)
        if b is None:
            _twins[("keyframes", name)] = res[b]
    runs, stats, bits = res[byte]
    for k, got in enumerate(runs):
        ref = Kc.reference(name, k)
        assert stats[k] == ref["stats"], (name, k, stats[k], ref["stats"])
        for key in K.KEYS:
            assert got[key].tobytes() == ref[key].tobytes(), (name, k, key)
        assert (got["guard"] == -7).all()
        assert all(got[key].tobytes() == res[None][0][k][key].tobytes() for key in got), (name, k)
    assert bits.tobytes() == c["bits"].tobytes()


# ---- (b) continued: the families whose comparison lives in their own test module ------------------------------------------------
# Each run(byte) builds a fresh handle under the byte, makes the one call, and returns (every output and the map afterwards as a
# list of arrays, what the family's own comparison takes).  The arrays must be the bytes of the unpoisoned run on another fresh
# handle -- computed once per case and shared by the three bytes --, which for the float64-compared families is the promise
# "three calls give the same bytes" held across handles and across what the workspace held before.


def _map_after(ctx, m, own_app):
    """points, appearances, the header's four words, and the lookup of the map's own rows (call it with the variable unset)"""
    pts, app = m.read()
    out = [pts, app, MS.header(ctx, m)]
    own = np.asarray(own_app, np.float32).reshape(-1, 10)
    if len(own):
        out.append(m.lookup(own)[1])
    return out


def _against_twin(family, name, byte, run, check):
    key = (family, name)
    if key not in _twins:
        _twins[key] = run(None)[0]
    arrays, payload = run(byte)
    check(payload)
    twin = _twins[key]
    assert len(arrays) == len(twin)
    for k, (x, y) in enumerate(zip(arrays, twin)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), f"{family} {name}: array {k} under 0x{byte:02X} is not the unpoisoned twin's"


@byte_ids
@pytest.mark.parametrize("name", list(Rc.CASES))
def test_refine(vo, ctx, name, byte):
    c = Rc.case(name)

    def run(b):
        d = None
        try:
            with poison(b):
                d = RefineDev(vo, ctx, c)
                d.clear_out()
                assert d.call(status=True, xyz=False) == 0, ctx.lib.vo_last_error()      # in place: the map moves
                status, _, raw = d.results()
            with poison(None):
                after = _map_after(ctx, d.m, c["map_app"])
                return [status, raw] + after, (status, after[0], d.stats(raw))
        finally:
            if d is not None:
                d.close()
    _against_twin("refine", name, byte, run, lambda p: TR._compare(name, p[0], p[1], c["map_pts"], p[2]))


@byte_ids
@pytest.mark.parametrize("name", list(Pc.CASES))
def test_pose_refinement(vo, ctx, name, byte):
    c = Pc.case(name)

    def run(b):
        d = None
        try:
            with poison(b):
                d = PoseDev(vo, ctx, c)
                d.clear_out()
                assert d.call() == 0, ctx.lib.vo_last_error()
                T16, status, H, raw = d.results()
            with poison(None):
                after = _map_after(ctx, d.m, c["map_app"])
                return [T16, status, H, raw] + after, (T16, status, H, d.stats(raw), d.T0)
        finally:
            if d is not None:
                d.close()
    _against_twin("pose_refine", name, byte, run, lambda p: TP._compare(name, *p))


@byte_ids
@pytest.mark.parametrize("name", list(Bc.CASES))
def test_bundle(vo, ctx, name, byte):
    c = Bc.case(name)

    def run(b):
        d = None
        try:
            with poison(b):
                d = BundleDev(vo, ctx, c)
                d.clear_bundle_out()
                assert d.bundle() == 0, ctx.lib.vo_last_error()
                ctx.synchronize()
            with poison(None):
                got = d.bundle_results()
                after = _map_after(ctx, d.m, c["map_app"])
                return list(got) + after, (d, got)
        finally:
            if d is not None:
                d.close()
    _against_twin("bundle", name, byte, run, lambda p: TB._compare(name, p[0], p[1], p[0].T0, np.asarray(c["map_pts"], np.float32)))


@byte_ids
@pytest.mark.parametrize("name", list(Qc.CASES))
def test_cull(vo, ctx, name, byte):
    c = Qc.case(name)

    def run(b):
        d = None
        try:
            with poison(b):
                d = CullDev(vo, ctx, c)
                d.clear_cull_out()
                assert d.cull() == 0, ctx.lib.vo_last_error()
                ctx.synchronize()
            with poison(None):
                got = d.cull_results()
                after = _map_after(ctx, d.m, c["map_app"])
                return [got[0], got[1], got[2].view(np.uint8), got[3]] + after + [d.lookups()], (d, got)
        finally:
            if d is not None:
                d.close()
    _against_twin("cull", name, byte, run, lambda p: TQ._compare(name, p[0], p[1]))


@byte_ids
@pytest.mark.parametrize("name", list(Grc.CASES))
def test_grow(vo, ctx, name, byte):
    c = Grc.case(name)

    def run(b):
        d = None
        try:
            with poison(b):
                d = GrowDev(vo, ctx, c)
                d.clear_grow_out()
                assert d.grow() == 0, ctx.lib.vo_last_error()
                ctx.synchronize()
            with poison(None):
                rows, tr, raw = d.grow_results()
                after = _map_after(ctx, d.m, c["map_app"])
                return [rows, tr.view(np.uint8), raw] + after + [d.lookups()], (d, (rows, tr, raw))
        finally:
            if d is not None:
                d.close()
    _against_twin("grow", name, byte, run, lambda p: TG._compare(name, p[0], p[1]))


@byte_ids
@pytest.mark.parametrize("name", list(Ac.CASES))
def test_align(vo, ctx, name, byte):
    c, ref = Ac.case(name), Ac.reference(name)

    def run(b):
        d = None
        try:
            with poison(b):
                d = AlignDev(vo, ctx, c)
                d.clear_out()
                assert d.align() == 0, ctx.lib.vo_last_error()
                got = d.results()
            with poison(None):
                after = _map_after(ctx, d.dst, c["dst_app"]) + _map_after(ctx, d.src, c["src_app"])
                return [got["S"], got["pairs"], got["mask"], got["counts"], got["raw_stats"]] + after, got
        finally:
            if d is not None:
                d.close()
    _against_twin("align", name, byte, run, lambda got: TA._check_against_reference(name, got, ref))


@byte_ids
@pytest.mark.parametrize("policy", [A.TAKE_SRC, A.KEEP_DST])
@pytest.mark.parametrize("name", list(Ac.MERGE_CASES) + ["example", "nan", "disjoint"])
def test_merge(vo, ctx, name, policy, byte):
    c, r = Ac.case(name), Ac.reference(name)
    S = r["S"] if r["status"] == A.OK else None
    ref = A.merge(c, S, policy)

    def run(b):
        d = None
        try:
            with poison(b):
                d = AlignDev(vo, ctx, c)
                d.clear_out()
                assert d.merge(S, policy) == 0, ctx.lib.vo_last_error()
                got = d.merge_results()
            with poison(None):
                dst, src = _map_after(ctx, d.dst, ref["app"]), _map_after(ctx, d.src, c["src_app"])
                st = got["stats"]
                return [got["remap"], np.array([st[k] for k in sorted(st)])] + dst + src, (got, dst, src)
        finally:
            if d is not None:
                d.close()

    def check(p):
        got, dst, src = p
        assert got["stats"] == ref["stats"], (got["stats"], ref["stats"])
        assert np.array_equal(got["remap"], ref["remap"])
        assert np.array_equal(dst[0], ref["pts"], equal_nan=True) and dst[1].tobytes() == ref["app"].tobytes()
        assert src[0].tobytes() == np.asarray(c["src_pts"], np.float32).tobytes() and src[1].tobytes() == np.asarray(c["src_app"], np.float32).tobytes()
    _against_twin("merge", f"{name}-{policy}", byte, run, check)


@byte_ids
@pytest.mark.parametrize("name", list(Cc.CASES))
def test_covis_and_window(vo, ctx, name, byte):
    c, ref = Cc.case(name), Cc.reference(name)

    def run(b):
        d = None
        try:
            with poison(b):
                d = CovisDev(vo, ctx, c)
                d.clear_covis_out()
                assert d.covis() == 0, ctx.lib.vo_last_error()
                bits, counts, raw, guard = d.covis_results()
                wins = []
                for prm in c["windows"]:
                    d.clear_window_out()
                    assert d.window(prm) == 0, ctx.lib.vo_last_error()
                    wins.append(d.window_results())
            with poison(None):
                after = d.map_state()
                flat = [w[k] for w in wins for k in sorted(w)]
                return [bits, counts, raw, guard] + flat + after, (d.cstats(raw), bits, counts, guard, wins, d)
        finally:
            if d is not None:
                d.close()

    def check(p):
        st, bits, counts, guard, wins, d = p
        assert st == ref["stats"], (st, ref["stats"])
        assert bits.tobytes() == ref["bits"].tobytes() and (guard == 0xA5A5A5A5).all() and counts.tobytes() == ref["counts"].tobytes()
        for k, got in enumerate(wins):
            TCv._check_window(d, name, k, got)
    _against_twin("covis", name, byte, run, check)


@byte_ids
@pytest.mark.parametrize("name", list(Cc.WINDOW_CASES))
def test_window_on_given_bits(vo, ctx, name, byte):
    c = Cc.case(name)

    def run(b):
        d = None
        try:
            with poison(b):
                d = CovisDev(vo, ctx, c)
                wins = []
                for prm in c["windows"]:
                    d.clear_window_out()
                    assert d.window(prm) == 0, ctx.lib.vo_last_error()
                    wins.append(d.window_results())
            return [w[k] for w in wins for k in sorted(w)], (wins, d)
        finally:
            if d is not None:
                d.close()

    def check(p):
        for k, got in enumerate(p[0]):
            TCv._check_window(p[1], name, k, got)
    _against_twin("window", name, byte, run, check)


@byte_ids
@pytest.mark.parametrize("name", ["frames17", "map2049", "example"])
def test_apply_correction(vo, ctx, name, byte):
    """the reference frames exactly (the NumPy minimum key), the moved points within the one ulp of tests/test_gpu_map_apply_correction.py
    and the bytes of the unpoisoned call"""
    c, S_old, S_new = TAp._scene(name)

    def run(b):
        m = None
        try:
            with poison(b):
                m = TAp._fresh(vo, ctx, c)
                ref, st = m.apply_correction(c["frames"], S_old, S_new)
            with poison(None):
                after = _map_after(ctx, m, c["map_app"])
                return [ref, np.array([st[k] for k in sorted(st)])] + after, (ref, st, after[0])
        finally:
            if m is not None:
                m.close()

    def check(p):
        ref, st, pts1 = p
        m = TAp._fresh(vo, ctx, c)
        try:
            ref_np, _ = TAp._min_keys(m, c)
        finally:
            m.close()
        pts0 = np.asarray(c["map_pts"], np.float32)
        assert np.array_equal(ref, ref_np)
        changed = np.array([f >= 0 and S_old[f].tobytes() != S_new[f].tobytes() for f in ref_np])
        assert st == dict(n_entries=len(pts0), n_seen=int((ref_np >= 0).sum()), n_moved=int(changed.sum()))
        assert pts1[~changed].tobytes() == pts0[~changed].tobytes()
        want32 = np.array([TAp._moved64(pts0[e], S_old[ref_np[e]], S_new[ref_np[e]]) for e in np.nonzero(changed)[0]]).astype(np.float32)
        ulps = np.abs(pts1[changed].astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
        assert changed.any() and ulps.max() <= 1.0
    _against_twin("apply_correction", name, byte, run, check)


# ---- (b) continued: the families without named cases, on the window of tests/map_state_cases.py -----------------------------
STATE = "replayed"                                                # 900 entries, 7 frames x 312 rows; the twin of that state holds them all


def _struct(cls, raw, k=0):
    s = cls()
    C.memmove(C.byref(s), np.ascontiguousarray(raw).ctypes.data + k * C.sizeof(cls), C.sizeof(cls))
    return s.as_dict()


def _ints(d, *drop):
    return {k: v for k, v in d.items() if not isinstance(v, float) and k not in drop}


def _window_run(vo, ctx, c, call, byte):
    """call(win, m, outs, size) on a fresh map holding cut(c), built under the byte; (outputs, map afterwards)"""
    st = win = o = None
    try:
        with poison(byte):
            st = MS.build_exact(vo, ctx, *S.cut(c))
            win = Win(vo, ctx, c)
            o = Outs(ctx)
            call(win, st.m, o, c["kept"])
            out = o.read()
        with poison(None):
            return out, MS.content(ctx, st.m, st.cap)
    finally:
        for x in (o, win, st):
            if x is not None:
                x.close()


def _window_family(vo, ctx, family, call, byte, check):
    c = S.case(STATE)
    if (family, STATE) not in _twins:
        _twins[(family, STATE)] = _window_run(vo, ctx, c, call, None)
    t_out, t_map = _twins[(family, STATE)]
    out, after = _window_run(vo, ctx, c, call, byte)
    check(c, out, after)
    assert out.keys() == t_out.keys()
    for k in out:
        assert out[k].tobytes() == t_out[k].tobytes(), f"{family}: '{k}' under 0x{byte:02X} is not the unpoisoned twin's"
    assert all(x.tobytes() == y.tobytes() for x, y in zip(after, t_map)), f"{family}: the map afterwards is not the twin's"


def _check_lookup(c, out, after):
    F, n = len(c["frames"]), S.ROWS
    cnt, ent = i32(out["counts"]), i32(out["entries"]).reshape(F, n)
    pairs, xyz = i32(out["pairs"]).reshape(F, n, 2), out["xyz"].view(np.float32).reshape(F, n, 3)
    for f, (e_ref, p_ref, x_ref) in enumerate(S.reference(STATE, "lookup")):
        k = len(p_ref)
        assert cnt[f] == k and np.array_equal(ent[f], e_ref) and np.array_equal(pairs[f, :k], p_ref)
        assert xyz[f, :k].tobytes() == np.ascontiguousarray(x_ref, np.float32).tobytes()
        assert MS.untouched(out["pairs"].reshape(F, n, 8)[f, k:]) and MS.untouched(out["xyz"].reshape(F, n, 12)[f, k:])


@byte_ids
def test_lookup(vo, ctx, byte):
    _window_family(vo, ctx, "lookup", lambda w, m, o, size: w.lookup(m, o, size), byte, _check_lookup)


@byte_ids
def test_localise(vo, ctx, byte):
    def check(c, out, after):
        for f, (e_ref, p_ref, _) in enumerate(S.reference(STATE, "lookup")):
            st = _struct(vo.MapLocaliseStats, out["stats"], f)
            assert st["n_rows"] == S.ROWS and st["n_hits"] == len(p_ref) and st["status"] == 0, (f, st)
    _window_family(vo, ctx, "localise", lambda w, m, o, size: w.localise(m, o, size), byte, check)


@byte_ids
def test_adjust(vo, ctx, byte):
    def check(c, out, after):
        ref = S.run("adjust", c)
        assert np.array_equal(i32(out["pose_status"]), ref["pose_status"]) and np.array_equal(i32(out["point_status"]), ref["point_status"])
        for k, sw in enumerate(ref["sweeps"]):
            assert _ints(_struct(vo.MapPoseRefineStats, out["stats"][96 * k:])) == _ints(sw["poses"])
            assert _ints(_struct(vo.MapRefineStats, out["stats"][96 * k + 48:])) == _ints(sw["points"])
    _window_family(vo, ctx, "adjust", lambda w, m, o, size: w.adjust(m, o, size, S.ADJUST), byte, check)


@byte_ids
def test_update(vo, ctx, byte):
    """two updates under the byte -- 600 new rows, then 300 rows the map holds (the same points) with 300 new ones -- leave the
    rows in order, bit for bit, and every row is found at its index"""
    c = S.case(STATE)
    pts, app = S.cut(c)
    with poison(byte):
        m = vo.Map(ctx, capacity=4096)
        try:
            m.update(pts[:600], app[:600])
            m.update(pts[300:], app[300:])
            with poison(None):
                p, a, h = MS.content(ctx, m, 4096)
                assert h[0] == 900 and h[1] == 600 and h[2] == 600 and h[3] == 0, h
                assert p.tobytes() == pts.tobytes() and a.tobytes() == app.tobytes()
                assert np.array_equal(m.lookup(app)[1], np.arange(900))
        finally:
            m.close()


# ---- (c) reuse without the hook ---------------------------------------------------------------------------------------------------
# What poison overwrites: real leftovers at shifted offsets, and what a handle holds that is no DevBuf.  The "used" map runs calls
# on the full window (7 frames x 312 rows) first, then the call under test on frames 2 .. 5 cut to 200 rows each, by pointer
# offset into the same device arrays; the twin is a fresh map that runs the short call alone.
F0, F1, SHORT_ROWS = 2, 6, 200
FUSE = dict(radius_xyz=0.5, radius=0.8)
NEAREST = dict(radius=0.5, ratio=0.8)
GUIDED = dict(radius_px=6.0, radius=0.5, ratio=0.8)
KEYFRAMES = dict(min_observers=1, share_permille=500, min_seen=1, max_gap=0, max_dropped=2)
LOOPS = dict(gap=1, ref_window=1, min_shared=5, separation=0, max_loops=2, threshold_px=2.0, n_hypotheses=64, seed=0, kernel_threshold=10000.0, n_iters=10,
             min_inliers=6, w_loop=(1.0, 1.0, 1.0))
V = MS.V


class SubWin(Win):
    """frames [f0, f1) of a window, the first n_max rows of each: the same device arrays at an offset, the same strides"""

    def __init__(self, full, f0, f1, n_max):
        self.vo, self.ctx, self.lib, self.K = full.vo, full.ctx, full.lib, full.K
        self.F, self.n_max, self.stride = f1 - f0, n_max, full.stride
        self.T0 = np.ascontiguousarray(full.T0[f0:f1])
        self.d_uv, self.d_app, self.d_fixed = full.d_uv + 8 * f0 * full.stride, full.d_app + 40 * f0 * full.stride, full.d_fixed + f0
        self.rows = self.F * self.n_max

    def close(self):
        pass


def _short_case(c, f0=F0, f1=F1):
    return dict(c, frames=[(uv[:SHORT_ROWS], a[:SHORT_ROWS]) for uv, a in c["frames"][f0:f1]], poses=c["poses"][f0:f1], fixed=c["fixed"][f0:f1])


def _restore(st, c):
    """the map's points back where the case has them (an update of rows the map holds), and the host's bound back at the size"""
    st.m.update(*S.cut(c))
    assert len(st.m) == c["kept"]
    st.check_bound()


# the calls on a window: name -> (call(win, map, outs, size), changes the map).  Every one is a `_dev` form on guarded output arrays
# (Outs: 64 elements behind each array, read back).  `unique` is 1 on the full window and 0 on the short one, where the call has it.
def _unique(w):
    return 0 if isinstance(w, SubWin) else 1


def _nearest(w, m, o, n):
    prm = w.vo.MapNearestParams(NEAREST["radius"], NEAREST["ratio"], _unique(w), 0)
    w._ok(w.lib.voe_map_nearest_batch_dev(m.h, C.c_int(w.F), V(w.d_app), C.c_size_t(w.stride), C.c_int(w.n_max), None, C.byref(prm),
                                          V(o.new("entry", w.rows, 4)), V(o.new("status", w.rows, 4)), V(o.new("dist2", w.rows, 4)),
                                          V(o.new("app_out", w.F * w.stride, 40)), V(o.new("stats", 1, 32))))


def _guided(w, m, o, n):
    prm = w.vo.MapGuidedParams(GUIDED["radius_px"], GUIDED["radius"], GUIDED["ratio"], _unique(w), MS.CAM[2], MS.CAM[3])
    w._ok(w.lib.voe_map_guided_batch_dev(m.h, C.c_int(w.F), w.K.ctypes.data_as(C.c_void_p), V(w.d_uv), C.c_size_t(w.stride), V(w.d_app),
                                         C.c_size_t(w.stride), C.c_int(w.n_max), None, V(w.poses(o)), C.byref(prm), V(o.new("entry", w.rows, 4)),
                                         V(o.new("status", w.rows, 4)), V(o.new("dist2", w.rows, 4)), V(o.new("pix2", w.rows, 4)),
                                         V(o.new("app_out", w.F * w.stride, 40)), V(o.new("stats", 1, 48))))


def _fuse_dry(w, m, o, n):
    prm = w.vo.MapFuseParams(FUSE["radius_xyz"], FUSE["radius"], 1, 1, 1)      # the midpoint, the veto of a shared frame, dry_run
    w._ok(w.lib.voe_map_fuse_batch_dev(m.h, C.c_int(w.F), V(w.d_app), C.c_size_t(w.stride), C.c_int(w.n_max), None, C.byref(prm),
                                       V(o.new("partner", n, 4)), V(o.new("dist2", n, 4)), V(o.new("gap2", n, 4)), V(o.new("verdict", n, 4)),
                                       V(o.new("remap", n, 4)), V(o.new("app_out", w.F * w.stride, 40)), V(o.new("stats", 1, 56))))


def _loops(w, m, o, n):
    p = dict(LOOPS, max_loops=min(LOOPS["max_loops"], w.F))
    L_ = p["max_loops"]
    prm = w.vo.MapLoopsParams(p["gap"], p["ref_window"], p["min_shared"], p["separation"], L_, 0,
                              w.vo.RansacParams(p["n_hypotheses"], p["threshold_px"], p["seed"]), p["kernel_threshold"], p["n_iters"], p["min_inliers"],
                              (C.c_float * 3)(*p["w_loop"]), 0)
    I, Z = C.c_int, C.c_size_t
    w._ok(w.lib.voe_map_loops_batch_dev(m.h, I(w.F), *map(I, MS.CAM), w.K.ctypes.data_as(C.c_void_p), V(w.d_uv), Z(w.stride), V(w.d_app), Z(w.stride),
                                        I(w.n_max), None, V(o.new("S", w.F, 64, w.T0)), C.byref(prm), V(o.new("edges", L_, 8)), V(o.new("Z", L_, 64)),
                                        V(o.new("weights", L_, 12)), V(o.new("records", L_, 40)), V(o.new("hist", w.F * w.F, 4)),
                                        V(o.new("ref_frame", n, 4)), V(o.new("stats", 1, 32))))


def _keyframes(w, m, o, n):
    p = KEYFRAMES
    w.covis(m, o, n, S.N_WORDS)                                   # the bit rows it reads: the call's own covisibility, on the device
    prm = w.vo.MapKeyframesParams(p["min_observers"], p["share_permille"], p["min_seen"], p["max_gap"], p["max_dropped"], (C.c_int32 * 3)(0, 0, 0))
    F = w.F
    w._ok(w.lib.voe_map_keyframes_dev(m.h, C.c_int(F), C.c_int(S.N_WORDS), V(o["bits"]), None, C.c_int(w.n_max), None, C.byref(prm),
                                      V(o.new("verdict", F, 4)), V(o.new("n_rows", F, 4)), V(o.new("keep", F, 1)), V(o.new("step", F, 4)),
                                      V(o.new("order", F, 4)), V(o.new("seen", F, 4)), V(o.new("red", F, 4)), V(o.new("kstats", 1, 32))))


def _apply_dry(w, m, o, n):
    """a dry run towards the frames' poses in reverse order: every seen entry would move, none does"""
    w._ok(w.lib.voe_map_apply_correction_batch_dev(m.h, C.c_int(w.F), None, C.c_size_t(w.stride), V(w.d_app), C.c_size_t(w.stride), C.c_int(w.n_max), None,
                                                   V(o.new("S_old", w.F, 64, w.T0)), V(o.new("S_new", w.F, 64, np.ascontiguousarray(w.T0[::-1]))), C.c_int(1),
                                                   V(o.new("ref_frame", n, 4)), V(o.new("stats", 1, 16))))


WIN_CALLS = {
    "lookup": (lambda w, m, o, n: w.lookup(m, o, n), False),
    "localise": (lambda w, m, o, n: w.localise(m, o, n), False),
    "refine_out_of_place": (lambda w, m, o, n: w.refine(m, o, n, S.REFINE, xyz=True), False),
    "refine": (lambda w, m, o, n: w.refine(m, o, n, S.REFINE), True),
    "refine_poses": (lambda w, m, o, n: w.refine_poses(m, o, n, S.POSES), False),
    "adjust": (lambda w, m, o, n: w.adjust(m, o, n, S.ADJUST), True),
    "bundle": (lambda w, m, o, n: w.bundle(m, o, n, S.BUNDLE), True),
    "cull_dry": (lambda w, m, o, n: w.cull(m, o, n, S.CULL, dry_run=True), False),
    "grow_dry": (lambda w, m, o, n: w._ok(w.grow(m, o, n, S.GROW, dry_run=True)), False),
    "covis_and_window": (lambda w, m, o, n: (w.covis(m, o, n, S.N_WORDS), w.window(m, o, S.N_WORDS, dict(S.WINDOW, query=1, k_free=2, k_fixed=1))), False),
    "nearest": (_nearest, False),
    "guided": (_guided, False),
    "fuse_dry": (_fuse_dry, False),
    "loops": (_loops, False),
    "keyframes": (_keyframes, False),
    "apply_correction_dry": (_apply_dry, False),
}


def _same_outs(a, b, what):
    assert a.keys() == b.keys(), (what, a.keys(), b.keys())
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f"{what}: '{k}' differs between the used map and the fresh twin"


def _same_content(st_a, st_b, ctx, what, words=1):
    a, b = MS.content(ctx, st_a.m, st_a.cap), MS.content(ctx, st_b.m, st_b.cap)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2][:words], b[2][:words]), (what, a[2], b[2])


def _stats_equal(cls, raw, ref):
    got = _struct(cls, raw)
    assert {k: got[k] for k in ref} == ref, (got, ref)


def _short_ints(vo, name, out, c):
    """the integer outputs of a short call against the restatement of the short window `c` (tests/map_state_cases.run and the
    families' own restatements); a call without a branch here is an error, not a pass"""
    F, n = len(c["frames"]), SHORT_ROWS
    pts, app = S.cut(c)
    apps = [a for _, a in c["frames"]]
    if name == "lookup":
        cnt, ent, pairs = i32(out["counts"]), i32(out["entries"]).reshape(F, n), i32(out["pairs"]).reshape(F, n, 2)
        for f, (e_ref, p_ref, x_ref) in enumerate(S.run("lookup", c)):
            assert cnt[f] == len(p_ref) and np.array_equal(ent[f], e_ref) and np.array_equal(pairs[f, : len(p_ref)], p_ref)
    elif name == "localise":
        for f, (e_ref, p_ref, _) in enumerate(S.run("lookup", c)):
            st = _struct(vo.MapLocaliseStats, out["stats"], f)
            assert st["n_rows"] == n and st["n_hits"] == len(p_ref) and st["status"] == 0, (f, st)
    elif name in ("refine", "refine_out_of_place"):
        ref = S.run("refine", c)
        assert np.array_equal(i32(out["status"]), ref["status"]) and _ints(_struct(vo.MapRefineStats, out["stats"])) == _ints(ref["stats"])
    elif name == "refine_poses":
        ref = S.run("poses", c)
        assert np.array_equal(i32(out["status"]), ref["status"]) and _ints(_struct(vo.MapPoseRefineStats, out["stats"])) == _ints(ref["stats"])
    elif name == "adjust":
        ref = S.run("adjust", c)
        assert np.array_equal(i32(out["pose_status"]), ref["pose_status"]) and np.array_equal(i32(out["point_status"]), ref["point_status"])
    elif name == "bundle":
        ref = S.run("bundle", c)
        assert np.array_equal(i32(out["pose_status"]), ref["pose_status"]) and np.array_equal(i32(out["point_status"]), ref["point_status"])
        assert _ints(_struct(vo.MapBundleStats, out["stats"])) == _ints(ref["stats"])
    elif name == "cull_dry":
        ref = S.run("cull", c)
        assert np.array_equal(i32(out["verdict"]), ref["verdict"]) and np.array_equal(i32(out["remap"]), ref["remap"])
        assert _struct(vo.MapCullStats, out["stats"]) == ref["stats"]
    elif name == "grow_dry":
        ref = S.run("grow", c)
        assert _struct(vo.MapGrowStats, out["stats"]) == dict(ref["stats"]) and np.array_equal(i32(out["rows"]).reshape(F, n), ref["rows"])
    elif name == "covis_and_window":
        ref = S.run("covis", c)
        assert np.array_equal(out["bits"].view(np.uint32).reshape(F, S.N_WORDS), ref["bits"]) and np.array_equal(i32(out["counts"]).reshape(F, F), ref["counts"])
    elif name == "nearest":
        ref = N.run(app, apps, None, n, NEAREST["radius"], NEAREST["ratio"], 0)
        assert np.array_equal(i32(out["entry"]).reshape(F, n), ref["entry"]) and np.array_equal(i32(out["status"]).reshape(F, n), ref["status"])
        assert out["dist2"].tobytes() == np.ascontiguousarray(ref["dist2"], np.float32).tobytes()
        _stats_equal(vo.MapNearestStats, out["stats"], ref["stats"])
    elif name == "guided":
        ref = G.run(pts, app, c["K"], c["frames"], c["poses"], None, n, GUIDED["radius_px"], GUIDED["radius"], GUIDED["ratio"], 0, MS.CAM[2], MS.CAM[3])
        assert np.array_equal(i32(out["entry"]).reshape(F, n), ref["entry"]) and np.array_equal(i32(out["status"]).reshape(F, n), ref["status"])
        _stats_equal(vo.MapGuidedStats, out["stats"], ref["stats"])
    elif name == "fuse_dry":
        ref = Fr.run(pts, app, apps, None, n, FUSE["radius_xyz"], FUSE["radius"], 1, 1, 1)
        for k in ("partner", "verdict", "remap"):
            assert np.array_equal(i32(out[k]), ref[k]), k
        _stats_equal(vo.MapFuseStats, out["stats"], ref["stats"])
        assert MS.untouched(out["app_out"])                        # a dry run rewrites no row
    elif name == "loops":
        p = dict(LOOPS, max_loops=min(LOOPS["max_loops"], F))
        ref = L.run(c["K"], MS.CAM, pts, app, c["frames"], np.asarray(c["poses"], np.float32), None, n, **p)
        assert np.array_equal(i32(out["ref_frame"]), ref["ref_frame"]) and np.array_equal(i32(out["hist"]).reshape(F, F), ref["hist"])
        assert np.array_equal(i32(out["edges"]).reshape(-1, 2), ref["edges"])
        _stats_equal(vo.MapLoopsStats, out["stats"], ref["stats"])
        rec = out["records"].view(vo.MAP_LOOP_RECORD_DTYPE)
        for l, s in enumerate(ref["slots"]):
            for k in ("i", "j", "c", "n_pairs", "ransac_status", "ransac_inliers", "status"):
                assert int(rec[l][k]) == int(s[k]), (l, k, int(rec[l][k]), int(s[k]))
    elif name == "keyframes":
        bits = S.run("covis", c)["bits"]
        ref = K.run(bits, None, n_rows=None, n_max=n, **KEYFRAMES)
        for k in K.KEYS:
            got = out[k] if k == "keep" else i32(out[k])
            assert np.array_equal(got, ref[k]), (k, got.tolist(), ref[k].tolist())
        _stats_equal(vo.MapKeyframesStats, out["kstats"], ref["stats"])
    elif name == "apply_correction_dry":
        key = np.full(len(pts), np.iinfo(np.int64).max, np.int64)
        for f, (e_ref, _, _) in enumerate(S.run("lookup", c)):
            hit = np.nonzero(e_ref >= 0)[0]
            np.minimum.at(key, e_ref[hit], f * n + hit)
        ref = np.where(key == np.iinfo(np.int64).max, -1, key // n).astype(np.int32)
        assert np.array_equal(i32(out["ref_frame"]), ref)
        moved = int(sum(1 for f in ref if f >= 0 and (F - 1 - f) != f))      # reversed poses: every frame but the middle one of an odd count
        assert i32(out["stats"]).tolist() == [len(pts), int((ref >= 0).sum()), moved, 0]
    else:
        raise KeyError(f"no restatement is compared for '{name}'")


class Reuse:
    """the used map and its fresh twin on the window of the state's case, and a small map of rows the two hold (the other side of
    the alignment and the merge that dirty align_ws, merge_ws, look_ws and the update's scratch on the used map)"""

    def __init__(self, vo, ctx):
        self.vo, self.ctx, self.c = vo, ctx, S.case(STATE)
        self.c_short = _short_case(self.c)
        pts, app = S.cut(self.c)
        self.used, self.twin = MS.build_exact(vo, ctx, pts, app), MS.build_exact(vo, ctx, pts, app)
        self.part = MS.build_exact(vo, ctx, pts[:120], app[:120])
        self.full = Win(vo, ctx, self.c)
        self.short = SubWin(self.full, F0, F1, SHORT_ROWS)
        self.outs = []

    def warm(self, names):
        """the named calls on the used map over the full window.  A call that moves the map (refine in place, adjust, bundle: they
        have no dry_run) is followed by its restoration: an update of the rows the map holds, which puts every point back, and a
        read of the size, which puts the host's bound back; the map is compared with the twin's before the call under test."""
        for name in names:
            o = Outs(self.ctx); self.outs.append(o)
            if name in WIN_CALLS:
                call, changes = WIN_CALLS[name]
                call(self.full, self.used.m, o, self.c["kept"])
                o.read()
                if changes:
                    _restore(self.used, self.c)
            elif name == "update_known":
                _restore(self.used, self.c)
            elif name == "align":
                MS.align(self.vo, self.ctx, self.used.m, self.part.m, o, self.part.m.size_bound(), S.ALIGN)
                o.read()
            elif name == "merge_known":                           # KEEP_DST of entries the map holds: nothing is appended, every byte stays
                MS.merge(self.vo, self.ctx, self.used.m, self.part.m, o, self.part.m.size_bound(), np.eye(4, dtype=np.float32), 1)
                assert i32(o.read()["mstats"]).tolist() == [120, 120, 0, self.c["kept"]]
                assert len(self.used.m) == self.c["kept"]          # (the host counted src's bound more: a read of the size takes it back)
                self.used.check_bound()
            else:
                raise KeyError(name)
        self.ctx.synchronize()
        _same_content(self.used, self.twin, self.ctx, "after the calls on the full window")

    def under_test(self, name):
        call = WIN_CALLS[name][0]
        res = []
        for s in (self.used, self.twin):
            o = Outs(self.ctx); self.outs.append(o)
            call(self.short, s.m, o, self.c["kept"])
            res.append(o.read())                                  # (asserts the 64 guard elements behind every array)
        _same_outs(res[0], res[1], name)
        _short_ints(self.vo, name, res[0], self.c_short)
        _same_content(self.used, self.twin, self.ctx, f"the map after {name}", words=1)

    def close(self):
        for o in self.outs:
            o.close()
        self.full.close(); self.used.close(); self.twin.close(); self.part.close()


EVERY_CALL = ["lookup", "localise", "refine_out_of_place", "refine_poses", "adjust", "bundle", "cull_dry", "grow_dry", "covis_and_window", "refine",
              "nearest", "guided", "fuse_dry", "loops", "keyframes", "apply_correction_dry", "align", "merge_known", "update_known"]


@pytest.mark.parametrize("name", list(WIN_CALLS))
def test_a_short_call_on_a_map_that_ran_every_call_on_the_full_window(vo, ctx, name):
    r = Reuse(vo, ctx)
    try:
        r.warm(EVERY_CALL)
        r.under_test(name)
    finally:
        r.close()


# the pairs that share a buffer: ref_ws (the observation lists of refine / bundle / cull / grow / fuse), cull_ws (the cull's and the
# fuse's compaction), the map's scratch (update and grow), look_ws (every lookup)
NEIGHBOURS = [(["fuse_dry"], "cull_dry"), (["cull_dry"], "fuse_dry"), (["grow_dry"], "refine"), (["refine_out_of_place"], "bundle"),
              (["bundle"], "cull_dry"), (["update_known"], "grow_dry"), (["lookup"], "localise_one")]


@pytest.mark.parametrize("before,name", NEIGHBOURS, ids=[f"{b[0]}-then-{n}" for b, n in NEIGHBOURS])
def test_a_short_call_behind_the_neighbour_that_shares_its_buffer(vo, ctx, before, name):
    r = Reuse(vo, ctx)
    try:
        r.warm(before)
        if name == "localise_one":                                # the lookup of 7 frames, then the localisation of one
            r.short = SubWin(r.full, F0, F0 + 1, SHORT_ROWS)
            r.c_short = _short_case(r.c, F0, F0 + 1)
            name = "localise"
        r.under_test(name)
    finally:
        r.close()


# ---- (d) the context's workspaces -------------------------------------------------------------------------------------------------
# The session context under the three bytes: scratch, best, table and the sorted searches' workspace (matcher, join, triangulation),
# epi_ws / ransac_ws / refine_ws / pose_ws / pose_batch_ws, pose_graph_ws, and the batched frames' buffers.  The oracles and the
# comparisons are the ones the operators' own tests use.

_ctx_cache = {}


@byte_ids
@pytest.mark.parametrize("n", [1, 65, 257, 1025])
def test_matcher_join_and_triangulation(vo, ctx, o32, n, byte):
    """every search form of the matcher in both argument orders, the join and the triangulation on its output: bit for bit"""
    if n not in _ctx_cache:
        fp = TS._frame(vo, n, 7000 + n)
        m = o32.match(fp["ref_app"], fp["cur_app"])
        _ctx_cache[n] = (fp, m, o32.match(fp["cur_app"], fp["ref_app"]), o32.join(m, fp["model_pairs"]),
                         o32.triangulate(fp["K"], fp["X_gt"], m, fp["ref_pts"], fp["cur_pts"], fp["cur_app"]))
    fp, exp_m, exp_rev, exp_j, (e_xyz, e_pairs, e_app) = _ctx_cache[n]
    with poison(byte):
        try:
            for mode in (1, 2, 3, 0):
                assert ctx.lib.vo_match_set_mode(ctx.h, mode) == 0
                m = vo.compute_correspondences_images(fp["ref_app"], fp["cur_app"], ctx=ctx)
                assert np.array_equal(m, exp_m), mode
                assert np.array_equal(vo.compute_correspondences_images(fp["cur_app"], fp["ref_app"], ctx=ctx), exp_rev), mode
        finally:
            assert ctx.lib.vo_match_set_mode(ctx.h, 0) == 0
        assert np.array_equal(vo.extract_correspondences_world(m, fp["model_pairs"], ctx=ctx), exp_j)
        xyz, pairs, app = vo.triangulate_points(fp["K"], fp["X_gt"], m, fp["ref_pts"], fp["cur_pts"], fp["cur_app"], ctx=ctx)
        assert np.array_equal(pairs, e_pairs) and np.array_equal(app, e_app) and np.array_equal(xyz, e_xyz)


def _small_epi(vo):
    if "epi" not in _ctx_cache:
        fp = vo.synth.frame_pair(2000, seed=4200, noise_px=0.25)
        _ctx_cache["epi"] = (fp, Rr.corrupt(fp["gt_matches"], len(fp["cur_pts"]), 0.3, seed=4)[0])
    return _ctx_cache["epi"]


@byte_ids
@pytest.mark.parametrize("n", TES.SIZES[:2])
def test_estimate_transform(vo, ctx, o32, n, byte):
    """vo_estimate_transform and its device form at the two smallest sizes of tests/test_gpu_epi_sizes.py, within its tolerance of
    the float64 restatement, host form and device form bit for bit"""
    if ("images", n) not in _ctx_cache:
        fp = vo.synth.frame_pair(2000, seed=4100)
        p1 = np.concatenate([fp["ref_pts"], [[np.nan, np.nan], [-5, -7], [1280, 3], [2, 960]]]).astype(np.float32)
        p2 = np.concatenate([fp["cur_pts"], [[np.nan, 4], [-9, np.nan], [1280.5, 1], [3, 961]]]).astype(np.float32)
        pr = TES._pairs(fp, n)
        _ctx_cache[("images", n)] = (fp, p1, p2, pr, TES.R.estimate_transform(o32, fp["K"], pr, p1, p2))
    fp, p1, p2, pr, X_ref = _ctx_cache[("images", n)]
    with poison(byte):
        X = vo.estimate_transform(fp["K"], pr, p1, p2, ctx=ctx)
        assert np.abs(X - X_ref).max() < TES.TOL, np.abs(X - X_ref).max()
        rc, X_dev = TES._transform_dev(ctx, fp["K"], pr, n, p1, p2)
        assert rc == 0 and X_dev.tobytes() == X.tobytes()


@byte_ids
@pytest.mark.parametrize("n_hyp,n,n_max", TRS.EPI_CASES[:2])
def test_estimate_transform_ransac(vo, ctx, n_hyp, n, n_max, byte):
    fp, pairs = _small_epi(vo)
    with poison(byte):
        TRS._epi_check(vo, ctx, fp, pairs, n_hyp, n, n_max, seed=n_hyp + n)


@byte_ids
@pytest.mark.parametrize("n_hyp,n,n_max", TRS.POSE_CASES[:2])
def test_estimate_pose_ransac(vo, ctx, n_hyp, n, n_max, byte):
    if "pose" not in _ctx_cache:
        fp, world, meas, pairs, bad, clean = TRS.P.tracking_problem(vo, 2000, seed=4300, noise_px=0.5, frac=0.3, max_angle=0.3, max_t=0.5)
        _ctx_cache["pose"] = (fp, np.asarray(world, np.float32), np.asarray(meas, np.float32), pairs)
    fp, world, meas, pairs = _ctx_cache["pose"]
    with poison(byte):
        TRS._pose_check(vo, ctx, fp["K"], world, meas, pairs, n_hyp, n, n_max, seed=n_hyp + n)


@byte_ids
@pytest.mark.parametrize("case", ["true pairs", "30% mismatched, huber 1 px"])
def test_refine_transform(vo, ctx, noisy, case, byte):  # noqa: F811
    with poison(byte):
        TER.test_parity_with_the_restatement(vo, ctx, noisy, case)


@byte_ids
def test_estimate_pose_ransac_batch(vo, ctx, byte):
    """the batched call on problems of 0, 3, 4, 5 and 257 pairs at 1 and 65 hypotheses: every problem the bytes of its single call
    (made without the hook, once)"""
    live, hyps = (0, 3, 4, 5, 257), (1, 65)
    if "batch" not in _ctx_cache:
        probs = [TPB._sized(vo, n, 3100 + i) for i, n in enumerate(live)]
        K = probs[0][0]
        probs = [p for _, p in probs]
        with poison(None):
            _ctx_cache["batch"] = (K, probs, [single_results(vo, ctx, K, p, TPB.STRIDE, hyps) for p in probs])
    K, probs, singles = _ctx_cache["batch"]
    with poison(byte):
        b = BatchDev(vo, ctx, K, probs, pairs_stride=TPB.STRIDE)
        try:
            for H in hyps:
                assert b.call(n_hyp=H) == 0, ctx.lib.vo_last_error()
                r = b.results(H)
                for p in range(len(probs)):
                    assert same_problem(b.problem(r, p), singles[p][H]), (H, live[p])
                assert r["st"][0] == 1 and r["st"][1] == 1 and r["nin"][0] == 0 and r["nin"][1] == 3
        finally:
            b.close()


@byte_ids
@pytest.mark.parametrize("name", ["n3", "n257", "hub17", "held_middle_257"])
def test_pose_graph(vo, ctx, name, byte):
    """pose_graph_cases.compare against the float64 restatement, and every output the bytes of the unpoisoned call"""
    case = PGc.CASES[name]

    def run(b):
        d = TPG.Dev(vo, ctx, case)
        try:
            with poison(b):
                d.reset()
                assert d.call() == 0, ctx.lib.vo_last_error()
                return d.results(), d.F
        finally:
            d.close()
    if ("pg", name) not in _ctx_cache:
        _ctx_cache[("pg", name)] = run(None)[0]
    res, F = run(byte)
    d = TPG.Dev(vo, ctx, case)
    try:
        got = d.got(res)
    finally:
        d.close()
    log = []
    bad = PGc.compare(name, got, reach_of=np.full(F, TPG.BUDGET[name]["reach_max"]), log=log)
    assert bad == [], (bad, log)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res, _ctx_cache[("pg", name)])), f"{name}: not the bytes of the unpoisoned call"


@byte_ids
@pytest.mark.parametrize("n,F", [(700, 7), (700, 8)])
def test_batched_frames(vo, ctx, o32, n, F, byte):
    """vo_frames_batch_dev on either side of its grid's switch-over, as test_batched_frames_at_frame_count_edges compares it"""
    if ("frames", n, F) not in _ctx_cache:
        fps, want = [], []
        for i in range(F):
            f = vo.synth.frame_pair(n, seed=7600 + 33 * i + n, distractors=13)
            keep = np.random.default_rng(100 + i).permutation(n)[: n - n // 8]
            f["model_pairs"] = np.ascontiguousarray(f["model_pairs"][np.sort(keep)])
            fps.append(f)
            m_o = o32.match(f["ref_app"], f["cur_app"]); j_o = o32.join(m_o, f["model_pairs"])
            r = o32.picp_solve(OCam(480, 640, 0, 10, f["K"], np.eye(4)), f["model"], f["cur_pts"], j_o, 7, 10000.0, False, trace=False)
            want.append((m_o, j_o, r["T"], r["num_inliers"]))
        _ctx_cache[("frames", n, F)] = (fps, want)
    fps, want = _ctx_cache[("frames", n, F)]
    with poison(byte):
        bp = vo.BatchPipeline(ctx, fps, n_iters=7, kernel_threshold=10000.0)
        try:
            bp.run()
            poses, stats, counts = bp.poses(), bp.stats(), bp.counts()
            for i, (f, (m_o, j_o, T, n_in)) in enumerate(zip(fps, want)):
                assert np.array_equal(bp.fetch("match", i), m_o) and np.array_equal(bp.fetch("join", i), j_o), i
                assert counts[0, i] == len(m_o) and counts[1, i] == len(j_o)
                assert np.abs(poses[i] - T).max() < 1e-4 and int(stats[i, 2]) == n_in, i
                xo, po, ao = o32.triangulate(f["K"], poses[i], m_o, f["ref_pts"], f["cur_pts"], f["cur_app"])
                assert np.array_equal(bp.fetch("tri_pairs", i), po) and np.array_equal(bp.fetch("tri_app", i), ao), i
                assert np.array_equal(bp.fetch("tri_xyz", i), xo), i
        finally:
            bp.close()
