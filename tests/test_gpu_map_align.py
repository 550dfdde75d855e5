"""voe_map_align[_dev] and voe_map_merge[_dev] on the GPU: every case of tests/map_align_cases.py against the float64
restatement (tests/map_align_restatement.py), equal bytes (three calls, the host form, with and without the optional outputs,
capture and replay), the refusals, and the merge of both policies against the explicit vo_map_update.

Against float64: pairs, n_matches, status, best_hypothesis, best_count, n_valid, refit_kept, the mask and n_inliers are equal
exactly -- tests/test_map_align_cpu.py asserts on the same cases that no pair lies in the band of a model that decides --; a
hypothesis count is equal where its band is empty and within the band's population elsewhere; S, scale and rms lie within
4 x the recorded spread + 2 x the a-priori bound of profiles/map_align_budget.json (S: one float32 ulp more)."""
import ctypes as C

import numpy as np
import pytest

import map_align_cases as Cc
import map_align_restatement as A
from map_align_dev import AlignDev

pytestmark = pytest.mark.gpu


def _check_against_reference(name, got, ref):
    assert got["n_matches"] == ref["n_matches"] and np.array_equal(got["pairs"], ref["pairs"])
    st = got["stats"]
    for k in ("status", "n_matches", "n_inliers", "best_hypothesis", "best_count", "n_valid", "refit_kept"):
        assert st[k] == ref["stats"][k], (k, st, ref["stats"])
    n = ref["n_matches"]
    assert np.array_equal(got["mask"][:n].astype(bool), ref["mask"]) and not got["mask"][n:].any()
    exact = ref["band_pop"] == 0
    assert np.array_equal(got["counts"][exact], ref["counts"][exact])
    assert (np.abs(got["counts"][~exact] - ref["counts"][~exact]) <= ref["band_pop"][~exact]).all()
    assert (got["S"][3] == [0, 0, 0, 1]).all()
    if ref["status"] != A.OK:
        assert got["S"].tobytes() == np.eye(4, dtype=np.float32).tobytes() and st["scale"] == 1.0 and st["rms"] == 0.0 and st["n_inliers"] == 0
        return
    ceil = Cc.ceilings(Cc.load_budget()[name])
    dS = np.abs(got["S"].astype(np.float64) - ref["S"].astype(np.float64))
    lim = ceil["S"] + np.spacing(np.abs(ref["S"])).astype(np.float64)
    print(f"{name}: S off by {dS.max():.3g} (ceiling {ceil['S']:.3g} + an ulp), scale by {abs(st['scale'] - ref['scale']):.3g} ({ceil['scale']:.3g}), "
          f"rms by {abs(st['rms'] - ref['rms']):.3g} ({ceil['rms']:.3g}); rms {st['rms']:.6g}, scale {st['scale']:.12g}")
    assert (dS <= lim).all()
    assert abs(st["scale"] - ref["scale"]) <= ceil["scale"] and abs(st["rms"] - ref["rms"]) <= ceil["rms"]


@pytest.mark.parametrize("name", list(Cc.CASES))
def test_case_against_the_restatement(vo, ctx, name):
    c, ref = Cc.case(name), Cc.reference(name)
    d = AlignDev(vo, ctx, c)
    try:
        before = [d.state(d.dst), d.state(d.src)]
        look = [d.lookups(d.dst, c["src_app"]), d.lookups(d.src, c["dst_app"])]
        d.clear_out()
        assert d.align() == 0, ctx.lib.vo_last_error()
        got = d.results()
        _check_against_reference(name, got, ref)
        # both maps keep every byte and every lookup
        after = [d.state(d.dst), d.state(d.src)]
        assert all(x.tobytes() == y.tobytes() for a, b in zip(before, after) for x, y in zip(a, b))
        assert np.array_equal(look[0], d.lookups(d.dst, c["src_app"])) and np.array_equal(look[1], d.lookups(d.src, c["dst_app"]))
        assert np.array_equal(got["pairs"][:, 1], look[0][got["pairs"][:, 0]])      # the pairs ARE the public lookup's
    finally:
        d.close()


@pytest.mark.parametrize("name", ["example", "nan", "collinear", "refit_rejected", "two"])
def test_same_bytes_from_every_form(vo, ctx, name):
    lib = ctx.lib
    c = Cc.case(name)
    d = AlignDev(vo, ctx, c)
    try:
        d.clear_out()
        assert d.align() == 0
        first = d.results()
        for _ in range(2):
            d.clear_out()
            assert d.align() == 0
            assert d.same_bytes(d.results(), first)
        d.clear_out()
        assert d.align(optional=False) == 0
        bare = d.results()
        assert d.same_bytes(bare, first, optional=False) and (bare["mask"] == 7).all() and (bare["counts"] == -7).all()
        # the host form
        p = c["params"]
        h = d.dst.align(d.src, p["threshold"], p["n_hypotheses"], p["seed"], p["with_scale"], p["n_refits"], p["min_inliers"], want_counts=True)
        assert h["S"].tobytes() == first["S"].tobytes() and h["pairs"].tobytes() == first["pairs"].tobytes()
        assert np.array_equal(h["mask"], first["mask"][: first["n_matches"]].astype(bool)) and np.array_equal(h["counts"], first["counts"])
        assert h["stats"] == first["stats"]
        # capture and replay
        g = C.c_void_p()
        d.clear_out()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.align()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        for _ in range(2):
            d.clear_out()
            assert lib.vo_graph_launch(g) == 0
            assert d.same_bytes(d.results(), first)
        assert lib.vo_graph_destroy(g) == 0
    finally:
        d.close()


def test_a_capture_that_would_grow_a_workspace_is_refused(vo, ctx):
    lib = ctx.lib
    d = AlignDev(vo, ctx, Cc.case("matches_257"))             # fresh maps: no call has sized dst's workspaces
    try:
        g = C.c_void_p()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc, msg = d.align(), lib.vo_last_error()
        rc2 = d.merge(None, A.KEEP_DST)
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
        if g.value:
            assert lib.vo_graph_destroy(g) == 0
        assert rc == -6 and b"capture" in msg and rc2 == -6
    finally:
        d.close()


def test_refusals(vo, ctx):
    lib = ctx.lib
    d = AlignDev(vo, ctx, Cc.case("matches_4"))
    other = vo.Context(0)
    foreign = vo.Map(other)
    try:
        bad = lambda rc: rc == -1
        assert bad(d.align(src=d.dst.h)) and b"one map" in lib.vo_last_error()
        assert bad(d.align(src=foreign.h)) and b"different contexts" in lib.vo_last_error()
        assert bad(d.align(dst=None)) and bad(d.align(src=None)) and bad(d.align(prm=None))
        for kw in (dict(n_hypotheses=0), dict(n_hypotheses=65537), dict(n_refits=-1), dict(n_refits=A.MAX_REFITS + 1), dict(min_inliers=-1),
                   dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
                   dict(d_S=None), dict(d_pairs=None), dict(d_nm=None), dict(d_stats=None), dict(d_pairs=d.d_pairs + 4), dict(d_stats=d.d_stats + 4)):
            assert bad(d.align(**kw)), kw
        assert bad(d.merge(None, A.TAKE_SRC, src=d.dst.h)) and bad(d.merge(None, A.TAKE_SRC, src=foreign.h)) and bad(d.merge(None, 2))
        assert bad(d.merge(None, A.KEEP_DST, d_stats=None)) and bad(d.merge(None, A.KEEP_DST, dst=None))
        assert d.align(n_hypotheses=64, n_refits=A.MAX_REFITS) == 0      # the largest refit count runs
        d.results()
    finally:
        foreign.close(); other.close(); d.close()


# ---- merge ----
def _dev_ptrs(lib, m):
    x, a, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.vo_map_dev_ptrs(m.h, C.byref(x), C.byref(a), C.byref(n)) == 0
    return x.value, a.value, n.value


@pytest.mark.parametrize("name", list(Cc.MERGE_CASES) + ["example", "nan", "disjoint"])
@pytest.mark.parametrize("policy", [A.TAKE_SRC, A.KEEP_DST])
def test_merge_against_the_explicit_update(vo, ctx, name, policy):
    lib = ctx.lib
    c, r = Cc.case(name), Cc.reference(name)
    S = r["S"] if r["status"] == A.OK else None
    ref = A.merge(c, S, policy)
    d = AlignDev(vo, ctx, c)
    twin = vo.Map(ctx)
    try:
        twin.update(c["dst_pts"], c["dst_app"])
        src_before = d.state(d.src)
        d.clear_out()
        assert d.merge(S, policy) == 0, lib.vo_last_error()
        got = d.merge_results()
        pts, app = d.state(d.dst)
        assert got["stats"] == ref["stats"], (got["stats"], ref["stats"])
        # the explicit update on a twin of dst: all of src's rows (TAKE_SRC), or the misses in src order (KEEP_DST)
        x, a, n = _dev_ptrs(lib, d.src)
        if policy == A.TAKE_SRC:
            twin.update_dev(x, a, d.n_max, n, d.d_S_in if S is not None else None)
        else:
            rows = ref["rows"]
            assert np.array_equal(rows, np.nonzero(d.lookups(twin, c["src_app"]) < 0)[0])
            if len(rows):
                twin.update(c["src_pts"][rows], c["src_app"][rows], S)
            assert pts[: len(c["dst_pts"])].tobytes() == c["dst_pts"].tobytes() and app[: len(c["dst_app"])].tobytes() == c["dst_app"].tobytes()
            assert app[len(c["dst_app"]):].tobytes() == c["src_app"][rows].tobytes()
        tp, ta = twin.read()
        assert pts.tobytes() == tp.tobytes() and app.tobytes() == ta.tobytes() and len(d.dst) == len(twin)
        assert np.array_equal(pts, ref["pts"], equal_nan=True) and app.tobytes() == ref["app"].tobytes()      # and the restatement's map
        # the remap is a lookup afterwards, on either map; src keeps every byte
        assert np.array_equal(got["remap"], d.lookups(d.dst, c["src_app"])) and np.array_equal(got["remap"], d.lookups(twin, c["src_app"]))
        assert np.array_equal(got["remap"], ref["remap"])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(src_before, d.state(d.src)))
        # the host form on fresh maps: the same map, remap and statistics
        d.reset()
        remap, st = d.dst.merge(d.src, S, policy)
        hp, ha = d.state(d.dst)
        assert np.array_equal(remap, got["remap"]) and st == got["stats"] and hp.tobytes() == pts.tobytes() and ha.tobytes() == app.tobytes()
    finally:
        twin.close(); d.close()


def test_merge_capture_and_replay(vo, ctx):
    lib = ctx.lib
    c, r = Cc.case("miss_257"), Cc.reference("miss_257")
    d = AlignDev(vo, ctx, c, dst_capacity=4096)
    try:
        d.clear_out()
        assert d.merge(r["S"], A.KEEP_DST) == 0
        eager, eager_map = d.merge_results(), d.state(d.dst)
        d.reset()
        g = C.c_void_p()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.merge(r["S"], A.KEEP_DST, upload=False)
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        d.clear_out()
        assert lib.vo_graph_launch(g) == 0
        got = d.merge_results()
        assert got["stats"] == eager["stats"] and np.array_equal(got["remap"], eager["remap"])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(d.state(d.dst), eager_map))
        # replayed on the merged map: every src entry is found now, nothing is appended
        assert lib.vo_graph_launch(g) == 0
        again = d.merge_results()
        assert again["stats"] == dict(n_src=557, n_shared=557, n_appended=0, n_dst_after=560) and np.array_equal(again["remap"], eager["remap"])
        assert lib.vo_graph_destroy(g) == 0
    finally:
        d.close()


def test_align_then_merge_puts_src_onto_dst(vo, ctx):
    """example: the aligned and merged map holds src's clean landmarks within float32 rounding of dst's own"""
    c = Cc.case("example")
    d = AlignDev(vo, ctx, c)
    try:
        al = d.dst.align(d.src, 0.05, 64, 1)
        assert al["stats"]["status"] == 0 and al["stats"]["n_inliers"] == 910
        remap, st = d.dst.merge(d.src, al["S"], vo.MAP_MERGE_TAKE_SRC)
        assert st == dict(n_src=950, n_shared=950, n_appended=0, n_dst_after=1000)
        pts, _ = d.dst.read()
        clean = np.setdiff1d(np.arange(950), c["pushed_src"])
        off = np.abs(pts[remap[clean]].astype(np.float64) - c["dst_pts"][remap[clean]]).max()
        print(f"largest move of a clean landmark: {off:.3g}")
        assert off < 5e-6                                      # float32 rounding of coordinates up to 10, twice
    finally:
        d.close()


# ---- composition: align, merge, similarity_pose, then a cull over src's frames on the merged map ----
def test_cull_over_moved_poses_on_the_merged_map_judges_as_on_src_alone(vo, ctx):
    """src's frames see src's landmarks under the poses T (p_cam = T p_src).  After dst.merge(src, S) the same frames, under
    similarity_pose(T, S), see the moved landmarks at T' S p = c T p in exact arithmetic for ANY similarity S: every projection
    is the same, so a dry-run cull gives every src landmark the verdict it has on src alone.  Both culls run on the device in
    double from float32 inputs; what differs are the inputs' float32 roundings.  With u = 2^-24 and m = sqrt(3) max|p'| + max|t'|
    (a bound of every partial result of T' p'): the moved point p' = fl(t + M p) carries 4 u m (three products and sums, dot3's
    order), T' rounded to float32 adds u sqrt(3) max|p'| + u max|t'| <= u m, and S's 3x3 block rounded to float32 is a rotation
    times c only to 4 u per entry (each entry within u, R^T R - I within 4 u to first order), which moves T' M p by
    4 sqrt(3) u c |p| <= 7 u m.  Together D = 12 u m in camera coordinates.  A pixel is f X / Z + c0 with |X / Z| <= 1.5 inside
    this camera's image (half its width over f), so it moves by at most f / Z (1 + 1.5) D, Z >= c min_z of the landmark on src
    alone; and mean_sq_px = mean |e|^2 moves by at most 2 sqrt(max_sq_px) dpx sqrt(2) + 2 dpx^2.  The cull's own budget
    (profiles/map_cull_budget.json) covers another ORDER of its double sums, which is the same here -- same lists, same lanes --
    so its term is the double rounding of the sum alone, n_obs 2^-53 max_sq_px."""
    import map_refine_restatement as R
    P = R.example_problem()
    c = Cc.case("example")
    cs, Rm, t = c["truth"]
    S_true = np.eye(4); S_true[:3, :3] = cs * Rm; S_true[:3, 3] = t
    T_src = [A.similarity_pose(T, np.linalg.inv(S_true)).astype(np.float32) for T in P["poses"]]      # the frames' poses in src
    cam = vo.Camera(*P["cam"], P["K"], np.eye(4), ctx=ctx)
    d = AlignDev(vo, ctx, c)
    try:
        kw = dict(min_obs=3, min_frames=2, max_rms_px=1.0, dry_run=True)
        alone = d.src.cull(cam, P["frames"], T_src, **kw)
        al = d.dst.align(d.src, 0.05, 64, 1)
        assert al["stats"]["status"] == 0
        remap, st = d.dst.merge(d.src, al["S"], vo.MAP_MERGE_TAKE_SRC)
        assert (remap >= 0).all() and st["n_appended"] == 0
        T_new = [vo.similarity_pose(T, al["S"]).astype(np.float32) for T in T_src]
        merged = d.dst.cull(cam, P["frames"], T_new, **kw)
        assert np.array_equal(merged["verdict"][remap], alone["verdict"])
        ea, em = alone["entries"], merged["entries"][remap]
        assert np.array_equal(ea["n_obs"], em["n_obs"]) and np.array_equal(ea["n_frames"], em["n_frames"])
        pushed = c["pushed_src"]
        seen3 = ea["n_obs"] >= 3
        assert (alone["verdict"][pushed][seen3[pushed]] == 6).all() and int((alone["verdict"] == 6).sum()) == int(seen3[pushed].sum())      # HIGH_ERROR
        u = 2.0 ** -24
        pts, _ = d.dst.read()
        m = np.sqrt(3) * np.abs(pts).max() + max(np.abs(T[:3, 3]).max() for T in T_new)
        f = max(P["K"][0][0], P["K"][1][1])
        ok = ea["n_obs"] > 0
        dpx = 2.5 * f / (al["stats"]["scale"] * ea["min_z"][ok]) * 12 * u * m
        tol = 2 * np.sqrt(2 * ea["max_sq_px"][ok]) * dpx + 2 * dpx ** 2 + ea["n_obs"][ok] * 2.0 ** -53 * ea["max_sq_px"][ok]
        diff = np.abs(em["mean_sq_px"][ok] - ea["mean_sq_px"][ok])
        print(f"{int(ok.sum())} landmarks seen: mean_sq_px differs by at most {diff.max():.3g}, largest fraction of its tolerance {(diff / tol).max():.3g}")
        assert (ea["min_z"][ok] > 0).all() and (diff <= tol).all()
    finally:
        d.close()


# ---- end to end: vo_complete's map against the world, a known answer by derivation ----
def test_align_map_on_vo_complete_beats_evaluates_pure_scaling(tmp_path):
    """With a threshold so large that every match is an inlier and one refit, the refit is the least-squares optimum over ALL
    similarities of sum |S a - b|^2 over the matches; evaluate's map correction, a pure scaling by median_ratio_inv, is one of
    them.  So rms <= rmse_map but for float32 rounding, with u = 2^-24: S rounded to float32 moves a residual coordinate by at
    most u m_a, m_a = max_i sum_j |M_ij a_j| + |t_i| (each of the 12 numbers within u of itself), i.e. rms by sqrt(3) u m_a;
    evaluate forms e = fl(fl(x r) - w) in float32, within u (2 |x r| + |w|) <= 3 u m_w of exact, and rounds its result once:
    rmse_map(exact) <= rmse_map (1 + u) + 3 sqrt(3) u m_w; its printed 9 digits add 1e-8 relative."""
    import os
    import re
    import subprocess
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    BIN, DATA = os.path.join(ROOT, "apps", "bin"), os.path.join(ROOT, "tests", "golden", "example_data", "data")
    assert os.path.exists(os.path.join(BIN, "align_map")), "apps/bin/align_map is missing: build() makes it"
    out = str(tmp_path)
    r = subprocess.run([os.path.join(BIN, "vo_complete"), DATA, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    a = subprocess.run([os.path.join(BIN, "align_map"), DATA, out, "--threshold=1000", "--refits=1", "--hypotheses=64"], capture_output=True,
                       text=True, timeout=120)
    print(a.stdout)
    assert a.returncode == 0, a.stdout + a.stderr
    g = lambda pat: [float(x) for x in re.search(pat, a.stdout).groups()]
    n_matches, n_inliers = g(r"status OK: (\d+) matches, (\d+) inliers")
    scale, rms = g(r"scale ([-0-9.e+]+), rms ([-0-9.e+]+)")
    ratio, rmse_map, n_eval = g(r"median_ratio_inv ([-0-9.e+]+), rmse_map ([-0-9.e+]+) over (\d+) points")
    assert n_matches == n_inliers == n_eval > 100 and "refit kept" in a.stdout
    S = np.array([[float(x) for x in row.split()] for row in re.search(r"S =\n((?:\s+[-0-9.e+ ]+\n){4})", a.stdout).group(1).strip().split("\n")])
    est = np.loadtxt(os.path.join(out, "map.txt")).reshape(-1, 3)
    world = np.loadtxt(os.path.join(DATA, "world.dat"))[:, 1:4]
    u = 2.0 ** -24
    m_a = (np.abs(S[:3, :3]) @ np.abs(est).T).max() + np.abs(S[:3, 3]).max()
    m_w = np.abs(est).max() * ratio + np.abs(world).max()
    bound = rmse_map * (1 + u + 1e-8) + 3 * np.sqrt(3) * u * m_w + np.sqrt(3) * u * m_a
    print(f"rms of the similarity {rms:.9g} <= rmse_map of the pure scaling {rmse_map:.9g} (+ {bound - rmse_map:.3g}); scale {scale:.9g} beside "
          f"median_ratio_inv {ratio:.9g}")
    assert rms <= bound
    # --merge: the estimate's landmarks are all the world's, nothing is appended
    b = subprocess.run([os.path.join(BIN, "align_map"), DATA, out, "--merge"], capture_output=True, text=True, timeout=120)
    print(b.stdout[-400:])
    assert b.returncode == 0 and re.search(r"merged: (\d+) of the estimate's (\d+) landmarks were in the world already, 0 appended", b.stdout)
    # a threshold nothing meets: FEW_INLIERS is a status, the exit code 1
    e = subprocess.run([os.path.join(BIN, "align_map"), DATA, out, "--threshold=1e-12", "--refits=0"], capture_output=True, text=True, timeout=120)
    assert e.returncode == 1 and "status FEW_INLIERS" in e.stdout, e.stdout
