"""The cases of tests/map_state_cases.py under the float64 restatements alone: the conditions that keep
tests/test_gpu_map_states.py from passing vacuously.  They are conditions on the cases, not measurements of any device: a case
that stopped meeting them would leave the GPU test comparing a faulty path with a correct one on entries neither touches.

  - at least 20 entries at or above the edge (the smaller bound a faulty path would use) end OK / KEPT with at least min_obs
    observations, and at least 20 below it; the same for the free points of the bundle;
  - every frame has live rows that hit entries on both sides of the edge;
  - the cull drops at least 10 entries on each side and keeps at least 10;
  - the grow ADDS at least 30 tracks, and under `overflowed` at least 10 open rows belong to dropped classes;
  - under `overflowed` the calls on the 1024 rows kept can be told from the calls on all 1200 rows;
  - no restatement takes a marginal decision, so every integer the GPU test compares is a function of the case.

The slack states hold 300 entries and their edge is 300: there the first condition is asked of the whole map.  The capture in
front of an update (the last test of tests/test_gpu_map_states.py) replays on the first 300, 600 and 900 rows of the `replayed` case: its edges are 300 and 600.
No output of any call turned out to differ in its bytes between a state's map and its twin, so there is no
float64 ceiling to re-measure here and no profiles/map_states_budget.json."""
import numpy as np
import pytest

import map_bundle_restatement as B
import map_cull_restatement as Q
import map_grow_restatement as Gr
import map_refine_restatement as R
import map_state_cases as S

BEYOND = [(s, S.SHAPE[s][1], S.SHAPE[s][2]) for s in ("replayed", "overflowed")] + [("replayed", 900, 300), ("replayed", 600, 300)]


def _sides(mask, edge):
    return int(np.asarray(mask)[:edge].sum()), int(np.asarray(mask)[edge:].sum())


@pytest.mark.parametrize("state", S.STATES)
def test_the_case_is_what_the_builders_want(state):
    c = S.case(state)
    rows, kept, edge = S.SHAPE[state]
    assert len(c["map_pts"]) == len(c["map_app"]) == rows and c["kept"] == kept and c["edge"] == edge
    assert not np.isnan(c["map_app"]).any() and len({r.tobytes() for r in c["map_app"]}) == rows
    assert 6 <= len(c["frames"]) <= 8 and all(len(a) == S.ROWS <= 320 for _, a in c["frames"])
    assert max(S.REFINE["n_rounds"], S.POSES["n_rounds"], S.BUNDLE["n_rounds"], S.GROW["n_rounds"]) <= 3


@pytest.mark.parametrize("state", ("slack_1", "slack_300"))
def test_slack_states_have_work_in_every_call(state):
    r, q, b, g = (S.reference(state, k) for k in ("refine", "cull", "bundle", "grow"))
    assert ((r["status"] == R.OK) & (r["n_obs"] >= S.REFINE["min_obs"])).sum() >= 20 and not r["marginal"].any()
    assert (q["verdict"] == Q.KEPT).sum() >= 20 and (~q["keep"]).sum() >= 10 and not q["marginal"].any()
    assert (b["point_status"] == 0).sum() >= 20 and b["status"] == B.OK and not b["marginal"]
    assert g["stats"]["n_added"] >= 30 and not g["marginal"].any()
    p = S.reference(state, "poses")
    assert (p["status"][1:] == 0).all() and not p["marginal"].any()


@pytest.mark.parametrize("state,n,edge", BEYOND)
def test_entries_on_both_sides_of_the_edge_decide(state, n, edge):
    c = S.case(state)
    r = S.reference(state, "refine", n)
    ok = (r["status"] == R.OK) & (r["n_obs"] >= S.REFINE["min_obs"])
    assert min(_sides(ok, edge)) >= 20, _sides(ok, edge)
    assert not r["marginal"].any()
    q = S.reference(state, "cull", n)
    kept = (q["verdict"] == Q.KEPT) & (q["n_obs"] >= S.CULL["min_obs"])
    assert min(_sides(kept, edge)) >= 20 and min(_sides(~q["keep"], edge)) >= 10 and min(_sides(q["keep"], edge)) >= 10
    assert not q["marginal"].any() and q["stats"]["status"] == Q.OK
    b = S.reference(state, "bundle", n)
    assert min(_sides(b["point_status"] == 0, edge)) >= 20 and b["status"] == B.OK and not b["marginal"]
    assert all(x["accepted"] == 1 and x["cg_iterations"] == S.BUNDLE["n_cg"] for x in b["rounds"])
    p = S.reference(state, "poses", n)
    assert (p["status"][1:] == 0).all() and p["status"][0] == 1 and not p["marginal"].any()
    for ent, _, _ in S.reference(state, "lookup", n):           # every frame has live rows on both sides
        assert ((ent >= 0) & (ent < edge)).sum() >= 10 and (ent >= edge).sum() >= 10
    a = S.run("adjust", c, n)
    assert min(_sides(a["point_status"] == 0, edge)) >= 20 and (a["pose_status"][1:] == 0).all()


@pytest.mark.parametrize("state", S.STATES)
def test_the_grow_adds_and_the_alignment_is_clear(state):
    c = S.case(state)
    g = S.reference(state, "grow")
    assert g["stats"]["n_added"] >= 30 and g["stats"]["status"] == Gr.OK and not g["marginal"].any()
    if state == "overflowed":
        dropped = {r.tobytes() for r in c["map_app"][c["kept"]:]}
        code, _, _ = Gr.open_rows(S.cut(c)[1], c["frames"])
        n_open_dropped = sum(1 for f, i in zip(*np.nonzero(code == 0)) if c["frames"][f][1][i].tobytes() in dropped)
        assert n_open_dropped >= 10
    for side in ("dst", "src"):
        a = S.align_reference(state, side)
        assert a["status"] == 0 and a["n_matches"] == S.N_SHARED and a["band_pop"].sum() == 0 and not any(a["band_models"])
        pairs = a["pairs"]
        col = 1 if side == "dst" else 0                        # the state's entries among the matches
        if c["kept"] > c["edge"]:
            assert (pairs[:, col] >= c["edge"]).sum() >= 20 and (pairs[:, col] < c["edge"]).sum() >= 20
    cv = S.reference(state, "covis")
    assert cv["stats"]["n_entries_seen"] >= 250
    if c["kept"] > c["edge"]:
        assert cv["sees"][:, c["edge"]:].sum(1).min() >= 10


def test_the_rows_kept_can_be_told_from_all_rows():
    """`overflowed`: the restatements on the 1024 rows kept against the restatements on all 1200.  Every landmark is judged on its
    own, so an entry's status is the same in both; what differs is what the test reads: the number of entries, the rows that
    hit (a dropped class is a miss), hence every frame's observations, the bits, and the grow's rows and tracks."""
    c = S.case("overflowed")
    cut, full = S.reference("overflowed", "lookup"), S.reference("overflowed", "lookup", 1200)
    for (e0, _, _), (e1, _, _) in zip(cut, full):
        assert ((e0 == -1) & (e1 >= 1024)).sum() >= 10 and np.array_equal(e0[e1 < 1024], e1[e1 < 1024])
    p0, p1 = S.reference("overflowed", "poses"), S.reference("overflowed", "poses", 1200)
    assert (p0["n_obs"] < p1["n_obs"]).all()
    r0, r1 = S.reference("overflowed", "refine"), S.reference("overflowed", "refine", 1200)
    assert len(r0["status"]) == 1024 and len(r1["status"]) == 1200 and r0["stats"]["by_status"] != r1["stats"]["by_status"]
    g0, g1 = S.reference("overflowed", "grow"), S.reference("overflowed", "grow", 1200)
    assert not np.array_equal(g0["rows"], g1["rows"]) and g0["stats"]["n_tracks"] > g1["stats"]["n_tracks"]
    q0, q1 = S.reference("overflowed", "cull"), S.reference("overflowed", "cull", 1200)
    assert q0["stats"]["by_verdict"] != q1["stats"]["by_verdict"]
