"""How a tail-form solve is submitted (capi.hip, picp_tail_policy; VO_PICP_TAIL_SUBMIT): replayed from a captured graph behind a
plain launch of round 0, or as plain launches throughout.  The kernels and their arguments are the same, so every byte a
solve leaves is; what differs is what the handle keeps (no graph is captured or looked up for a plain solve) and what
voe_picp_submit_info counts.  Unset, a handle submits plainly the solves at an M it has learned -- the learned ring tier and the
early tier -- and everything else as before.

Every expectation is the launch-per-round solve (VO_PICP_TAIL=0) on a fresh handle.  Pairs, sizes (2 and 33 workgroups) and
first repeats (k, j) are those of test_gpu_tail_launch.py / test_gpu_tail_early.py:
    all-gated 257 (1, 0)   seed 7 at 257 (19, 17)   seed 3 at 8193 (10, 8)   seed 5 at 8193 (14, 9)   seed 4 at 8193 (34, 33)"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_tail_early import EARLY_LEARN, LEARN, expected
from test_gpu_tail_launch import M_DEFAULT, Case, env, gated_pair, state

gpu = pytest.mark.gpu
REPEATS = {"gated257": (1, 0), "p257": (19, 17), "p8193_early": (10, 8), "p8193": (14, 9), "p8193_late": (34, 33)}


@pytest.fixture(scope="module")
def cases(vo, ctx):
    c = {
        "gated257": Case(vo, ctx, gated_pair(vo, 257)),
        "p257": Case(vo, ctx, vo.synth.frame_pair(257, seed=7)),
        "p8193_early": Case(vo, ctx, vo.synth.frame_pair(8193, seed=3)),
        "p8193_late": Case(vo, ctx, vo.synth.frame_pair(8193, seed=4)),
        "p8193": Case(vo, ctx, vo.synth.frame_pair(8193, seed=5)),
    }
    for name, case in c.items():
        assert len(case.corr) == (257 if "257" in name else 8193), name
    return c


def everything(case, n, s, **kv):
    """all a solve of n rounds leaves: (pose, T16, H, b, chi sums in hex, inliers), cycleInfo, tailInfo, tailCloseInfo"""
    st, info, tail = case.solve(n, s, **kv)
    return st, info, tail, s.tailCloseInfo()


def both_forms(case, n, m, rep, early, plain, graph):
    """one solve per form at a forced M on the two handles; returns whether the solve had a tail launch"""
    kv = dict(tail_from=m, tail_early=1 if early else None)
    g0, p0, n_graphs = plain.submitInfo() + (plain.graphInfo()[1],)
    got_p = everything(case, n, plain, tail_submit="plain", **kv)
    got_g = everything(case, n, graph, tail_submit="graph", **kv)
    want_st, want_info = case.ref(n)
    want_tail, want_how = expected(want_info, n, m, rep, early)
    print(f"N = {n}, M = {m}, early {early}: plain {got_p[1:]}, graph {got_g[1:]} (expected {want_tail}, {want_how})")
    assert got_p == got_g
    assert got_p[0] == want_st and got_p[1] == want_info
    assert got_p[2] == want_tail and got_p[3] == (want_how, m if want_how != "none" else 0)
    # the plain handle captured nothing for a tail-form solve; a solve that is not eligible at this M is a graph solve
    if want_tail[0]:
        assert plain.submitInfo() == (g0, p0 + 1) and plain.graphInfo()[1] == n_graphs
    else:
        assert plain.submitInfo() == (g0 + 1, p0)
    return want_tail[0]


@gpu
@pytest.mark.parametrize("name", sorted(REPEATS))
def test_same_bytes_in_both_forms(vo, ctx, cases, name):
    case, (k, j) = cases[name], REPEATS[name]
    assert case.first_repeat(k) == (k, j)
    plain, graph = vo.PICPSolver(ctx), vo.PICPSolver(ctx)
    tails = 0
    for m in [m for m in (k - 2, k - 1, k, k + 1) if m >= 1]:
        for n in list(range(k + 2, k + 5 + (k - j))) + [50]:
            for early in (False, True):
                tails += both_forms(case, n, m, (k, j), early, plain, graph)
    assert tails > 0
    assert graph.submitInfo()[1] == 0 and plain.graphInfo()[2] == 0 and graph.graphInfo()[2] == 0
    plain.close()
    graph.close()


@gpu
def test_loop_path_submitted_plainly(vo, ctx, cases):
    """seed 4 over 12 rounds at M = 1: ten real in-launch rounds, counter barriers and all, behind plain launches"""
    case = cases["p8193_late"]
    assert case.first_repeat(34) == (34, 33)
    plain, graph = vo.PICPSolver(ctx), vo.PICPSolver(ctx)
    for early in (False, True):
        assert both_forms(case, 12, 1, (34, 33), early, plain, graph)
        assert plain.tailInfo() == (True, 10, False) and plain.cycleInfo() == (0, 0, 0) and plain.tailCloseInfo() == ("looped", 1)
    plain.close()
    graph.close()


def unforced(case, s, n=30, **kv):
    got = everything(case, n, s, **kv)
    assert got[:2] == case.ref(n)
    return got[2], got[3], s.submitInfo(), s.graphInfo()[1]


@gpu
def test_who_takes_it(vo, ctx, cases):
    """no switch set, getters behind every solve (each report has arrived before the next enqueue): the schedule of
    test_the_host_takes_the_form_behind_enough_witnesses.  Seed 3: M = 16 for LEARN solves -- graph solves --, 12 from the next
    -- the learned ring tier, the first plain solve --, the early form at M = 9 from solve EARLY_LEARN + 1.  From the first plain
    solve on the handle captures nothing.  A seed 5 solve runs real rounds inside the launch: M back to 16, the next solve back
    on the graph."""
    early, mid = cases["p8193_early"], cases["p8193"]
    s = vo.PICPSolver(ctx)
    ran = [unforced(early, s) for _ in range(EARLY_LEARN + 6)]
    print(ran)
    for i, (tail, close, submit, n_graphs) in enumerate(ran):
        assert tail == (True, 0, False)
        assert close == (("ring", M_DEFAULT) if i < LEARN else ("ring", 12) if i < EARLY_LEARN else ("early", 9)), (i, close)
        assert submit == (min(i + 1, LEARN), max(0, i + 1 - LEARN)), (i, submit)
        assert n_graphs == ran[min(i, LEARN - 1)][3], (i, n_graphs)
    g, p = ran[-1][2]
    n_graphs = ran[-1][3]
    assert unforced(mid, s) == ((True, 4, False), ("early", 9), (g, p + 1), n_graphs)
    got = unforced(mid, s)
    assert got[:3] == ((True, 0, False), ("ring", M_DEFAULT), (g + 1, p + 1))
    got = unforced(early, s)
    assert got[:3] == ((True, 0, False), ("ring", M_DEFAULT), (g + 2, p + 1))
    # solves that are no tail form at any M are graph solves, whatever the switch says
    for n, kv in ((5, {}), (7, {}), (5, {"tail_submit": "plain"}), (7, {"tail_submit": "plain"})):
        before = s.submitInfo()
        got = everything(early, n, s, **kv)
        assert got[:2] == early.ref(n) and got[2] == (False, 0, False)
        assert s.submitInfo() == (before[0] + 1, before[1])
    s.close()
    # VO_PICP_TAIL_SUBMIT=graph: the same tiers, never a plain solve
    s = vo.PICPSolver(ctx)
    ran = [unforced(early, s, tail_submit="graph") for _ in range(EARLY_LEARN + 2)]
    assert [r[1] for r in ran[LEARN:]] == [("ring", 12)] * (EARLY_LEARN - LEARN) + [("early", 9)] * 2
    assert all(r[2] == (i + 1, 0) for i, r in enumerate(ran)), ran
    s.close()


@gpu
def test_mixed_stream(vo, ctx, cases):
    """plain and graph solves alternating on one handle, then six oneRound calls, against a handle that only ever used the
    graph: every solve and the chain behind them leave the same bytes"""
    a = cases["p8193_early"]
    mixed, graph = vo.PICPSolver(ctx), vo.PICPSolver(ctx)
    for i in range(40):
        got = everything(a, 30, mixed, tail_submit="plain" if i % 2 == 0 else "graph")
        want = everything(a, 30, graph, tail_submit="graph")
        assert got == want, i
        assert got[:2] == a.ref(30)
    assert mixed.submitInfo() == (20, 20) and graph.submitInfo() == (40, 0)

    def chain(h):
        a.start(h)
        for _ in range(6):
            h.oneRound(a.corr, a.keep)
        return state(vo, ctx, h)

    assert chain(mixed) == chain(graph)
    mixed.close()
    graph.close()


@gpu
def test_under_a_callers_capture(vo, ctx, cases):
    """a solve captured into a caller's graph keeps a launch per round, also on a handle that submits plainly and with
    VO_PICP_TAIL_SUBMIT=plain set, and replays to the reference's bytes; it is counted as neither form"""
    a = cases["p8193_early"]
    lib = ctx.lib
    s = vo.PICPSolver(ctx)
    for _ in range(LEARN + 2):
        unforced(a, s)
    assert s.tailCloseInfo() == ("ring", 12) and s.submitInfo() == (LEARN, 2)
    d_pairs = ctx.to_device(np.ascontiguousarray(a.corr, np.int32))
    d_ident = ctx.to_device(np.ascontiguousarray(np.eye(4, dtype=np.float32)))
    g = C.c_void_p()
    with env(tail_submit="plain"):
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        try:
            rc = lib.vo_picp_set_pose_dev(s.h, C.c_void_p(d_ident))
            rc2 = lib.vo_picp_solve_dev(s.h, C.c_void_p(d_pairs), C.c_int(len(a.corr)), None, C.c_int(int(a.keep)), C.c_int(30))
        finally:
            assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0
        assert rc == 0 and rc2 == 0, lib.vo_last_error()
    try:
        for _ in range(2):
            assert lib.vo_graph_launch(g) == 0
            assert (state(vo, ctx, s), s.cycleInfo()) == a.ref(30)
            assert s.tailInfo() == (False, 0, False)
        assert s.submitInfo() == (LEARN, 2)
    finally:
        lib.vo_graph_destroy(g)
        ctx.free(d_pairs)
        ctx.free(d_ident)
        s.close()
